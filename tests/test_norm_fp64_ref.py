"""CPU pins of the normalisation references of tests/fp64_ref.py (batchnorm_fp64, groupnorm_fp64, add_layernorm_fp64), and the
place where the constants of tests/test_norm_fp64_gpu.py are fixed.

1. The references equal nn.BatchNorm1d (+ add + relu), F.group_norm on the NCHW view and nn.LayerNorm(x + r), evaluated in
   float64 with autograd, to 1e-12 of their terms (+ 2^-29 of the conditioning allowance), running statistics included, on every
   input family and shape of the GPU tests; |value| <= mag everywhere.
2. The SAME PyTorch ops in fp32 -- what the kernels replace -- are held against the references on the CPU.  The worst err / bound
   at c = 1 per family and output is printed; the figures are recorded in FIG_BN / FIG_GN / FIG_LN of the GPU test file, from
   which its constants follow as c = min(16, 4 x figure) rounded up to a power of two and at least 1; the tests here assert that
   the composite passes at that c, so every bar is known to be attainable before a GPU is involved.  The share of ReLU ties
   (`near_zero`) is asserted to be at most 0.1 % in every ReLU case.
   One exception, as for the focal loss (tests/test_det_loss_fp64_ref.py): ATen's CPU kernels do not subtract the mean first (y = x
   scale + shift in all three ops; dx = c1 dy + c2 x + c3 in GroupNorm and LayerNorm), which cancels when |mean| is large against the
   spread and loses every digit of dx on the offset family.  That is an error of the formulation and not of the definition, so
   those outputs of the ATen ops are held to the bar + 4 x the size of the cancelling terms (`aten_cancellation`), the definition
   written out in fp32 with plain torch (`formula_norm32`, mean subtracted first, as the kernels do) is held to the bar itself, and
   the recorded figure is the larger of the two."""
import pytest
import torch
import torch.nn.functional as F

from fp64_ref import U32, add_layernorm_fp64, assert_elementwise, batchnorm_fp64
from test_norm_fp64_gpu import (BN_EPS, BN_MOMENTUM, BN_NHWC_SHAPE, BN_SHAPES, C_BN, C_GN, C_LN, FAMILIES, FIG_BN, FIG_GN,
                                FIG_LN, GN_EPS, GN_SHAPES, LN_CS, LN_EPS, LN_LONG, LN_ROWS, NEAR_ZERO_CAP, bar_constant,
                                bn_cases, bn_problem, bn_reference, check, gn_problem, gn_reference, ln_problem, ln_reference,
                                ratios)

CPU = torch.device("cpu")
F64_COND = 2.0 ** -29      # float64's unit roundoff over float32's: the conditioning allowance of a float64 evaluation


def _same(name, got, ref):
    """Two float64 evaluations of one formula: every output equal to 1e-12 of the terms (+ the conditioning at float64's
    roundoff); |value| <= mag."""
    for k, g in got.items():
        r, mag, cond = ref[k], ref[k + "_mag"], ref[k + "_cond"]
        assert g.dtype == torch.float64 and g.shape == r.shape, "%s %s" % (name, k)
        bad = (g - r).abs() > 1e-12 * mag + F64_COND * cond + 1e-300
        assert not bool(bad.any()), "%s %s: %d elements differ, worst %.3g" % (name, k, int(bad.sum()), float((g - r).abs().max()))
        assert bool((r.abs() <= mag * (1 + 1e-12) + 1e-300).all()), "%s %s: magnitude below |value|" % (name, k)
        assert bool((cond >= 0).all()) and bool(torch.isfinite(cond).all()), "%s %s: allowance" % (name, k)


# ---- the composites (plain PyTorch, any dtype) ----------------------------------------------------------------------------------
def composite_bn(p, relu, dtype, dy_ones=False):
    c = p["w"].numel()
    bn = torch.nn.BatchNorm1d(c, eps=BN_EPS, momentum=BN_MOMENTUM).to(dtype).train()
    with torch.no_grad():
        bn.weight.copy_(p["w"])
        bn.bias.copy_(p["b"])
        bn.running_mean.copy_(p["running_mean"])
        bn.running_var.copy_(p["running_var"])
    x = p["x"].clone().to(dtype).requires_grad_(True)
    r = p["residual"].clone().to(dtype).requires_grad_(True) if p["residual"] is not None else None
    y = bn(x)
    if r is not None:
        y = y + r
    if relu:
        y = torch.relu(y)
    y.backward(torch.ones_like(y) if dy_ones else p["dy"].to(dtype))
    assert int(bn.num_batches_tracked) == 1
    got = dict(y=y.detach(), dx=x.grad, dweight=bn.weight.grad, dbias=bn.bias.grad, running_mean=bn.running_mean.clone(),
               running_var=bn.running_var.clone())
    if r is not None:
        got["dresidual"] = r.grad
    return got


def composite_gn(p, groups, dtype, dy_ones=False):
    x = p["x"].clone().to(dtype).requires_grad_(True)
    w, b = p["w"].clone().to(dtype).requires_grad_(True), p["b"].clone().to(dtype).requires_grad_(True)
    y = F.group_norm(x.movedim(-1, 1), groups, w, b, GN_EPS).movedim(1, -1)
    y.backward(torch.ones_like(y) if dy_ones else p["dy"].to(dtype))
    return dict(y=y.detach(), dx=x.grad, dweight=w.grad, dbias=b.grad)


def composite_ln(p, dtype, dy_ones=False):
    """LayerNorm(x + r).  The fp32 sum z = x + r is the op's saved tensor: the float64 evaluation starts from that fp32 z."""
    c = p["w"].numel()
    norm = torch.nn.LayerNorm(c, eps=LN_EPS).to(dtype)
    with torch.no_grad():
        norm.weight.copy_(p["w"])
        norm.bias.copy_(p["b"])
    if dtype == torch.float32:
        x = p["x"].clone().requires_grad_(True)
        r = p["residual"].clone().requires_grad_(True) if p["residual"] is not None else None
        z = x if r is None else x + r
    else:
        x = z = (p["x"] if p["residual"] is None else p["x"] + p["residual"]).to(dtype).requires_grad_(True)
        r = z if p["residual"] is not None else None
    y = norm(z)
    y.backward(torch.ones_like(y) if dy_ones else p["dy"].to(dtype))
    got = dict(y=y.detach(), dx=x.grad, dweight=norm.weight.grad, dbias=norm.bias.grad)
    if r is not None:
        got["dresidual"] = r.grad
    return got


def formula_norm32(x, stat_dims, par_dims, w, b, eps, dy, res=None, relu=False):
    """The definition and its backward as the reference writes them -- mu, the biased variance about mu, xhat = (x - mu) rstd,
    y = relu?(xhat w + b + res?), dx = rstd (g - mean(g) - xhat mean(g xhat)) with g = w dy [y > 0], dw = sum dy' xhat, db = sum dy'
    -- in fp32 with plain torch; all tensors in the view in which `stat_dims` are the statistics axes.  Returns a dict: y, dx,
    dresidual (= dy'), dweight, dbias, mean, var."""
    x, w, b, dy = (t.detach().float() for t in (x, w, b, dy))
    mu = x.mean(stat_dims, keepdim=True)
    xc = x - mu
    var = (xc * xc).mean(stat_dims, keepdim=True)
    rstd = (var + eps) ** -0.5
    xh = xc * rstd
    y = xh * w + b
    if res is not None:
        y = y + res.float()
    if relu:
        dy = dy * (y > 0)
        y = y.clamp(min=0)
    g = w * dy
    dx = rstd * (g - g.mean(stat_dims, keepdim=True) - xh * (g * xh).mean(stat_dims, keepdim=True))
    return dict(y=y, dx=dx, dresidual=dy, dweight=(dy * xh).sum(par_dims), dbias=dy.sum(par_dims), mean=mu, var=var)


def aten_cancellation(x, stat_dims, w, dy, eps):
    """What the formulation of ATen's GroupNorm / LayerNorm CPU kernels adds to the error of y and dx, per 2^-24.  They evaluate
    y = x (rstd w) + (b - mean rstd w) and dx = rstd w dy + c2 x + c3 with c2 = (mean sum(g) - sum(g x)) rstd^3 / n and c3 = -c2
    mean - sum(g) rstd / n (g = w dy): differences of terms of the size of |x| and |mean| for results of the size of the spread.
    With the data far from 0 (x = 1000 +- 0.01) the gradient loses every digit; that is an error of this formulation, not of the
    definition -- the kernels and the reference subtract the mean first.  Sizes of the cancelling terms: (|x| + |mean|) rstd |w|
    for y, (rstd^3 / n (|mean| sum |g| + sum |g x|) + |c2|) (|x| + |mean|) for dx.  View tensors in, float64 (y, dx) like x out."""
    x, w, g = x.double(), w.double(), (w * dy).double()
    n = 1
    for d in stat_dims:
        n *= x.shape[d]
    mean = x.mean(stat_dims, keepdim=True)
    rstd = (((x - mean) ** 2).mean(stat_dims, keepdim=True) + eps) ** -0.5
    size = rstd ** 3 / n * (mean.abs() * g.abs().sum(stat_dims, keepdim=True) + (g * x).abs().sum(stat_dims, keepdim=True))
    c2 = rstd ** 3 / n * (mean * g.sum(stat_dims, keepdim=True) - (g * x).sum(stat_dims, keepdim=True))
    return (x.abs() + mean.abs()) * rstd * w.abs(), (size + c2.abs()) * (x.abs() + mean.abs())


def _pin(name, ref, got64, got32, consts, worst, aten=None, formula=None):
    """The float64 composite equals the reference; the fp32 composite passes at the GPU test's constants; its figures go into
    `worst`.  `aten` = the sizes of the terms that cancel in ATen's kernels (`aten_cancellation`: y of all three ops, dx of
    GroupNorm and LayerNorm): the composite's y, dx and d residual are held to the bar + 4 x that cancellation, `formula` -- the
    written-out definition in fp32 -- to the bar itself, and the figure of an output is the larger of the two."""
    if aten is None:
        _same(name, got64, ref)
        fig = check(name + " fp32 composite", got32, ref, consts)
    else:
        loose = dict(ref)
        for k, extra in (("y", aten[0]), ("dx", aten[1]), ("dresidual", aten[1])):
            if k in got32 and extra is not None:
                loose[k + "_cond"] = ref[k + "_cond"] + 4 * U32 * extra.reshape(ref[k].shape)
        _same(name, got64, loose)
        bare = ratios(got32, ref)
        print("%s: the fp32 composite without the allowance for its cancellation: y %.3g, dx %.3g" % (name, bare["y"], bare["dx"]))
        fig = check(name + " fp32 composite + its cancellation", got32, loose, consts)
        for k, v in check(name + " fp32 formula", formula, ref, consts).items():
            fig[k] = max(fig[k], v)
    for k, v in fig.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _report(op, family, worst, recorded, consts):
    print("%s %s: fp32 composite, worst err / bound at c = 1: %s" % (op, family, ", ".join("%s=%.2f" % kv for kv in sorted(worst.items()))))
    assert set(worst) == set(recorded) == set(consts), "%s %s: outputs %s" % (op, family, sorted(worst))
    for k in consts:
        assert consts[k] == bar_constant(recorded[k]) and 1 <= consts[k] <= 16


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_batchnorm_reference_and_the_fp32_composite(family):
    """batchnorm_fp64 == nn.BatchNorm1d + add + relu + autograd in float64 on every case of the GPU test, and the fp32 modules
    inside the bar at the GPU test's constants.  Worst err / bound at c = 1 of the fp32 composite (CPU): FIG_BN in
    tests/test_norm_fp64_gpu.py; the largest figure of each family:
        plain    y, running_mean 1.08   offset   running_var 1.96   scales   running_var 2.09
        constant running_var 1.59       strided  y 0.91
    ATen's forward is y = x (rstd w) + (b - mean rstd w) (`aten_cancellation`): bare, two y of plain [2, 516] miss the bar at c = 8.
    It is held to the bar + 4 x that cancellation, the written-out definition in fp32 to the bar itself, and the figure of an
    output is the larger of the two.
    Two things in the allowance go past the first-order effect of d_mu = sqrt(n) 2^-24 mean|x| and d_rstd / rstd = (sqrt(n) + 2)
    2^-24, and both are measured needs of the offset family (x = 1000 +- 0.01).  Without the variance taken about the ROUNDED
    mean (d_mu^2 / (2 (var + eps)) in d_rstd / rstd) the fp32 modules miss the bar at the cap c = 16: err / bound 1.29 on dx of
    [8161, 516] (and 2.13 / 1.01 for the GroupNorm / LayerNorm yardsticks).  Without the second-order Taylor terms the written-out
    definition in fp32 misses it on LayerNorm [32785, 4]: 2.1 at c = 16, at elements whose first-order term happens to vanish."""
    worst = {}
    if family == "strided":
        cases = [(2079, 516, family, True, True), (33, 96, family, False, False)]
    else:
        cases = [case for case in bn_cases() if case[2] == family]
        assert len(cases) == len(BN_SHAPES)
        if family == "plain":
            bsz, c, h, w = BN_NHWC_SHAPE
            cases += [(bsz * h * w, c, family, True, False), (bsz * h * w, c, family, False, False)]
    combos = set()
    for m, c, _, relu, with_res in cases:
        p = bn_problem(m, c, family, with_res)
        ref = bn_reference(p, relu, CPU, dy_ones=family == "strided")
        assert ref["near_zero_share"] <= NEAR_ZERO_CAP and (relu or ref["near_zero_share"] == 0)
        combos.add((relu, with_res))
        dy = torch.ones_like(p["x"]) if family == "strided" else p["dy"]
        f32 = formula_norm32(p["x"], (0,), (0,), p["w"][None], p["b"][None], BN_EPS, dy, p["residual"], relu)
        formula = {k: f32[k] for k in ("y", "dx", "dweight", "dbias") + (("dresidual",) if with_res else ())}
        formula["running_mean"] = (1 - BN_MOMENTUM) * p["running_mean"] + BN_MOMENTUM * f32["mean"][0]
        formula["running_var"] = (1 - BN_MOMENTUM) * p["running_var"] + BN_MOMENTUM * f32["var"][0] * (m / (m - 1))
        _pin("bn %s [%d, %d] relu=%d res=%d" % (family, m, c, relu, with_res), ref,
             composite_bn(p, relu, torch.float64, family == "strided"), composite_bn(p, relu, torch.float32, family == "strided"),
             C_BN[family], worst, aten=(aten_cancellation(p["x"], (0,), p["w"][None], dy, BN_EPS)[0], None), formula=formula)
    if family in ("plain", "scales", "constant"):
        assert len(combos) == 4
    _report("BatchNorm", family, worst, FIG_BN[family], C_BN[family])


def test_batchnorm_reference_by_hand():
    """Two rows, one channel, by hand: x = (1, 3): mu = 2, var = 1, rstd = (1 + eps)^-1/2; y = +-rstd w + b; the unbiased
    variance is 2; and with ReLU the negative element is cut in y and in every gradient."""
    x = torch.tensor([[1.0], [3.0]]).repeat(1, 4)
    one, zero = torch.ones(4), torch.zeros(4)
    dy = torch.tensor([[5.0], [7.0]]).repeat(1, 4)
    r = batchnorm_fp64(x, None, 2 * one, 0.5 * one, zero, one, 0.3, 1e-5, True, dy)
    s = (1 + 1e-5) ** -0.5
    assert torch.allclose(r["y"][:, 0], torch.tensor([0.0, 2 * s + 0.5], dtype=torch.float64), rtol=1e-14, atol=0)
    assert abs(float(r["running_mean"][0]) - 0.6) < 1e-15 and abs(float(r["running_var"][0]) - (0.7 + 0.3 * 2)) < 1e-14
    assert abs(float(r["dbias"][0]) - 7) < 1e-14 and abs(float(r["dweight"][0]) - 7 * s) < 1e-14
    # g = (0, 14): mean 7, mean(g xhat) = 7 s; dx = s (g - 7 - xhat 7 s) with xhat = -+s
    want = torch.tensor([s * (0 - 7 + 7 * s * s), s * (14 - 7 - 7 * s * s)], dtype=torch.float64)
    assert torch.allclose(r["dx"][:, 0], want, rtol=1e-10, atol=1e-15)
    assert r["near_zero_share"] == 0 and r["dx_n"] == 2 and r["dweight_n"] == 2


def test_relu_ties_are_marked_and_enter_the_allowance():
    """A pre-activation of exactly 0 is a tie: marked near_zero, and its |dy| is in dbias_cond."""
    x = torch.tensor([[1.0], [3.0], [2.0]]).repeat(1, 4)           # xhat of the third row is 0; with b = 0 so is y
    dy = torch.tensor([[1.0], [1.0], [11.0]]).repeat(1, 4)
    r = batchnorm_fp64(x, None, torch.ones(4), torch.zeros(4), torch.zeros(4), torch.ones(4), 0.1, 1e-5, True, dy)
    assert r["near_zero"].tolist() == [[False] * 4, [False] * 4, [True] * 4]
    assert bool((r["dbias_cond"] >= 11).all()) and bool((r["dbias_cond"] < 11.01).all())
    assert bool((r["dx_cond"][0] > 1.2 * 11 / 3).all())      # rstd |w dy| / n of the tie, inside the mean of dx


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_groupnorm_reference_and_the_fp32_composite(family):
    """groupnorm_fp64 == F.group_norm on the NCHW view + autograd in float64 on every case of the GPU test, and the fp32 op
    inside the bar.  Worst err / bound at c = 1 of the fp32 composite (CPU): FIG_GN; the largest figure of each family:
        plain    y 0.91           offset   dbias 0.61         scales   y 1.02
        constant y 0.96           strided  y 0.84
    ATen's GroupNorm cancels in y and in dx (`aten_cancellation`): bare, its dx stands at 121 x the unit bar on the offset family
    ((4, 15, 1024, 256)).  Same treatment as BatchNorm's y."""
    worst = {}
    shapes = [(3, 33, 16, 4), (2, 40, 516, 3)] if family == "strided" else GN_SHAPES
    for shape in shapes:
        p = gn_problem(shape, family)
        ref = gn_reference(p, shape[3], CPU, dy_ones=family == "strided")
        bsz, rows, c, groups = shape
        view = lambda t: t.reshape(-1, groups, c // groups) if t.dim() == 1 else t.reshape(bsz, rows, groups, c // groups)   # noqa: E731
        x, w, b = view(p["x"]), view(p["w"])[None], view(p["b"])[None]
        dy = torch.ones_like(x) if family == "strided" else view(p["dy"])
        f32 = formula_norm32(x, (1, 3), (0, 1), w, b, GN_EPS, dy)
        extra = dict(aten=aten_cancellation(x, (1, 3), w, dy, GN_EPS),
                     formula={k: f32[k].reshape(ref[k].shape) for k in ("y", "dx", "dweight", "dbias")})
        _pin("gn %s %s" % (family, shape), ref, composite_gn(p, shape[3], torch.float64, family == "strided"),
             composite_gn(p, shape[3], torch.float32, family == "strided"), C_GN[family], worst, **extra)
    _report("GroupNorm", family, worst, FIG_GN[family], C_GN[family])


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_add_layernorm_reference_and_the_fp32_composite(family):
    """add_layernorm_fp64 == nn.LayerNorm(fp32(x + r)) + autograd in float64 on every case of the GPU test, and the fp32 add +
    LayerNorm inside the bar.  Worst err / bound at c = 1 of the fp32 composite (CPU): FIG_LN; the largest figure of each
    family:
        plain    y 1.03           offset   y, dx 0.86         scales   dbias 1.38
        constant y 1.13           strided  y 0.43
    ATen's LayerNorm cancels like its GroupNorm (`aten_cancellation`): bare, its dx stands at 5.0e3 x the unit bar on the offset
    family ([65539, 8]) and one y of the constant family's [32785, 4] misses the bar at c = 16 by 1 %.  Same treatment as there."""
    worst = {}
    if family == "strided":
        shapes = [(77, 260), (17, 1020), (16, 36)]
    else:
        shapes = [(rows, c) for c in LN_CS for rows in LN_ROWS] + LN_LONG
    for rows, c in shapes:
        for with_res in (True, False):
            p = ln_problem(rows, c, family, with_res)
            ref = ln_reference(p, CPU, dy_ones=family == "strided")
            got64, got32 = (composite_ln(p, dt, family == "strided") for dt in (torch.float64, torch.float32))
            z = p["x"] if not with_res else p["x"] + p["residual"]
            dy = torch.ones_like(z) if family == "strided" else p["dy"]
            f32 = formula_norm32(z, (1,), (0,), p["w"][None], p["b"][None], LN_EPS, dy)
            formula = {k: f32[k] for k in ("y", "dx", "dweight", "dbias")}
            if with_res:
                formula["dresidual"] = f32["dx"]
            extra = dict(aten=aten_cancellation(z, (1,), p["w"][None], dy, LN_EPS), formula=formula)
            _pin("ln %s [%d, %d] res=%d" % (family, rows, c, with_res), ref, got64, got32, C_LN[family], worst, **extra)
            if with_res:
                assert torch.equal(ref["dresidual"], ref["dx"])
    _report("LayerNorm", family, worst, FIG_LN[family], C_LN[family])


def test_add_layernorm_reference_forms_the_sum_in_fp32():
    """z = fp32(x + r): 1 + 2^-25 rounds to 1 in fp32, so the row (1 + 2^-25, 2, 3, 4) is normalised as (1, 2, 3, 4)."""
    x = torch.tensor([[1.0, 2.0, 3.0, 4.0]])
    r = torch.tensor([[2.0 ** -25, 0.0, 0.0, 0.0]])
    ref = add_layernorm_fp64(x, r, torch.ones(4), torch.zeros(4), 1e-5, torch.ones(1, 4))
    assert torch.equal(ref["z"], x.double())
    assert abs(float(ref["y"].sum())) < 1e-15 and abs(float(ref["y"][0, 3]) - 1.5 * (1.25 + 1e-5) ** -0.5) < 1e-15
    assert float(ref["dx"].abs().max()) < 1e-15          # dy = 1 lies in the null space of the LayerNorm backward


# ---- the bar has teeth ------------------------------------------------------------------------------------------------------------
def test_bar_catches_a_small_element_off_by_1e_4_and_a_biased_running_variance():
    """On the scales family a well-conditioned dx element of a small channel, scaled by 1 + 1e-4, fails at the cap c = 16 although
    it is 1e-9 of the tensor's largest; so does the running variance with M in place of M - 1."""
    p = bn_problem(33, 96, "scales", False)
    ref = bn_reference(p, False, CPU)
    got = composite_bn(p, False, torch.float32)
    quiet = (ref["dx_cond"] < 1e-6 * ref["dx"].abs()) & (ref["dx_mag"] < 4 * ref["dx"].abs())
    flat = torch.where(quiet, ref["dx"].abs(), torch.full_like(ref["dx"], float("inf"))).reshape(-1)
    i = int(torch.argmin(flat))
    assert float(flat[i]) < 1e-9 * float(ref["dx"].abs().max())
    bad = got["dx"].clone()
    bad.view(-1)[i] *= 1 + 1e-4
    with pytest.raises(AssertionError, match="1 of"):
        assert_elementwise("scaled element", bad, ref["dx"], ref["dx_mag"], ref["dx_n"], 16, geo64=ref["dx_cond"])
    biased = got["running_var"] - BN_MOMENTUM * p["x"].double().var(0, unbiased=True).float() / 33
    with pytest.raises(AssertionError):
        assert_elementwise("biased", biased, ref["running_var"], ref["running_var_mag"], 1, 16, geo64=ref["running_var_cond"])
    assert ratios(got, ref)["running_var"] <= 16
