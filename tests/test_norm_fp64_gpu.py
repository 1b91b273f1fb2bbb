"""GPU: the normalisation kernels (csrc/batchnorm.hip: BatchNorm1d / 2d (+ residual) (+ ReLU), channels-last GroupNorm;
csrc/layernorm.hip: residual-add + LayerNorm) against the float64 references of tests/fp64_ref.py, element by element, on every
output: |got - ref| <= c * sqrt(n) * 2^-24 * |terms| + cond.  `cond` is the reference's own allowance for the rounded mean and
rstd (fp64_ref.py); the constants c come from tests/test_norm_fp64_ref.py, where the fp32 PyTorch ops that the kernels replace
are measured against the same references on the same inputs on the CPU: c = min(16, 4 x the worst err / bound at c = 1),
rounded up to a power of two and at least 1, per op, input family and output.

Input families (CPU generators, fixed seeds, so the CPU pins see the same numbers), `set` = the statistics set of the op (a
channel for BatchNorm, a (sample, group) for GroupNorm, a row for LayerNorm):
    plain     N(0.3, 2)
    offset    1000 + 0.01 N(0, 1): two-pass / Chan statistics hold, a one-pass variance does not
    scales    plain, every set times its own log-uniform factor in [1e-4, 1e4]; dy log-uniform in [1e-3, 1e3] with random signs
    constant  plain with one set equal to 3.0 (var = 0, rstd = eps^-1/2)
    strided   plain, x a transposed view and the backward started from y.sum() (dy a stride-0 expand)
ReLU (BatchNorm only) is not combined with `offset`: there the allowance for the rounded mean, rstd |w| sqrt(n) 2^-24 * 1000, is
of the size of the pre-activation itself and every element would be a tie.  The constant channel of a ReLU case has bias 2.0,
which keeps it clear of 0 whatever the residual."""
import math

import pytest
import torch

from fp64_ref import U32, add_layernorm_fp64, assert_elementwise, batchnorm_fp64, groupnorm_fp64, log_uniform_signed

pytestmark = pytest.mark.gpu

FAMILIES = ("plain", "offset", "scales", "constant", "strided")
NEAR_ZERO_CAP = 1e-3            # at most 0.1 % of a ReLU case's elements may be ties (a condition on the inputs)
BN_MOMENTUM, BN_EPS, GN_EPS, LN_EPS = 0.3, 1e-5, 1e-5, 1e-5

# ---- the fp32 yardsticks' worst err / bound at c = 1 per family and output, measured on the CPU by tests/test_norm_fp64_ref.py
# (the larger of the fp32 ATen op, held to the bar + its own cancellation, and the written-out definition in fp32; see there), and
# the constants of the bars that follow from them ---------------------------------------------------------------------------------
FIG_BN = {
    "plain": dict(y=1.08, dx=0.64, dresidual=0.0, dweight=0.59, dbias=0.69, running_mean=1.08, running_var=1.06),
    "offset": dict(y=0.62, dx=0.61, dresidual=0.0, dweight=0.36, dbias=0.70, running_mean=1.08, running_var=1.96),
    "scales": dict(y=2.01, dx=0.66, dresidual=0.0, dweight=0.66, dbias=0.68, running_mean=1.95, running_var=2.09),
    "constant": dict(y=1.28, dx=0.60, dresidual=0.0, dweight=0.63, dbias=0.66, running_mean=1.15, running_var=1.59),
    "strided": dict(y=0.91, dx=0.37, dresidual=0.0, dweight=0.11, dbias=0.0, running_mean=0.24, running_var=0.24),
}
FIG_GN = {
    "plain": dict(y=0.91, dx=0.27, dweight=0.20, dbias=0.47),
    "offset": dict(y=0.50, dx=0.40, dweight=0.49, dbias=0.61),
    "scales": dict(y=1.02, dx=0.31, dweight=0.35, dbias=0.45),
    "constant": dict(y=0.96, dx=0.28, dweight=0.33, dbias=0.52),
    "strided": dict(y=0.84, dx=0.33, dweight=0.02, dbias=0.0),
}
FIG_LN = {
    "plain": dict(y=1.03, dx=0.82, dresidual=0.82, dweight=0.31, dbias=0.76),
    "offset": dict(y=0.86, dx=0.86, dresidual=0.86, dweight=0.48, dbias=0.74),
    "scales": dict(y=1.15, dx=1.15, dresidual=1.15, dweight=0.30, dbias=1.38),
    "constant": dict(y=1.13, dx=0.97, dresidual=0.97, dweight=0.06, dbias=0.72),
    "strided": dict(y=0.43, dx=0.21, dresidual=0.21, dweight=0.08, dbias=0.0),
}


def bar_constant(figure):
    """min(16, 4 x figure), rounded up to a power of two and at least 1."""
    return 2.0 ** math.ceil(math.log2(max(1.0, min(16.0, 4.0 * figure))))


C_BN, C_GN, C_LN = ({f: {k: bar_constant(v) for k, v in fig.items()} for f, fig in table.items()} for table in (FIG_BN, FIG_GN, FIG_LN))

# ---- shapes: the smallest that reach each path of the kernels ------------------------------------------------------------------
# BatchNorm [M, C]: chunks = min(1024, ceil(M / 32)): M = 2079 -> 65, 8161 -> 256, 32769 -> the cap with 33 rows per chunk and 31
# empty trailing chunks, 40000 -> the cap with 40 rows and 24 empty chunks; C = 516 / 1020 leave 127 / 1 idle threads per block
# (256 % (C / 4) != 0).  Every M with C = 4, every M up to 8161 with C = 516, every C with M = 33 and 2079, and the two large M
# with C = 96 as their widest (a [32769, 516] case would be 68 MB per tensor).
BN_SHAPES = ([(m, 4) for m in (2, 33, 2079, 8161, 32769, 40000)] + [(m, 516) for m in (2, 33, 2079, 8161)]
             + [(m, 96) for m in (33, 2079, 32769, 40000)] + [(m, c) for c in (1020, 1024) for m in (33, 2079)])
BN_COMBOS = [(True, False), (True, True), (False, False), (False, True)]          # (relu, residual)
BN_NHWC_SHAPE = (2, 8, 5, 7)
# GroupNorm (B, rows, C, groups): channels per group 4 .. 1024, single-row statistics, (chunk, channel) item counts on both
# sides of the merge kernel's 512-item unroll, 65 and 256 chunks, the chunk cap
GN_SHAPES = [(2, 1, 8, 2), (3, 33, 16, 4), (2, 2079, 64, 16), (1, 32769, 8, 2), (2, 8161, 8, 1), (2, 17, 1024, 1),
             (4, 15, 1024, 256), (2, 40, 516, 3)]
# LayerNorm: C on both sides of the 1 / 2 / 4 float4-per-lane kernels with full and partly filled last passes; rows around the
# 16 rows of a workgroup; and the second and third trip of the backward's grid-stride loop (2048 workgroups x 16 rows)
LN_CS = (4, 36, 252, 256, 260, 320, 512, 516, 768, 1020, 1024)
LN_ROWS = (1, 15, 16, 17, 77)
LN_LONG = [(32768 + 17, 4), (32768 + 17, 8), (2 * 32768 + 3, 4), (2 * 32768 + 3, 8)]


def bn_cases():
    """(m, c, family, relu, with_residual): every shape in every family, the four (relu, residual) combinations in turn."""
    out = []
    for fi, family in enumerate(FAMILIES[:4]):
        for si, (m, c) in enumerate(BN_SHAPES):
            relu, res = BN_COMBOS[(si + fi) % 4]
            out.append((m, c, family, relu and family != "offset", res))
    return out


# ---- input families -------------------------------------------------------------------------------------------------------------
def _seed(op, family, shape):
    return 7919 * sum((i + 1) * int(s) for i, s in enumerate(shape)) + 31 * FAMILIES.index(family) + len(op)


def _family_x(family, shape, set_shape, const_index, gen):
    """x of `shape` (float32, CPU) and the per-set factor (or None); `set_shape` broadcasts over the statistics sets,
    `const_index` indexes the set that the constant family overwrites."""
    x = torch.randn(shape, generator=gen) * 2 + 0.3
    factor = None
    if family == "offset":
        x = 1000 + 0.01 * torch.randn(shape, generator=gen)
    elif family == "scales":
        factor = torch.exp(torch.empty(set_shape, dtype=torch.float64).uniform_(math.log(1e-4), math.log(1e4), generator=gen)).float()
        x = x * factor
    elif family == "constant":
        x[const_index] = 3.0
    return x, factor


def _family_dy(family, shape, gen):
    return log_uniform_signed(shape, 1e-3, 1e3, gen) if family == "scales" else torch.randn(shape, generator=gen)


def _affine(c, gen):
    return torch.randn(c, generator=gen) * 0.5 + 1, torch.randn(c, generator=gen) * 0.3


def bn_problem(m, c, family, with_res):
    """CPU float32 tensors of a BatchNorm case: x, residual (or None), w, b, running_mean, running_var, dy."""
    gen = torch.Generator().manual_seed(_seed("bn", family, (m, c)))
    ch = c // 2
    x, _ = _family_x(family, (m, c), (1, c), (slice(None), ch), gen)
    w, b = _affine(c, gen)
    if family == "constant":
        b[ch] = 2.0
    return dict(x=x, residual=torch.randn(m, c, generator=gen) if with_res else None, w=w, b=b,
                running_mean=torch.randn(c, generator=gen) * 0.2, running_var=torch.rand(c, generator=gen) + 0.5,
                dy=_family_dy(family, (m, c), gen))


def gn_problem(shape, family):
    """CPU float32 tensors of a GroupNorm case: x [B, rows, C], w, b, dy."""
    bsz, rows, c, groups = shape
    cpg = c // groups
    gen = torch.Generator().manual_seed(_seed("gn", family, shape))
    x, _ = _family_x(family, (bsz, rows, groups, cpg), (bsz, 1, groups, 1), (bsz - 1, slice(None), groups // 2), gen)
    w, b = _affine(c, gen)
    return dict(x=x.reshape(bsz, rows, c), w=w, b=b, dy=_family_dy(family, (bsz, rows, c), gen))


def ln_problem(rows, c, family, with_res):
    """CPU float32 tensors of a LayerNorm case: x [rows, C], residual (or None), w, b, dy.  The residual follows the family (the
    statistics are those of x + residual): 0.01 N(0, 1) on the offset, the row's factor on the scales, 0.5 in the constant row."""
    gen = torch.Generator().manual_seed(_seed("ln", family, (rows, c)))
    row = rows // 2
    x, factor = _family_x(family, (rows, c), (rows, 1), row if rows else slice(0, 0), gen)
    w, b = _affine(c, gen)
    r = None
    if with_res:
        r = torch.randn(rows, c, generator=gen)
        if family == "offset":
            r = r * 0.01
        elif family == "scales":
            r = r * factor
        elif family == "constant" and rows:
            r[row] = 0.5
    return dict(x=x, residual=r, w=w, b=b, dy=_family_dy(family, (rows, c), gen))


def transposed(t):
    """The same values as a transposed view of a contiguous tensor (last two axes)."""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


# ---- references and the comparison ------------------------------------------------------------------------------------------------
def bn_reference(p, relu, device, dy_ones=False):
    t = {k: (v.to(device) if v is not None else None) for k, v in p.items()}
    return batchnorm_fp64(t["x"], t["residual"], t["w"], t["b"], t["running_mean"], t["running_var"], BN_MOMENTUM, BN_EPS, relu,
                          torch.ones_like(t["x"]) if dy_ones else t["dy"])


def gn_reference(p, groups, device, dy_ones=False):
    t = {k: v.to(device) for k, v in p.items()}
    return groupnorm_fp64(t["x"], t["w"], t["b"], groups, GN_EPS, torch.ones_like(t["x"]) if dy_ones else t["dy"])


def ln_reference(p, device, dy_ones=False):
    t = {k: (v.to(device) if v is not None else None) for k, v in p.items()}
    return add_layernorm_fp64(t["x"], t["residual"], t["w"], t["b"], LN_EPS, torch.ones_like(t["x"]) if dy_ones else t["dy"])


def ratios(got, ref):
    """err / bound at c = 1 of every output in `got` (a dict of tensors) against the reference dict -- what
    assert_elementwise computes, as a figure; dx and dresidual without the ReLU ties."""
    out = {}
    for k, g in got.items():
        r, mag, cond = ref[k], ref[k + "_mag"], ref[k + "_cond"]
        if r.numel() == 0:
            out[k] = 0.0
            continue
        n = torch.as_tensor(ref[k + "_n"], dtype=torch.float64).clamp_min(1.0)
        ratio = (g.detach().to(r.device, torch.float64) - r).abs() / (torch.sqrt(n) * U32 * mag + cond + 1e-30)
        if k in ("dx", "dresidual"):
            ratio = ratio[~ref["near_zero"]]
        out[k] = float(ratio.max()) if ratio.numel() else 0.0
    return out


def check(name, got, ref, consts):
    """assert_elementwise on every output of `got` with the constants of its family; the share of ReLU ties under its cap.
    Returns the err / bound figures at c = 1."""
    assert ref["near_zero_share"] <= NEAR_ZERO_CAP, "%s: %.3g of the elements are ReLU ties" % (name, ref["near_zero_share"])
    fig = ratios(got, ref)
    print("%s: err / bound at c = 1: %s" % (name, "  ".join("%s %.3g" % kv for kv in fig.items())))
    for k, g in got.items():
        r, mag, cond = ref[k], ref[k + "_mag"], ref[k + "_cond"]
        assert g.shape == r.shape, "%s %s: shape %s vs %s" % (name, k, tuple(g.shape), tuple(r.shape))
        if r.numel() == 0:
            continue
        if k in ("dx", "dresidual") and bool(ref["near_zero"].any()):
            keep = ~ref["near_zero"]
            g, r, mag, cond = g.detach().to(r.device)[keep], r[keep], mag[keep], cond[keep]
        assert_elementwise("%s %s" % (name, k), g, r, mag, ref[k + "_n"], consts[k], geo64=cond)
    return fig


# ---- the kernels --------------------------------------------------------------------------------------------------------------
def _bn_module(p, dev, cls=torch.nn.BatchNorm1d):
    bn = cls(p["w"].numel(), eps=BN_EPS, momentum=BN_MOMENTUM).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(p["w"])
        bn.bias.copy_(p["b"])
        bn.running_mean.copy_(p["running_mean"])
        bn.running_var.copy_(p["running_var"])
    return bn


def run_bn_kernel(p, relu, dev, strided=False):
    from efg_amd.operators.batchnorm import bn_act, fusable

    bn = _bn_module(p, dev)
    x = p["x"].to(dev)
    x = (transposed(x) if strided else x).requires_grad_(True)
    r = p["residual"].to(dev).requires_grad_(True) if p["residual"] is not None else None
    assert fusable(bn, x)
    y = bn_act(x, bn, relu=relu, residual=r)
    if strided:
        assert not x.is_contiguous()
        y.sum().backward()
    else:
        y.backward(p["dy"].to(dev))
    assert int(bn.num_batches_tracked) == 1
    got = dict(y=y.detach(), dx=x.grad, dweight=bn.weight.grad, dbias=bn.bias.grad, running_mean=bn.running_mean.clone(),
               running_var=bn.running_var.clone())
    if r is not None:
        got["dresidual"] = r.grad
    return got


def run_gn_kernel(p, groups, dev, strided=False):
    from efg_amd.operators.groupnorm import group_norm_nhwc

    c = p["w"].numel()
    gn = torch.nn.GroupNorm(groups, c, eps=GN_EPS).to(dev)
    with torch.no_grad():
        gn.weight.copy_(p["w"])
        gn.bias.copy_(p["b"])
    x = p["x"].to(dev)
    x = (transposed(x) if strided else x).requires_grad_(True)
    y = group_norm_nhwc(x, gn)
    if strided:
        assert not x.is_contiguous() or x.shape[1] == 1
        y.sum().backward()
    else:
        y.backward(p["dy"].to(dev))
    return dict(y=y.detach(), dx=x.grad, dweight=gn.weight.grad, dbias=gn.bias.grad)


def run_ln_kernel(p, dev, strided=False):
    from efg_amd.operators.layernorm import add_layer_norm

    c = p["w"].numel()
    norm = torch.nn.LayerNorm(c, eps=LN_EPS).to(dev)
    with torch.no_grad():
        norm.weight.copy_(p["w"])
        norm.bias.copy_(p["b"])
    x = p["x"].to(dev)
    x = (transposed(x) if strided else x).requires_grad_(True)
    r = p["residual"].to(dev).requires_grad_(True) if p["residual"] is not None else None
    y = add_layer_norm(x, r, norm)
    if strided:
        y.sum().backward()
    else:
        y.backward(p["dy"].to(dev))
    got = dict(y=y.detach(), dx=x.grad, dweight=norm.weight.grad, dbias=norm.bias.grad)
    if r is not None:
        got["dresidual"] = r.grad
    return got


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c,family,relu,with_res", bn_cases())
def test_bn_act_elementwise(dev, m, c, family, relu, with_res):
    p = bn_problem(m, c, family, with_res)
    ref = bn_reference(p, relu, dev)
    check("bn %s [%d, %d] relu=%d res=%d" % (family, m, c, relu, with_res), run_bn_kernel(p, relu, dev), ref, C_BN[family])


@pytest.mark.parametrize("m,c,relu,with_res", [(2079, 516, True, True), (33, 96, False, False)])
def test_bn_act_strided_input_and_expanded_dy(dev, m, c, relu, with_res):
    p = bn_problem(m, c, "strided", with_res)
    ref = bn_reference(p, relu, dev, dy_ones=True)
    check("bn strided [%d, %d]" % (m, c), run_bn_kernel(p, relu, dev, strided=True), ref, C_BN["strided"])


@pytest.mark.parametrize("relu", [True, False])
def test_bn_act_nhwc_elementwise(dev, relu):
    """BatchNorm2d over a channels-last [2, 8, 5, 7] map through bn_act_nhwc: the [70, 8] row problem."""
    from efg_amd.operators.batchnorm import bn_act_nhwc, fusable_nhwc

    bsz, c, h, w = BN_NHWC_SHAPE
    p = bn_problem(bsz * h * w, c, "plain", False)
    ref = bn_reference(p, relu, dev)
    bn = _bn_module(p, dev, torch.nn.BatchNorm2d)
    nchw = lambda t: t.to(dev).view(bsz, h, w, c).permute(0, 3, 1, 2)   # noqa: E731
    x = nchw(p["x"]).requires_grad_(True)
    assert fusable_nhwc(bn, x)
    y = bn_act_nhwc(x, bn, relu=relu)
    assert y.shape == x.shape and y.is_contiguous(memory_format=torch.channels_last)
    y.backward(nchw(p["dy"]))
    assert int(bn.num_batches_tracked) == 1
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, c)   # noqa: E731
    got = dict(y=rows(y.detach()), dx=rows(x.grad), dweight=bn.weight.grad, dbias=bn.bias.grad,
               running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone())
    check("bn nhwc relu=%d" % relu, got, ref, C_BN["plain"])


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES[:4])
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_group_norm_elementwise(dev, shape, family):
    p = gn_problem(shape, family)
    ref = gn_reference(p, shape[3], dev)
    check("gn %s %s" % (family, shape), run_gn_kernel(p, shape[3], dev), ref, C_GN[family])


@pytest.mark.parametrize("shape", [(3, 33, 16, 4), (2, 40, 516, 3)])
def test_group_norm_strided_input_and_expanded_dy(dev, shape):
    p = gn_problem(shape, "strided")
    ref = gn_reference(p, shape[3], dev, dy_ones=True)
    check("gn strided %s" % (shape,), run_gn_kernel(p, shape[3], dev, strided=True), ref, C_GN["strided"])


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
def _ln_case(dev, rows, c, family, with_res, strided=False):
    p = ln_problem(rows, c, family, with_res)
    ref = ln_reference(p, dev, dy_ones=strided)
    got = run_ln_kernel(p, dev, strided=strided)
    fig = check("ln %s [%d, %d] res=%d" % (family, rows, c, with_res), got, ref, C_LN[family])
    if with_res:
        assert torch.equal(got["dresidual"], got["dx"]), "d residual and dx are the same gradient"
    return fig


@pytest.mark.parametrize("family", FAMILIES[:4])
@pytest.mark.parametrize("c", LN_CS)
def test_add_layer_norm_elementwise(dev, c, family):
    for rows in LN_ROWS:
        for with_res in (True, False):
            _ln_case(dev, rows, c, family, with_res)


@pytest.mark.parametrize("family", FAMILIES[:4])
@pytest.mark.parametrize("rows,c", LN_LONG)
def test_add_layer_norm_backward_grid_stride_trips(dev, rows, c, family):
    """More than 2048 x 16 rows: the backward's workgroups take a second (and third) group of rows; dgamma / dbeta, summed
    over all of them, are compared per channel with n = rows."""
    for with_res in (True, False):
        _ln_case(dev, rows, c, family, with_res)


@pytest.mark.parametrize("rows,c", [(77, 260), (17, 1020), (16, 36)])
def test_add_layer_norm_strided_input_and_expanded_dy(dev, rows, c):
    _ln_case(dev, rows, c, "strided", True, strided=True)
    _ln_case(dev, rows, c, "strided", False, strided=True)


@pytest.mark.parametrize("with_res", [True, False])
def test_add_layer_norm_no_rows(dev, with_res):
    p = ln_problem(0, 256, "plain", with_res)
    got = run_ln_kernel(p, dev)
    assert got["y"].shape == (0, 256) and got["dx"].shape == (0, 256)
    assert bool((got["dweight"] == 0).all()) and bool((got["dbias"] == 0).all())
    if with_res:
        assert got["dresidual"].shape == (0, 256)


# ---- determinism: fixed-order reductions, so two runs agree bit for bit ---------------------------------------------------------
def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k + " differs between two runs"


def test_bn_act_is_deterministic(dev):
    p = bn_problem(40000, 96, "plain", True)
    _same_bits(run_bn_kernel(p, True, dev), run_bn_kernel(p, True, dev))


def test_group_norm_is_deterministic(dev):
    p = gn_problem((2, 2079, 64, 16), "plain")
    _same_bits(run_gn_kernel(p, 16, dev), run_gn_kernel(p, 16, dev))


def test_add_layer_norm_is_deterministic(dev):
    p = ln_problem(2 * 32768 + 3, 8, "plain", True)
    _same_bits(run_ln_kernel(p, dev), run_ln_kernel(p, dev))
