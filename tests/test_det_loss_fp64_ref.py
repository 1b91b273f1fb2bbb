"""CPU pins of the detection-loss references of tests/fp64_ref.py (match_cost_fp64, focal_fp64, box_loss_fp64), and the place
where the constants of tests/test_det_loss_fp64_gpu.py are fixed.

1. The references equal the project's PyTorch composites evaluated in float64 (HungarianMatcher3d.cost_matrices,
   sigmoid_focal_loss, paired_box3d_giou + l1_loss, with their autograd gradients) to 1e-12 of their terms, on random inputs
   and on the dyadic grid; |value| <= mag everywhere.
2. For every input family of the GPU tests the SAME composites in fp32 -- what the kernels replace -- are held against the
   references on the CPU.  The worst err / bound at c = 1 of each family is printed and recorded in the docstrings below; the
   GPU tests use c = min(16, 4 x that) (a kernel may be no worse than 4 x the composite it replaces), and the tests here assert
   that the composite passes at that c, so every bar is known to be attainable before a GPU is involved.  One exception,
   explained at the focal test: ATen's BCE-with-logits cancels, so the focal constant comes from the same definition written
   without that cancellation."""
import pytest
import torch
import torch.nn.functional as F

from fp64_ref import U32, assert_elementwise, box_loss_fp64, focal_fp64, focal_terms, match_cost_fp64
from test_det_loss_fp64_gpu import (BOX_CASES, C_ASSEMBLY, C_BOX, C_COST, C_FOCAL, COST_SHAPES, FOCAL_SHAPES, TOL_ASSEMBLY,
                                    WEIGHTS, box_problem, check_det3d, cost_problem, det3d_inputs, focal_problem, run_det3d)

CPU = torch.device("cpu")
F64_COND = 2.0 ** -29      # float64's unit roundoff over float32's: the conditioning allowance of a float64 evaluation


def _ratio(got, ref, mag, n, cond):
    """Worst |got - ref| / (sqrt(n) * 2^-24 * mag + cond) -- assert_elementwise's err / bound at c = 1."""
    if ref.numel() == 0:
        return 0.0
    n = torch.as_tensor(n, dtype=torch.float64).clamp_min(1.0)
    return float(((got.double() - ref).abs() / (torch.sqrt(n) * U32 * mag + cond + 1e-30)).max())


def _same(name, got, ref, mag, cond):
    """Two float64 evaluations of one formula: equal to 1e-12 of the terms (+ the conditioning at float64's roundoff)."""
    assert got.dtype == torch.float64 and got.shape == ref.shape, name
    bad = (got - ref).abs() > 1e-12 * mag + F64_COND * cond + 1e-300
    assert not bool(bad.any()), "%s: %d elements differ, worst %.3g" % (name, int(bad.sum()), float((got - ref).abs().max()))
    assert bool((ref.abs() <= mag * (1 + 1e-12) + F64_COND * cond + 1e-300).all()), name + ": magnitude below |value|"


# ---- the composites (project code, any dtype) -------------------------------------------------------------------------------
def composite_cost(logits, boxes, labels, tgt, dtype, monkeypatch):
    """HungarianMatcher3d.cost_matrices layer by layer -> [L * B, Q, G].  The method casts to fp32 with .float(); for the
    float64 evaluation that cast is patched to .double() for the duration of the call."""
    from efg_amd.detection3d.matcher import HungarianMatcher3d

    matcher = HungarianMatcher3d(*WEIGHTS)
    with monkeypatch.context() as m:
        if dtype == torch.float64:
            m.setattr(torch.Tensor, "float", lambda self: self.double())
        targets = [{"labels": labels[s], "gt_boxes": tgt[s].to(dtype)} for s in range(labels.shape[0])]
        mats = []
        for layer in range(logits.shape[0]):
            mats += matcher.cost_matrices({"pred_logits": logits[layer].to(dtype), "pred_boxes": boxes[layer].to(dtype)}, targets)
    assert all(m.dtype == dtype for m in mats)
    return torch.stack(mats)


def composite_focal(logits, tcls, denom, alpha, gamma, grad_out, dtype):
    from efg_amd.detection3d.utils import sigmoid_focal_loss

    x = logits.detach().to(dtype).requires_grad_(True)
    c = x.shape[-1]
    onehot = F.one_hot(tcls.long().clamp(min=0), c).to(dtype) * (tcls >= 0)[..., None]
    out = sigmoid_focal_loss(x, onehot, alpha=alpha, gamma=gamma, reduction="none").sum(dim=(1, 2)) / denom
    out.backward(grad_out.to(dtype))
    return out.detach(), x.grad


def composite_box(boxes, tgt, idx, denom, grad_out, dtype):
    from efg_amd.detection3d.utils import box_cxcyczlwh_to_xyxyxy, paired_box3d_giou

    bx = boxes.detach().to(dtype).requires_grad_(True)
    ok = idx[2] >= 0
    li, bi, qi, gi = (t[ok] for t in idx)
    src, t = bx[li, bi, qi], tgt.to(dtype)[bi, gi]
    l1 = F.l1_loss(src, t, reduction="none")
    giou = 1 - paired_box3d_giou(box_cxcyczlwh_to_xyxyxy(src[:, :6]), box_cxcyczlwh_to_xyxyxy(t[:, :6]))
    per = torch.stack((l1[:, :6].sum(1), giou, l1[:, 6:].sum(1)), dim=1)
    out = per.new_zeros(bx.shape[0], 3).index_add_(0, li, per) / denom
    out.backward(grad_out.to(dtype))
    return out.detach(), bx.grad


# ---- matching cost --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logit_family", ["normal", "uniform12"])
@pytest.mark.parametrize("box_family", ["random", "dyadic", "padded"])
def test_match_cost_reference_and_the_fp32_composite(monkeypatch, box_family, logit_family):
    """match_cost_fp64 == cost_matrices in float64 on every shape of the GPU test, and the fp32 cost_matrices inside the bar.
    Worst err / bound at c = 1 of the fp32 composite over the five shapes (CPU):
        random  normal 3.17   uniform12 3.14        dyadic  normal 1.10   uniform12 1.05        padded  normal 3.17   uniform12 3.14
    """
    worst = 0.0
    for shape in COST_SHAPES:
        logits, boxes, labels, tgt = cost_problem(shape, box_family, logit_family, CPU)
        ref = match_cost_fp64(logits, boxes, labels, tgt, *WEIGHTS)
        assert ref["cost"].dtype == torch.float64 and bool(torch.isfinite(ref["cost"]).all())
        assert bool((ref["cost_cond"] >= 0).all()) and bool(torch.isfinite(ref["cost_cond"]).all())
        _same("cost %s" % (shape,), composite_cost(logits, boxes, labels, tgt, torch.float64, monkeypatch), ref["cost"],
              ref["cost_mag"], ref["cost_cond"])
        got = composite_cost(logits, boxes, labels, tgt, torch.float32, monkeypatch)
        worst = max(worst, _ratio(got, ref["cost"], ref["cost_mag"], 1, ref["cost_cond"]))
        assert_elementwise("fp32 composite cost %s" % (shape,), got, ref["cost"], ref["cost_mag"], 1,
                           C_COST[box_family, logit_family], geo64=ref["cost_cond"])
    print("match cost %s %s: fp32 composite err / bound at c = 1: %.3g" % (box_family, logit_family, worst))
    assert C_COST[box_family, logit_family] <= 16


def test_match_cost_dyadic_grid_holds_every_relation():
    """The dyadic family really contains identical, nested, face-touching and disjoint (prediction, target) pairs."""
    _, boxes, _, tgt = cost_problem((3, 2, 300, 3, 17), "dyadic", "normal", CPU)
    b, t = boxes.double()[:, :, :, None], tgt.double()[None, :, None]
    gap = (b[..., :3] - t[..., :3]).abs() - 0.5 * (b[..., 3:6] + t[..., 3:6])        # < 0 overlap, == 0 touching, > 0 apart
    assert bool((b[..., :6] == t[..., :6]).all(-1).any())
    assert bool((((b[..., :3] - t[..., :3]).abs() + 0.5 * b[..., 3:6] < 0.5 * t[..., 3:6]).all(-1)).any())          # nested
    assert bool(((gap == 0).sum(-1) == 1)[(gap <= 0).all(-1)].any())                                               # one face
    assert bool((gap > 0).any(-1).any())


# ---- focal loss -----------------------------------------------------------------------------------------------------------
def formula_focal(logits, tcls, denom, alpha, gamma, grad_out, dtype):
    """The definition as the reference writes it (ce = max(x, 0) - x t + log1p(exp(-|x|)): no cancellation) in `dtype`, plain
    torch + autograd."""
    x = logits.detach().to(dtype).requires_grad_(True)
    hit = tcls[..., None].long() == torch.arange(x.shape[-1])
    p = torch.sigmoid(x)
    out = focal_terms(x, hit, alpha, gamma, p, 1 - p)[0].sum(dim=(1, 2)) / denom
    out.backward(grad_out.to(dtype))
    return out.detach(), x.grad


def bce_cancellation(logits, tcls, denom, alpha, gamma, grad_out):
    """What F.binary_cross_entropy_with_logits adds to the composite's error, per 2^-24: ATen evaluates ce as (1 - t) x -
    logsigmoid(x), two terms of size |x| for a result that may be tiny, and the loss and (through the saved ce) its gradient
    inherit (|(1 - t) x| + |logsigmoid(x)|) * |d . / d ce|.  Returns (per-layer sums, per gradient element), float64."""
    x = logits.double()
    hit = tcls[..., None].long() == torch.arange(x.shape[-1])
    p = torch.sigmoid(x)
    d_loss, _, d_grad = focal_terms(x, hit, alpha, gamma, p, 1 - p)
    ce = focal_terms(x, hit, -1.0, 0.0, p, 1 - p)[0]                      # alpha < 0, gamma = 0: ce itself
    size = (x * (~hit)).abs() + F.logsigmoid(x).abs()
    go = (grad_out.double() / denom).abs().view(-1, 1, 1)
    return (size * d_loss / ce).sum((1, 2)) / denom, size * d_grad.abs() / ce * go


def _focal_pin(shape, logit_family, pattern, alpha, gamma):
    logits, tcls, grad_out = focal_problem(shape, logit_family, pattern, CPU)
    denom = 37.0
    ref = focal_fp64(logits, tcls, denom, alpha, gamma, grad_out)
    bce_sum, bce_grad = bce_cancellation(logits, tcls, denom, alpha, gamma, grad_out)
    out64, g64 = composite_focal(logits, tcls, denom, alpha, gamma, grad_out, torch.float64)
    _same("focal sums", out64, ref["loss"], ref["loss_mag"], ref["loss_cond"] + 4 * U32 * bce_sum)
    _same("focal grad", g64, ref["grad"], ref["grad_mag"], ref["grad_cond"] + 4 * U32 * bce_grad)
    _same("focal grad, closed form", ref["grad_formula"], ref["grad"], ref["grad_mag"], ref["grad_cond"])
    c = C_FOCAL[logit_family if logit_family != "normal3" else "normal"]
    # the fp32 yardstick: the definition in its cancellation-free form, plain torch
    out32, g32 = formula_focal(logits, tcls, denom, alpha, gamma, grad_out, torch.float32)
    r = _ratio(out32, ref["loss"], ref["loss_mag"], ref["loss_n"], ref["loss_cond"])
    rg = _ratio(g32, ref["grad"], ref["grad_mag"], 1, ref["grad_cond"])
    assert_elementwise("fp32 formula focal sums", out32, ref["loss"], ref["loss_mag"], ref["loss_n"], c, geo64=ref["loss_cond"])
    if g32.numel():
        assert_elementwise("fp32 formula focal grad", g32, ref["grad"], ref["grad_mag"], 1, c, geo64=ref["grad_cond"])
    # the fp32 composite: the same bar + its BCE's own cancellation
    o32, c32 = composite_focal(logits, tcls, denom, alpha, gamma, grad_out, torch.float32)
    rc = _ratio(o32, ref["loss"], ref["loss_mag"], ref["loss_n"], ref["loss_cond"])
    rcg = _ratio(c32, ref["grad"], ref["grad_mag"], 1, ref["grad_cond"])
    assert_elementwise("fp32 composite focal sums", o32, ref["loss"], ref["loss_mag"], ref["loss_n"], c,
                       geo64=ref["loss_cond"] + 4 * U32 * bce_sum)
    if c32.numel():
        assert_elementwise("fp32 composite focal grad", c32, ref["grad"], ref["grad_mag"], 1, c, geo64=ref["grad_cond"] + 4 * U32 * bce_grad)
    return (r, rg, rc, rcg), ref, g32


@pytest.mark.parametrize("logit_family", ["normal3", "uniform30"])
def test_focal_reference_and_the_fp32_composite(logit_family):
    """focal_fp64 == sigmoid_focal_loss + autograd in float64 on every shape and target pattern of the GPU test (and
    alpha = -1, gamma = 1.5 on two), up to the cancellation of ATen's BCE-with-logits (`bce_cancellation`).

    The fp32 composite cannot set the gradient's bar: its ce = (1 - t) x - logsigmoid(x) cancels (a background element at
    x = -4 has ce 217 x 2^-24 off), an error of that formulation and not of the definition, and it misses the per-element bar at
    the cap c = 16 (err / bound 1.5 and 3.0 on the smallest shape).  It is held to the bar + 4 x that cancellation, and the
    constant comes from the definition in its cancellation-free form (what focal_elem evaluates), in fp32 with plain torch
    (`formula_focal`).  Worst err / bound at c = 1 (CPU), sums / gradient elements:
        fp32 formula    normal3 0.24 / 2.7      uniform30 0.19 / 3.1
        fp32 composite  normal3 0.21 / 5.6      uniform30 0.19 / 4.5     (without the BCE allowance)"""
    worst = [0.0] * 4
    cases = [(s, p, 0.25, 2.0) for s in FOCAL_SHAPES for p in ("sparse", "mixed")]
    if logit_family == "normal3":
        cases += [((2, 7, 4), "sparse", -1.0, 1.5), ((3, 5462, 3), "sparse", -1.0, 1.5)]
    for shape, pattern, alpha, gamma in cases:
        r, _, _ = _focal_pin(shape, logit_family, pattern, alpha, gamma)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print("focal %s: err / bound at c = 1: fp32 formula sums %.3g, gradient %.3g; fp32 composite sums %.3g, gradient %.3g"
          % (logit_family, *worst))


def test_focal_bar_catches_a_small_gradient_element_off_by_1e_4():
    """One well-conditioned gradient element of the smallest magnitude, scaled by 1 + 1e-4, fails at the cap c = 16."""
    _, ref, g32 = _focal_pin((3, 5462, 3), "normal3", "sparse", 0.25, 2.0)
    well = (ref["grad_cond"] < 1e-6 * ref["grad"].abs()) & (ref["grad"] != 0)
    flat = torch.where(well, ref["grad"].abs(), torch.full_like(ref["grad"], float("inf"))).reshape(-1)
    i = int(torch.argmin(flat))
    print("smallest well-conditioned element: %.3g of the largest" % (float(flat[i]) / float(ref["grad"].abs().max())))
    assert float(flat[i]) < 1e-3 * float(ref["grad"].abs().max())
    bad = g32.clone()
    bad.view(-1)[i] *= 1 + 1e-4
    with pytest.raises(AssertionError, match="1 of"):
        assert_elementwise("scaled element", bad, ref["grad"], ref["grad_mag"], 1, 16, geo64=ref["grad_cond"])


# ---- box loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["random", "dyadic"])
def test_box_loss_reference_and_the_fp32_composite(family):
    """box_loss_fp64 == l1_loss + paired_box3d_giou + autograd in float64 on every case of the GPU test (ties of the dyadic
    grid included: both are autograd), and the fp32 composite inside the bar.  Worst err / bound at c = 1 of the fp32
    composite (CPU), sums / gradient elements:
        random 0.41 / 4.78        dyadic 0.17 / 1.05
    """
    worst = [0.0, 0.0]
    for case in BOX_CASES:
        boxes, tgt, idx, grad_out = box_problem(case, family, CPU)
        denom = 11.0
        ref = box_loss_fp64(boxes, tgt, *idx, denom, grad_out)
        out64, g64 = composite_box(boxes, tgt, idx, denom, grad_out, torch.float64)
        _same("box sums", out64, ref["loss"], ref["loss_mag"], ref["loss_cond"])
        _same("box grad", g64, ref["grad"], ref["grad_mag"], ref["grad_cond"])
        assert int(ref["rows"].sum()) == int((idx[2] >= 0).sum()) and bool((ref["grad"][~ref["rows"]] == 0).all())
        out32, g32 = composite_box(boxes, tgt, idx, denom, grad_out, torch.float32)
        rows = ref["rows"]
        worst[0] = max(worst[0], _ratio(out32, ref["loss"], ref["loss_mag"], ref["loss_n"], ref["loss_cond"]))
        worst[1] = max(worst[1], _ratio(g32[rows], ref["grad"][rows], ref["grad_mag"][rows], 1, ref["grad_cond"][rows]))
        assert_elementwise("fp32 composite box sums", out32, ref["loss"], ref["loss_mag"], ref["loss_n"], C_BOX[family],
                           geo64=ref["loss_cond"])
        assert_elementwise("fp32 composite box grad", g32[rows], ref["grad"][rows], ref["grad_mag"][rows], 1, C_BOX[family],
                           geo64=ref["grad_cond"][rows])
        assert bool((g32[~rows] == 0).all())
    print("box loss %s: fp32 composite err / bound at c = 1: sums %.3g, gradient %.3g" % (family, *worst))


def test_box_loss_face_touching_pair_takes_autograds_gradient():
    """Two boxes of side 0.5 at (0.25, 0.5, 0.5) and (0.75, 0.625, 0.5) touch exactly on an x face: clamp(min=0) passes the
    gradient at 0, so d (1 - GIoU) / d (centre x of the first) is -0.95; treating the touching side as separated gives -0.80."""
    boxes = torch.tensor([0.25, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0]).view(1, 1, 1, 7)
    tgt = torch.tensor([0.75, 0.625, 0.5, 0.5, 0.5, 0.5, 0.0]).view(1, 1, 7)
    z = torch.zeros(1, dtype=torch.int64)
    ref = box_loss_fp64(boxes, tgt, z, z, z, z, 1.0, torch.tensor([[0.0, 1.0, 0.0]]))
    assert abs(float(ref["grad"][0, 0, 0, 0]) + 0.95) < 1e-12
    boxes, tgt, idx, _ = box_problem("pairs102", "dyadic", CPU)
    li, bi, qi, gi = idx
    hit = (boxes[li, bi, qi.clamp(min=0)] == torch.tensor([0.25, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5])).all(-1) & (qi >= 0)
    assert int(hit.sum()) == 1 and bool((tgt[bi[hit], gi[hit], :6] == torch.tensor([0.75, 0.625, 0.5, 0.5, 0.5, 0.5])).all())


def test_box_bar_catches_a_small_gradient_element_off_by_1e_4():
    boxes, tgt, idx, grad_out = box_problem("pairs3000", "random", CPU)
    ref = box_loss_fp64(boxes, tgt, *idx, 11.0, grad_out)
    _, g32 = composite_box(boxes, tgt, idx, 11.0, grad_out, torch.float32)
    well = (ref["grad_cond"] < 1e-6 * ref["grad"].abs()) & (ref["grad"] != 0)
    flat = torch.where(well, ref["grad"].abs(), torch.full_like(ref["grad"], float("inf"))).reshape(-1)
    i = int(torch.argmin(flat))
    assert float(flat[i]) < 1e-2 * float(ref["grad"].abs().max())
    bad = g32.clone()
    bad.view(-1)[i] *= 1 + 1e-4
    with pytest.raises(AssertionError, match="1 of"):
        assert_elementwise("scaled element", bad, ref["grad"], ref["grad_mag"], 1, 16, geo64=ref["grad_cond"])


# ---- the assembly ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["dn", "topk"])
def test_det3d_loss_fp32_module_against_the_float64_module(route):
    """Det3DLoss (composite path) in fp32 against itself in float64 on the inputs of the GPU assembly test, one assignment.
    Measured (CPU), dn / topk: terms at most 0.42 / 0.25 of sqrt(n) * 2^-24 * |ref|; gradients at most 5.0e-7 / 4.0e-7 of max |ref|
    of their tensor.  The GPU test uses 4 x the larger: c = 1.7, tol = 2.0e-6."""
    inp = det3d_inputs(route)
    ref = run_det3d(inp, CPU, torch.float64)
    got = run_det3d(inp, CPU, torch.float32, q_of_g=ref[2])
    keys = sorted(ref[0])
    if route == "dn":
        assert len(keys) == 24 and "loss_ce_dn_1" in keys and "loss_giou_0" in keys and "loss_rad_dn" in keys
    else:
        assert keys == ["loss_bbox", "loss_ce", "loss_giou", "loss_rad"]
    assert all(float(v) > 0 for v in ref[0].values())
    wt, wg = check_det3d(got, ref, C_ASSEMBLY, TOL_ASSEMBLY)
    print("Det3DLoss %s: fp32 module terms %.3g of the unit bar, gradients %.3g of max |ref|" % (route, wt, wg))
