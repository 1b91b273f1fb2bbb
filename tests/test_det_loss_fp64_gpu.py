"""GPU: the detection-loss and matching kernels (csrc/det_loss.hip, csrc/matcher.hip) against the float64 references of
tests/fp64_ref.py, element by element: |got - ref| <= c * sqrt(n) * 2^-24 * |terms| + cond, where `cond` is the reference's own
first-order conditioning allowance (fp64_ref.py) and the constants c come from tests/test_det_loss_fp64_ref.py: there the
fp32 PyTorch composite that the kernels replace is measured against the same references on the same inputs on the CPU, and
c = min(16, 4 x its worst err / bound at c = 1) per input family (focal loss: the fp32 evaluation of the definition in its
cancellation-free form, because ATen's BCE-with-logits cancels; see there).

The input families below are device-agnostic (built from CPU generators) so that the CPU pins see the same numbers."""
import math

import numpy as np
import pytest
import torch

from fp64_ref import U32, assert_elementwise, box_loss_fp64, focal_fp64, match_cost_fp64

pytestmark = pytest.mark.gpu

WEIGHTS = (1.0, 4.0, 2.0, 4.0)     # w_class, w_bbox, w_giou, w_rad (the model's matcher)

# ---- constants of the bars: min(16, 4 x the fp32 yardstick's worst err / bound at c = 1), tests/test_det_loss_fp64_ref.py ------
C_COST = {("random", "normal"): 12.7, ("random", "uniform12"): 12.6, ("dyadic", "normal"): 4.4, ("dyadic", "uniform12"): 4.2,
          ("padded", "normal"): 12.7, ("padded", "uniform12"): 12.6}
C_FOCAL = {"normal": 10.8, "uniform30": 12.5}          # forward sums and gradient elements alike
C_BOX = {"random": 16.0, "dyadic": 4.2}                # (random: 4 x 4.8 is past the cap)
C_ASSEMBLY, TOL_ASSEMBLY = 1.7, 2.0e-6                 # 4 x 0.42 of the unit bar; 4 x 5.0e-7 of max |ref|

COST_SHAPES = [(3, 2, 300, 3, 17), (1, 1, 1, 1, 1), (2, 3, 257, 3, 1), (1, 2, 5, 4, 33), (2, 2, 1000, 1, 64)]
FOCAL_SHAPES = [(2, 7, 4), (2, 5461, 3), (2, 16384, 1), (3, 5462, 3), (1, 70688, 1), (1, 262157, 1), (2, 0, 3)]
BOX_CASES = {"pairs102": (3, 2, 300, 17, (0, 1, 2)), "pairs3000": (2, 1, 2000, 1500, (0, 1)), "empty_layer": (3, 2, 50, 9, (0, 2))}


# ---- input families -----------------------------------------------------------------------------------------------------
def random_boxes(shape, gen):
    """(centre, size, angle) rows: centres and angles uniform in [0, 1), sides in [0.01, 0.2)."""
    boxes = torch.rand(*shape, 7, generator=gen)
    boxes[..., 3:6] = boxes[..., 3:6] * 0.19 + 0.01
    return boxes


def dyadic_boxes(shape, gen):
    """Centres k / 64 (k in 24 .. 40, so the boxes crowd), sides in {1/32, 1/16, 1/8}, angles k / 8: every corner and every
    product of sides is exact in fp32."""
    boxes = torch.empty(*shape, 7)
    boxes[..., :3] = torch.randint(24, 41, (*shape, 3), generator=gen) / 64.0
    boxes[..., 3:6] = 2.0 ** -torch.randint(3, 6, (*shape, 3), generator=gen).float()
    boxes[..., 6] = torch.randint(0, 8, shape, generator=gen) / 8.0
    return boxes


def dyadic_near(tgt, gen):
    """Dyadic boxes around the dyadic boxes `tgt` [..., 7]: each centre coordinate moved by d / 64, d in -8 .. 8 (0 in two
    cases of five), sides drawn anew from {1/32, 1/16, 1/8} (kept in two cases of five): identical, nested, face-touching
    (|d| / 64 == half the sum of the sides), overlapping and disjoint pairs all occur, exactly."""
    shape = tgt.shape[:-1]
    d = torch.randint(-8, 9, (*shape, 3), generator=gen)
    d = torch.where(torch.rand(*shape, 3, generator=gen) < 0.4, torch.zeros_like(d), d)
    out = dyadic_boxes(shape, gen)
    out[..., :3] = tgt[..., :3] + d / 64.0
    keep = torch.rand(*shape, 3, generator=gen) < 0.4
    out[..., 3:6] = torch.where(keep, tgt[..., 3:6], out[..., 3:6])
    return out


def make_logits(family, shape, gen):
    if family == "normal":
        return torch.randn(shape, generator=gen) * 2 - 2
    if family == "normal3":
        return torch.randn(shape, generator=gen) * 3
    bound = {"uniform12": 12.0, "uniform30": 30.0}[family]
    return (torch.rand(shape, generator=gen) * 2 - 1) * bound


def cost_problem(shape, box_family, logit_family, device):
    """logits [L, B, Q, C], boxes [L, B, Q, 7], tgt_labels [B, G], tgt_boxes [B, G, 7] of one family on `device`.
    "padded": random boxes whose last third (rounded up) of target columns are zero boxes with label 0 (losses._pad_targets)."""
    nl, b, q, c, g = shape
    gen = torch.Generator().manual_seed(1000 * sum(shape) + 7 * len(box_family) + len(logit_family))
    logits = make_logits(logit_family, (nl, b, q, c), gen)
    labels = torch.randint(0, c, (b, g), generator=gen)
    if box_family == "dyadic":
        tgt = dyadic_boxes((b, g), gen)
        boxes = dyadic_near(tgt[None, :, torch.arange(q) % g].expand(nl, b, q, 7), gen)
        boxes[:, :, 0] = tgt[:, 0]                                   # an identical pair in every (layer, scene)
    else:
        tgt, boxes = random_boxes((b, g), gen), random_boxes((nl, b, q), gen)
        if box_family == "padded":
            n_pad = (g + 2) // 3
            tgt[:, g - n_pad:] = 0
            labels[:, g - n_pad:] = 0
    return logits.to(device), boxes.to(device), labels.to(device), tgt.to(device)


def focal_problem(shape, logit_family, pattern, device):
    """logits [L, N, C], tcls int32 [L, N] (-1 background), grad_out [L].  pattern "sparse": 5 % foreground rows in every
    layer; "mixed": layer 0 all background, the last layer every row foreground (a single layer: every row), 5 % between."""
    nl, n, c = shape
    gen = torch.Generator().manual_seed(1000 * sum(shape) + len(logit_family) + 3 * len(pattern))
    logits = make_logits(logit_family, shape, gen)
    cls = torch.randint(0, c, (nl, n), generator=gen, dtype=torch.int32)
    fg = torch.rand(nl, n, generator=gen) < 0.05
    if pattern == "mixed":
        fg[0] = False
        fg[-1] = True
    tcls = torch.where(fg, cls, torch.full_like(cls, -1))
    grad_out = torch.randn(nl, generator=gen) + torch.arange(nl) * 0.5
    return logits.to(device), tcls.to(device), grad_out.to(device)


def box_problem(case, family, device):
    """boxes [L, B, Q, 7], tgt_boxes [B, G, 7], pair vectors (l, b, q, g) int64 and grad_out [L, 3].  Every (layer, scene) of the
    case's layers pairs each target with a distinct query; the pair order is shuffled and 5 % of the q entries are -1.  The
    dyadic family puts every matched prediction near its target (`dyadic_near`) and starts with three fixed pairs: an
    identical one, a nested one, and two boxes of side 0.5 that touch exactly on an x face ((0.25, 0.5, 0.5) against
    (0.75, 0.625, 0.5))."""
    nl, b, q, g, layers = BOX_CASES[case]
    gen = torch.Generator().manual_seed(17 * len(case) + len(family))
    tgt = (dyadic_boxes if family == "dyadic" else random_boxes)((b, g), gen)
    boxes = (dyadic_boxes if family == "dyadic" else random_boxes)((nl, b, q), gen)
    li, bi, qi, gi = [], [], [], []
    for layer in layers:
        for scene in range(b):
            li.append(torch.full((g,), layer))
            bi.append(torch.full((g,), scene))
            qi.append(torch.randperm(q, generator=gen)[:g])
            gi.append(torch.arange(g))
    li, bi, qi, gi = (torch.cat(t).long() for t in (li, bi, qi, gi))
    if family == "dyadic":
        if g >= 3:
            tgt[0, 2] = torch.tensor([0.75, 0.625, 0.5, 0.5, 0.5, 0.5, 0.25])
        near = dyadic_near(tgt[bi, gi], gen)
        near[0] = tgt[bi[0], gi[0]]
        if g >= 3:
            near[1, :6] = tgt[bi[1], gi[1], :6] * torch.tensor([1, 1, 1, 0.5, 0.5, 0.5])
            near[2] = torch.tensor([0.25, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
        boxes[li, bi, qi] = near
    order = torch.randperm(li.numel(), generator=gen)
    li, bi, qi, gi = (t[order] for t in (li, bi, qi, gi))
    drop = torch.rand(li.numel(), generator=gen) < 0.05
    drop[-1] = True
    if family == "dyadic" and g >= 3:
        drop &= ~(order < 3)                                        # the three fixed pairs stay
    qi = torch.where(drop, torch.full_like(qi, -1), qi)
    grad_out = torch.randn(nl, 3, generator=gen) + 1.5
    return boxes.to(device), tgt.to(device), [t.to(device) for t in (li, bi, qi, gi)], grad_out.to(device)


def det3d_inputs(route):
    """fp32 CPU inputs of the Det3DLoss assembly test: B = 3 scenes with 5, 0 and 12 boxes, C = 3.  route "dn": L = 3 layers
    (two aux_outputs) of Q = 64 queries plus 2 denoising groups of 12 padded queries; route "topk": the encoder-proposal form,
    one layer of 200 tokens whose 64 proposals carry the boxes (topk_indexes / topk_boxes)."""
    gen = torch.Generator().manual_seed(len(route))
    b, q, c, counts = 3, 64, 3, [5, 0, 12]
    gmax = max(counts)
    labels = torch.zeros(b, gmax, dtype=torch.int64)
    tboxes = torch.zeros(b, gmax, 7)
    for s, n in enumerate(counts):
        labels[s, :n] = torch.randint(0, c, (n,), generator=gen)
        tboxes[s, :n] = random_boxes((n,), gen) + torch.tensor([0, 0, 0, 0.04, 0.04, 0.04, 0])
    leaves = {}

    def layer_set(prefix, n_layers, n_q):
        for i in range(n_layers):
            leaves["%s_logits_%d" % (prefix, i)] = torch.randn(b, n_q, c, generator=gen) * 2 - 2
            bx = random_boxes((b, n_q), gen)
            bx[..., 3:6] += 0.04
            leaves["%s_boxes_%d" % (prefix, i)] = bx

    extra = {}
    if route == "dn":
        layer_set("pred", 3, q)
        layer_set("dn", 3, 24)
    else:
        leaves["pred_logits_0"] = torch.randn(b, 200, c, generator=gen) * 2 - 2
        bx = random_boxes((b, q), gen)
        bx[..., 3:6] += 0.04
        leaves["topk_boxes"] = bx
        extra["topk_indexes"] = torch.stack([torch.randperm(200, generator=gen)[:q] for _ in range(b)])[..., None]
    return dict(labels=labels, boxes=tboxes, counts=counts, leaves=leaves, extra=extra, route=route)


def run_det3d(inp, device, dtype, q_of_g=None):
    """Det3DLoss on `device` in `dtype` over `det3d_inputs`: returns ({key: term}, {leaf name: gradient of sum_k w_k term_k},
    q_of_g, {key: summed elements of the term}).  The assignment is the given one, or this module's own (CPU: scipy)."""
    from efg_amd.detection3d.losses import Det3DLoss, PaddedTargets
    from efg_amd.detection3d.matcher import HungarianMatcher3d

    crit = Det3DLoss(HungarianMatcher3d(*WEIGHTS), {}, ["focal_labels", "boxes"])
    lv = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in inp["leaves"].items()}
    targets = PaddedTargets(inp["labels"].to(device), inp["boxes"].to(device=device, dtype=dtype), inp["counts"])
    dn_meta = None
    if inp["route"] == "dn":
        def stacked(prefix):
            ls = [{"pred_logits": lv["%s_logits_%d" % (prefix, i)], "pred_boxes": lv["%s_boxes_%d" % (prefix, i)]} for i in range(3)]
            return dict(ls[-1], aux_outputs=ls[:-1])
        outputs = stacked("pred")
        dn_meta = {"output_known_lbs_bboxes": stacked("dn"), "num_dn_group": 2, "pad_size": 24}
    else:
        outputs = {"pred_logits": lv["pred_logits_0"], "topk_boxes": lv["topk_boxes"],
                   "topk_indexes": inp["extra"]["topk_indexes"].to(device)}
    pr = crit.prepare(outputs, targets)
    if q_of_g is None:
        q_of_g = crit.matcher.match_layers(pr["m_logits"], pr["m_boxes"], pr["tgt_labels"], pr["tgt_boxes"], pr["counts"])
    out = crit(outputs, targets, dn_meta=dn_meta, prepared=pr, q_of_g=q_of_g.to(device))
    keys = sorted(out)
    total = sum((0.5 + (0.37 * i) % 1.0) * out[k] for i, k in enumerate(keys))
    total.backward()
    n_pairs, n_dn = sum(inp["counts"]), 2 * sum(max(n - 1, 0) for n in inp["counts"])
    n_terms = {}
    for k in keys:
        dn = "_dn" in k
        pairs = n_dn if dn else n_pairs
        if k.startswith("loss_ce"):
            n_terms[k] = inp["leaves"]["dn_logits_0" if dn else "pred_logits_0"].numel()
        else:
            n_terms[k] = pairs * (6 if k.startswith("loss_bbox") else 1)
    return {k: out[k].detach() for k in keys}, {k: v.grad for k, v in lv.items()}, q_of_g, n_terms


def check_det3d(got, ref, c, tol):
    """Identical key sets; every term within c * sqrt(n) * 2^-24 * |ref| of the float64 one; every gradient within
    tol x max |ref| of its tensor.  Returns the worst (term err / bound at c = 1, gradient err / max |ref|)."""
    terms, grads, _, n_terms = got
    rterms, rgrads, _, _ = ref
    assert sorted(terms) == sorted(rterms)
    worst_t = worst_g = 0.0
    for k in sorted(rterms):
        r = float(rterms[k])
        assert r >= 0
        err, unit = abs(float(terms[k]) - r), math.sqrt(max(n_terms[k], 1)) * U32 * r + 1e-30
        worst_t = max(worst_t, err / unit)
        assert err <= c * unit, "%s: got %.9g, ref %.9g, err / bound %.3g" % (k, float(terms[k]), r, err / (c * unit))
    for k in sorted(rgrads):
        assert grads[k] is not None and rgrads[k] is not None, k
        r = rgrads[k].double()
        scale = float(r.abs().max())
        err = float((grads[k].detach().double().cpu() - r.cpu()).abs().max())
        worst_g = max(worst_g, err / max(scale, 1e-300))
        assert err <= tol * scale, "grad %s: max err %.3g against max |ref| %.3g (tol %.3g)" % (k, err, scale, tol)
    return worst_t, worst_g


# ---- matching cost --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logit_family", ["normal", "uniform12"])
@pytest.mark.parametrize("box_family", ["random", "dyadic", "padded"])
@pytest.mark.parametrize("shape", COST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_match_cost_per_element(dev, shape, box_family, logit_family):
    """Every cost entry inside its own bar, for C = 1, G = 1, a single entry, Q off the 256-thread block, zero padded target
    columns (finite), identical / nested / face-touching boxes, and logits out to +-12."""
    from efg_amd.operators.det_loss import match_cost

    logits, boxes, labels, tgt = cost_problem(shape, box_family, logit_family, dev)
    got = match_cost(logits, boxes, labels, tgt, *WEIGHTS)
    ref = match_cost_fp64(logits, boxes, labels, tgt, *WEIGHTS)
    assert bool(torch.isfinite(got).all())
    r = assert_elementwise("cost", got, ref["cost"], ref["cost_mag"], ref["cost_n"], C_COST[box_family, logit_family],
                           geo64=ref["cost_cond"])
    print("match cost %s %s %s: err / bound %.3g" % (shape, box_family, logit_family, r))


def test_match_cost_into_a_slice_leaves_the_rest_of_the_buffer(dev):
    from efg_amd.operators.det_loss import match_cost

    logits, boxes, labels, tgt = cost_problem((2, 3, 257, 3, 1), "random", "normal", dev)
    plain = match_cost(logits, boxes, labels, tgt, *WEIGHTS)
    buf = torch.full((plain.shape[0] + 3, 257, 1), 123.0, device=dev)
    out = match_cost(logits, boxes, labels, tgt, *WEIGHTS, out=buf[1:1 + plain.shape[0]])
    assert out.data_ptr() == buf[1].data_ptr()
    assert torch.equal(buf[1:1 + plain.shape[0]], plain)
    assert bool((buf[0] == 123.0).all()) and bool((buf[1 + plain.shape[0]:] == 123.0).all())


def test_match_cost_saturated_logits_follow_the_fp32_formula(dev):
    """Logits in {+-20, +-40, +-100}: fp32 p is exactly 1 on the positive side (the log sees 1e-8 alone) and the negative side
    is well conditioned, so the fp32 formula is the definition there; the existing 1e-5 / 1e-5 bar."""
    from efg_amd.detection3d.utils import box_cxcyczlwh_to_xyxyxy, pairwise_box3d_giou
    from efg_amd.operators.det_loss import match_cost

    nl, b, q, c, g = 2, 2, 64, 3, 9
    gen = torch.Generator().manual_seed(4)
    values = torch.tensor([20.0, -20.0, 40.0, -40.0, 100.0, -100.0])
    logits = values[torch.randint(0, 6, (nl, b, q, c), generator=gen)].to(dev)
    boxes, tgt = random_boxes((nl, b, q), gen).to(dev), random_boxes((b, g), gen).to(dev)
    labels = torch.randint(0, c, (b, g), generator=gen).to(dev)
    got = match_cost(logits, boxes, labels, tgt, *WEIGHTS).view(nl, b, q, g)
    p = logits.sigmoid()
    neg = 0.75 * p ** 2 * (-(1 - p + 1e-8).log())
    pos = 0.25 * (1 - p) ** 2 * (-(p + 1e-8).log())
    lab = labels[None, :, None, :].expand(nl, b, q, g)
    cc = torch.gather(pos, 3, lab) - torch.gather(neg, 3, lab)
    cb = (boxes[..., None, :6] - tgt[None, :, None, :, :6]).abs().sum(-1)
    cr = (boxes[..., None, 6:] - tgt[None, :, None, :, 6:]).abs().sum(-1)
    cg = -pairwise_box3d_giou(box_cxcyczlwh_to_xyxyxy(boxes[..., :6]), box_cxcyczlwh_to_xyxyxy(tgt[..., :6])[None])
    ref = WEIGHTS[1] * cb + WEIGHTS[0] * cc + WEIGHTS[2] * cg + WEIGHTS[3] * cr
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)


# ---- assignment on the kernel's cost --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 300, 3, 17), (2, 2, 1000, 1, 64)], ids=lambda s: "x".join(map(str, s)))
def test_assignment_is_optimal_up_to_the_rounding_of_the_cost(dev, shape):
    """match_layers (cost kernel + device Hungarian) with one scene of fewer boxes than G and one of none: every valid column
    gets a distinct query, padded columns -1, and the assignment's total ON THE FLOAT64 COST is at most scipy's optimum on the
    float64 cost + 2 x the bars of the entries of the two assignments -- whichever way ties and near-ties were broken."""
    from scipy.optimize import linear_sum_assignment

    from efg_amd.detection3d.matcher import HungarianMatcher3d

    nl, b, q, c, g = shape
    counts = [g - 3, 0]
    logits, boxes, labels, tgt = cost_problem(shape, "random", "normal", dev)
    for s, n in enumerate(counts):
        tgt[s, n:] = 0
        labels[s, n:] = 0
    q_of_g = HungarianMatcher3d(*WEIGHTS).match_layers(logits, boxes, labels, tgt, counts)
    assert q_of_g.shape == (nl, b, g) and q_of_g.dtype == torch.int64
    ref = match_cost_fp64(logits, boxes, labels, tgt, *WEIGHTS)
    cost = ref["cost"].view(nl, b, q, g).cpu().numpy()
    bar = (C_COST["padded", "normal"] * U32 * ref["cost_mag"] + ref["cost_cond"]).view(nl, b, q, g).cpu().numpy()
    got = q_of_g.cpu().numpy()
    for layer in range(nl):
        for s, n in enumerate(counts):
            rows = got[layer, s, :n]
            assert (got[layer, s, n:] == -1).all()
            assert ((rows >= 0) & (rows < q)).all() and len(set(rows.tolist())) == n
            if n == 0:
                continue
            ri, ci = linear_sum_assignment(cost[layer, s, :, :n])
            entries = set(zip(rows.tolist(), range(n))) | set(zip(ri.tolist(), ci.tolist()))
            slack = 2 * sum(bar[layer, s, i, j] for i, j in entries)
            total, best = cost[layer, s, rows, np.arange(n)].sum(), cost[layer, s, ri, ci].sum()
            assert total <= best + slack, (layer, s, total, best, slack)


# ---- focal loss -----------------------------------------------------------------------------------------------------------
def _focal_case(dev, shape, logit_family, pattern, alpha, gamma):
    from efg_amd.operators.det_loss import FocalLossLayers, device_scalar

    logits, tcls, grad_out = focal_problem(shape, logit_family, pattern, dev)
    denom = 37.0
    logits.requires_grad_(True)
    out = FocalLossLayers.apply(logits, tcls, device_scalar(denom, dev), alpha, gamma)
    out.backward(grad_out)
    ref = focal_fp64(logits, tcls, denom, alpha, gamma, grad_out)
    c = C_FOCAL[logit_family if logit_family != "normal3" else "normal"]
    r = assert_elementwise("focal sums", out, ref["loss"], ref["loss_mag"], ref["loss_n"], c, geo64=ref["loss_cond"])
    assert logits.grad.shape == logits.shape
    rg = 0.0
    if logits.numel():
        rg = assert_elementwise("grad logits", logits.grad, ref["grad"], ref["grad_mag"], ref["grad_n"], c, geo64=ref["grad_cond"])
    print("focal %s %s %s a=%g g=%g: sums %.3g, grad %.3g" % (shape, logit_family, pattern, alpha, gamma, r, rg))


@pytest.mark.parametrize("pattern", ["sparse", "mixed"])
@pytest.mark.parametrize("logit_family", ["normal3", "uniform30"])
@pytest.mark.parametrize("shape", FOCAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_focal_sums_and_gradient_per_element(dev, shape, logit_family, pattern):
    """The per-layer sums (n = N * C terms) and every gradient element, under a different grad_out per layer, on either side of
    the single-workgroup / split threshold (16383, 16384 elements per layer), with ragged tails of the split, all-background
    and all-foreground layers, an empty layer set, and logits out to +-30."""
    _focal_case(dev, shape, logit_family, pattern, 0.25, 2.0)


@pytest.mark.parametrize("shape", [(2, 7, 4), (3, 5462, 3)], ids=lambda s: "x".join(map(str, s)))
def test_focal_general_gamma_without_alpha(dev, shape):
    """alpha = -1 (no class weighting) and gamma = 1.5: the powf branch."""
    _focal_case(dev, shape, "normal3", "sparse", -1.0, 1.5)


# ---- box loss -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["random", "dyadic"])
@pytest.mark.parametrize("case", list(BOX_CASES))
def test_box_loss_sums_and_gradient_per_element(dev, case, family):
    """Per-layer sums [L, 3] and every element of the matched rows' gradient inside their bars; every other row exactly zero.
    Shuffled pair order, q = -1 entries, two and three trips of the forward kernel's 1024-thread loop, a layer without pairs.
    On the dyadic family corners coincide exactly, so the reference's gradient is autograd's choice at every tie of min / max /
    clamp(min=0) -- among them two boxes that touch on a face, where clamp(min=0) still passes the gradient."""
    from efg_amd.operators.det_loss import BoxLossLayers, device_scalar

    boxes, tgt, idx, grad_out = box_problem(case, family, dev)
    denom = 11.0
    boxes.requires_grad_(True)
    out = BoxLossLayers.apply(boxes, tgt, *idx, device_scalar(denom, dev))
    out.backward(grad_out)
    ref = box_loss_fp64(boxes, tgt, *idx, denom, grad_out)
    c = C_BOX[family]
    r = assert_elementwise("box sums", out, ref["loss"], ref["loss_mag"], ref["loss_n"], c, geo64=ref["loss_cond"])
    grad = boxes.grad
    assert bool((grad[~ref["rows"]] == 0).all()), "gradient in an unmatched row"
    rg = assert_elementwise("grad boxes", grad[ref["rows"]], ref["grad"][ref["rows"]], ref["grad_mag"][ref["rows"]], ref["grad_n"], c,
                            geo64=ref["grad_cond"][ref["rows"]])
    print("box loss %s %s: sums %.3g, grad %.3g" % (case, family, r, rg))


# ---- the assembly ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("route", ["dn", "topk"])
def test_det3d_loss_assembly_against_the_float64_module(dev, monkeypatch, route, fused):
    """Det3DLoss on the GPU (EFG_FUSED_LOSS=1: the fused kernels; 0: the composite) against the same module on the CPU in
    float64, both on one assignment: pair lists, the denoising groups (which leave out each scene's last box), the top-k
    route's full-token classification targets, denominators.  Identical keys; terms within c * sqrt(n) * 2^-24 * |ref|;
    gradients to every layer's logits and boxes within TOL_ASSEMBLY x max |ref| (constants: tests/test_det_loss_fp64_ref.py)."""
    monkeypatch.setenv("EFG_FUSED_LOSS", fused)
    inp = det3d_inputs(route)
    ref = run_det3d(inp, torch.device("cpu"), torch.float64)
    got = run_det3d(inp, dev, torch.float32, q_of_g=ref[2])
    wt, wg = check_det3d(got, ref, C_ASSEMBLY, TOL_ASSEMBLY)
    print("Det3DLoss %s fused=%s: terms %.3g of the unit bar, gradients %.3g of max |ref|" % (route, fused, wt, wg))
