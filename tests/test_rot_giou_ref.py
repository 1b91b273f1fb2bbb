"""CPU pins of the heading-aware 3-D GIoU (detection3d.utils.rot_giou3d, the float64 yardstick of tests/test_rot_giou_gpu.py):
against a brute-force evaluation written here (Sutherland-Hodgman clipping + monotone-chain hull in float64), against the
reference's own values (tests/golden/rot_giou_ref.npz, scripts/make_golden_rot_giou.py), closed-form cases, and the
`model.loss.giou_type` plumbing through the matcher, the loss module and the detection heads."""
import math

import numpy as np
import pytest
import torch

from conftest import golden

METRIC = (1.0, 1.0, 1.0, 0.0)


@pytest.fixture(autouse=True)
def _leave_the_global_generators_alone():
    """The tests here seed and draw from torch's global generators (model construction, dropout); later test files build
    modules from whatever state they inherit, so hand it on as it was found."""
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


# ---- brute force: plain float64, global frame ------------------------------------------------------------------------------
def _corners(box):
    x, y, l, w, yaw = box[0], box[1], box[3], box[4], box[6]
    c, s = math.cos(yaw), math.sin(yaw)
    return [(x + su * 0.5 * l * c - sv * 0.5 * w * s, y + su * 0.5 * l * s + sv * 0.5 * w * c)
            for su, sv in ((1, 1), (-1, 1), (-1, -1), (1, -1))]


def _shoelace(poly):
    return 0.5 * sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[i][1] * poly[(i + 1) % len(poly)][0]
                     for i in range(len(poly)))


def _clip(subject, clipper):
    """Sutherland-Hodgman: the counter-clockwise polygon `subject` inside the counter-clockwise convex `clipper`."""
    out = subject
    for i in range(len(clipper)):
        (ax, ay), (bx, by) = clipper[i], clipper[(i + 1) % len(clipper)]
        inp, out = out, []
        if not inp:
            break
        side = [(bx - ax) * (py - ay) - (by - ay) * (px - ax) for px, py in inp]
        for j in range(len(inp)):
            k = (j + 1) % len(inp)
            if side[j] >= 0:
                out.append(inp[j])
            if (side[j] >= 0) != (side[k] >= 0):
                t = side[j] / (side[j] - side[k])
                out.append((inp[j][0] + t * (inp[k][0] - inp[j][0]), inp[j][1] + t * (inp[k][1] - inp[j][1])))
    return out


def _hull(points):
    """Andrew's monotone chain."""
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h

    lower, upper = half(pts), half(pts[::-1])
    return lower[:-1] + upper[:-1]


def brute_giou(a, b):
    ca, cb = _corners(a), _corners(b)
    inter_poly = _clip(ca, cb)
    inter = max(_shoelace(inter_poly), 0.0) if len(inter_poly) >= 3 else 0.0
    hull = _shoelace(_hull(ca + cb))
    zo = max(min(a[2] + 0.5 * a[5], b[2] + 0.5 * b[5]) - max(a[2] - 0.5 * a[5], b[2] - 0.5 * b[5]), 0.0)
    zr = max(a[2] + 0.5 * a[5], b[2] + 0.5 * b[5]) - min(a[2] - 0.5 * a[5], b[2] - 0.5 * b[5])
    i3 = inter * zo
    u3 = a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - i3
    h3 = hull * zr
    return i3 / u3 - (h3 - u3) / h3


def random_pairs(n, seed, shift=0.0):
    """float64 metric boxes [n, 7] x 2: centres within +-1.5 m of (shift, shift), l in [0.5, 6], w, h in [0.5, 3], any yaw."""
    rng = np.random.default_rng(seed)

    def boxes():
        b = np.empty((n, 7))
        b[:, :2] = rng.uniform(-1.5, 1.5, (n, 2)) + shift
        b[:, 2] = rng.uniform(-1.0, 1.0, n)
        b[:, 3] = rng.uniform(0.5, 6.0, n)
        b[:, 4:6] = rng.uniform(0.5, 3.0, (n, 2))
        b[:, 6] = rng.uniform(-math.pi, math.pi, n)
        return b

    return boxes(), boxes()


# ---- 1. the formulation against the brute force ------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shift", [("near", 0.0), ("far", 70.0)])
def test_formulation_matches_brute_force_value_and_gradient(family, shift):
    """1000 pairs per family (2000 in all): value to 1e-10; autograd gradient of all 14 parameters against a central
    difference (h = 1e-6) of the brute-force value to 1e-6 (1 + max |grad| of the pair)."""
    from efg_amd.detection3d.utils import paired_rot_giou3d

    a, b = random_pairs(1000, 11 if family == "near" else 12, shift)
    ta, tb = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    got = paired_rot_giou3d(ta, tb, METRIC)
    ga, gb = torch.autograd.grad(got.sum(), (ta, tb))
    want = np.array([brute_giou(x, y) for x, y in zip(a, b)])
    err = np.abs(got.detach().numpy() - want)
    print("%s: value max |err| %.3g" % (family, err.max()))
    assert err.max() <= 1e-10, (family, int(err.argmax()), err.max())
    grad = np.concatenate((ga.numpy(), gb.numpy()), axis=1)                 # [n, 14]
    h, worst = 1e-6, 0.0
    for i in range(len(a)):
        fd = np.empty(14)
        for k in range(14):
            p = [a[i].copy(), b[i].copy()]
            m = [a[i].copy(), b[i].copy()]
            p[k // 7][k % 7] += h
            m[k // 7][k % 7] -= h
            fd[k] = (brute_giou(*p) - brute_giou(*m)) / (2 * h)
        r = np.abs(grad[i] - fd).max() / (1e-6 * (1 + np.abs(grad[i]).max()))
        worst = max(worst, r)
        assert r <= 1.0, (family, i, grad[i], fd)
    print("%s: gradient worst err / bar %.3g" % (family, worst))


# ---- 2. against the reference's values ---------------------------------------------------------------------------------------
def test_formulation_matches_the_reference_on_the_near_family():
    from efg_amd.detection3d.utils import paired_rot_giou3d

    g = golden("rot_giou_ref.npz")
    a, b = torch.from_numpy(g["a_near"]).double(), torch.from_numpy(g["b_near"]).double()
    assert a.shape == (500, 7) and np.array_equal(g["a_far"][:, 2:], g["a_near"][:, 2:])
    err = (paired_rot_giou3d(a, b, METRIC) - torch.from_numpy(g["giou_near"]).double()).abs().max()
    print("reference (float32) against the float64 formulation, near: %.3g" % float(err))
    assert float(err) <= 5e-5


# ---- 3. closed forms ---------------------------------------------------------------------------------------------------------
def _aligned(a, b):
    from efg_amd.detection3d.utils import box_cxcyczlwh_to_xyxyxy, paired_box3d_giou

    return paired_box3d_giou(box_cxcyczlwh_to_xyxyxy(a[:, :6]), box_cxcyczlwh_to_xyxyxy(b[:, :6]))


def test_closed_form_cases():
    from efg_amd.detection3d.utils import box_cxcyczlwh_to_xyxyxy, paired_rot_giou3d, pairwise_rot_giou3d, rot_giou3d

    a, b = (torch.from_numpy(x) for x in random_pairs(300, 5))
    # identical boxes: 1 (also at yaw 0 and far from the origin)
    same = torch.cat((a[:50], a[:50] * torch.tensor([1, 1, 1, 1, 1, 1, 0.0]), a[:50] + torch.tensor([70.0, 70, 0, 0, 0, 0, 0])))
    giou, iou = rot_giou3d(same, same.clone(), METRIC)
    assert float((giou - 1).abs().max()) <= 1e-12 and float((iou - 1).abs().max()) <= 1e-12
    # yaw 0 on arbitrary boxes: the axis-aligned IoU.  The GIoU is the axis-aligned one only where the convex hull IS the
    # enclosing box (the hull of two axis-aligned rectangles in general position cuts two corners off it, so the rotated
    # GIoU is the larger): equal to 1e-12 for boxes that share their y extent, overlapping and disjoint, and >= everywhere.
    a0, b0 = a.clone(), b.clone()
    a0[:, 6] = b0[:, 6] = 0.0
    giou0, iou0 = rot_giou3d(a0, b0, METRIC)
    ali0 = _aligned(a0, b0)
    lo, hi = box_cxcyczlwh_to_xyxyxy(a0[:, :6]), box_cxcyczlwh_to_xyxyxy(b0[:, :6])
    inter = (torch.min(lo[:, 3:], hi[:, 3:]) - torch.max(lo[:, :3], hi[:, :3])).clamp(min=0).prod(-1)
    iou_aligned = inter / (a0[:, 3:6].prod(-1) + b0[:, 3:6].prod(-1) - inter)
    assert float((iou0 - iou_aligned).abs().max()) <= 1e-12 and int((inter > 0).sum()) > 100
    assert bool((giou0 >= ali0 - 1e-12).all())
    b1 = b0.clone()
    b1[:, 1], b1[:, 4] = a0[:, 1], a0[:, 4]
    assert float((paired_rot_giou3d(a0, b1, METRIC) - _aligned(a0, b1)).abs().max()) <= 1e-12
    # disjoint axis-aligned boxes
    d1 = b1.clone()
    d1[:, 0] += 20.0
    got = paired_rot_giou3d(a0, d1, METRIC)
    assert float((got - _aligned(a0, d1)).abs().max()) <= 1e-12 and bool((got < 0).all())
    # symmetric in its arguments; a heading turned by pi is the same box
    full = paired_rot_giou3d(a, b, METRIC)
    assert float((full - paired_rot_giou3d(b, a, METRIC)).abs().max()) <= 1e-12
    turned = a.clone()
    turned[:, 6] += math.pi
    assert float((full - paired_rot_giou3d(turned, b, METRIC)).abs().max()) <= 1e-12
    # the heading matters: a 4.8 x 2 m car at 45 degrees against the same car at 0
    car = torch.tensor([[0.0, 0, 0, 4.8, 2.0, 1.5, 0.0]], dtype=torch.float64)
    car45 = car.clone()
    car45[0, 6] = math.pi / 4
    assert float(paired_rot_giou3d(car45, car, METRIC)) < 0.5 and float(_aligned(car45, car)) == 1.0
    # the code frame is the metric frame of the decoded boxes; pairwise is the paired value of every combination
    code_a, code_b = a.clone(), b.clone()
    for c in (code_a, code_b):
        c[:, 0], c[:, 1], c[:, 3], c[:, 4] = c[:, 0] / 150.4, c[:, 1] / 140.0, c[:, 3] / 150.4, c[:, 4] / 140.0
        c[:, 6] = (c[:, 6] + math.pi) / (2 * math.pi)
    frame = (150.4, 140.0, 2 * math.pi, -math.pi)
    assert float((paired_rot_giou3d(code_a, code_b, frame) - full).abs().max()) <= 1e-11
    mat = pairwise_rot_giou3d(code_a[:7].reshape(1, 7, 7), code_b[:5].reshape(1, 5, 7), frame)
    assert mat.shape == (1, 7, 5)
    for i in range(7):
        assert float((mat[0, i] - paired_rot_giou3d(code_a[i:i + 1].expand(5, 7), code_b[:5], frame)).abs().max()) <= 1e-12
    # a padded (all-zero) target row is finite
    assert bool(torch.isfinite(pairwise_rot_giou3d(code_a[:3], torch.zeros(2, 7, dtype=torch.float64), frame)).all())


# ---- 4. config plumbing --------------------------------------------------------------------------------------------------------
PC_RANGE = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
FRAME = (150.4, 150.4, 2 * math.pi, -math.pi)


def _config(giou_type=None):
    from test_model_golden import cfg_of

    loss = {"bbox_loss_coef": 4, "giou_loss_coef": 2, "class_loss_coef": 1, "rad_loss_coef": 4,
            "matcher": {"class_weight": 1, "bbox_weight": 4, "giou_weight": 2, "rad_weight": 4}}
    if giou_type is not None:
        loss["giou_type"] = giou_type
    return cfg_of({"model": {"hidden_dim": 32, "loss": loss, "transformer": {"dec_layers": 2}},
                   "dataset": {"pc_range": PC_RANGE}})


def _head(giou_type=None):
    from efg_amd.detection3d.heads import Det3DHead

    torch.manual_seed(0)
    return Det3DHead(_config(giou_type), with_aux=True, with_metrics=True, num_classes=3, num_layers=2)


def _tiny_case():
    """L = 2 layers, B = 2 scenes (3 and 1 boxes), Q = 6 queries near their targets, C = 3."""
    gen = torch.Generator().manual_seed(3)
    tgt = [torch.tensor([[0.50, 0.50, 0.5, 0.030, 0.013, 0.08, 0.10], [0.52, 0.51, 0.5, 0.030, 0.013, 0.08, 0.35],
                         [0.30, 0.70, 0.4, 0.010, 0.010, 0.10, 0.80]]),
           torch.tensor([[0.70, 0.20, 0.6, 0.050, 0.020, 0.15, 0.60]])]
    targets = [{"labels": torch.tensor([0, 2, 1]), "gt_boxes": tgt[0]}, {"labels": torch.tensor([1]), "gt_boxes": tgt[1]}]
    boxes = torch.empty(2, 2, 6, 7)
    for b in range(2):
        base = tgt[b][torch.arange(6) % len(tgt[b])]
        boxes[:, b] = base[None] + (torch.rand(2, 6, 7, generator=gen) - 0.5) * torch.tensor([.01, .01, .02, .01, .005, .02, .2])
    logits = torch.randn(2, 2, 6, 3, generator=gen)
    return logits, boxes.clamp(min=1e-3), targets


def _outputs(logits, boxes):
    return {"pred_logits": logits[-1], "pred_boxes": boxes[-1],
            "aux_outputs": [{"pred_logits": logits[0], "pred_boxes": boxes[0]}]}


def test_giou_type_bogus_raises_and_the_default_is_aligned():
    from efg_amd.config import _DEFAULTS
    from efg_amd.detection3d.matcher import HungarianMatcher3d

    with pytest.raises(ValueError):
        _head("bogus")
    with pytest.raises(ValueError):
        HungarianMatcher3d(giou_type="rotated")          # no frame
    assert _DEFAULTS["model"]["loss"]["giou_type"] == "aligned"
    head = _head()
    assert head.losses.giou_type == head.losses.matcher.giou_type == "aligned"
    head = _head("rotated")
    assert head.losses.giou_type == head.losses.matcher.giou_type == "rotated"
    assert head.losses.frame == pytest.approx(FRAME) and head.losses.matcher.frame == pytest.approx(FRAME)


def test_rotated_matcher_cost_and_loss_giou_equal_the_formulation():
    from scipy.optimize import linear_sum_assignment

    from efg_amd.detection3d.utils import paired_rot_giou3d, pairwise_rot_giou3d

    logits, boxes, targets = _tiny_case()
    head, plain = _head("rotated"), _head("aligned")
    matcher = head.losses.matcher
    # the host (per-scene) path: its cost differs from the aligned matcher's by exactly the swapped GIoU term
    outs = {"pred_logits": logits[-1], "pred_boxes": boxes[-1]}
    for b, (rot, ali) in enumerate(zip(matcher.cost_matrices(outs, targets), plain.losses.matcher.cost_matrices(outs, targets))):
        from efg_amd.detection3d.utils import box_cxcyczlwh_to_xyxyxy, generalized_box3d_iou

        tb = targets[b]["gt_boxes"]
        want = ali + 2 * generalized_box3d_iou(box_cxcyczlwh_to_xyxyxy(boxes[-1, b, :, :6]), box_cxcyczlwh_to_xyxyxy(tb[:, :6])) \
            - 2 * pairwise_rot_giou3d(boxes[-1, b], tb, FRAME)
        assert float((rot - want).abs().max()) <= 1e-5
        assert float((rot - ali).abs().max()) > 1e-2          # the heading changes the cost
    # the layer-stacked path gives the assignment of that cost
    out = head.compute_losses(_outputs(logits, boxes), targets)
    q_of_g = _outputs(logits, boxes)
    head.losses(q_of_g, targets)
    assigned = q_of_g["matched_query_of_gt"]
    for b, cost in enumerate(matcher.cost_matrices(outs, targets)):
        i, j = linear_sum_assignment(cost.numpy())
        assert assigned[b, torch.as_tensor(j)].tolist() == list(i)
    # loss_giou of the last layer = giou_loss_coef * sum (1 - rotated GIoU of the matched pairs) / num_boxes
    src = torch.cat([boxes[-1, b, assigned[b, :len(t["labels"])]] for b, t in enumerate(targets)])
    tgt = torch.cat([t["gt_boxes"] for t in targets])
    want = 2 * (1 - paired_rot_giou3d(src.double(), tgt.double(), FRAME)).sum() / 4
    assert abs(float(out["loss_giou"]) - float(want)) <= 1e-5
    assert abs(float(out["loss_giou"]) - float(plain.compute_losses(_outputs(logits, boxes), targets)["loss_giou"])) > 1e-3


def test_rotated_loss_is_differentiable_on_the_cpu():
    logits, boxes, targets = _tiny_case()
    boxes.requires_grad_(True)
    out = _head("rotated").compute_losses(_outputs(logits, boxes), targets)
    out["loss_giou"].backward()
    assert bool(torch.isfinite(boxes.grad).all()) and float(boxes.grad[-1].abs().sum()) > 0
    assert float(boxes.grad[-1, :, :, 6].abs().sum()) > 0      # the heading receives a gradient from the GIoU term


def test_absent_key_is_bit_identical_to_aligned():
    """Every loss term of a small CPU step with the key absent == with giou_type: aligned == the axis-aligned composition
    written out here from the pre-existing helpers."""
    from efg_amd.detection3d.utils import box_cxcyczlwh_to_xyxyxy, paired_box3d_giou

    logits, boxes, targets = _tiny_case()
    absent = _head().compute_losses(_outputs(logits, boxes), targets)
    aligned = _head("aligned").compute_losses(_outputs(logits, boxes), targets)
    assert set(absent) == set(aligned)
    for k in absent:
        assert torch.equal(absent[k], aligned[k]), k
    o = _outputs(logits, boxes)
    _head().losses(o, targets)
    assigned = o["matched_query_of_gt"]
    src = torch.cat([boxes[-1, b, assigned[b, :len(t["labels"])]] for b, t in enumerate(targets)])
    tgt = torch.cat([t["gt_boxes"] for t in targets])
    want = 2 * ((1 - paired_box3d_giou(box_cxcyczlwh_to_xyxyxy(src[:, :6]), box_cxcyczlwh_to_xyxyxy(tgt[:, :6]))).sum() / 4)
    assert abs(float(absent["loss_giou"]) - float(want)) <= 1e-6


def test_rotated_model_builds_on_the_cpu_from_the_shipped_config():
    """`model.loss.giou_type: rotated` through load_config + VoxelDETR (the full-model golden's reduced configuration): both
    heads read the frame off the box coder's range; without the override the shipped YAML gives the default."""
    from test_model_full_golden import _build

    cpu = torch.device("cpu")
    base, _ = _build(cpu, False)
    assert base.config.model.loss.giou_type == "aligned"
    assert base.transformer.decoder.detection_head.losses.giou_type == "aligned"
    model, _ = _build(cpu, False, extra={"model.loss.giou_type": "rotated"})
    size = model.box_coder.pc_size[:2].tolist()
    for head in (model.transformer.proposal_head, model.transformer.decoder.detection_head):
        assert head.losses.giou_type == head.losses.matcher.giou_type == "rotated"
        assert head.losses.frame == pytest.approx((size[0], size[1], 2 * math.pi, -math.pi))
        assert head.losses.matcher.frame == head.losses.frame
    with pytest.raises(ValueError):
        _build(cpu, False, extra={"model.loss.giou_type": "bogus"})
