"""GPU: the heading-aware 3-D GIoU kernels (csrc/rot_giou.hip) against the float64 PyTorch formulation
(detection3d.utils.rot_giou3d, pinned on the CPU by tests/test_rot_giou_ref.py), on the fixture's pairs near the origin and
70 m from it, in the metric frame and in the ConQueR code frame (VoxelBoxCoder3D, 150.4 m range).

Bars.  Value: 5e-5 absolute -- about 2.5 x the error of the reference's own float32 function near the origin (1.9e-5; 1.4e-4 at
70 m, where its global-frame evaluation loses a digit).  Gradient: 5e-5 (1 + max |grad| of the pair) -- the reference's float32
autograd measures 2.2e-5 near and 1.1e-4 far in that normalisation.  A pair is left out of the gradient check only if a
corner of one rectangle lies within 1e-4 m of an edge line of the other (a kink of the gradient), at most 1 % of the pairs.

Measured on an MI355X (max over n = 1000 pairs; value | grad_a | grad_b, the gradients in the bar's normalisation):
  near metric 2.1e-07 | 2.3e-07 | 2.4e-07      near code 9.1e-07 | 1.3e-06 | 3.3e-06
  far  metric 2.0e-07 | 1.9e-07 | 1.9e-07      far  code 8.6e-07 | 1.3e-06 | 3.3e-06
2 of the 1000 pairs of each family are at a kink and left out of the gradient check."""
import math

import pytest
import torch

from conftest import golden
from fp64_ref import U32, assert_elementwise, match_cost_fp64
from test_det_loss_fp64_gpu import C_COST, WEIGHTS, cost_problem

pytestmark = pytest.mark.gpu

PC_RANGE = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
FRAMES = {"metric": (1.0, 1.0, 1.0, 0.0), "code": (150.4, 150.4, 2 * math.pi, -math.pi)}
VALUE_BAR = GRAD_BAR = 5e-5
_CACHE = {}


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


def family(name, frame):
    """1000 float32 pairs of a fixture family (its 500 pairs, then box i against box i + 1 of the other set) in `frame`, with
    the float64 value, gradients and kink mask of the formulation -- computed once."""
    key = (name, frame)
    if key not in _CACHE:
        from efg_amd.detection3d.box_coder import VoxelBoxCoder3D
        from efg_amd.detection3d.utils import rot_giou3d

        g = golden("rot_giou_ref.npz")
        a, b = torch.from_numpy(g["a_" + name]), torch.from_numpy(g["b_" + name])
        a, b = torch.cat((a, a)), torch.cat((b, b.roll(-1, 0)))
        metric = (a.double(), b.double())
        if frame == "code":
            coder = VoxelBoxCoder3D([0.1, 0.1, 0.15], PC_RANGE)
            a, b = (coder.encode({"labels": torch.ones(len(x), dtype=torch.int64), "gt_boxes": x.clone()})["gt_boxes"]
                    for x in (a, b))
            assert a.dtype == torch.float32
        a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
        giou, iou = rot_giou3d(a64, b64, FRAMES[frame])
        ga, gb = torch.autograd.grad(giou.sum(), (a64, b64))
        _CACHE[key] = dict(a=a, b=b, giou=giou.detach(), iou=iou.detach(), ga=ga, gb=gb, kink=near_kink(*metric))
    return _CACHE[key]


def near_kink(a, b, tol=1e-4):
    """float64 metric boxes [n, 7]: True where some corner of one rectangle lies within `tol` metres of an edge LINE of the
    other."""
    def corners(box, origin):
        c, s = torch.cos(box[:, 6:7]), torch.sin(box[:, 6:7])
        su, sv = box.new_tensor([1.0, -1, -1, 1]), box.new_tensor([1.0, 1, -1, -1])
        x = box[:, 0:1] - origin[:, 0:1] + su * 0.5 * box[:, 3:4] * c - sv * 0.5 * box[:, 4:5] * s
        y = box[:, 1:2] - origin[:, 1:2] + su * 0.5 * box[:, 3:4] * s + sv * 0.5 * box[:, 4:5] * c
        return x, y

    def dist(px, py, qx, qy):       # corners p [n, 4] to the edge lines of q [n, 4] -> min over both
        ex, ey = qx.roll(-1, 1) - qx, qy.roll(-1, 1) - qy
        ln = torch.sqrt(ex * ex + ey * ey)
        d = (ex[:, None, :] * (py[:, :, None] - qy[:, None, :]) - ey[:, None, :] * (px[:, :, None] - qx[:, None, :])) / ln[:, None, :]
        return d.abs().flatten(1).min(1).values

    ax, ay = corners(a, b)
    bx, by = corners(b, b)
    return torch.minimum(dist(ax, ay, bx, by), dist(bx, by, ax, ay)) < tol


def normalised(got, ref):
    """max |got - ref| of every row over (1 + max |ref| of the row)"""
    return (got.detach().cpu().double() - ref).abs().max(1).values / (1 + ref.abs().max(1).values)


# ---- 1. paired forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("frame", ["metric", "code"])
@pytest.mark.parametrize("name", ["near", "far"])
def test_paired_forward(dev, name, frame, n):
    from efg_amd.operators.rot_giou import rot_giou_paired

    f = family(name, frame)
    giou, iou = rot_giou_paired(f["a"][:n].to(dev), f["b"][:n].to(dev), FRAMES[frame])
    assert giou.shape == iou.shape == (n,)
    ev = float((giou.cpu().double() - f["giou"][:n]).abs().max())
    ei = float((iou.cpu().double() - f["iou"][:n]).abs().max())
    print("paired forward %s %s n=%d: giou %.3g, iou %.3g" % (name, frame, n, ev, ei))
    assert ev <= VALUE_BAR and ei <= VALUE_BAR


def test_paired_forward_of_nothing_and_of_padded_targets(dev):
    from efg_amd.operators.rot_giou import rot_giou_paired

    giou, iou = rot_giou_paired(torch.zeros(0, 7, device=dev), torch.zeros(0, 7, device=dev), FRAMES["metric"])
    assert giou.shape == iou.shape == (0,)
    f = family("near", "code")
    giou, iou = rot_giou_paired(f["a"][:65].to(dev), torch.zeros(65, 7, device=dev), FRAMES["code"])
    assert bool(torch.isfinite(giou).all()) and bool((iou == 0).all())
    nan = f["a"][:4].clone()
    nan[0, 0] = float("nan")
    assert bool(torch.isfinite(rot_giou_paired(nan.to(dev), f["b"][:4].to(dev), FRAMES["code"])[0]).all())


# ---- 2. paired backward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("frame", ["metric", "code"])
@pytest.mark.parametrize("name", ["near", "far"])
def test_paired_backward(dev, name, frame, n):
    from efg_amd.operators.rot_giou import rot_giou_paired

    f = family(name, frame)
    keep = ~f["kink"][:n]
    assert int((~keep).sum()) <= n // 100, "more than 1 % of the pairs at a kink"
    a, b = f["a"][:n].to(dev).requires_grad_(True), f["b"][:n].to(dev).requires_grad_(True)
    rot_giou_paired(a, b, FRAMES[frame])[0].sum().backward()
    ea, eb = normalised(a.grad, f["ga"][:n])[keep], normalised(b.grad, f["gb"][:n])[keep]
    print("paired backward %s %s n=%d: grad_a %.3g, grad_b %.3g, left out %d" % (name, frame, n, float(ea.max()), float(eb.max()),
                                                                             int((~keep).sum())))
    assert float(ea.max()) <= GRAD_BAR and float(eb.max()) <= GRAD_BAR
    # a non-unit upstream gradient scales the rows; without a gradient for b the kernel gets NULL and writes a alone
    up = torch.linspace(-2.0, 3.0, n, device=dev)
    a2, b2 = f["a"][:n].to(dev).requires_grad_(True), f["b"][:n].to(dev)
    (rot_giou_paired(a2, b2, FRAMES[frame])[0] * up).sum().backward()
    assert b2.grad is None
    e2 = normalised(a2.grad, f["ga"][:n] * up.cpu().double()[:, None])[keep]
    assert float(e2.max()) <= GRAD_BAR * 3.0         # |upstream| <= 3


# ---- 3. matching cost ---------------------------------------------------------------------------------------------------------
def rotated_cost_fp64(logits, boxes, labels, tgt, frame):
    """match_cost_fp64 with the rotated GIoU swapped in for the axis-aligned one (float64)."""
    from efg_amd.detection3d.utils import box_cxcyczlwh_to_xyxyxy, pairwise_box3d_giou, pairwise_rot_giou3d

    ref = match_cost_fp64(logits, boxes, labels, tgt, *WEIGHTS)
    bx, tb = boxes.double(), tgt.double()[None]
    aligned = pairwise_box3d_giou(box_cxcyczlwh_to_xyxyxy(bx[..., :6]), box_cxcyczlwh_to_xyxyxy(tb[..., :6]))
    rotated = pairwise_rot_giou3d(bx, tb, frame)
    w_giou = WEIGHTS[2]
    ref["cost"] = ref["cost"] + w_giou * (aligned - rotated).reshape(ref["cost"].shape)
    ref["cost_mag"] = ref["cost_mag"] + abs(w_giou) * rotated.abs().reshape(ref["cost"].shape)
    return ref


@pytest.mark.parametrize("shape", [(4, 2, 70, 3, 1), (4, 2, 70, 3, 17), (2, 1, 257, 3, 5)], ids=lambda s: "x".join(map(str, s)))
def test_match_cost_rotated(dev, shape):
    """(L * B, B, Q, C, G) shapes; every cost entry inside the bar of the existing match-cost test plus 5e-5 w_giou for the GIoU
    term; the padded (all-zero) target columns of the 17-column case are finite."""
    from efg_amd.operators.det_loss import match_cost

    lb, b, q, c, g = shape
    box_family = "padded" if g == 17 else "random"
    logits, boxes, labels, tgt = cost_problem((lb // b, b, q, c, g), box_family, "normal", dev)
    got = match_cost(logits, boxes, labels, tgt, *WEIGHTS, giou_type="rotated", frame=FRAMES["code"])
    assert got.shape == (lb, q, g) and bool(torch.isfinite(got).all())
    ref = rotated_cost_fp64(logits, boxes, labels, tgt, FRAMES["code"])
    if box_family == "padded":
        assert bool((tgt[:, -1] == 0).all())
    assert bool(torch.isfinite(ref["cost"]).all())
    r = assert_elementwise("rotated cost", got, ref["cost"], ref["cost_mag"], ref["cost_n"], C_COST[box_family, "normal"],
                           geo64=ref["cost_cond"] + VALUE_BAR * abs(WEIGHTS[2]))
    print("rotated match cost %s: err / bound %.3g" % (shape, r))
    assert float((got - match_cost(logits, boxes, labels, tgt, *WEIGHTS)).abs().max()) > 1e-2   # the heading is in the cost


def test_match_cost_rotated_into_a_slice_and_aligned_through_the_new_argument(dev):
    from efg_amd.operators.det_loss import match_cost

    logits, boxes, labels, tgt = cost_problem((2, 1, 257, 3, 5), "random", "normal", dev)
    plain = match_cost(logits, boxes, labels, tgt, *WEIGHTS, giou_type="rotated", frame=FRAMES["code"])
    buf = torch.full((plain.shape[0] + 3, 257, 5), 123.0, device=dev)
    out = match_cost(logits, boxes, labels, tgt, *WEIGHTS, out=buf[1:1 + plain.shape[0]], giou_type="rotated",
                     frame=FRAMES["code"])
    assert out.data_ptr() == buf[1].data_ptr() and torch.equal(buf[1:1 + plain.shape[0]], plain)
    assert bool((buf[0] == 123.0).all()) and bool((buf[1 + plain.shape[0]:] == 123.0).all())
    assert torch.equal(match_cost(logits, boxes, labels, tgt, *WEIGHTS, giou_type="aligned"),
                       match_cost(logits, boxes, labels, tgt, *WEIGHTS))
    with pytest.raises(ValueError):
        match_cost(logits, boxes, labels, tgt, *WEIGHTS, giou_type="rotated")
    empty = match_cost(logits, boxes, labels[:, :0], tgt[:, :0], *WEIGHTS, giou_type="rotated", frame=FRAMES["code"])
    assert empty.shape == (2, 257, 0)


# ---- 4. box loss --------------------------------------------------------------------------------------------------------------
def box_case(n, device):
    """L = 3, B = 2, Q = 70, G = 9: n matched pairs on distinct (layer, scene, query) rows, predictions near their targets."""
    gen = torch.Generator().manual_seed(40 + n)
    nl, nb, nq, ng = 3, 2, 70, 9
    tgt = torch.rand(nb, ng, 7, generator=gen)
    tgt[..., :2] = 0.2 + 0.6 * tgt[..., :2]
    tgt[..., 3:5] = 0.004 + 0.03 * tgt[..., 3:5]                     # 0.6 .. 5.1 m
    tgt[..., 5] = 0.05 + 0.1 * tgt[..., 5]
    boxes = torch.rand(nl, nb, nq, 7, generator=gen)
    rows = torch.randperm(nl * nb * nq, generator=gen)[:n]
    li, bi, qi = rows // (nb * nq), (rows // nq) % nb, rows % nq
    gi = torch.randint(0, ng, (n,), generator=gen)
    noise = (torch.rand(n, 7, generator=gen) - 0.5) * torch.tensor([0.01, 0.01, 0.05, 0.01, 0.01, 0.05, 0.2])
    boxes[li, bi, qi] = (tgt[bi, gi] + noise).clamp(min=1e-3)
    grad_out = torch.randn(nl, 3, generator=gen) + 1.5
    return boxes.to(device), tgt.to(device), [t.to(device) for t in (li, bi, qi, gi)], grad_out.to(device), float(max(n, 1))


@pytest.mark.parametrize("n", [0, 1, 40])
def test_box_loss_rotated(dev, n):
    from efg_amd.detection3d.box_coder import VoxelBoxCoder3D
    from efg_amd.detection3d.utils import rot_giou3d
    from efg_amd.operators.det_loss import BoxLossLayers, device_scalar

    boxes, tgt, idx, grad_out, denom = box_case(n, dev)
    li, bi, qi, gi = idx
    frame = FRAMES["code"]
    src64, tgt64 = boxes[li, bi, qi].cpu().double().requires_grad_(True), tgt[bi, gi].cpu().double()
    giou = rot_giou3d(src64, tgt64, frame)[0]
    dgiou, = torch.autograd.grad(giou.sum(), src64) if n else (torch.zeros(0, 7, dtype=torch.float64),)
    if n:   # no pair of this fixed case sits at a kink of the gradient
        coder = VoxelBoxCoder3D([0.1, 0.1, 0.15], PC_RANGE)
        assert not bool(near_kink(coder.decode(src64.detach().clone()), coder.decode(tgt64.clone())).any())

    def run(fn, *extra):
        bx = boxes.clone().requires_grad_(True)
        out = fn.apply(bx, tgt, *idx, device_scalar(denom, dev), *extra)
        (out * grad_out).sum().backward()
        return out.detach(), bx.grad

    out, grad = run(BoxLossLayers, frame)
    out2, grad2 = run(BoxLossLayers, frame)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)                     # deterministic reduction
    plain, _ = run(BoxLossLayers)
    assert torch.equal(out[:, 0], plain[:, 0]) and torch.equal(out[:, 2], plain[:, 2])
    # column 1: sum (1 - rotated GIoU) / denom per layer; 5e-5 per pair plus the rounding of an fp32 sum of n terms <= 2
    want = torch.zeros(3, dtype=torch.float64).index_add_(0, li.cpu(), 1 - giou.detach()) / denom
    count = torch.zeros(3, dtype=torch.float64).index_add_(0, li.cpu(), torch.ones(n, dtype=torch.float64))
    bar = (count * VALUE_BAR + 2 * count * (count + 2) * U32) / denom + 1e-30
    err = (out[:, 1].cpu().double() - want).abs()
    print("rotated box loss n=%d: column 1 err / bar %.3g" % (n, float((err / bar).max())))
    assert bool((err <= bar).all()), (err, bar)
    # gradient: L1 signs exactly as the aligned kernel's; the GIoU share inside 5e-5 (1 + max |d giou|) |upstream|
    w = grad_out.cpu().double()[li.cpu()] / denom                                # [n, 3]
    diff = (src64.detach() - tgt64)
    want_g = torch.cat((w[:, :1] * diff[:, :6].sign(), w[:, 2:] * diff[:, 6:].sign()), 1) - w[:, 1:2] * dgiou
    got_g = grad[li, bi, qi].cpu().double()
    if n:
        gbar = w[:, 1].abs() * GRAD_BAR * (1 + dgiou.abs().max(1).values) + 4 * U32 * want_g.abs().max(1).values
        gerr = (got_g - want_g).abs().max(1).values
        print("rotated box loss n=%d: gradient err / bar %.3g" % (n, float((gerr / gbar).max())))
        assert bool((gerr <= gbar).all())
        assert float(got_g[:, 6].abs().min()) > 0
    mask = torch.ones(boxes.shape[:3], dtype=torch.bool, device=dev)
    mask[li, bi, qi] = False
    assert bool((grad[mask] == 0).all())


# ---- 5. model level -------------------------------------------------------------------------------------------------------------
def _model_step(dev, extra):
    """One training step of the full-model golden's reduced ConQueR configuration; returns the loss terms, the gradients and
    the matched query of every ground truth (decoder and encoder-proposal heads)."""
    from test_model_full_golden import _build, _run

    model, _ = _build(dev, False, extra=extra)
    matched = {}
    heads = {"dec": model.transformer.decoder.detection_head, "enc": model.transformer.proposal_head}
    hooks = [h.losses.register_forward_hook(lambda m, args, out, k=k: matched.update({k: args[0]["matched_query_of_gt"].clone()}))
             for k, h in heads.items()]
    try:
        _, losses, _ = _run(model, dev)
    finally:
        for h in hooks:
            h.remove()
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in losses.items()}, grads, matched


def test_model_step_rotated_fused_against_the_pytorch_losses(dev, monkeypatch):
    monkeypatch.setenv("EFG_DETERMINISTIC", "1")
    rotated = {"model.loss.giou_type": "rotated"}
    fused, _, m_fused = _model_step(dev, rotated)
    monkeypatch.setenv("EFG_FUSED_LOSS", "0")
    plain, _, m_plain = _model_step(dev, rotated)
    assert set(fused) == set(plain) and any("giou" in k for k in fused)
    worst = max((abs(float(fused[k]) - float(plain[k])), k) for k in fused)
    print("rotated step, fused against EFG_FUSED_LOSS=0: worst term %s off by %.3g" % (worst[1], worst[0]))
    for k in fused:
        assert abs(float(fused[k]) - float(plain[k])) <= 1e-4 * max(1.0, abs(float(plain[k]))), k
    for k in m_fused:
        assert torch.equal(m_fused[k], m_plain[k]), k


def test_model_step_without_the_key_is_bit_identical_to_aligned(dev, monkeypatch):
    monkeypatch.setenv("EFG_DETERMINISTIC", "1")
    absent_l, absent_g, absent_m = _model_step(dev, None)
    aligned_l, aligned_g, aligned_m = _model_step(dev, {"model.loss.giou_type": "aligned"})
    assert set(absent_l) == set(aligned_l) and set(absent_g) == set(aligned_g) and len(absent_g) > 100
    for k in absent_l:
        assert torch.equal(absent_l[k], aligned_l[k]), k
    for k in absent_g:
        assert torch.equal(absent_g[k], aligned_g[k]), k
    for k in absent_m:
        assert torch.equal(absent_m[k], aligned_m[k]), k
