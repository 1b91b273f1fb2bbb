"""The bits of the matching-cost, box-loss and paired rotated-GIoU kernels (csrc/det_loss.hip, csrc/rot_giou.hip over
csrc/giou3d.h) on fixed inputs, and their launch times.  GPU box.

  python scripts/record_det_loss_bits.py                 print the SHA-256 of every case's output bytes, compare with the fixture
  python scripts/record_det_loss_bits.py --write         and write them to tests/golden/det_loss_bits.json
  python scripts/record_det_loss_bits.py --time          one round of launch times at the training shape (one JSON line)
  ... --tree DIR                                         import efg_amd from DIR (another checkout, built) instead of this one

tests/golden/det_loss_bits.json was written ONCE, by the build of the commit before the axis-aligned and the rotated kernels
became one templated source (066a8e9: match cost, box-loss sum and box-loss gradient twice, in det_loss.hip and in
rot_giou.hip), and tests/test_det_loss_bits_gpu.py holds every later build to it: same operations in the same order, same
reduction tree, same guards.  A change that moves a hash changed the arithmetic; the fixture is not re-recorded to follow it.
The matching cost goes through expf, powf and logf of the device library, so the fixture belongs to the ROCm release it
names ("rocm").

Everything goes through operators.det_loss.match_cost, Det3DLoss._layer_losses and operators.rot_giou.rot_giou_paired, whose
signatures are the same before and after that change.  Inputs are integer arithmetic on torch.arange (no random generator):
targets of 0.6 to 5 m in the code frame, as tests/test_rot_giou_gpu.py::box_case, and predictions a few percent off them, so
the GIoU terms are away from 0 and -1."""
import argparse
import hashlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "det_loss_bits.json")
RECORDED_AT = "066a8e9"
# variant -> (giou_type, frame)
VARIANTS = {"aligned": ("aligned", None),
            "rotated_code": ("rotated", (150.4, 150.4, 2 * math.pi, -math.pi)),
            "rotated_metric": ("rotated", (1.0, 1.0, 1.0, 0.0))}
WEIGHTS = (1.0, 4.0, 2.0, 4.0)     # w_class, w_bbox, w_giou, w_rad
_MOD = 16777213                    # the largest prime under 2^24: v / 2^24 is an exact fp32 number


def unit(shape, salt):
    """fp32 host tensor of `shape`, values in [0, 1)."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    v = (i * i * 7919 + i * 104729 + (i % 7) * 15485863 + salt * 1299709 + 12345) % _MOD
    return (v.to(torch.float32) * 2.0 ** -24).view(shape)


def targets(b, g, salt):
    """[b, g, 7] target codes: centres inside the range, 0.6 .. 5.1 m long and wide in the code frame."""
    t = unit((b, g, 7), salt)
    t[..., :2] = 0.2 + 0.6 * t[..., :2]
    t[..., 3:5] = 0.004 + 0.03 * t[..., 3:5]
    t[..., 5] = 0.05 + 0.1 * t[..., 5]
    return t


def near(t, salt):
    """Boxes a few percent off the boxes t [..., 7]."""
    scale = torch.tensor([0.01, 0.01, 0.05, 0.01, 0.01, 0.05, 0.2])
    return (t + (unit(tuple(t.shape), salt) - 0.5) * scale).clamp(min=1e-3)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def cost_inputs(nl, b, q, c, g, padded, salt, dev):
    """Query q of every layer and scene sits near target q % g of its scene."""
    tgt = targets(b, g, salt)
    if padded:
        tgt[:, -1] = 0
    boxes = near(tgt[:, torch.arange(q) % g][None].expand(nl, b, q, 7).contiguous(), salt + 1)
    logits = unit((nl, b, q, c), salt + 2) * 8 - 4
    labels = (torch.arange(b * g, dtype=torch.int64) * 5 % c).view(b, g)
    return logits.to(dev), boxes.to(dev), labels.to(dev), tgt.to(dev)


def box_inputs(n, salt, dev, nl=3, b=2, q=200, g=9):
    """n matched pairs on distinct (layer, scene, query) rows (n <= nl * b * q), the predictions near their targets; from
    n >= 3 on three of the pairs are unmatched columns (q = -1)."""
    tgt = targets(b, g, salt)
    boxes = unit((nl, b, q, 7), salt + 1)
    rows = (torch.arange(n, dtype=torch.int64) * 7 + 3) % (nl * b * q)      # 7 is coprime to the row count
    assert n <= nl * b * q and (nl * b * q) % 7 != 0 and len(set(rows.tolist())) == n
    li, bi, qi = rows // (b * q), (rows // q) % b, rows % q
    gi = (torch.arange(n, dtype=torch.int64) * 4 + 1) % g
    boxes[li, bi, qi] = near(tgt[bi, gi], salt + 2)
    if n >= 3:
        qi[torch.tensor([n // 200, n // 2, n - 1])] = -1
    weight = 0.5 + unit((3 * nl,), salt + 3)                                  # of the [3 L] family-major loss vector
    return boxes.to(dev), tgt.to(dev), [t.to(dev) for t in (li, bi, qi, gi)], weight.to(dev)


def box_loss(det, boxes, tgt, sel, weight, giou_type, frame, denom):
    """([3 L] sums / denom, gradient to the boxes) through Det3DLoss._layer_losses."""
    loss = det.Det3DLoss(matcher=None, weight_dict={}, losses=["boxes"], giou_type=giou_type, frame=frame)
    bx = boxes.clone().requires_grad_(True)
    labels = torch.zeros(tgt.shape[:2], dtype=torch.int64, device=tgt.device)
    out, _ = loss._layer_losses(None, bx, sel, labels, tgt, denom, parts=("box",))
    sums = out["loss_bbox|loss_giou|loss_rad"]
    (sums * weight).sum().backward()
    return sums.detach(), bx.grad


def cases(variant):
    """{case: output tensor} of one variant, on the smallest shapes that reach every branch of the kernels."""
    from efg_amd.detection3d import losses as det
    from efg_amd.operators.det_loss import match_cost
    from efg_amd.operators.rot_giou import rot_giou_paired

    giou_type, frame = VARIANTS[variant]
    dev = torch.device("cuda")
    out = {}
    # 1400 entries: six 256-thread blocks, the last one ragged; then a padded (all-zero) last target column
    for name, shape, padded in (("match_cost_2_2_70_3_5", (2, 2, 70, 3, 5), False),
                                ("match_cost_padded_1_2_70_3_17", (1, 2, 70, 3, 17), True)):
        logits, boxes, labels, tgt = cost_inputs(*shape, padded, 10 + shape[4], dev)
        out[name] = match_cost(logits, boxes, labels, tgt, *WEIGHTS, giou_type=giou_type, frame=frame)
    # one pair; then 1100: the 1024-thread workgroup's strided loop runs twice, the second time ragged
    for n in (1, 1100):
        boxes, tgt, sel, weight = box_inputs(n, 20 + n, dev)
        out["box_loss_sums_n%d" % n], out["box_loss_grad_n%d" % n] = box_loss(det, boxes, tgt, sel, weight, giou_type, frame,
                                                                              float(n))
    if frame is not None:
        b = targets(1, 65, 30)[0]
        a = near(b, 31)
        a, b = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        giou, iou = rot_giou_paired(a, b, frame)
        (giou * (0.5 + unit((65,), 32)).to(dev)).sum().backward()
        out["paired_giou_n65"], out["paired_iou_n65"], out["paired_grad_a_n65"], out["paired_grad_b_n65"] = giou, iou, a.grad, b.grad
    torch.cuda.synchronize()
    return out


def hashes():
    return {variant: {name: sha(t) for name, t in cases(variant).items()} for variant in VARIANTS}


# ---- launch times ---------------------------------------------------------------------------------------------------------
def replayed(fn, reps):
    """`reps` calls of fn captured into one device graph: replaying it runs their kernels without the host between them (the
    box loss through autograd is host-bound when launched call by call: ~100 us of Python for ~20 us of kernels)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    return graph.replay


def time_round(launches=200, batches=5, reps=10):
    """Median over `batches` of the device time of `launches` back-to-back calls (graph replays of `reps` calls each), in us
    per call, at the training shape 7 x 2 x 900 queries x 80 targets: the match cost, and the box loss forward + backward
    over the 7 x 2 x 80 matched pairs (with the few elementwise kernels autograd puts around the two)."""
    from efg_amd.detection3d import losses as det
    from efg_amd.operators.det_loss import match_cost

    dev = torch.device("cuda")
    nl, b, q, c, g = 7, 2, 900, 3, 80
    logits, boxes, labels, tgt = cost_inputs(nl, b, q, c, g, False, 40, dev)
    cost = torch.empty((nl * b, q, g), dtype=torch.float32, device=dev)
    n = nl * b * g
    i = torch.arange(n, dtype=torch.int64)
    sel = [t.to(dev) for t in (i // (b * g), (i // g) % b, (i % g) * 11 % q, i % g)]      # target g: query 11 g, near it
    matched = boxes.clone()
    matched[sel[0], sel[1], sel[2]] = near(tgt[sel[1], sel[3]].cpu(), 42).to(dev)
    weight = (0.5 + unit((3 * nl,), 41)).to(dev)
    denom = torch.tensor(float(n), device=dev)
    zeros = torch.zeros((b, g), dtype=torch.int64, device=dev)
    result = {}
    for variant, (giou_type, frame) in VARIANTS.items():
        if variant == "rotated_metric":
            continue
        loss = det.Det3DLoss(matcher=None, weight_dict={}, losses=["boxes"], giou_type=giou_type, frame=frame)
        bx = matched.clone().requires_grad_(True)

        def run_cost():
            match_cost(logits, boxes, labels, tgt, *WEIGHTS, out=cost, giou_type=giou_type, frame=frame)

        def run_box():
            bx.grad = None
            out, _ = loss._layer_losses(None, bx, sel, zeros, tgt, denom, parts=("box",))
            (out["loss_bbox|loss_giou|loss_rad"] * weight).sum().backward()

        for name, fn in (("match_cost", run_cost), ("box_loss_fwd_bwd", run_box)):
            replay = replayed(fn, reps)
            for _ in range(5):
                replay()
            times = []
            for _ in range(batches):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                for _ in range(launches // reps):
                    replay()
                stop.record()
                stop.synchronize()
                times.append(start.elapsed_time(stop) * 1e3 / (launches // reps * reps))
            result["%s_%s_us" % (name, variant)] = round(sorted(times)[len(times) // 2], 3)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write tests/golden/det_loss_bits.json (see the module docstring)")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--time", action="store_true", help="print one round of launch times as a JSON line instead")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import efg_amd from")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("record_det_loss_bits.py runs the kernels: no device found")
    if args.time:
        print(json.dumps(dict(tree=os.path.relpath(os.path.abspath(args.tree), ROOT), **time_round())))
        return 0
    got = {"recorded_at": RECORDED_AT, "rocm": torch.version.hip, "hashes": hashes()}
    print(json.dumps(got, indent=1))
    if args.write:
        with open(args.out, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
    elif os.path.exists(args.out):
        with open(args.out) as f:
            want = json.load(f)["hashes"]
        bad = [(v, name) for v in VARIANTS for name in got["hashes"][v] if want[v].get(name) != got["hashes"][v][name]]
        print("differs from %s: %s" % (os.path.relpath(args.out, ROOT), bad or "nothing"))
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
