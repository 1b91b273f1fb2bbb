"""GPU: the detection-evaluation kernels (csrc/det_eval.hip) and the evaluator's device path against the fp64 host
formulation (pinned by tests/test_det_eval_ref.py) on crowded synthetic frames: clusters of pedestrians and cyclists, 0-3
jittered detections per object, clutter, 5 % wrong labels; frames without predictions, without ground truths, without a
class, with more and with fewer predictions than ground truths, one 65 x 65 problem of a single class (more than one wave
of columns, more than one 64-row tile) and one problem with 1024 predictions (the kernel's limit).

Bars.  Weights: bit for bit boxes_iou3d_gpu (the same code).  Matching: counts equal to scipy's on the device's own fp32
weights at all 101 cutoffs, matched weight within 1e-12 (1 + total) of scipy's optimum (fp64 sums of the same fp32 numbers in
another order).  End to end: on seeds whose fp64 IoUs all stay 1e-4 away from their class threshold (asserted first) and whose
optimal pairings do not depend on which of the two IoU functions weighs them (det_eval_cases.py E2E_SEEDS), counts equal, AP within 1e-12 (the same integers), APH within 1e-6 (heading accuracy is rounded to 2^-30 on both sides and summed
exactly; the headings are the same float32 numbers)."""
import numpy as np
import pytest
import torch

import det_eval_cases as cases
from det_eval_cases import KEYS, PEDESTRIAN

pytestmark = pytest.mark.gpu

SEEDS, MATCH_SEED = cases.E2E_SEEDS, cases.MATCH_SEED      # chosen on the CPU: see det_eval_cases.py
_CACHE = {}


@pytest.fixture(autouse=True)
def _leave_the_global_generators_alone():
    cpu = torch.get_rng_state()
    gpu = torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if gpu is not None:
        torch.cuda.set_rng_state_all(gpu)


def frames_of(seed):
    if ("frames", seed) not in _CACHE:
        _CACHE["frames", seed] = cases.device_test_frames(seed)
    return _CACHE["frames", seed]


def host_result(seed):
    if ("host", seed) not in _CACHE:
        _CACHE["host", seed] = cases.run(frames_of(seed), torch.device("cpu"))
    return _CACHE["host", seed]


def device_problem(seed, dev):
    """The prepared frames of `seed` on the device with the kernels' outputs -- computed once."""
    if ("device", seed) not in _CACHE:
        from efg_amd.evaluator import WaymoDetEvaluator
        from efg_amd.operators import det_eval as ops

        frames = frames_of(seed)
        prep = WaymoDetEvaluator(device=dev)._prepare([f[0] for f in frames], [f[1] for f in frames])
        pred_off = np.concatenate(([0], np.cumsum([len(f["ps"]) for f in prep])))
        gt_off = np.concatenate(([0], np.cumsum([len(f["gl"]) for f in prep])))
        problems = []
        for i, f in enumerate(prep):
            for c in range(3):
                p0, p1 = np.searchsorted(f["pl"], [c + 1, c + 2])
                g0, g1 = np.searchsorted(f["gl"], [c + 1, c + 2])
                problems.append((i, pred_off[i] + p0, p1 - p0, gt_off[i] + g0, g1 - g0, c))
        problems = np.array(problems, dtype=np.int64)

        def up(key, dtype, tail=()):
            return torch.from_numpy(np.concatenate([f[key] for f in prep]).astype(dtype).reshape((-1,) + tail)).to(dev)

        pb, gb = up("pb", np.float32, (7,)), up("gb", np.float32, (7,))
        weights, blk = ops.pair_weights(pb, up("pl", np.int32), pred_off, gb, up("gl", np.int32), gt_off)
        counts, sums, _ = ops.prefix_assign(weights, blk, pred_off, gt_off, problems, up("ps", np.float32), pb, gb,
                                            up("level", np.int32))
        torch.cuda.synchronize()
        _CACHE["device", seed] = dict(prep=prep, pred_off=pred_off, gt_off=gt_off, problems=problems, pb=pb, gb=gb,
                                      weights=weights, blk=blk, counts=counts.cpu().numpy(), sums=sums.cpu().numpy())
    return _CACHE["device", seed]


def test_frames_cover_the_shapes():
    d = [(len(f[1]["scores"]), len(f[0][1]["annotations"]["labels"])) for f in frames_of(SEEDS[0])]
    assert any(p == 0 and g > 0 for p, g in d) and any(g == 0 and p > 0 for p, g in d)
    assert any(p > g > 0 for p, g in d) and any(0 < p < g for p, g in d)
    assert (65, 65) in d and d[-1][0] == 1024


def test_weights_equal_boxes_iou3d_bit_for_bit(dev):
    from efg_amd.operators import det_eval as ops
    from efg_amd.operators.iou3d_nms import boxes_iou3d_gpu

    d = device_problem(MATCH_SEED, dev)
    thr = torch.tensor((0.0,) + ops.IOU_THRESHOLDS, device=dev)
    n_adm = n_below = 0
    for i, f in enumerate(d["prep"]):
        p, g = len(f["ps"]), len(f["gl"])
        if p == 0 or g == 0:
            assert d["blk"][i + 1] == d["blk"][i]
            continue
        got = d["weights"][d["blk"][i]:d["blk"][i + 1]].view(p, g)
        iou = boxes_iou3d_gpu(d["pb"][d["pred_off"][i]:d["pred_off"][i + 1]], d["gb"][d["gt_off"][i]:d["gt_off"][i + 1]])
        pl, gl = torch.from_numpy(f["pl"]).to(dev), torch.from_numpy(f["gl"]).to(dev)
        adm = (pl[:, None] == gl[None, :]) & (iou >= thr[pl][:, None]) & torch.isfinite(iou)
        assert torch.equal(got[adm].view(torch.int32), iou[adm].view(torch.int32))
        assert (got[~adm].view(torch.int32) == 0).all()           # exactly +0
        n_adm += int(adm.sum())
        n_below += int(((iou > 0) & ~adm).sum())
    assert n_adm > 100 and n_below > 100                          # both kinds of entries were seen


def test_matching_equals_scipy_on_the_device_weights(dev):
    from scipy.optimize import linear_sum_assignment

    from efg_amd.evaluator.waymo import heading_accuracy, score_cutoffs

    d = device_problem(MATCH_SEED, dev)
    weights, cutoffs = d["weights"].cpu().numpy().astype(np.float64), score_cutoffs()
    greedy_differs = 0
    for p, (i, r0, n_pred, g0, n_gt, c) in enumerate(d["problems"]):
        f = d["prep"][i]
        gf = len(f["gl"])
        block = weights[d["blk"][i]:d["blk"][i + 1]].reshape(len(f["ps"]), gf)
        lr, lg = r0 - d["pred_off"][i], g0 - d["gt_off"][i]
        w, ps, level = block[lr:lr + n_pred, lg:lg + n_gt], f["ps"][lr:lr + n_pred], f["level"][lg:lg + n_gt]
        done = None
        for k in range(101):
            n = int(np.count_nonzero(ps >= cutoffs[k]))
            if done is None or done[0] != n:
                rows, cols = linear_sum_assignment(w[:n], maximize=True) if n and n_gt else ((), ())
                rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
                hit = w[rows, cols] > 0
                rows, cols = rows[hit], cols[hit]
                matched = np.zeros(n_gt, bool)
                matched[cols] = True
                acc = heading_accuracy(f["pb"][lr + rows, 6], f["gb"][lg + cols, 6])
                done = (n, [(level[cols] <= 1).sum(), (level[cols] <= 2).sum(), n - len(rows),
                            (~matched & (level <= 1)).sum(), (~matched & (level <= 2)).sum()], w[rows, cols].sum(),
                        [acc[level[cols] <= 1].sum(), acc[level[cols] <= 2].sum()])
            assert d["counts"][p, k].tolist() == [int(v) for v in done[1]], (p, k)
            assert abs(d["sums"][p, k, 2] - done[2]) <= 1e-12 * (1 + done[2]), (p, k)
            assert d["sums"][p, k, :2].tolist() == done[3], (p, k)     # grid-rounded heading accuracies: exact sums
        greedy_differs += int((cases.greedy_counts(w, ps, level) != d["counts"][p, :, 1]).sum())
    assert greedy_differs > 0       # a score-first greedy kernel does not pass


@pytest.mark.parametrize("seed", SEEDS)
def test_end_to_end_equals_the_host_formulation(dev, seed):
    want = host_result(seed)
    margin = want["evaluator"].min_threshold_margin
    print("seed %d: min |IoU - threshold| of the fp64 formulation %.3e" % (seed, margin))
    assert margin > 1e-4            # the condition of the comparison: no pair within 1e-4 of its class threshold
    got = cases.run(frames_of(seed), dev)
    assert got["evaluator"]._counts.is_cuda
    assert torch.equal(got["counts"][..., :3], want["counts"][..., :3])
    assert want["counts"][..., 0].sum() > 1000
    for k in KEYS:
        print("%s device %.9f host %.9f" % (k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= (1e-12 if k.endswith("/AP") else 1e-6), k


HAND = {"perfect": cases.perfect, "heading_flip": cases.heading_flip, "no_predictions": cases.no_predictions,
        "no_cyclist_gt": cases.no_cyclist_gt, "greedy": cases.greedy_is_not_optimal,
        "levels_both": lambda: cases.levels(True), "levels_hard_only": lambda: cases.levels(False),
        "score_edges": cases.score_edges, "masks": cases.masks}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(dev, name):
    got, want = cases.run(HAND[name](), dev), cases.run(HAND[name](), torch.device("cpu"))
    assert got["evaluator"]._counts.is_cuda
    assert torch.equal(got["counts"][..., :3], want["counts"][..., :3])
    for k in KEYS:
        assert abs(got[k] - want[k]) <= (1e-12 if k.endswith("/AP") else 1e-6), k
    if name == "greedy":
        row = got["counts"][PEDESTRIAN - 1, 0].numpy()
        assert (row[:81, :3] == [2, 0, 0]).all() and (row[81:91, :3] == [1, 0, 1]).all() and (row[91:, :3] == [0, 0, 2]).all()
        assert got["OBJECT_TYPE_TYPE_PEDESTRIAN_LEVEL_1/AP"] == pytest.approx(1.0, abs=1e-12)
    if name == "perfect":
        assert all(got[k] == pytest.approx(1.0, abs=1e-12) for k in KEYS)
    if name == "levels_hard_only":
        assert (got["counts"][PEDESTRIAN - 1, 0, :71, :3].numpy() == [0, 0, 1]).all()
        assert (got["counts"][PEDESTRIAN - 1, 1, :71, :3].numpy() == [1, 0, 1]).all()


def test_streaming_and_determinism(dev):
    frames = frames_of(MATCH_SEED)[:8]
    runs = [cases.run(frames, dev), cases.run(frames, dev, chunk=2), cases.run(frames, dev)]
    first = runs[0]["evaluator"]
    assert first._counts.sum() > 0
    for r in runs[1:]:
        assert torch.equal(r["evaluator"]._counts, first._counts)
        assert torch.equal(r["evaluator"]._sums.view(torch.int64), first._sums.view(torch.int64))
        assert torch.equal(r["counts"].view(torch.int64), runs[0]["counts"].view(torch.int64))


def test_limit_is_an_error_not_a_truncation(dev):
    inp, out = cases.many_predictions_frame(SEEDS[0], n_pred=1025)
    from efg_amd.evaluator import WaymoDetEvaluator

    ev = WaymoDetEvaluator(device=dev)
    with pytest.raises(RuntimeError, match="1025 predictions of one class in one frame exceed the limit of 1024"):
        ev.process([inp], [out])
    assert int(ev._counts.sum()) == 0


def test_model_smoke(dev):
    """The small ConQueR of the golden tests in eval mode over two synthetic scenes."""
    from golden_init import INFER_OVERRIDES, full_inputs
    from test_model_full_golden import _build

    from efg_amd.evaluator import WaymoDetEvaluator, inference_on_dataset

    model, _ = _build(dev, full_graph=False, extra=INFER_OVERRIDES)
    points_list, annos = full_inputs()
    loader = [[({"points": torch.from_numpy(p).to(dev)}, {"annotations": a})] for p, a in zip(points_list, annos)]
    res = inference_on_dataset(model, loader, WaymoDetEvaluator(device=dev))
    assert model.training                                   # the mode it came in with is restored
    assert sorted(k for k in res if k != "counts") == sorted(KEYS)
    for k in KEYS:
        assert np.isfinite(res[k]) and 0.0 <= res[k] <= 1.0, (k, res[k])
    assert res["counts"].shape == (3, 2, 101, 4)
