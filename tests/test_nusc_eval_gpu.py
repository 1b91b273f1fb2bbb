"""GPU: the nuScenes-evaluation kernels (csrc/nusc_eval.hip) and the evaluator's device path against the fp64 host
formulation (pinned by tests/test_nusc_eval_ref.py) on synthetic frames (nusc_eval_cases.device_test_frames): clustered
objects of all ten classes, 0-3 jittered detections per object, clutter 0.3-5 m away, 5 % wrong labels, NaN ground-truth
velocities and empty attributes, and the shapes test_frames_cover_the_shapes lists.

Bars.  The distance is the same fp64 expression on the same float32 centres on both sides, built without contraction, so
`match` (all four thresholds) equals the host formulation's exactly, on every seed.  The five errors agree within 1e-12
relative with NaN in the same places (fp64 on both sides, a handful of operations; fmod and the division may differ in the last
bits).  End to end, every returned number within 1e-9."""
import math

import numpy as np
import pytest
import torch

import nusc_eval_cases as cases

pytestmark = pytest.mark.gpu

SEEDS = cases.SEEDS
_CACHE = {}


def frames_of(seed):
    if ("frames", seed) not in _CACHE:
        _CACHE["frames", seed] = cases.device_test_frames(seed)
    return _CACHE["frames", seed]


def prepared(seed):
    """(evaluator, prepared frames, problem table, the host formulation's records of the frames as one call)."""
    if ("host", seed) not in _CACHE:
        ev = cases.evaluator(torch.device("cpu"))
        frames = frames_of(seed)
        prep = ev._prepare([f[0] for f in frames], [f[1] for f in frames])
        _CACHE["host", seed] = (ev, prep, ev.problems(prep), {k: v.numpy() for k, v in ev.host_records(prep).items()})
    return _CACHE["host", seed]


def host_result(seed):
    if ("result", seed) not in _CACHE:
        _CACHE["result", seed] = cases.run(frames_of(seed), torch.device("cpu"))[0]
    return _CACHE["result", seed]


def close(got, want, tol):
    assert sorted(got) == sorted(want)
    for k in want:
        assert math.isnan(got[k]) == math.isnan(want[k]), k
        assert math.isnan(want[k]) or abs(got[k] - want[k]) <= tol, (k, got[k], want[k])


def test_frames_cover_the_shapes():
    from efg_amd.evaluator.nuscenes import centre_distances
    from efg_amd.operators import nusc_eval as ops

    ev, prep, problems, host = prepared(SEEDS[0])
    n_cls = len(cases.CLASSES)
    shapes = {(int(p), int(g)) for _, p, _, g, _ in problems}
    assert any(p == 0 and g > 0 for p, g in shapes) and any(g == 0 and p > 0 for p, g in shapes)
    assert any(g == 1 and p > 1 for p, g in shapes) and any(g == 65 and p > 0 for p, g in shapes)
    assert ops.max_gt() == 1024 and any(g == 1024 and p > 100 for p, g in shapes)
    assert any(p == 500 for p, g in shapes)
    per_frame = problems.reshape(len(prep), n_cls, 5)
    assert any((f[:, 3] > 0).all() and (f[:, 1] > 0).all() for f in per_frame)            # a frame holding all ten classes
    trailer = per_frame[:, cases.LABEL["trailer"] - 1]
    assert any(p > 0 and g == 0 for _, p, _, g, _ in trailer) and any(p == 0 and g > 0 for _, p, _, g, _ in trailer)
    tie = exact = False
    pb, gb = np.concatenate([f["pb"] for f in prep]), np.concatenate([f["gb"] for f in prep])
    for p0, n_p, g0, n_g, _ in problems:
        if 0 < n_p <= 8 and 0 < n_g <= 8:
            d = centre_distances(pb[p0:p0 + n_p, :2], gb[g0:g0 + n_g, :2])
            tie |= any(n_g > 1 and np.sort(row)[0] == np.sort(row)[1] for row in d)
            exact |= bool(np.isin(d, ev.thresholds).any())
    assert tie and exact
    # the data exercise what they should: both outcomes at every threshold, every kind of NaN
    assert all(((host["tp_bits"] >> t) & 1).sum() > 100 and ((~host["tp_bits"] >> t) & 1).sum() > 100 for t in range(4))
    matched = host["match"][ops.TP_THRESHOLD] >= 0
    assert np.isnan(host["err"][matched, 3]).sum() > 10 and np.isnan(host["err"][matched, 4]).sum() > 10
    assert not np.isnan(host["err"][matched, :3]).any() and np.isnan(host["err"][~matched]).all()
    assert len({int(b) for b in host["tp_bits"]}) >= 5                                    # the thresholds disagree


@pytest.mark.parametrize("seed", SEEDS)
def test_match_equals_the_host_formulation_exactly(dev, seed):
    ev, prep, problems, host = prepared(seed)
    got = ev.device_records(prep, dev)
    torch.cuda.synchronize()
    match = got["match"].cpu().numpy()
    differ = np.argwhere(match != host["match"])
    print("seed %d: %d predictions, %d matched at 2 m, %d entries differ" % (seed, match.shape[1], (match[2] >= 0).sum(),
                                                                           len(differ)))
    assert match.shape == host["match"].shape and len(differ) == 0, differ[:10]
    assert np.array_equal(got["tp_bits"].cpu().numpy(), host["tp_bits"])
    assert np.array_equal(got["cls"].cpu().numpy(), host["cls"]) and np.array_equal(got["score"].cpu().numpy(), host["score"])
    err = got["err"].cpu().numpy()
    assert np.array_equal(np.isnan(err), np.isnan(host["err"]))
    ok = ~np.isnan(err)
    rel = np.abs(err[ok] - host["err"][ok]) / np.maximum(np.abs(host["err"][ok]), 1e-300)
    rel[err[ok] == host["err"][ok]] = 0.0
    print("seed %d: largest relative error of the five errors %.3e over %d values" % (seed, rel.max(), rel.size))
    assert rel.max() <= 1e-12


@pytest.mark.parametrize("seed", SEEDS)
def test_end_to_end_equals_the_host_formulation(dev, seed):
    want = host_result(seed)
    got, ev = cases.run(frames_of(seed), dev)
    assert ev._records[0][3].is_cuda and ev._records[0][0].is_cuda
    assert want["mAP"] > 0.05 and 0.0 < want["NDS"] < 1.0
    print("seed %d: mAP device %.12f host %.12f, NDS device %.12f host %.12f" % (seed, got["mAP"], want["mAP"], got["NDS"],
                                                                           want["NDS"]))
    close(got, want, 1e-9)


def test_one_call_and_three_calls_are_identical(dev):
    frames = frames_of(SEEDS[0])
    (one, ev1), (three, ev3) = cases.run(frames, dev), cases.run(frames, dev, chunk=5)
    assert len(ev1._records) == 1 and len(ev3._records) == 3
    for a, b in zip(ev1.records(), ev3.records()):
        assert a.tobytes() == b.tobytes()
    close(three, one, 0.0)


def test_limit_is_an_error_not_a_truncation(dev, monkeypatch):
    import types

    from efg_amd import _lib

    inp, out = cases.too_many_ground_truths()
    ev = cases.evaluator(dev)
    lib = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: types.SimpleNamespace(efg_nusc_eval_max_gt=lib.efg_nusc_eval_max_gt))
    with pytest.raises(RuntimeError, match="1025 ground truths of one class in one frame exceed the limit of 1024"):
        ev.process([inp], [out])                # raised on the host: the stand-in library has no kernel to launch
    assert not ev._records and ev._npos.sum() == 0


def test_hand_cases(dev):
    for frames in ([cases.planted_frame()], [cases.frame([], [])], []):
        got, want = cases.run(frames, dev)[0], cases.run(frames, torch.device("cpu"))[0]
        close(got, want, 1e-9)


class _HeadModel(torch.nn.Module):
    """A CenterHead over given BEV maps: what VoxelNet.forward does behind its neck."""

    def __init__(self, head, post_process):
        super().__init__()
        self.center_head, self.post_process = head, post_process

    def forward(self, batched_inputs):
        x = torch.stack([b[0]["bev"] for b in batched_inputs])
        return self.center_head.predict({}, self.center_head(x), self.post_process)


def nuscenes_head(dev):
    """The six-task, ten-class nuScenes layout (tasks of 1, 2, 2, 1, 2, 2 classes, `vel` among the common heads) over a
    16 x 16 BEV map of 3.2 m cells, deterministic weights."""
    from golden_init import deterministic_state

    from efg_amd.centerpoint.center_head import CenterHead
    from efg_amd.config import to_attr

    names = cases.CLASSES
    tasks = [{"num_classes": len(t), "class_names": list(t)} for t in (names[0:1], names[1:3], names[3:5], names[5:6],
                                                                       names[6:8], names[8:10])]
    cfg = to_attr({"model": {
        "neck": {"norm": "BN"},
        "head": {"in_channels": 32, "tasks": tasks,
                 "misc": {"dataset": "nuscenes", "weight": 0.25, "code_weights": [1.0] * 8 + [0.2, 0.2],
                          "common_heads": {"reg": [2, 2], "height": [1, 2], "dim": [3, 2], "rot": [2, 2], "vel": [2, 2]}}},
        "post_process": {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                         "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": 80, "nms_iou_threshold": 0.2},
                         "score_threshold": 0.1, "pc_range": [-25.6, -25.6], "out_size_factor": 8, "voxel_size": [0.4, 0.4]}}})
    torch.manual_seed(0)
    head = CenterHead(cfg)
    head.load_state_dict(deterministic_state(head.state_dict()), strict=True)
    return _HeadModel(head.to(dev), cfg.model.post_process), cfg


def test_centerpoint_nuscenes_head_through_the_inference_loop(dev):
    from efg_amd.evaluator import NuScenesDetEvaluator, inference_on_dataset

    model, cfg = nuscenes_head(dev)
    rng = np.random.default_rng(11)
    g = torch.Generator().manual_seed(5)
    loader = [[({"bev": torch.randn(32, 16, 16, generator=g).to(dev)}, cases.synthetic_frame(rng, 30, extent=18.0)[0][1])
               for _ in range(2)] for _ in range(2)]
    seen = []

    class Spy(NuScenesDetEvaluator):
        def process(self, inputs, outputs):
            seen.append((inputs, outputs))
            super().process(inputs, outputs)

    ev = Spy(classes=cases.CLASSES, meta=cases.meta(), device=dev)
    got = inference_on_dataset(model, loader, ev)
    outputs = [o for _, outs in seen for o in outs]
    assert len(outputs) == 4 and all(set(o) == {"scores", "labels", "boxes3d"} for o in outputs)
    assert all(o["boxes3d"].shape[1] == 9 and len(o["scores"]) > 10 for o in outputs)
    labels = torch.cat([o["labels"] for o in outputs])
    assert int(labels.min()) >= 1 and int(labels.max()) <= 10 and len(labels.unique()) >= 6
    host = NuScenesDetEvaluator(classes=cases.CLASSES, meta=cases.meta(), device="cpu")
    for inputs, outs in seen:
        host.process(inputs, outs)
    want = host.evaluate()
    assert ev._records[0][3].is_cuda and sum(len(r[0]) for r in ev._records) > 40 and ev._npos.sum() > 40
    close(got, want, 1e-9)
