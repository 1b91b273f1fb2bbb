"""GPU: CenterPoint inference with the circular NMS as a device chain (csrc/center_decode.hip) against the host
formulation (efg_amd/centerpoint/circular_host.py, pinned to the reference's own code by tests/test_center_circular_ref.py).

Bars.  Kept lists, their order and the labels are identical; scores within 1e-5 and boxes within 1e-4 (the tolerances of
tests/test_centerpoint_golden.py::_check_inference; sigmoid, exp and atan2 may differ in the last bits between the device
and torch's CPU kernels).  The fixture keeps every decision away from those last bits by construction; in the dyadic
family every fp32 operation of the centre and distance arithmetic is exact, so the two sides agree even where the squared
distance equals the radius -- no case is skipped or filtered."""
import types

import numpy as np
import pytest
import torch

import center_circular_cases as cases

pytestmark = pytest.mark.gpu

_HOST = {}


def host(key, preds, pp, num_classes):
    """The host formulation's result of a case: computed once."""
    from efg_amd.centerpoint.circular_host import predict_circular_host

    if key not in _HOST:
        _HOST[key] = predict_circular_host(preds, pp, num_classes)
    return _HOST[key]


def device(preds, pp, num_classes, dev):
    from efg_amd.operators.center_decode import predict_circular_device

    return predict_circular_device(cases.to(preds, dev), pp, num_classes)


def test_fixture_from_the_reference(dev):
    preds, pp, num_classes, ref = cases.fixture()
    cases.same_results(device(preds, pp, num_classes, dev), ref)


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_cases(dev, name):
    preds, pp, num_classes, expected = cases.hand_cases()[name]
    got = device(preds, pp, num_classes, dev)
    cases.check_expected(got, expected)
    cases.same_results(got, host(("hand", name), preds, pp, num_classes))


@pytest.mark.parametrize("name", sorted(cases.DYADIC))
def test_dyadic_family(dev, name):
    from efg_amd.operators.center_decode import center_predict_circular

    preds, pp, num_classes = cases.dyadic(name)
    want = host(("dyadic", name), preds, pp, num_classes)
    got = device(preds, pp, num_classes, dev)
    cases.same_results(got, want)
    batch, h, w, classes, radii, post_max, n_cand, vel = cases.DYADIC[name]
    assert all(r["boxes3d"].shape[1] == (9 if vel else 7) for r in got)
    # the centres are exact on both sides
    assert all(torch.equal(g["boxes3d"][:, :3], w["boxes3d"][:, :3]) for g, w in zip(got, want))
    boxes, scores, labels, counts = center_predict_circular(cases.to(preds, dev), pp, num_classes)
    assert boxes.shape == (batch, len(classes) * post_max, 9 if vel else 7) and counts.shape == (batch, len(classes))
    assert boxes.is_cuda and scores.is_cuda and labels.is_cuda and counts.is_cuda
    counts = counts.cpu()
    assert int(counts.sum()) == sum(len(r["scores"]) for r in want) and int(counts.max()) <= post_max
    if name == "40x40_all":
        full = cases.post_process(radii, post_max=h * w)       # untruncated: more survivors than post_max_size
        assert len(host(("dyadic", name, "full"), preds, full, num_classes)[0]["scores"]) > post_max == int(counts[0, 0])
    if name == "16x16_few":
        assert int(counts.max()) <= 12
    # a squared distance EQUAL to the radius occurs between a kept box and a candidate (it then suppresses)
    if name in ("12x20_b3", "40x40_all"):
        cand = _candidate_centres(preds[0], pp)
        kept = want[0]["boxes3d"][want[0]["labels"] <= classes[0], :2]
        d2 = ((kept[:, None, :] - cand[None, :, :]) ** 2).sum(-1)
        assert (d2 == radii[0]).any()


def _candidate_centres(maps, pp):
    """Centres of scene 0's candidates of one task (dyadic family: exact in fp32)."""
    hm = torch.sigmoid(maps["hm"][0]).amax(0).reshape(-1)
    h, w = maps["hm"].shape[2:]
    iy, ix = np.divmod(np.arange(h * w), w)
    x = (torch.from_numpy(ix).float() + maps["reg"][0, 0].reshape(-1)) * 2.0 - 16.0
    y = (torch.from_numpy(iy).float() + maps["reg"][0, 1].reshape(-1)) * 2.0 - 16.0
    z = maps["height"][0, 0].reshape(-1)
    lim = pp.post_center_limit_range
    ok = (hm > pp.score_threshold) & (z >= lim[2]) & (z <= lim[5])
    return torch.stack([x, y], 1)[ok]


@pytest.mark.parametrize("n", [0, 1, 65, 1600])
def test_circle_nms_stand_alone(dev, n):
    from efg_amd.centerpoint.circular_host import circle_nms_host
    from efg_amd.operators.center_decode import circle_nms

    rng = np.random.default_rng(n)
    xy = rng.integers(0, 160, (n, 2)) / 4.0                      # multiples of 1/4 in [0, 40): exact squared distances
    score = rng.permutation(np.linspace(0.05, 0.95, n))
    boxes = torch.from_numpy(np.concatenate([xy, score[:, None]], 1).astype(np.float32))
    for radius, post_max in ((4.0, 83), (1.0, 2000)):
        got = circle_nms(boxes.to(dev), radius, post_max_size=post_max)
        want = circle_nms_host(boxes[:, 0].numpy(), boxes[:, 1].numpy(), boxes[:, 2].numpy(), radius, post_max)
        assert got.is_cuda and got.dtype == torch.int64
        assert got.cpu().tolist() == want.tolist()
        assert n < 1600 or (len(want) == 83 if post_max == 83 else len(want) > 83)
    if n:
        assert circle_nms(boxes.to(dev), 4.0).cpu().tolist() == circle_nms_host(*boxes.numpy().T, 4.0).tolist()   # default 83


def test_circle_nms_equal_scores_go_by_index(dev):
    from efg_amd.centerpoint.circular_host import circle_nms_host
    from efg_amd.operators.center_decode import circle_nms

    rng = np.random.default_rng(3)
    xy = rng.integers(0, 80, (300, 2)) / 4.0
    score = rng.integers(1, 5, 300) / 8.0                       # four distinct scores: long runs of equal ones
    boxes = torch.from_numpy(np.concatenate([xy, score[:, None]], 1).astype(np.float32))
    got = circle_nms(boxes.to(dev), 4.0, post_max_size=300).cpu().tolist()
    assert got == circle_nms_host(*boxes.numpy().T, 4.0, 300).tolist()
    s = boxes[got, 2].tolist()
    assert s == sorted(s, reverse=True) and len(set(s)) > 1
    for v in set(s):                                             # inside a run of equal scores the indices ascend
        run = [i for i in got if boxes[i, 2] == v]
        assert run == sorted(run) and len(run) > 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        circle_nms(boxes, 4.0)


def test_limit_is_an_error_not_a_truncation(dev, monkeypatch):
    from efg_amd import _lib
    from efg_amd.operators import center_decode as ops

    lib = _lib.lib()
    limit = ops.max_cells()
    assert limit == 36864
    h, w = 193, 192                                              # 37 056 cells
    preds = [{"hm": torch.zeros(1, 1, h, w, device=dev), "reg": torch.zeros(1, 2, h, w, device=dev),
              "height": torch.zeros(1, 1, h, w, device=dev), "dim": torch.zeros(1, 3, h, w, device=dev),
              "rot": torch.zeros(1, 2, h, w, device=dev)}]
    monkeypatch.setattr(_lib, "lib", lambda: types.SimpleNamespace(efg_center_decode_max_cells=lib.efg_center_decode_max_cells))
    with pytest.raises(RuntimeError, match="37056 cells in one list exceed the limit of 36864"):
        ops.center_predict_circular(preds, cases.post_process([4.0]), [1])   # on the host: the stand-in has no kernel
    with pytest.raises(RuntimeError, match="36865 cells in one list exceed the limit of 36864"):
        ops.circle_nms(torch.zeros(limit + 1, 3, device=dev), 4.0)


def test_chain_makes_no_host_wait(dev):
    from efg_amd.operators.center_decode import center_predict_circular

    preds, pp, num_classes = cases.dyadic("12x20_b3")
    preds = cases.to(preds, dev)
    center_predict_circular(preds, pp, num_classes)             # (loads the library and the code object)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = center_predict_circular(preds, pp, num_classes)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert len(out) == 4 and all(t.is_cuda for t in out)
    assert int(out[3].sum()) == sum(len(r["scores"]) for r in host(("dyadic", "12x20_b3"), *cases.dyadic("12x20_b3")))


# ---- end to end -----------------------------------------------------------------------------------------------------
class _HeadModel(torch.nn.Module):
    """A CenterHead over given BEV maps: what VoxelNet.forward does behind its neck."""

    def __init__(self, head, post_process):
        super().__init__()
        self.center_head, self.post_process = head, post_process
        self.maps = []

    def forward(self, batched_inputs):
        x = torch.stack([b[0]["bev"] for b in batched_inputs])
        preds = self.center_head(x)
        self.maps.append([{k: v.detach().cpu() for k, v in p.items()} for p in preds])
        return self.center_head.predict({}, preds, self.post_process)


def circular_nuscenes_head(dev):
    """The six-task, ten-class nuScenes layout (tasks of 1, 2, 2, 1, 2, 2 classes, `vel` among the common heads) over a
    16 x 16 BEV map of 3.2 m cells, deterministic weights, `circular_nms: True`."""
    import nusc_eval_cases as nusc
    from golden_init import deterministic_state

    from efg_amd.centerpoint.center_head import CenterHead
    from efg_amd.config import to_attr

    names = nusc.CLASSES
    tasks = [{"num_classes": len(t), "class_names": list(t)} for t in (names[0:1], names[1:3], names[3:5], names[5:6],
                                                                       names[6:8], names[8:10])]
    cfg = to_attr({"model": {
        "neck": {"norm": "BN"},
        "head": {"in_channels": 32, "tasks": tasks,
                 "misc": {"dataset": "nuscenes", "weight": 0.25, "code_weights": [1.0] * 8 + [0.2, 0.2],
                          "common_heads": {"reg": [2, 2], "height": [1, 2], "dim": [3, 2], "rot": [2, 2], "vel": [2, 2]}}},
        "post_process": {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                         "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": 80, "nms_iou_threshold": 0.2},
                         "score_threshold": 0.1, "pc_range": [-25.6, -25.6], "out_size_factor": 8, "voxel_size": [0.4, 0.4],
                         "circular_nms": True, "min_radius": [4, 12, 10, 1, 0.85, 0.175]}}})
    torch.manual_seed(0)
    head = CenterHead(cfg)
    head.load_state_dict(deterministic_state(head.state_dict()), strict=True)
    return _HeadModel(head.to(dev), cfg.model.post_process), cfg


def test_circular_head_through_the_inference_loop(dev):
    import nusc_eval_cases as nusc

    from efg_amd.evaluator import NuScenesDetEvaluator, inference_on_dataset

    model, cfg = circular_nuscenes_head(dev)
    rng = np.random.default_rng(11)
    g = torch.Generator().manual_seed(5)
    loader = [[({"bev": torch.randn(32, 16, 16, generator=g).to(dev)}, nusc.synthetic_frame(rng, 30, extent=18.0)[0][1])
               for _ in range(2)] for _ in range(2)]
    seen = []

    class Spy(NuScenesDetEvaluator):
        def process(self, inputs, outputs):
            seen.append((inputs, outputs))
            super().process(inputs, outputs)

    ev = Spy(classes=nusc.CLASSES, meta=nusc.meta(), device=dev)
    got = inference_on_dataset(model, loader, ev)
    outputs = [o for _, outs in seen for o in outs]
    assert len(outputs) == 4 and all(set(o) == {"scores", "labels", "boxes3d"} for o in outputs)
    assert all(o["boxes3d"].shape[1] == 9 and len(o["scores"]) > 10 for o in outputs)
    labels = torch.cat([o["labels"] for o in outputs])
    assert int(labels.min()) >= 1 and int(labels.max()) <= 10
    host_ev = NuScenesDetEvaluator(classes=nusc.CLASSES, meta=nusc.meta(), device="cpu")
    for inputs, outs in seen:
        host_ev.process(inputs, outs)
    want = host_ev.evaluate()
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.isnan(got[k]) == np.isnan(want[k]), k
        assert np.isnan(want[k]) or abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
    # the same head over the same maps on the CPU: the host formulation
    on_cpu = [r for maps in model.maps for r in model.center_head.predict({}, maps, model.post_process)]
    cases.same_results(outputs, on_cpu)
