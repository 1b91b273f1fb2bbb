"""GPU: the tracking-evaluation kernel (csrc/track_eval.hip) and the evaluator's device path against the fp64 host
formulation (pinned by tests/test_track_eval_ref.py) on the synthetic sequences of track_eval_cases.py: 3 sequences x 12
frames of clustered pedestrians and cyclists whose tracks drop out, take fresh ids and swap ids, with ghosts and scores on
cutoffs; one frame with exactly 1024 pedestrian tracks (the kernel's limit) and one 65 x 65 problem (more than one wave of
columns).

Bars.  State machine: on the device's own float32 weights, copied back, the host state machine gives the same counts at
every (problem, cutoff), the same cost sums bit for bit (terms are rounded to 2^-30 on both sides and summed exactly) and
the same map `last`.  End to end: on seeds without a pair within 1e-4 of its class threshold (asserted first) and whose
table does not depend on the IoU function (track_eval_cases.E2E_SEEDS), integer totals equal, MOTA / MISS / MISMATCH / FP
within 1e-12 (the same integers), MOTP within track_eval_cases.MOTP_BOUND, the difference of the two IoU functions measured
on the CPU.  Hand cases: counts exact; the one pair of a case with a cost has it within 2e-6 of the closed form -- the
float32 pair function on axis-aligned unit boxes is an intersection, two volumes, a sum and a division, about a dozen
roundings of 2^-24 relative on values below 2."""
import numpy as np
import pytest
import torch

import track_eval_cases as cases
from det_eval_cases import PEDESTRIAN, box

pytestmark = pytest.mark.gpu

SEEDS, MATCH_SEED = cases.E2E_SEEDS, cases.MATCH_SEED      # chosen on the CPU: see track_eval_cases.py
DEVICE_COST_TOL = 2e-6
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
        _CACHE["frames", seed] = cases.sequences(seed)
    return _CACHE["frames", seed]


def host_result(seed):
    if ("host", seed) not in _CACHE:
        _CACHE["host", seed] = cases.run(cases.flat(frames_of(seed)), torch.device("cpu"))
    return _CACHE["host", seed]


def segments_of(seed, dev):
    """[(prepared frames of a whole sequence, number of its dense ground-truth ids)] -- the evaluator's own preparation,
    recorded where it would launch."""
    if ("segments", seed) not in _CACHE:
        from efg_amd.evaluator import WaymoTrackEvaluator

        class Recorder(WaymoTrackEvaluator):
            def _flush_device(self, frames):
                self.recorded.append((frames, len(self._gt_dense)))

        ev = Recorder(device=dev, flush_frames=10 ** 9)
        ev.recorded = []
        for inp, out in cases.flat(frames_of(seed)):
            ev.process([inp], [out])
        ev.evaluate()
        assert [len(s[0]) for s in ev.recorded] == [cases.N_FRAMES] * cases.N_SEQUENCES
        _CACHE["segments", seed] = ev.recorded
    return _CACHE["segments", seed]


def launch(segments, dev):
    """One launch over whole sequences, each with its own columns of a fresh `last` table."""
    from efg_amd.evaluator.waymo_track import device_mot, score_cutoffs
    from efg_amd.operators.track_eval import IOU_THRESHOLDS

    columns = np.concatenate(([0], np.cumsum([n for _, n in segments])))
    last = torch.full((11, int(columns[-1])), -1, dtype=torch.int32, device=dev)
    run = device_mot([(frames, int(col)) for (frames, _), col in zip(segments, columns)], score_cutoffs(), IOU_THRESHOLDS,
                     last, dev)
    torch.cuda.synchronize()
    return dict(run, last=last.cpu().numpy(), columns=columns, counts=run["counts"].cpu().numpy(),
                sums=run["sums"].cpu().numpy(), weights=run["weights"].cpu().numpy())


def test_state_machine_equals_the_host_one_on_the_device_weights(dev):
    from efg_amd.evaluator.waymo_track import class_ranges, clear_mot_frame, score_cutoffs

    segments = segments_of(MATCH_SEED, dev)
    run = launch(segments, dev)
    assert run["ranges"][:, PEDESTRIAN - 1, 1].max() == 1024                          # the limit
    assert (run["ranges"][:, PEDESTRIAN - 1, [1, 3]] == [65, 65]).all(1).any()       # more than one wave of columns
    cutoffs, first, plain_differs = score_cutoffs(), 0, 0
    for s, (frames, n_ids) in enumerate(segments):
        for c in range(3):
            last, plain_last = [{} for _ in cutoffs], [{} for _ in cutoffs]
            counts, sums = np.zeros((11, 9), np.int64), np.zeros((11, 2))
            plain = np.zeros((11, 9), np.int64)
            for i, f in enumerate(frames, first):
                p0, n_p, g0, n_g = class_ranges(f)[c]
                block = run["weights"][run["blk_off"][i]:run["blk_off"][i + 1]].reshape(len(f["ps"]), len(f["gl"]))
                args = (block[p0:p0 + n_p, g0:g0 + n_g], f["ps"][p0:p0 + n_p], f["td"][p0:p0 + n_p].tolist(),
                        f["gd"][g0:g0 + n_g].tolist(), f["level"][g0:g0 + n_g], cutoffs)
                got = clear_mot_frame(*args, last)
                counts += got[0]
                sums += got[1]
                plain += clear_mot_frame(*args, plain_last, carry_over=False)[0]
            assert run["counts"][3 * s + c].tolist() == counts.tolist(), (s, c)
            assert run["sums"][3 * s + c].view(np.int64).tolist() == sums.view(np.int64).tolist(), (s, c)
            for k in range(11):
                want = np.full(n_ids, -1, np.int64)
                for g, t in last[k].items():
                    want[g] = t
                mine = [g for f in frames for g in f["gd"][f["gl"] == c + 1]]        # the ids of this class
                got = run["last"][k, run["columns"][s]:run["columns"][s] + n_ids]
                assert got[mine].tolist() == want[mine].tolist(), (s, c, k)
            plain_differs += int((plain != counts).sum())
        first += len(frames)
    assert run["counts"][:, :, 5].sum() > 100 and run["counts"][:, :, 0].sum() > 1000
    assert plain_differs > 0          # a kernel without the carry-over step does not pass


@pytest.mark.parametrize("seed", SEEDS)
def test_end_to_end_equals_the_host_formulation(dev, seed):
    want = host_result(seed)
    margin = want["evaluator"].min_threshold_margin
    print("seed %d: min |IoU - threshold| of the fp64 formulation %.3e" % (seed, margin))
    assert margin > 1e-4            # the condition of the comparison: no pair within 1e-4 of its class threshold
    got = cases.run(cases.flat(frames_of(seed)), dev)
    assert got["evaluator"]._counts.is_cuda
    assert torch.equal(got["counts"], want["counts"])
    assert want["counts"][..., 0].sum() > 1000 and want["counts"][..., 5].sum() > 0
    assert torch.equal(got["score_cutoff"], want["score_cutoff"])
    for k in cases.KEYS:
        print("%s device %.9f host %.9f" % (k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= (cases.MOTP_BOUND if k.endswith("/MOTP") else 1e-12), k


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_cases(dev, name):
    frames, kw, _ = cases.hand_cases()[name]
    res = cases.run(frames, dev, **kw)
    assert res["evaluator"]._counts.is_cuda
    cases.check_hand_case(name, res, DEVICE_COST_TOL)


def test_chunking_and_determinism(dev):
    frames = cases.flat(frames_of(MATCH_SEED))
    runs = [cases.run(frames, dev), cases.run(frames, dev, flush_frames=5), cases.run(frames, dev)]
    first = runs[0]["evaluator"]
    assert first._counts.is_cuda and first._counts[..., 5].sum() > 0
    for r in runs[1:]:
        assert torch.equal(r["evaluator"]._counts, first._counts)
        assert torch.equal(r["evaluator"]._sums.view(torch.int64), first._sums.view(torch.int64))
        assert all(r[k] == runs[0][k] for k in cases.KEYS)


def test_two_sequences_in_one_launch_equal_two_launches(dev):
    a, b = segments_of(MATCH_SEED, dev)[1:]
    both, one_a, one_b = launch([a, b], dev), launch([a], dev), launch([b], dev)
    assert one_a["counts"][:, :, 0].sum() > 0 and one_b["counts"][:, :, 0].sum() > 0
    assert both["counts"].tolist() == np.concatenate((one_a["counts"], one_b["counts"])).tolist()
    assert both["sums"].view(np.int64).tolist() == np.concatenate((one_a["sums"], one_b["sums"])).view(np.int64).tolist()
    assert both["last"].tolist() == np.concatenate((one_a["last"], one_b["last"]), 1).tolist()


def test_limit_is_an_error_not_a_truncation(dev):
    from efg_amd.evaluator import WaymoTrackEvaluator

    rng = np.random.default_rng(0)
    tracks = [(box(float(x), float(y)), 0.5, PEDESTRIAN, i) for i, (x, y) in enumerate(rng.uniform(-30, 30, (1025, 2)))]
    inp, out = cases.frame("big", 0, tracks, [(box(0.0), PEDESTRIAN, 0, 20, "a")])
    ev = WaymoTrackEvaluator(device=dev)
    with pytest.raises(RuntimeError, match="1025 tracks of one class in one frame exceed the limit of 1024"):
        ev.process([inp], [out])
    assert ev._counts.is_cuda and int(ev._counts.sum()) == 0
    assert not ev.evaluate()["counts"].any()


def test_model_smoke(dev):
    """The small TrajectoryFormer of test_trajectoryformer_online.py over its synthetic drive, through inference_on_dataset."""
    import os

    from conftest import ROOT
    from golden_init import ONLINE_SEQUENCE, deterministic_state

    from efg_amd.config import load_config
    from efg_amd.evaluator import WaymoTrackEvaluator, inference_on_dataset
    from efg_amd.tracking import TrajectoryFormer
    from efg_amd.tracking.synthetic import make_tracking_sequence

    cfg = load_config(os.path.join(ROOT, "configs", "trajectoryformer_waymo_centerpoint.yaml"),
                      {"model.device": str(dev), "task": "val", "model.eval_class": "VEHICLE"})
    torch.manual_seed(0)
    model = TrajectoryFormer(cfg)
    model.load_state_dict(deterministic_state(model.state_dict()))
    loader = [[item] for item in make_tracking_sequence(**ONLINE_SEQUENCE)]
    evaluator = WaymoTrackEvaluator(classes=("VEHICLE",), device=dev)
    res = inference_on_dataset(model, loader, evaluator)
    assert evaluator._counts.is_cuda
    assert sorted(k for k in res if k.startswith("OBJECT")) == sorted(cases.KEYS)
    for k in cases.KEYS:
        assert np.isfinite(res[k]), (k, res[k])
        if k.endswith("/MOTA"):
            assert res[k] <= 1.0, (k, res[k])
        if "VEHICLE" not in k:
            assert res[k] == 0.0, (k, res[k])
    counts = res["counts"]
    assert counts.shape == (3, 11, 9) and (counts[0, :, 8] > 0).all() and not counts[1:].any()
    assert res["score_cutoff"].shape == (3, 2)
    print({k: round(res[k], 4) for k in cases.KEYS if "VEHICLE" in k}, counts[0, 0].tolist())
