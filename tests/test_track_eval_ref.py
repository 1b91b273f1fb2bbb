"""CPU: the fp64 host formulation of the Waymo-protocol tracking evaluator (efg_amd/evaluator/waymo_track.py: rot_giou3d for
the IoU, a dict for the map `last`, scipy for the residual assignment) on hand cases whose count rows are known, its
invariance under chunking, its errors, and the conditions of the seeds that the device test (test_track_eval_gpu.py)
compares end to end on.

The count table is result["counts"] int64 [class, cutoff, 9] = [match1, match2, fp, miss1, miss2, mismatch1, mismatch2, gt1,
gt2], result["cost"] fp64 [class, cutoff, 2] the sums of 1 - IoU over the matches of level <= 1, <= 2.

MOTP bar of the device test.  The device weighs pairs with the float32 clipper of iou3d_nms.hip, the host with the exact
fp64 IoU.  Where both paths hold the same pairs, their MOTPs (means of 1 - IoU over those pairs) differ by at most the
largest |clipper - fp64 IoU| of a matched pair plus 2^-31 of grid rounding.  test_iou_functions_on_the_matched_pairs
measures that difference with the clipper's CPU twin (oracle.boxes_iou3d) over the matched pairs of E2E_SEEDS: 1.942e-2
(seed 1) and 1.945e-2 (seed 2); track_eval_cases.MOTP_BOUND = 1.95e-2 is that measurement rounded up."""
import numpy as np
import pytest
import torch

import track_eval_cases as cases
from det_eval_cases import PEDESTRIAN, box

CPU = torch.device("cpu")
_CACHE = {}


def probe_class():
    from efg_amd.evaluator.waymo_track import WaymoTrackEvaluator, class_ranges

    class Probe(WaymoTrackEvaluator):
        """The host path with a choice of IoU function; records the largest difference of the two over the matched pairs."""
        oracle, use_clipper = None, False

        def reset(self):
            super().reset()
            self.carry_stats["pairs"] = set()
            self.max_iou_diff, self._both = 0.0, None

        def harvest(self):
            if self._both is not None:
                for r, g in self.carry_stats["pairs"]:
                    self.max_iou_diff = max(self.max_iou_diff, abs(float(self._both[0][r, g]) - float(self._both[1][r, g])))
            self.carry_stats["pairs"].clear()

        def host_weights(self, f, c):
            self.harvest()
            w64 = super().host_weights(f, c)
            p0, n_p, g0, n_g = class_ranges(f)[c]
            iou32 = np.zeros((n_p, n_g), np.float32)
            if iou32.size:
                iou32 = np.asarray(self.oracle.boxes_iou3d(f["pb"][p0:p0 + n_p], f["gb"][g0:g0 + n_g]), np.float32)
            w32 = np.where(iou32 >= np.float32(self.thresholds[c]), iou32, 0.0).astype(np.float64)
            self._both = (w64, iou32.astype(np.float64))
            return w32 if self.use_clipper else w64

        def evaluate(self):
            res = super().evaluate()
            self.harvest()
            return res

    return Probe


def probe_run(seed, oracle_mod, use_clipper=False, carry_over=True):
    key = (seed, use_clipper, carry_over)
    if key not in _CACHE:
        ev = probe_class()(device=CPU, carry_over=carry_over)
        ev.oracle, ev.use_clipper = oracle_mod, use_clipper
        for inp, out in cases.flat(cases.sequences(seed)):
            ev.process([inp], [out])
        res = ev.evaluate()
        res["evaluator"] = ev
        _CACHE[key] = res
    return _CACHE[key]


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_cases(name):
    frames, kw, _ = cases.hand_cases()[name]
    res = cases.run(frames, CPU, **kw)
    assert sorted(k for k in res if k.startswith("OBJECT")) == sorted(cases.KEYS)
    assert res["counts"].dtype == torch.int64 and res["cost"].dtype == torch.float64
    cases.check_hand_case(name, res, 1e-9)


def test_plain_hungarian_counts_a_mismatch_where_the_carry_over_keeps_the_track():
    res = cases.run(cases.hand_cases()["carry"][0], CPU, carry_over=False)
    assert res["counts"][PEDESTRIAN - 1, 0].tolist() == [2, 2, 1, 0, 0, 1, 1, 2, 2]
    assert res["cost"][PEDESTRIAN - 1, 0, 1] == 0.0


def test_summary_of_an_empty_evaluator():
    from efg_amd.evaluator import WaymoTrackEvaluator

    res = WaymoTrackEvaluator(device=CPU).evaluate()
    assert all(res[k] == 0.0 for k in cases.KEYS) and not res["counts"].any()
    assert res["counts"].shape == (3, 11, 9) and res["score_cutoff"].shape == (3, 2)


def test_cutoffs_are_an_argument():
    from efg_amd.evaluator import WaymoTrackEvaluator

    frames = cases.hand_cases()["cutoff"][0]
    res = cases.run(frames, CPU, cutoffs=[0.3, 0.36])
    assert res["counts"].shape == (3, 2, 9)
    assert res["counts"][PEDESTRIAN - 1].tolist() == [[3, 3, 1, 0, 0, 0, 0, 3, 3], [3, 3, 0, 0, 0, 2, 2, 3, 3]]
    for bad in ([0.5, 0.4], [0.5, 0.5], list(np.linspace(0, 1, 102)), []):
        with pytest.raises(ValueError, match="cutoffs"):
            WaymoTrackEvaluator(device=CPU, cutoffs=bad)
    assert len(WaymoTrackEvaluator(device=CPU, cutoffs=np.linspace(0, 1, 101)).cutoffs) == 101


def test_chunking_does_not_change_a_bit():
    frames = cases.flat(cases.sequences(cases.E2E_SEEDS[0])[1:])        # two sequences, without the 1024-track frame
    runs = [cases.run(frames, CPU), cases.run(frames, CPU, flush_frames=5), cases.run(frames, CPU, chunk=4, flush_frames=1)]
    assert runs[0]["counts"][..., 5].sum() > 0
    for r in runs[1:]:
        assert torch.equal(r["counts"], runs[0]["counts"])
        assert torch.equal(r["cost"].view(torch.int64), runs[0]["cost"].view(torch.int64))
        assert all(r[k] == runs[0][k] for k in cases.KEYS)


def test_errors():
    from efg_amd.evaluator import WaymoTrackEvaluator

    def one(seq, n, ids=(1,), gt_ids=("a",)):
        return cases.frame(seq, n, [(box(float(i)), 0.9, PEDESTRIAN, t) for i, t in enumerate(ids)],
                           [(box(float(i)), PEDESTRIAN, 0, 20, g) for i, g in enumerate(gt_ids)])

    def feed(*frames):
        ev = WaymoTrackEvaluator(device=CPU)
        for inp, out in frames:
            ev.process([inp], [out])
        return ev

    with pytest.raises(ValueError, match="after frame"):
        feed(one("s", 3), one("s", 2))
    with pytest.raises(ValueError, match="after frame"):
        feed(one("s", 3), one("s", 3))
    with pytest.raises(ValueError, match="closed"):
        feed(one("s", 0), one("t", 0), one("s", 1))
    with pytest.raises(ValueError, match="duplicate track_ids"):
        feed(one("s", 0, ids=(4, 4)))
    with pytest.raises(ValueError, match="duplicate gt_ids"):
        feed(one("s", 0, gt_ids=("a", "a")))
    inp, out = one("s", 0)
    del inp[1]["annotations"]["gt_ids"]
    with pytest.raises(ValueError, match="without gt_ids"):
        feed((inp, out))
    inp, out = one("s", 0)
    del out["track_ids"]
    with pytest.raises(ValueError, match="without track_ids"):
        feed((inp, out))
    inp, out = one("s", 0)
    inp[1]["token"] = "no-frame-number"
    with pytest.raises(ValueError, match="token"):
        feed((inp, out))
    inp, out = one("s", 0)
    inp[1]["metadata"] = {"token": inp[1].pop("token")}                 # the other place a token may stand
    assert feed((inp, out)).evaluate()["counts"][PEDESTRIAN - 1, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 1]


def test_synthetic_drive_carries_its_ground_truths():
    from golden_init import ONLINE_SEQUENCE

    from efg_amd.tracking.synthetic import make_tracking_sequence

    seq = make_tracking_sequence(**ONLINE_SEQUENCE)
    ann = [info["annotations"] for _, info in seq]
    n = ONLINE_SEQUENCE["n_objects"]
    for a in ann:
        assert a["gt_boxes"].shape == (n, 7) and a["gt_boxes"].dtype == np.float32 and len(set(a["gt_ids"].tolist())) == n
        assert a["labels"].tolist() == ann[0]["labels"].tolist() and a["gt_ids"].tolist() == ann[0]["gt_ids"].tolist()
        assert (a["num_points_in_gt"] > 5).all() and not a["difficulty"].any()
        # the detections are jittered copies of these boxes: every seen object has one within 0.5 m
        d = np.hypot(*(a["pred_boxes3d"][:, None, :2] - a["gt_boxes"][None, :, :2]).transpose(2, 0, 1))
        assert (d.min(0) < 0.5).sum() >= n - 4
    assert not np.allclose(ann[0]["gt_boxes"][:, :2], ann[-1]["gt_boxes"][:, :2])


def test_sequences_cover_the_shapes():
    seqs = cases.sequences(cases.MATCH_SEED)
    assert len(seqs) == cases.N_SEQUENCES and all(len(s) == cases.N_FRAMES for s in seqs)
    inp, out = seqs[cases.MANY_FRAME[0]][cases.MANY_FRAME[1]]
    assert int((out["track_labels"] == PEDESTRIAN).sum()) == 1024
    inp, out = seqs[cases.FULL_FRAME[0]][cases.FULL_FRAME[1]]
    assert len(out["track_ids"]) == 65 and len(inp[1]["annotations"]["labels"]) == 65
    assert 24 <= len(seqs[0][0][0][1]["annotations"]["labels"]) <= 30


@pytest.mark.parametrize("seed", cases.E2E_SEEDS)
def test_end_to_end_seeds_meet_their_conditions(seed, oracle_mod):
    """The seeds of the device's end-to-end comparison (track_eval_cases.py)."""
    exact = probe_run(seed, oracle_mod)
    assert exact["evaluator"].min_threshold_margin > 1e-4                                          # (i)
    clipper = probe_run(seed, oracle_mod, use_clipper=True)
    assert torch.equal(exact["counts"], clipper["counts"])                                         # (ii)
    counts = exact["counts"]
    assert counts[..., 0].sum() > 1000 and counts[..., 5].sum() > 0 and counts[..., 6].sum() > counts[..., 5].sum()   # (iii)
    assert any(not torch.equal(counts[:, k], counts[:, k + 1]) for k in range(9))
    assert exact["evaluator"].carry_stats["kept"] > 1000 and exact["evaluator"].carry_stats["conflicts"] > 0
    plain = probe_run(seed, oracle_mod, carry_over=False)
    assert not torch.equal(plain["counts"], counts)              # a kernel without the carry-over step does not pass
    assert int(plain["counts"][..., 5].sum()) > int(counts[..., 5].sum())


@pytest.mark.parametrize("seed", cases.E2E_SEEDS)
def test_iou_functions_on_the_matched_pairs(seed, oracle_mod):
    """The MOTP bar of the device test (module docstring): the largest |clipper - fp64 IoU| over the matched pairs."""
    diff = probe_run(seed, oracle_mod)["evaluator"].max_iou_diff
    print("seed %d: largest |oracle.boxes_iou3d - fp64 IoU| over the matched pairs %.3e" % (seed, diff))
    assert 0.0 < diff <= cases.MOTP_BOUND
