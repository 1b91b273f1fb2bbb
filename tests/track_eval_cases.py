"""Inputs of the tracking-evaluation tests (test_track_eval_ref.py on the CPU, test_track_eval_gpu.py on the device): the
hand cases with their expected count rows and the synthetic sequences.  No test in here.

A count row is [match1, match2, fp, miss1, miss2, mismatch1, mismatch2, gt1, gt2] (DESIGN.md "Tracking evaluation")."""
import math

import numpy as np
import torch

from det_eval_cases import CYCLIST, PEDESTRIAN, SIZES, VEHICLE, box

# Seeds of the device tests, chosen on the CPU (test_track_eval_ref.py asserts the conditions) out of seeds 0..7:
#   E2E_SEEDS: (i) the fp64 formulation has no same-class pair within 1e-4 of its class threshold; (ii) the whole count table
#     is the same under the fp64 IoU and under the float32 pair function of iou3d_nms.hip (its CPU twin,
#     oracle.boxes_iou3d), which is the reference's clipper and lies up to 2.5e-2 from the exact IoU for pedestrian-sized
#     boxes: enough to move a pair across its threshold or to swap two near-equal assignments, after which the two state
#     machines part ways for good; (iii) mismatches occur, the table differs between cutoffs, carry-overs lose claim
#     conflicts, and the table changes when the carry-over step is switched off.
#     Seeds 1 to 4 meet all of them; 5 to 7 miss (i).
#   MATCH_SEED: need not meet (i) or (ii) (seed 0 misses (ii): 42 entries of its table differ between the two IoU
#     functions): the device's state machine is compared with the host's on the device's own weights.
#   MOTP_BOUND: the largest |oracle.boxes_iou3d - fp64 IoU| over the matched pairs of E2E_SEEDS (1.942e-2, 1.945e-2),
#     rounded up: the bar of the device's MOTP against the fp64 formulation's (test_track_eval_ref.py measures it).
E2E_SEEDS = (1, 2)
MATCH_SEED = 0
MOTP_BOUND = 1.95e-2
N_SEQUENCES, N_FRAMES = 3, 12
MANY_FRAME, FULL_FRAME = (0, 7), (2, 6)          # (sequence, frame): 1024 pedestrian tracks; a 65 x 65 pedestrian problem
KEYS = ["OBJECT_TYPE_TYPE_%s_LEVEL_%d/%s" % (c, lv, m) for c in ("VEHICLE", "PEDESTRIAN", "CYCLIST") for lv in (1, 2)
        for m in ("MOTA", "MOTP", "MISS", "MISMATCH", "FP")]


def frame(sequence, number, tracks, gts):
    """tracks: [(box, score, label, track id)], gts: [(box, label, difficulty, num_points, gt id)] -> (input, output) as
    the loader and the online tracker hand them to an evaluator."""
    out = {"track_boxes3d": torch.tensor([t[0] for t in tracks], dtype=torch.float32).reshape(-1, 7),
           "track_scores": torch.tensor([t[1] for t in tracks], dtype=torch.float32),
           "track_labels": torch.tensor([t[2] for t in tracks], dtype=torch.float32),
           "track_ids": torch.tensor([t[3] for t in tracks], dtype=torch.int32)}
    tgt = {"gt_boxes": np.array([g[0] for g in gts], dtype=np.float32).reshape(-1, 7),
           "labels": np.array([g[1] for g in gts], dtype=np.int64),
           "difficulty": np.array([g[2] for g in gts], dtype=np.int64),
           "num_points_in_gt": np.array([g[3] for g in gts], dtype=np.int64),
           "gt_ids": np.array([str(g[4]) for g in gts], dtype=str)}
    return ({}, {"token": "%s_frame_%d.npy" % (sequence, number), "annotations": tgt}), out


def run(frames, device, chunk=1, **kw):
    """The evaluator's result over `frames` ([(input, output)]), `chunk` frames per `process` call."""
    from efg_amd.evaluator import WaymoTrackEvaluator

    ev = WaymoTrackEvaluator(device=device, **kw)
    ev.reset()
    for i in range(0, len(frames), chunk):
        ev.process([f[0] for f in frames[i:i + chunk]], [f[1] for f in frames[i:i + chunk]])
    res = ev.evaluate()
    res["evaluator"] = ev
    return res


# ---- the hand cases ---------------------------------------------------------------------------------------------------------
# One class (pedestrian), boxes 1 x 1 x 1.7 at (x, 0, 0), yaw 0; two such boxes dx apart have IoU (1 - dx) / (1 + dx).
def _hand(frames, sequence="hand"):
    """frames: [(tracks [(x, score, id)], gts [(x, gt id)] or [(x, gt id, num_points)])]."""
    out = []
    for n, (tracks, gts) in enumerate(frames):
        out.append(frame(sequence, n, [(box(t[0]), t[1], PEDESTRIAN, t[2]) for t in tracks],
                         [(box(g[0]), PEDESTRIAN, 0, g[2] if len(g) > 2 else 20, g[1]) for g in gts]))
    return out


def _cost(dx):
    dx = float(np.float32(dx))                   # the boxes are float32
    return 1.0 - (1.0 - dx) / (1.0 + dx)


def hand_cases():
    """name -> (frames, evaluator keywords, [(first cutoff, last cutoff, pedestrian count row, level-2 cost)])."""
    two = [(0.0, "a"), (5.0, "b")]
    masks = [frame("hand", 0,
                   [(box(0.0), 0.9, PEDESTRIAN, 1), (box(100.6), 0.9, PEDESTRIAN, 2), (box(15.0), 0.9, PEDESTRIAN, 3),
                    (box(30.0, size=SIZES[VEHICLE]), 0.9, VEHICLE, 4)],
                   [(box(100.6), PEDESTRIAN, 0, 20, "far"), (box(15.0), PEDESTRIAN, 0, 0, "empty"),
                    (box(30.0, size=SIZES[VEHICLE]), VEHICLE, 0, 20, "car"), (box(0.0), PEDESTRIAN, 0, 20, "a")])]
    return {
        "perfect": (_hand([([(0.0, 0.9, 1), (5.0, 0.9, 2)], two)] * 3), {},
                    [(0, 9, [6, 6, 0, 0, 0, 0, 0, 6, 6], 0.0), (10, 10, [0, 0, 0, 6, 6, 0, 0, 6, 6], 0.0)]),
        "switch": (_hand([([(0.0, 0.9, 7)], [(0.0, "a")]), ([(0.0, 0.9, 7)], [(0.0, "a")]), ([(0.0, 0.9, 8)], [(0.0, "a")])]), {},
                   [(0, 9, [3, 3, 0, 0, 0, 1, 1, 3, 3], 0.0)]),
        # plain Hungarian matching would pick id 2 in the second frame and count a mismatch
        "carry": (_hand([([(0.0, 0.9, 1)], [(0.0, "a")]), ([(0.3, 0.9, 1), (0.0, 0.8, 2)], [(0.0, "a")])]), {},
                  [(0, 8, [2, 2, 1, 0, 0, 0, 0, 2, 2], _cost(0.3)), (9, 9, [2, 2, 0, 0, 0, 0, 0, 2, 2], _cost(0.3))]),
        # the map survives a frame without tracks
        "gap": (_hand([([(0.0, 0.9, 1)], [(0.0, "a")]), ([], [(0.0, "a")]), ([(0.0, 0.9, 2)], [(0.0, "a")])]), {},
                [(0, 9, [2, 2, 0, 1, 1, 1, 1, 3, 3], 0.0)]),
        "cutoff": (_hand([([(0.0, 0.9, 1)], [(0.0, "a")]), ([(0.3, 0.35, 1), (0.0, 0.9, 2)], [(0.0, "a")]),
                          ([(0.0, 0.9, 1)], [(0.0, "a")])]), {},
                   [(0, 3, [3, 3, 1, 0, 0, 0, 0, 3, 3], _cost(0.3)), (4, 9, [3, 3, 0, 0, 0, 2, 2, 3, 3], 0.0)]),
        # both ground truths were last matched to track 1: in the third frame the one of lower id keeps it
        "claim": (_hand([([(0.0, 0.9, 1)], [(0.0, "a"), (0.2, "b")]), ([(0.2, 0.9, 1)], [(0.2, "b")]),
                         ([(0.1, 0.9, 1)], [(0.0, "a"), (0.2, "b")])]), {},
                  [(0, 9, [3, 3, 0, 2, 2, 0, 0, 5, 5], _cost(0.1))]),
        "hard": (_hand([([(0.0, 0.9, 1)], [(0.0, "a", 3)]), ([(0.0, 0.9, 2)], [(0.0, "a", 3)])]), {},
                 [(0, 9, [0, 2, 0, 0, 0, 0, 1, 0, 2], 0.0)]),
        # a frame without ground truths: its track is a false positive, the map survives
        "no_gt": (_hand([([(0.0, 0.9, 1)], [(0.0, "a")]), ([(0.0, 0.9, 1)], []), ([(0.0, 0.9, 1)], [(0.0, "a")])]), {},
                  [(0, 9, [2, 2, 1, 0, 0, 0, 0, 2, 2], 0.0)]),
        "one_frame": (_hand([([(0.0, 0.9, 1)], two)]), {}, [(0, 9, [1, 1, 0, 1, 1, 0, 0, 2, 2], 0.0)]),
        # beyond 100.5 m, without points, of a class that is not evaluated: all dropped, tracks and ground truths alike
        "masks": (masks, {"classes": ("PEDESTRIAN",)}, [(0, 9, [1, 1, 1, 0, 0, 0, 0, 1, 1], 0.0)]),
    }


def check_hand_case(name, res, cost_tol):
    """The pedestrian rows of result `res` against the table; the other classes hold nothing."""
    counts, cost = res["counts"].numpy(), res["cost"].numpy()
    assert counts.shape == (3, 11, 9) and cost.shape == (3, 11, 2)
    for lo, hi, row, want in hand_cases()[name][2]:
        for k in range(lo, hi + 1):
            assert counts[PEDESTRIAN - 1, k].tolist() == row, (name, k, counts[PEDESTRIAN - 1, k].tolist())
            assert abs(cost[PEDESTRIAN - 1, k, 1] - want) <= cost_tol, (name, k, cost[PEDESTRIAN - 1, k, 1], want)
            assert abs(cost[PEDESTRIAN - 1, k, 0] - (want if row[0] else 0.0)) <= cost_tol, (name, k)
    assert not counts[VEHICLE - 1].any() and not counts[CYCLIST - 1].any()
    ped = "OBJECT_TYPE_TYPE_PEDESTRIAN_LEVEL_%d/"
    if name == "perfect":
        assert res[ped % 1 + "MOTA"] == 1.0 and res[ped % 2 + "MOTA"] == 1.0 and res[ped % 1 + "MOTP"] == 0.0
    if name in ("switch", "cutoff"):
        assert abs(res[ped % 1 + "MOTA"] - 2.0 / 3.0) <= 1e-12 and res["score_cutoff"][PEDESTRIAN - 1, 0] == 0.0
    if name == "cutoff":
        assert abs(res[ped % 1 + "FP"] - 1.0 / 3.0) <= 1e-12 and res[ped % 1 + "MISMATCH"] == 0.0
    if name == "hard":
        assert res[ped % 1 + "MOTA"] == 0.0 and abs(res[ped % 2 + "MOTA"] - 0.5) <= 1e-12
        assert abs(res[ped % 2 + "MISMATCH"] - 0.5) <= 1e-12


# ---- synthetic sequences ---------------------------------------------------------------------------------------------------
def sequence(rng, name, n_obj, classes=(PEDESTRIAN, CYCLIST), spread=0.7, min_points=0, full_frame=None, many_frame=None,
             n_frames=N_FRAMES, n_ghost=3):
    """Clusters of `classes` objects `spread` metres apart, as det_eval_cases.crowded_frame; each walks randomly and keeps
    its gt id.  Tracks are jittered copies: per frame about 15 % are dropped, 5 % take a fresh id for good, 5 % swap ids with
    their nearest neighbour of the same class for good; `n_ghost` tracks next to nothing in particular; 30 % of the scores
    are rounded to one decimal, so they sit on cutoffs.  Frame `full_frame` has one track per object and nothing else;
    frame `many_frame` is filled up to exactly 1024 pedestrian tracks."""
    centres = rng.uniform(-40, 40, (max(n_obj // 6, 1), 2))
    label = rng.choice(classes, n_obj)
    pos = centres[rng.integers(len(centres), size=n_obj)] + rng.normal(0, spread, (n_obj, 2))
    z, yaw = rng.normal(0.5, 0.1, n_obj), rng.uniform(-math.pi, math.pi, n_obj)
    size = np.array([SIZES[int(c)] for c in label]) * rng.uniform(0.9, 1.1, (n_obj, 3))
    difficulty, base = rng.choice([0, 0, 0, 2], n_obj), rng.uniform(0.05, 1.0, n_obj)
    ids, next_id = list(range(n_obj)), n_obj
    frames = []
    for f in range(n_frames):
        pos = pos + rng.normal(0, 0.05, (n_obj, 2))
        yaw = yaw + rng.normal(0, 0.03, n_obj)
        points = rng.integers(min_points, 25, n_obj)
        gts = [([pos[i, 0], pos[i, 1], z[i], *size[i], yaw[i]], int(label[i]), int(difficulty[i]), int(points[i]),
                "%s/%d" % (name, i)) for i in range(n_obj)]
        tracks = []
        for i in range(n_obj):
            if rng.random() < 0.05:
                ids[i], next_id = next_id, next_id + 1
            if rng.random() < 0.05:
                same = [j for j in range(n_obj) if j != i and label[j] == label[i]]
                if same:
                    j = min(same, key=lambda j: float(np.hypot(*(pos[j] - pos[i]))))
                    ids[i], ids[j] = ids[j], ids[i]
        for i in range(n_obj):
            dropped = rng.random() < 0.15
            b = [pos[i, 0] + rng.normal(0, 0.1), pos[i, 1] + rng.normal(0, 0.1), z[i] + rng.normal(0, 0.05),
                 *(size[i] * rng.uniform(0.92, 1.08, 3)), yaw[i] + rng.normal(0, 0.15)]
            score = float(np.clip(base[i] + rng.normal(0, 0.1), 0.02, 1.0))
            if rng.random() < 0.3:
                score = round(score, 1)
            if not dropped or f == full_frame:
                tracks.append((b, score, int(label[i]), ids[i]))
        for _ in range(0 if f == full_frame else n_ghost):
            lab = int(rng.choice(classes))
            c = centres[rng.integers(len(centres))] + rng.normal(0, 2 * spread, 2)
            tracks.append(([c[0], c[1], 0.5, *SIZES[lab], rng.uniform(-math.pi, math.pi)], rng.uniform(0.0, 0.4), lab, next_id))
            next_id += 1
        if f == many_frame:
            peds = [i for i in range(n_obj) if label[i] == PEDESTRIAN]
            for _ in range(1024 - sum(1 for t in tracks if t[2] == PEDESTRIAN)):
                i = peds[rng.integers(len(peds))]
                b = [pos[i, 0] + rng.normal(0, 0.25), pos[i, 1] + rng.normal(0, 0.25), z[i], *size[i], yaw[i] + rng.normal(0, 0.2)]
                tracks.append((b, rng.uniform(0.0, 1.0), PEDESTRIAN, next_id))
                next_id += 1
        order = rng.permutation(len(tracks))
        frames.append(frame(name, f, [tracks[i] for i in order], gts))
    return frames


def sequences(seed):
    """[3 sequences x 12 frames]: 24-30 pedestrians and cyclists in clusters each in the first two (one frame of the first
    holds exactly 1024 pedestrian tracks), 65 pedestrians in the third (one frame of it is a 65 x 65 problem)."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(N_SEQUENCES):
        name = "drive%d-%d" % (seed, s)
        if s == FULL_FRAME[0]:
            out.append(sequence(rng, name, 65, classes=(PEDESTRIAN,), spread=1.2, min_points=1, full_frame=FULL_FRAME[1]))
        else:
            out.append(sequence(rng, name, int(rng.integers(24, 31)), many_frame=MANY_FRAME[1] if s == MANY_FRAME[0] else None))
    return out


def flat(seqs):
    return [f for s in seqs for f in s]
