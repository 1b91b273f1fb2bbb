"""Time the Waymo-protocol tracking evaluator on the device next to its fp64 host formulation on the same input:
`process` frame by frame + `evaluate` over 3 sequences x 200 frames x 60 objects (DESIGN.md "Tracking evaluation").
Prints one JSON line.  `python scripts/track_eval_time.py [--sequences 3] [--frames 200] [--objects 60] [--reps 3]`."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {1: (4.5, 2.0, 1.6), 2: (0.9, 0.8, 1.7), 3: (1.8, 0.8, 1.7)}


def make_sequence(rng, name, n_frames, n_obj):
    """Objects on a random walk; tracks are jittered copies, 10 % dropped per frame, 2 % take a fresh id, 5 ghosts."""
    labels = rng.integers(1, 4, n_obj)
    centres = rng.uniform(-60, 60, (10, 2))
    pos = centres[rng.integers(10, size=n_obj)] + rng.normal(0, 1, (n_obj, 2)) * np.where(labels == 1, 4.0, 1.0)[:, None]
    size = np.array([SIZES[int(c)] for c in labels]) * rng.uniform(0.9, 1.1, (n_obj, 3))
    yaw, base = rng.uniform(-math.pi, math.pi, n_obj), rng.uniform(0.2, 1.0, n_obj)
    ids, next_id, frames = np.arange(n_obj), n_obj, []
    for f in range(n_frames):
        pos = pos + rng.normal(0, 0.05, (n_obj, 2))
        gt = np.concatenate([pos, np.full((n_obj, 1), 0.5), size, yaw[:, None]], 1).astype(np.float32)
        fresh = rng.random(n_obj) < 0.02
        ids = np.where(fresh, next_id + np.arange(n_obj), ids)
        next_id += n_obj
        seen = rng.random(n_obj) > 0.1
        trk = gt[seen].copy()
        trk[:, :2] += rng.normal(0, 0.08, (len(trk), 2)).astype(np.float32)
        trk[:, 3:6] *= rng.uniform(0.95, 1.05, (len(trk), 3)).astype(np.float32)
        ghost = np.concatenate([rng.uniform(-60, 60, (5, 2)), np.full((5, 1), 0.5), np.tile(SIZES[2], (5, 1)),
                                rng.uniform(-math.pi, math.pi, (5, 1))], 1).astype(np.float32)
        out = {"track_boxes3d": torch.from_numpy(np.concatenate([trk, ghost])),
               "track_scores": torch.from_numpy(np.concatenate([np.clip(base[seen] + rng.normal(0, 0.05, len(trk)), 0, 1),
                                                                rng.uniform(0, 0.4, 5)]).astype(np.float32)),
               "track_labels": torch.from_numpy(np.concatenate([labels[seen], np.full(5, 2)]).astype(np.int64)),
               "track_ids": torch.from_numpy(np.concatenate([ids[seen], next_id + np.arange(5)]).astype(np.int64))}
        next_id += 5
        tgt = {"gt_boxes": gt, "labels": labels.astype(np.int64), "num_points_in_gt": rng.integers(1, 40, n_obj),
               "gt_ids": np.array(["%s/%d" % (name, i) for i in range(n_obj)])}
        frames.append((({}, {"token": "%s_frame_%d" % (name, f), "annotations": tgt}), out))
    return frames


def run(frames, device):
    from efg_amd.evaluator import WaymoTrackEvaluator

    ev = WaymoTrackEvaluator(device=device)
    t0 = time.perf_counter()
    for inp, out in frames:
        ev.process([inp], [out])
    res = ev.evaluate()                 # ends in a device-to-host copy of the totals
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--objects", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_eval_time: needs a GPU (a CPU run times nothing of interest)")
    rng = np.random.default_rng(0)
    frames = [f for s in range(args.sequences) for f in make_sequence(rng, "drive%d" % s, args.frames, args.objects)]
    dev = torch.device("cuda:0")
    run(frames[:args.frames], dev)      # warm-up: code objects, allocator
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t, got = run(frames, dev)
        times.append(t)
    host_s, want = run(frames, "cpu")
    keys = [k for k in want if k.startswith("OBJECT")]
    print(json.dumps({"sequences": args.sequences, "frames_per_sequence": args.frames, "objects": args.objects,
                      "device_ms": [round(1e3 * t, 3) for t in times], "device_ms_median": round(1e3 * float(np.median(times)), 3),
                      "host_formulation_s": round(host_s, 3),
                      "counts_equal": bool(torch.equal(got["counts"], want["counts"])),
                      "max_metric_diff": max(abs(got[k] - want[k]) for k in keys),
                      "mean_mota": float(np.mean([want[k] for k in keys if k.endswith("MOTA")]))}))


if __name__ == "__main__":
    main()
