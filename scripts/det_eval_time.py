"""Time the Waymo-protocol evaluator on the device next to its fp64 host formulation on the same input:
`process` + `evaluate` over 64 frames x 300 predictions x 60 ground truths (DESIGN.md "Detection evaluation").
Prints one JSON line.  `python scripts/det_eval_time.py [--frames 64] [--reps 5]`."""
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


def make_frame(rng, n_gt=60, n_pred=300):
    centres = rng.uniform(-60, 60, (10, 2))
    labels = rng.integers(1, 4, n_gt)
    gt = np.zeros((n_gt, 7), np.float32)
    for i, lb in enumerate(labels):
        gt[i, :2] = centres[rng.integers(10)] + rng.normal(0, 2.5 if lb == 1 else 0.8, 2)
        gt[i, 2] = rng.normal(0.5, 0.1)
        gt[i, 3:6] = np.array(SIZES[int(lb)]) * rng.uniform(0.9, 1.1, 3)
        gt[i, 6] = rng.uniform(-math.pi, math.pi)
    src = rng.integers(0, n_gt, n_pred)
    pred = gt[src].copy()
    pred[:, :2] += rng.normal(0, 0.12, (n_pred, 2)).astype(np.float32)
    pred[:, 3:6] *= rng.uniform(0.93, 1.07, (n_pred, 3)).astype(np.float32)
    pred[:, 6] += rng.normal(0, 0.15, n_pred).astype(np.float32)
    far = rng.random(n_pred) < 0.4                                   # clutter
    pred[far, :2] += rng.normal(0, 3.0, (int(far.sum()), 2)).astype(np.float32)
    out = {"boxes3d": torch.from_numpy(pred), "scores": torch.from_numpy(rng.uniform(0, 1, n_pred).astype(np.float32)),
           "labels": torch.from_numpy(labels[src].astype(np.int64))}
    tgt = {"gt_boxes": gt, "labels": labels.astype(np.int64), "num_points_in_gt": rng.integers(1, 40, n_gt)}
    return tgt, out


def run(frames, device):
    from efg_amd.evaluator import WaymoDetEvaluator

    ev = WaymoDetEvaluator(device=device)
    t0 = time.perf_counter()
    ev.process([f[0] for f in frames], [f[1] for f in frames])
    res = ev.evaluate()                 # ends in a device-to-host copy of the totals
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_eval_time: needs a GPU (a CPU run times nothing of interest)")
    rng = np.random.default_rng(0)
    frames = [make_frame(rng) for _ in range(args.frames)]
    dev = torch.device("cuda:0")
    run(frames, dev)                    # warm-up: code objects, allocator
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t, got = run(frames, dev)
        times.append(t)
    host_s, want = run(frames, "cpu")
    keys = [k for k in want if k != "counts"]
    print(json.dumps({"frames": args.frames, "predictions_per_frame": 300, "ground_truths_per_frame": 60,
                      "device_ms": [round(1e3 * t, 3) for t in times], "device_ms_median": round(1e3 * float(np.median(times)), 3),
                      "host_formulation_s": round(host_s, 3),
                      "counts_equal": bool(torch.equal(got["counts"][..., :3], want["counts"][..., :3])),
                      "max_ap_diff": max(abs(got[k] - want[k]) for k in keys),
                      "mean_ap": float(np.mean([want[k] for k in keys]))}))


if __name__ == "__main__":
    main()
