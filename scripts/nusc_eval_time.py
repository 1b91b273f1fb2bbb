"""Time the nuScenes-protocol evaluator on the device next to its fp64 host formulation on the same input:
`process` + `evaluate` over 64 frames x 300 predictions x 60 ground truths (DESIGN.md "nuScenes detection evaluation").
Prints one JSON line.  `python scripts/nusc_eval_time.py [--frames 64] [--reps 5]`.

Measured on one MI355X (64 x 300 x 60, a warm-up call first, 7 repetitions alternating between the two paths, each ending
in the copy of the records to the host): device path 9.7 ms (9.68-10.4 ms), host path 93.0 ms (92.6-96.1 ms), every returned
number equal.  Both times include the shared numpy preparation and the shared fp64 summary."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
           "traffic_cone")
SIZES = ((4.6, 1.9, 1.7), (6.9, 2.5, 2.8), (6.4, 2.8, 3.2), (11.0, 2.9, 3.5), (12.3, 2.9, 3.9), (0.5, 2.5, 1.0),
         (2.1, 0.8, 1.5), (1.7, 0.6, 1.3), (0.7, 0.7, 1.8), (0.4, 0.4, 1.1))
ATTRIBUTES = ("vehicle.moving", "vehicle.parked", "cycle.with_rider", "pedestrian.moving", "pedestrian.standing", "")
DEFAULTS = {"car": "vehicle.parked", "truck": "vehicle.parked", "construction_vehicle": "vehicle.parked", "bus": "vehicle.moving",
            "trailer": "vehicle.parked", "motorcycle": "cycle.with_rider", "bicycle": "cycle.with_rider",
            "pedestrian": "pedestrian.moving"}


def make_frame(rng, n_gt=60, n_pred=300):
    """Boxes in the models' layout (x, y, z, l, w, h, vx, vy, yaw): clustered objects, jittered detections, 40 % clutter."""
    centres = rng.uniform(-25, 25, (10, 2))
    labels = rng.integers(1, 11, n_gt)
    gt = np.zeros((n_gt, 9), np.float32)
    for i, lb in enumerate(labels):
        gt[i, :2] = centres[rng.integers(10)] + rng.normal(0, 2.5, 2)
        gt[i, 2] = rng.normal(0.5, 0.1)
        gt[i, 3:6] = np.array(SIZES[int(lb) - 1]) * rng.uniform(0.9, 1.1, 3)
        gt[i, 6:8] = rng.normal(0, 1.5, 2) * (rng.random() < 0.5)
        gt[i, 8] = rng.uniform(-math.pi, math.pi)
    src = rng.integers(0, n_gt, n_pred)
    pred = gt[src].copy()
    pred[:, :2] += rng.normal(0, 0.3, (n_pred, 2)).astype(np.float32)
    pred[:, 3:6] *= rng.uniform(0.93, 1.07, (n_pred, 3)).astype(np.float32)
    pred[:, 6:8] += rng.normal(0, 0.3, (n_pred, 2)).astype(np.float32)
    pred[:, 8] += rng.normal(0, 0.15, n_pred).astype(np.float32)
    far = rng.random(n_pred) < 0.4                                   # clutter
    pred[far, :2] += rng.normal(0, 3.0, (int(far.sum()), 2)).astype(np.float32)
    out = {"boxes3d": torch.from_numpy(pred), "scores": torch.from_numpy(rng.uniform(0, 1, n_pred).astype(np.float32)),
           "labels": torch.from_numpy(labels[src].astype(np.int64))}
    tgt = {"gt_boxes": gt, "labels": labels.astype(np.int64), "num_points_in_gt": rng.integers(1, 40, n_gt),
           "attributes": [str(a) for a in rng.choice(ATTRIBUTES, n_gt)]}
    return tgt, out


def run(frames, device):
    from efg_amd.evaluator import NuScenesDetEvaluator

    ev = NuScenesDetEvaluator(default_attributes=DEFAULTS, device=device)
    t0 = time.perf_counter()
    ev.process([f[0] for f in frames], [f[1] for f in frames])
    res = ev.evaluate()                 # ends in a device-to-host copy of the records
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nusc_eval_time: needs a GPU (a CPU run times nothing of interest)")
    rng = np.random.default_rng(0)
    frames = [make_frame(rng) for _ in range(args.frames)]
    dev = torch.device("cuda:0")
    run(frames, dev)                    # warm-up: code objects, allocator
    times, host_times = [], []
    for _ in range(args.reps):          # alternating: the two share the host with whatever else runs on it
        torch.cuda.synchronize()
        t, got = run(frames, dev)
        times.append(t)
        t, want = run(frames, "cpu")
        host_times.append(t)
    diff = max(abs(got[k] - want[k]) for k in want if not math.isnan(want[k]))
    print(json.dumps({"frames": args.frames, "predictions_per_frame": 300, "ground_truths_per_frame": 60,
                      "device_ms": [round(1e3 * t, 3) for t in times], "device_ms_median": round(1e3 * float(np.median(times)), 3),
                      "host_formulation_ms": [round(1e3 * t, 3) for t in host_times],
                      "host_formulation_ms_median": round(1e3 * float(np.median(host_times)), 3),
                      "nan_in_the_same_places": all(math.isnan(got[k]) == math.isnan(want[k]) for k in want),
                      "max_diff": diff, "mAP": want["mAP"], "NDS": want["NDS"]}))


if __name__ == "__main__":
    main()
