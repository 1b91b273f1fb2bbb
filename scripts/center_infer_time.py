"""Time CenterPoint's `CenterHead.predict` at the nuScenes workload's own shape -- 4 scenes, 180 x 180 cells, six tasks
(1, 2, 2, 1, 2, 2 classes) with `vel` -- on given head maps: the circular-NMS device chain (csrc/center_decode.hip) next to
the rotated-NMS path of the same tree on the same maps (DESIGN.md "CenterPoint circular-NMS inference").  Two inputs:
  sparse   quiet heat maps with --candidates (300) confident cells per (scene, task);
  plateau  every logit at the head's initial bias -2.19 (sigmoid 0.1007 > the threshold 0.1): every cell is a candidate,
           what a freshly initialised model produces.
Both paths end in their copy of the results to the host, so a host clock around a call is the call's time; the two are
timed alternately after a warm-up call each.  The chain alone (its three launches, no copy) is timed with device events.
Host waits per call are counted as the warnings of torch.cuda.set_sync_debug_mode("warn") (every blocking device-to-host
copy, .item() and nonzero raises one).  The two paths select differently (circular against rotated NMS), so their outputs
are not compared here; tests/test_center_circular_gpu.py compares the chain with the host formulation.
Prints one JSON line.  `python scripts/center_infer_time.py [--reps 20] [--out FILE]`.

Measured on one MI355X (--reps 200, profiles/center_infer_time.json), median: sparse -- chain 0.93 ms (0.69 ms on the device
alone), rotated 8.36 ms; plateau -- chain 1.33 ms (0.92 ms), rotated 11.25 ms; host waits per call 1 against 109."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NUM_CLASSES = (1, 2, 2, 1, 2, 2)
B, H, W = 4, 180, 180
POST_PROCESS = {"post_center_limit_range": [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": 83, "nms_iou_threshold": 0.2},
                "score_threshold": 0.1, "pc_range": [-54.0, -54.0], "out_size_factor": 8, "voxel_size": [0.075, 0.075],
                "min_radius": [4, 12, 10, 1, 0.85, 0.175]}


def make_maps(kind, candidates, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    tasks = []
    for ncls in NUM_CLASSES:
        if kind == "plateau":
            hm = torch.full((B, ncls, H, W), -2.19)
        else:
            hm = torch.full((B, ncls, H * W), -6.0) + 0.5 * torch.randn(B, ncls, H * W, generator=g)
            for b in range(B):
                cells = torch.randperm(H * W, generator=g)[:candidates]
                hm[b, torch.randint(0, ncls, (candidates,), generator=g), cells] = 3.0 * torch.rand(candidates, generator=g) - 1.5
            hm = hm.reshape(B, ncls, H, W)
        m = {"hm": hm, "reg": torch.rand(B, 2, H, W, generator=g), "height": torch.randn(B, 1, H, W, generator=g),
             "dim": 0.5 * torch.randn(B, 3, H, W, generator=g) + 0.5, "rot": torch.randn(B, 2, H, W, generator=g),
             "vel": torch.randn(B, 2, H, W, generator=g)}
        # the layout the GPU model hands over: channels-last storage behind an NCHW shape
        tasks.append({k: v.to(dev).contiguous(memory_format=torch.channels_last) for k, v in m.items()})
    return tasks


def head_of(circular):
    from efg_amd.centerpoint.center_head import CenterHead
    from efg_amd.config import to_attr

    tasks = [{"num_classes": n, "class_names": ["c%d_%d" % (t, i) for i in range(n)]} for t, n in enumerate(NUM_CLASSES)]
    cfg = to_attr({"model": {"neck": {"norm": "BN"},
                             "head": {"in_channels": 8, "tasks": tasks,
                                      "misc": {"dataset": "nuscenes", "weight": 0.25, "code_weights": [1.0] * 10,
                                               "common_heads": {"reg": [2, 2], "height": [1, 2], "dim": [3, 2],
                                                                "rot": [2, 2], "vel": [2, 2]}}},
                             "post_process": dict(POST_PROCESS, circular_nms=circular)}})
    return CenterHead(cfg), cfg.model.post_process


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()                         # ends in the copy of the results to the host
    return time.perf_counter() - t0, out


def host_waits(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message) for w in caught)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--candidates", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("center_infer_time: needs a GPU (a CPU run times nothing of interest)")
    from efg_amd.operators.center_decode import center_predict_circular

    dev = torch.device("cuda:0")
    (circ, circ_pp), (rot, rot_pp) = head_of(True), head_of(False)
    result = {"scenes": B, "map": [H, W], "tasks": list(NUM_CLASSES), "reps": args.reps, "candidates_sparse": args.candidates}
    for kind in ("sparse", "plateau"):
        maps = make_maps(kind, args.candidates, dev)
        run_c = lambda: circ.predict({}, maps, circ_pp)          # noqa: E731
        run_r = lambda: rot.predict({}, maps, rot_pp)            # noqa: E731
        out_c, out_r = run_c(), run_r()                          # warm-up: code objects, allocator
        tc, tr = [], []
        for _ in range(args.reps):                               # alternating: the two share the host and the device
            tc.append(timed(run_c)[0])
            tr.append(timed(run_r)[0])
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        chain = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            start.record()
            center_predict_circular(maps, circ_pp, NUM_CLASSES)
            stop.record()
            stop.synchronize()
            chain.append(start.elapsed_time(stop))
        ms = lambda ts: {"median": round(1e3 * float(np.median(ts)), 3), "min": round(1e3 * min(ts), 3),   # noqa: E731
                         "max": round(1e3 * max(ts), 3)}
        result[kind] = {
            "circular_chain_predict_ms": ms(tc), "rotated_predict_ms": ms(tr),
            "circular_chain_device_only_ms": {"median": round(float(np.median(chain)), 3), "min": round(min(chain), 3),
                                              "max": round(max(chain), 3)},
            "host_waits_per_call": {"circular_chain": host_waits(run_c), "rotated": host_waits(run_r)},
            "boxes_per_scene": {"circular_chain": [len(o["scores"]) for o in out_c], "rotated": [len(o["scores"]) for o in out_r]},
        }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
