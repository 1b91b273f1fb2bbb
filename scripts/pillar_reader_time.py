"""Time the PointPillars reader + BEV scatter on the GPU: the fused kernels (csrc/pillars.hip) next to the PyTorch composition
of the same modules (the reference's formulation: decorate, Linear, BatchNorm1d, ReLU, max; index scatter), DESIGN.md §5g.
Shapes: 2 scenes x 30 000 and 2 x 60 000 pillars of N = 20 rows with F = 5 features on a 468 x 468 grid (Waymo's range at
0.32 m pillars), 64 channels, training mode.  Two workloads per arm: forward (reader + scatter) and forward + backward (from a
fixed canvas gradient to the three parameter gradients).  The arms are timed alternately with device events after a warm-up
of each; medians are reported, with min and max.  The outputs of the two arms are compared at the timed size (largest
absolute difference of the canvas and of the gradients) so that the times are of the same computation.
The yardstick is the composition, never the fused path itself.  Needs a GPU; prints one JSON line.
`python scripts/pillar_reader_time.py [--reps 30] [--out FILE]`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, FEATURES, GRID, SCENES = 20, 5, 468, 2
VOXEL, LOW = 0.32, -74.88


def make_batch(per_scene, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    p = SCENES * per_scene
    cells = torch.cat([torch.randperm(GRID * GRID, generator=gen)[:per_scene].sort().values for _ in range(SCENES)])
    b = torch.arange(SCENES).repeat_interleave(per_scene)
    coors = torch.stack([b, torch.zeros_like(b), cells // GRID, cells % GRID], 1).int()
    counts = torch.randint(1, ROWS + 1, (p,), generator=gen, dtype=torch.int32)
    voxels = torch.rand(p, ROWS, FEATURES, generator=gen)
    voxels[:, :, 0] = LOW + (coors[:, 3:4].float() + voxels[:, :, 0]) * VOXEL
    voxels[:, :, 1] = LOW + (coors[:, 2:3].float() + voxels[:, :, 1]) * VOXEL
    voxels[:, :, 2] = 6 * voxels[:, :, 2] - 2
    voxels = voxels * (torch.arange(ROWS).view(1, ROWS, 1) < counts.view(p, 1, 1))
    dcanvas = torch.randn(SCENES, 64, GRID, GRID, generator=gen).contiguous(memory_format=torch.channels_last)
    return voxels.to(dev), counts.to(dev), coors.to(dev), dcanvas.to(dev)


def build(dev):
    from efg_amd.modeling.readers import PillarFeatureNet, PointPillarsScatter

    torch.manual_seed(0)
    net = PillarFeatureNet(num_input_features=FEATURES, num_filters=(64,), voxel_size=(VOXEL, VOXEL, 6.0),
                           pc_range=(LOW, LOW, -2.0, -LOW, -LOW, 4.0)).to(dev).train()
    net.pfn_layers[0].norm.weight.data.uniform_(0.5, 1.5)
    net.pfn_layers[0].norm.bias.data.normal_(0, 0.3)
    return net, PointPillarsScatter(num_input_features=64)


def arms(net, scatter, batch):
    voxels, counts, coors, dcanvas = batch
    shape = [GRID, GRID]

    def fused(backward):
        canvas = scatter(net(voxels, counts, coors), coors, SCENES, shape)
        if backward:
            canvas.backward(dcanvas)
        return canvas

    def composition(backward):
        canvas = scatter.forward_composition(net.forward_composition(voxels, counts, coors), coors, SCENES, shape)
        if backward:
            canvas.backward(dcanvas)
        return canvas

    return {"fused": fused, "composition": composition}


def grads(net):
    layer = net.pfn_layers[0]
    return [p.grad.clone() for p in (layer.linear.weight, layer.norm.weight, layer.norm.bias)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pillar_reader_time: needs a GPU (a CPU run times nothing of interest)")
    dev = torch.device("cuda:0")
    net, scatter = build(dev)
    result = {"rows": ROWS, "features": FEATURES, "channels": 64, "grid": [GRID, GRID], "scenes": SCENES, "reps": args.reps,
              "unit": "ms, device events around one call, median / min / max"}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for per_scene in (30000, 60000):
        batch = make_batch(per_scene, dev)
        assert net.usable(batch[0])
        run = arms(net, scatter, batch)
        # same computation: outputs of the two arms at this size
        same = {}
        outs = {}
        for name, fn in run.items():
            net.zero_grad(set_to_none=True)
            outs[name] = (fn(True).detach().clone(), grads(net))
        same["canvas_max_abs_diff"] = float((outs["fused"][0] - outs["composition"][0]).abs().max())
        same["canvas_max_abs"] = float(outs["composition"][0].abs().max())
        for k, a, b in zip(("dweight", "dgamma", "dbeta"), outs["fused"][1], outs["composition"][1]):
            same[k + "_max_rel_diff"] = float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        entry = {"pillars": SCENES * per_scene, "fused_vs_composition": same}
        for label, backward in (("forward", False), ("forward_backward", True)):
            for fn in run.values():                         # warm-up of this shape and workload
                for _ in range(3):
                    net.zero_grad(set_to_none=True)
                    fn(backward)
            times = {name: [] for name in run}
            for _ in range(args.reps):                      # alternating: the arms share the device and the host
                for name, fn in run.items():
                    net.zero_grad(set_to_none=True)
                    torch.cuda.synchronize()
                    start.record()
                    fn(backward)
                    stop.record()
                    stop.synchronize()
                    times[name].append(start.elapsed_time(stop))
            entry[label] = {name: {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
                            for name, t in times.items()}
            entry[label]["composition_over_fused"] = round(entry[label]["composition"]["median"] / entry[label]["fused"]["median"], 2)
        result["2x%dk" % (per_scene // 1000)] = entry
        del batch, run, outs
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
