"""The PointPillars model (efg_amd/centerpoint/pointpillars.py): PillarFeatureNet -> PointPillarsScatter -> RPN -> CenterHead
with VoxelNet's contract.  A tiny configuration built inline (the reference ships no pillar experiment): one task of two
classes, a 16 x 16 pillar grid, 64 -> 16 RPN.  CPU: construction, both input formats' plumbing, one training step and the
inference format on reference-format samples.  GPU: one training step from raw points against the same module and weights on
the CPU fed the same pillars in the reference format -- losses to 1e-4, gradients to 1e-3, the model-golden tolerances of
DESIGN.md §2 -- and eval mode returns `predict`'s format."""
import copy

import numpy as np
import pytest
import torch

PC_RANGE = [-3.2, -3.2, -2.0, 3.2, 3.2, 4.0]
VOXEL_SIZE = [0.4, 0.4, 6.0]
MAX_POINTS = 20


def make_config(device):
    from efg_amd.config import to_attr

    vox = {"pc_range": PC_RANGE, "voxel_size": VOXEL_SIZE, "max_points_in_voxel": MAX_POINTS, "max_voxel_num": 256}
    return to_attr({
        "dataset": {"classes": ["car", "ped"], "pc_range": PC_RANGE, "voxel_size": VOXEL_SIZE,
                    "processors": {"train": {"Voxelization": dict(vox)}, "val": {"Voxelization": dict(vox)}}},
        "model": {
            "device": str(device),
            "reader": {"num_input_features": 5, "num_filters": [64], "with_distance": False, "voxel_size": VOXEL_SIZE,
                       "pc_range": PC_RANGE, "norm": "BN1d"},
            "backbone": {"num_input_features": 64},
            "neck": {"num_input_features": 64, "layer_nums": [1], "ds_layer_strides": [1], "ds_num_filters": [16],
                     "us_layer_strides": [1], "us_num_filters": [16], "norm": "BN"},
            "head": {"in_channels": 16, "norm": {"type": "BN"}, "tasks": [{"num_classes": 2, "class_names": ["car", "ped"]}],
                     "misc": {"dataset": "waymo", "weight": 2, "code_weights": [1.0] * 8,
                              "common_heads": {"reg": [2, 2], "height": [1, 2], "dim": [3, 2], "rot": [2, 2]}}},
            "loss": {"out_size_factor": 1, "dense_reg": 1, "gaussian_overlap": 0.1, "max_objs": 20, "min_radius": 2},
            "post_process": {"post_center_limit_range": [-4.0, -4.0, -10.0, 4.0, 4.0, 10.0],
                             "nms": {"nms_pre_max_size": 100, "nms_post_max_size": 20, "nms_iou_threshold": 0.7},
                             "score_threshold": 0.1, "pc_range": PC_RANGE, "out_size_factor": 1, "voxel_size": VOXEL_SIZE}}})


def make_scenes(seed=0):
    """Two scenes: points [n, 5] inside the range and four boxes (x, y, z, l, w, h, vx, vy, yaw) each."""
    rng = np.random.default_rng(seed)
    scenes = []
    for n in (700, 450):
        pts = np.concatenate([rng.uniform(PC_RANGE[:3], PC_RANGE[3:], (n, 3)), rng.uniform(0, 1, (n, 2))], 1).astype(np.float32)
        boxes = np.concatenate([rng.uniform(-2.5, 2.5, (4, 2)), rng.uniform(-1, 1, (4, 1)), rng.uniform(0.4, 1.2, (4, 3)),
                                np.zeros((4, 2)), rng.uniform(-3, 3, (4, 1))], 1).astype(np.float32)
        scenes.append((pts, {"annotations": {"gt_boxes": boxes, "labels": rng.integers(1, 3, 4)}}))
    return scenes


def build(device, state=None):
    from efg_amd.centerpoint import PointPillars

    torch.manual_seed(0)
    model = PointPillars(make_config(device))
    if state is None:
        for m in model.modules():          # non-trivial norm parameters
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.normal_(0, 0.2)
    else:
        model.load_state_dict({k: v.to(device) for k, v in state.items()}, strict=True)
    return model.train()


def reference_samples(voxels, counts, coors, infos):
    """The host pipeline's sample dicts from one batched voxelization."""
    grid = np.round((np.array(PC_RANGE[3:]) - np.array(PC_RANGE[:3])) / np.array(VOXEL_SIZE)).astype(np.int64)
    out = []
    for b, info in enumerate(infos):
        rows = coors[:, 0] == b
        out.append(({"voxels": voxels[rows], "num_points_per_voxel": counts[rows], "coordinates": coors[rows][:, 1:],
                     "shape": grid, "range": np.array(PC_RANGE, np.float32), "size": np.array(VOXEL_SIZE, np.float32)},
                    copy.deepcopy(info)))
    return out


def host_voxelize(scenes):
    """A plain numpy pillar voxelizer for the CPU test (first MAX_POINTS points per pillar, pillars in first-seen order)."""
    vs, lo = np.array(VOXEL_SIZE, np.float32), np.array(PC_RANGE[:3], np.float32)
    vox, cnt, coo = [], [], []
    for b, (pts, _) in enumerate(scenes):
        cell = np.floor((pts[:, :3] - lo) / vs).astype(np.int32)
        order = {}
        for i, c in enumerate(map(tuple, cell)):
            order.setdefault(c, []).append(i)
        for (x, y, z), rows in order.items():
            rows = rows[:MAX_POINTS]
            v = np.zeros((MAX_POINTS, 5), np.float32)
            v[:len(rows)] = pts[rows]
            vox.append(v), cnt.append(len(rows)), coo.append((b, z, y, x))
    return np.stack(vox), np.array(cnt, np.int32), np.array(coo, np.int32)


def total_loss(losses):
    return sum(v for k, v in losses.items() if k.endswith("_loss") and v.requires_grad)


def test_pointpillars_trains_and_predicts_on_the_cpu(oracle_mod):
    from oracle import cpu_backend

    from efg_amd.centerpoint import PointPillars, VoxelNet
    from efg_amd.modeling.readers import PillarFeatureNet, PointPillarsScatter

    scenes = make_scenes()
    model = build(torch.device("cpu"))
    assert isinstance(model, VoxelNet) and isinstance(model, PointPillars)
    assert isinstance(model.reader, PillarFeatureNet) and isinstance(model.backbone, PointPillarsScatter)
    assert model.grid_size == [16, 16, 1]
    assert {"reader.pfn_layers.0.linear.weight", "reader.pfn_layers.0.norm.running_var"} <= set(model.state_dict())
    batch = reference_samples(*host_voxelize(scenes), [info for _, info in scenes])
    losses = model(batch)
    assert set(losses) == {"0_loss", "0_hm_loss", "0_loc_loss", "0_num_positive"}
    total_loss(losses).backward()
    grad = model.reader.pfn_layers[0].linear.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.any())
    assert int(model.reader.pfn_layers[0].norm.num_batches_tracked) == 1
    model.eval()
    with torch.no_grad(), cpu_backend.install():       # the rotated NMS of `predict` has no CPU form outside the checker
        res = model(batch)
    assert len(res) == 2 and all(set(r) == {"scores", "labels", "boxes3d"} for r in res)
    assert all(r["boxes3d"].shape[1] == 7 and r["scores"].shape[0] <= 20 for r in res)


@pytest.mark.gpu
def test_pointpillars_gpu_step_against_the_cpu(dev):
    from efg_amd.operators import voxelize_batch

    scenes = make_scenes()
    cpu = build(torch.device("cpu"))
    gpu = build(dev, state=cpu.state_dict())
    assert gpu.reader.usable(torch.zeros(1, MAX_POINTS, 5, device=dev))
    losses_g = gpu([({"points": torch.from_numpy(p).to(dev)}, copy.deepcopy(i)) for p, i in scenes])
    total_loss(losses_g).backward()
    torch.cuda.synchronize()
    vox = voxelize_batch([torch.from_numpy(p).to(dev) for p, _ in scenes], VOXEL_SIZE, PC_RANGE, MAX_POINTS, 256, with_mean=False)
    assert vox["voxels"].shape[0] > 200 and int(vox["num_points_per_voxel"].min()) >= 1
    batch = reference_samples(vox["voxels"].cpu().numpy(), vox["num_points_per_voxel"].cpu().numpy(),
                              vox["coordinates"].cpu().numpy(), [i for _, i in scenes])
    losses_c = cpu(batch)
    total_loss(losses_c).backward()
    assert set(losses_g) == set(losses_c)
    for k, v in losses_c.items():
        assert float(losses_g[k].detach()) == pytest.approx(float(v.detach()), rel=1e-4, abs=1e-5), k
    pc, pg = dict(cpu.named_parameters()), dict(gpu.named_parameters())
    for k, p in pc.items():
        if p.grad is None:
            assert pg[k].grad is None, k
            continue
        if k.endswith(".0.bias") and "center_head" in k:    # a conv bias in front of a BatchNorm: exactly zero, rounding noise on both sides
            continue
        scale = float(p.grad.abs().max())
        err = float((pg[k].grad.cpu() - p.grad).abs().max())
        assert err <= 1e-3 * max(scale, 1e-6), "%s: %.2e of %.2e" % (k, err, scale)
    bc, bg = dict(cpu.named_buffers()), dict(gpu.named_buffers())
    for k, b in bc.items():
        assert float((bg[k].cpu().double() - b.double()).abs().max()) <= 1e-4 * max(1.0, float(b.double().abs().max())), k
    # eval mode: predict's format, from raw points and from reference-format samples alike
    gpu.eval()
    with torch.no_grad():
        res = gpu([({"points": torch.from_numpy(p).to(dev)}, i) for p, i in scenes])
        res2 = gpu(batch)
    for r in (res, res2):
        assert len(r) == 2 and all(set(x) == {"scores", "labels", "boxes3d"} for x in r)
        assert all(x["boxes3d"].shape[1] == 7 and x["scores"].shape[0] <= 20 for x in r)
    for a, b in zip(res, res2):
        assert a["scores"].shape == b["scores"].shape and torch.allclose(a["scores"], b["scores"], rtol=0, atol=1e-5)
