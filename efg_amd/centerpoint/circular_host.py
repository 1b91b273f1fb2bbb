"""Host formulation of CenterPoint inference with the circular NMS: the decode of $CP1-nuScenes/center_head.py:194-339 with
`circular_nms: True` and the greedy loop of circle_nms_jit.py, in torch / NumPy on the CPU.  It is what `CenterHead.predict`
runs for CPU maps and what the device chain (csrc/center_decode.hip) is tested against; tests/golden/
centerpoint_nusc_circle.npz pins it to the reference's own code.

Two things are ours and documented as such (DESIGN.md "CenterPoint circular-NMS inference"):
  * equal scores are visited by ascending cell index (the reference's order is whatever `argsort` gives);
  * the arithmetic of the distance is fp32, like the arrays the reference hands to its loop.
The SQUARED centre distance is compared with `min_radius` itself, as the reference compares."""
import numpy as np
import torch


def check_min_radius(test_config, n_tasks):
    """The per-task radii of `post_process.min_radius` as floats; a clear ValueError when missing or of the wrong length."""
    radii = test_config.get("min_radius", None)
    if radii is None:
        raise ValueError("circular_nms needs post_process.min_radius: one radius per task (%d tasks)" % n_tasks)
    radii = [float(r) for r in radii]
    if len(radii) != n_tasks:
        raise ValueError("post_process.min_radius has %d entries for %d tasks" % (len(radii), n_tasks))
    return radii


def circle_nms_host(x, y, score, min_radius, post_max_size=83):
    """Greedy circular NMS over fp32 arrays -> kept indices (int64), in kept order.  Descending score, equal scores by
    ascending index; a kept entry suppresses every later one with (xi-xj)*(xi-xj) + (yi-yj)*(yi-yj) <= min_radius."""
    x, y, score = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, y, score))
    radius = np.float32(min_radius)
    order = np.argsort(-score, kind="stable")
    alive = np.ones(len(order), dtype=bool)           # over positions of `order`
    keep = []
    for p, i in enumerate(order):
        if len(keep) >= post_max_size:
            break
        if not alive[p]:
            continue
        keep.append(i)
        rest = order[p + 1:]
        dx, dy = x[i] - x[rest], y[i] - y[rest]
        alive[p + 1:] &= ~(dx * dx + dy * dy <= radius)
    return np.asarray(keep, dtype=np.int64)


@torch.no_grad()
def predict_circular_host(preds_dicts, test_config, num_classes):
    """preds_dicts: per task {"hm", "reg", "height", "dim", "rot"[, "vel"]} NCHW maps on the CPU -> per scene
    {"scores", "labels" (1-based, offset by task), "boxes3d"}, tasks concatenated in order."""
    radii = check_min_radius(test_config, len(preds_dicts))
    limit = test_config.post_center_limit_range
    limit = torch.tensor(limit, dtype=torch.float32) if len(limit) > 0 else None
    post_max = int(test_config.nms.nms_post_max_size)
    batch = preds_dicts[0]["hm"].shape[0]
    per_scene = [{"scores": [], "labels": [], "boxes3d": []} for _ in range(batch)]
    offset = 0
    for t, preds in enumerate(preds_dicts):
        p = {k: v.detach().float().cpu().permute(0, 2, 3, 1).contiguous() for k, v in preds.items()}  # N H W C
        hm = torch.sigmoid(p["hm"])
        b, h, w, ncls = hm.shape
        reg = p["reg"].reshape(b, h * w, 2)
        ys, xs = torch.meshgrid(torch.arange(h, dtype=hm.dtype), torch.arange(w, dtype=hm.dtype), indexing="ij")
        xs = (xs.reshape(1, -1, 1) + reg[..., 0:1]) * test_config.out_size_factor * test_config.voxel_size[0] + \
            test_config.pc_range[0]
        ys = (ys.reshape(1, -1, 1) + reg[..., 1:2]) * test_config.out_size_factor * test_config.voxel_size[1] + \
            test_config.pc_range[1]
        cols = [xs, ys, p["height"].reshape(b, h * w, 1), torch.exp(p["dim"]).reshape(b, h * w, 3)]
        if "vel" in p:
            cols.append(p["vel"].reshape(b, h * w, 2))
        cols.append(torch.atan2(p["rot"][..., 0:1], p["rot"][..., 1:2]).reshape(b, h * w, 1))
        boxes = torch.cat(cols, dim=2)
        for i in range(b):
            scores, labels = hm[i].reshape(h * w, ncls).max(dim=-1)    # the first class of equal scores
            keep = scores > test_config.score_threshold
            if limit is not None:
                keep &= (boxes[i, :, :3] >= limit[:3]).all(1) & (boxes[i, :, :3] <= limit[3:]).all(1)
            cand = torch.nonzero(keep).reshape(-1)                     # ascending cell index
            sel = circle_nms_host(boxes[i, cand, 0].numpy(), boxes[i, cand, 1].numpy(), scores[cand].numpy(), radii[t],
                                  post_max)
            sel = cand[torch.from_numpy(sel)]
            per_scene[i]["scores"].append(scores[sel])
            per_scene[i]["labels"].append(labels[sel] + offset + 1)
            per_scene[i]["boxes3d"].append(boxes[i, sel])
        offset += num_classes[t]
    return [{k: torch.cat(v) for k, v in r.items()} for r in per_scene]
