"""CenterPoint inference with the circular NMS on the device (csrc/center_decode.hip) -- thin wrappers over libefg_hip.so.

`center_predict_circular` is the chain candidates -> circular NMS -> boxes of the kept cells: three launches per call
whatever the number of tasks and scenes, and no device-to-host transfer (it runs under
torch.cuda.set_sync_debug_mode("error")); `predict_circular_device` adds the single final copy and the result format of
`CenterHead.predict`.  `circle_nms` is the stand-alone operator with the arguments of the reference's `_circle_nms`.
There is no CPU compute path here; the host formulation lives in efg_amd/centerpoint/circular_host.py.
"""
import ctypes

import torch

from .. import _lib

_HEADS = ("hm", "reg", "height", "dim", "rot", "vel")
_CHANNELS = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2}


def max_cells():
    """Cells (H * W) one map, and entries one `circle_nms` list, may hold."""
    return _lib.lib().efg_center_decode_max_cells()


def max_tasks():
    return _lib.lib().efg_center_decode_max_tasks()


def check_cells(n):
    """The host-side limit check: raises, never truncates."""
    limit = max_cells()
    if n > limit:
        raise RuntimeError("efg_amd center_decode: %d cells in one list exceed the limit of %d" % (n, limit))


def _nhwc(preds_dicts):
    """Per task the maps as NHWC-contiguous fp32 (no copy for the channels-last maps of the GPU model) + the shape."""
    tasks = []
    b, _, h, w = preds_dicts[0]["hm"].shape
    has_vel = "vel" in preds_dicts[0]
    for t, preds in enumerate(preds_dicts):
        maps = {}
        for k in _HEADS:
            if k == "vel" and not has_vel:
                if "vel" in preds:
                    raise ValueError("task %d has a vel map and task 0 has none" % t)
                continue
            v = preds[k]
            _lib.require_gpu(v)
            if v.dtype != torch.float32 or v.shape[0] != b or tuple(v.shape[2:]) != (h, w) \
                    or (k != "hm" and v.shape[1] != _CHANNELS[k]):
                raise ValueError("task %d: %s map %s %s, expected fp32 [%d, %s, %d, %d]"
                                 % (t, k, v.dtype, tuple(v.shape), b, _CHANNELS.get(k, "classes"), h, w))
            maps[k] = v.detach().permute(0, 2, 3, 1).contiguous()
        tasks.append(maps)
    return tasks, b, h, w, has_vel


def _chain(preds_dicts, post_process, num_classes):
    from ..centerpoint.circular_host import check_min_radius   # (the package above imports this one)

    num_classes = [int(n) for n in num_classes]
    n_tasks = len(preds_dicts)
    if len(num_classes) != n_tasks:
        raise ValueError("%d class counts for %d tasks" % (len(num_classes), n_tasks))
    radii = check_min_radius(post_process, n_tasks)
    shape = preds_dicts[0]["hm"].shape
    check_cells(int(shape[2]) * int(shape[3]))                   # before anything is launched
    if n_tasks > max_tasks():
        raise RuntimeError("efg_amd center_decode: %d tasks exceed the limit of %d" % (n_tasks, max_tasks()))
    tasks, b, h, w, has_vel = _nhwc(preds_dicts)
    for t, maps in enumerate(tasks):
        if maps["hm"].shape[3] != num_classes[t]:
            raise ValueError("task %d: heat map of %d classes, expected %d" % (t, maps["hm"].shape[3], num_classes[t]))
    dev = tasks[0]["hm"].device
    post_max = int(post_process.nms.nms_post_max_size)
    box_dim = 9 if has_vel else 7
    segs, cells, rows = b * n_tasks, h * w, b * n_tasks * post_max
    ptrs = (ctypes.c_void_p * (n_tasks * 6))(*[_lib.ptr(maps.get(k)) for maps in tasks for k in _HEADS])
    ncls = _lib.host_i32(num_classes, n_tasks)
    limit = post_process.post_center_limit_range
    limit = _lib.host_f32(limit, 6) if len(limit) > 0 else None
    score = torch.empty((segs, cells), dtype=torch.float32, device=dev)
    x, y = torch.empty_like(score), torch.empty_like(score)
    label = torch.empty((segs, cells), dtype=torch.int32, device=dev)
    keep = torch.empty((segs, post_max), dtype=torch.int32, device=dev)
    # boxes, scores, labels and counts in ONE buffer of 4-byte words: one copy takes all of them to the host
    packed = torch.zeros((rows * (box_dim + 2) + segs,), dtype=torch.float32, device=dev)
    boxes, scores, labels, counts = _split(packed, b, n_tasks, post_max, box_dim)
    lib, st = _lib.lib(), _lib.stream()
    with torch.cuda.device(dev):
        _lib.check(lib.efg_center_decode_candidates_f32(
            ptrs, ncls, n_tasks, b, h, w, float(post_process.out_size_factor), float(post_process.voxel_size[0]),
            float(post_process.voxel_size[1]), float(post_process.pc_range[0]), float(post_process.pc_range[1]),
            float(post_process.score_threshold), limit, _lib.ptr(score), _lib.ptr(label), _lib.ptr(x), _lib.ptr(y), st))
        _lib.check(lib.efg_circle_nms_f32(_lib.ptr(x), _lib.ptr(y), _lib.ptr(score), segs, cells,
                                          _lib.host_f32(radii, n_tasks), n_tasks, post_max, _lib.ptr(keep),
                                          _lib.ptr(counts), st))
        _lib.check(lib.efg_center_decode_boxes_f32(
            ptrs, ncls, n_tasks, b, h, w, post_max, _lib.ptr(x), _lib.ptr(y), _lib.ptr(score), _lib.ptr(label),
            _lib.ptr(keep), _lib.ptr(counts), _lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(labels), st))
    return packed, (b, n_tasks, post_max, box_dim)


def _split(packed, b, n_tasks, post_max, box_dim):
    """Views of the packed buffer: boxes [B, T * post_max, box_dim], scores [B, T * post_max], labels int32 alike, counts
    int32 [B, T]."""
    rows = b * n_tasks * post_max
    o1 = rows * box_dim
    o2, o3 = o1 + rows, o1 + 2 * rows
    return (packed[:o1].view(b, n_tasks * post_max, box_dim), packed[o1:o2].view(b, n_tasks * post_max),
            packed[o2:o3].view(torch.int32).view(b, n_tasks * post_max), packed[o3:].view(torch.int32).view(b, n_tasks))


def center_predict_circular(preds_dicts, post_process, num_classes):
    """preds_dicts: per task {"hm", "reg", "height", "dim", "rot"[, "vel"]} fp32 NCHW maps on the GPU; post_process: the
    model's `post_process` section with `min_radius` (one per task); num_classes: classes per task.
    -> device tensors (boxes [B, T * post_max, 9 or 7], scores [B, T * post_max], labels int32 [B, T * post_max]: 0-based,
    offset by task, counts int32 [B, T]).  The block of task t of a scene is rows t * post_max ..; its first counts[b, t]
    rows are the kept boxes in kept order, the rest is zero.  No host wait."""
    packed, shape = _chain(preds_dicts, post_process, num_classes)
    return _split(packed, *shape)


def predict_circular_device(preds_dicts, post_process, num_classes):
    """The chain + its single device-to-host copy -> per scene {"scores", "labels" (1-based, int64), "boxes3d"} on the
    CPU, tasks concatenated in order: the result format of `CenterHead.predict`."""
    packed, (b, n_tasks, post_max, box_dim) = _chain(preds_dicts, post_process, num_classes)
    boxes, scores, labels, counts = _split(packed.cpu(), b, n_tasks, post_max, box_dim)
    counts = counts.tolist()
    results = []
    for i in range(b):
        rows = torch.cat([torch.arange(t * post_max, t * post_max + counts[i][t]) for t in range(n_tasks)])
        results.append({"scores": scores[i, rows], "labels": labels[i, rows].long() + 1, "boxes3d": boxes[i, rows]})
    return results


def circle_nms(boxes, min_radius, post_max_size=83):
    """boxes [N, 3] = (x, y, score) fp32 on the GPU -> the kept indices, int64 on the device, in kept order: the arguments
    and meaning of the reference's `_circle_nms`.  Descending score, equal scores by ascending index; a kept box suppresses
    every later one whose SQUARED centre distance is <= min_radius.  Entries with a score of -inf or NaN are never kept.
    The length of the result is data: this one waits for the device (one 4-byte copy)."""
    _lib.require_gpu(boxes)
    assert boxes.dim() == 2 and boxes.shape[1] == 3 and boxes.dtype == torch.float32, "boxes must be fp32 (N, 3)"
    n, post_max = boxes.shape[0], int(post_max_size)
    check_cells(n)
    if n == 0 or post_max <= 0:
        return torch.zeros((0,), dtype=torch.int64, device=boxes.device)
    cols = boxes.detach().t().contiguous()                        # [3, N]
    keep = torch.empty((post_max,), dtype=torch.int32, device=boxes.device)
    count = torch.zeros((1,), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        _lib.check(_lib.lib().efg_circle_nms_f32(_lib.ptr(cols[0]), _lib.ptr(cols[1]), _lib.ptr(cols[2]), 1, n,
                                                 _lib.host_f32([min_radius], 1), 1, post_max, _lib.ptr(keep),
                                                 _lib.ptr(count), _lib.stream()))
    return keep[:int(count.item())].long()
