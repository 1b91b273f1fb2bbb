"""Detection-evaluation kernels (csrc/det_eval.hip) -- thin wrappers over libefg_hip.so.

Frame-segmented (CSR) layout: the predictions and ground truths of the frames of one call are concatenated, frame f owns
rows pred_off[f]:pred_off[f + 1] and gt_off[f]:gt_off[f + 1] and a dense P_f x G_f block of the flat weight buffer at
blk_off[f].  Offsets are host lists (the caller built the concatenation on the host); everything else is on the device.
There is no CPU compute path here; the fp64 host formulation lives in efg_amd/evaluator/waymo.py.
"""
import numpy as np
import torch

from .. import _lib

NUM_CUTOFFS = 101
IOU_THRESHOLDS = (0.7, 0.5, 0.5)      # vehicle, pedestrian, cyclist
# counts[..., :] = tp level 1, tp level 2, unmatched predictions, unmatched ground truths level <= 1, level <= 2
# sums[..., :] = heading accuracy of the level-1 true positives, of the level-2 ones, matched weight
NUM_COUNTS, NUM_SUMS = 5, 3


def limits():
    """(predictions, ground truths) one (frame, class) problem may hold."""
    lib = _lib.lib()
    return lib.efg_det_eval_max_pred(), lib.efg_det_eval_max_gt()


def _i32(values, device):
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)).to(device)


def block_offsets(pred_off, gt_off):
    """Host int64 [F + 1]: start of every frame's P_f x G_f block, and the total size."""
    p, g = np.diff(np.asarray(pred_off, dtype=np.int64)), np.diff(np.asarray(gt_off, dtype=np.int64))
    return np.concatenate(([0], np.cumsum(p * g)))


def pair_weights(pred_boxes, pred_labels, pred_off, gt_boxes, gt_labels, gt_off, thresholds=IOU_THRESHOLDS):
    """pred_boxes [sum P, 7], pred_labels int32 [sum P], gt_boxes [sum G, 7], gt_labels int32 [sum G] on the device,
    pred_off / gt_off host [F + 1] -> (weights fp32 [sum P_f G_f] on the device, blk_off host int64 [F + 1]).
    weight = boxes_iou3d_gpu of the pair (bit for bit) where the labels agree and the IoU reaches the class threshold,
    0 elsewhere.  One launch."""
    _lib.require_gpu(pred_boxes, pred_labels, gt_boxes, gt_labels)
    assert pred_boxes.shape[1:] == (7,) and gt_boxes.shape[1:] == (7,), "boxes must be (N, 7)"
    assert pred_boxes.dtype == gt_boxes.dtype == torch.float32
    assert pred_labels.dtype == gt_labels.dtype == torch.int32
    pred_off, gt_off = np.asarray(pred_off, dtype=np.int64), np.asarray(gt_off, dtype=np.int64)
    assert pred_off[-1] == pred_boxes.shape[0] and gt_off[-1] == gt_boxes.shape[0] and len(pred_off) == len(gt_off)
    dev, n_frames = pred_boxes.device, len(pred_off) - 1
    blk = block_offsets(pred_off, gt_off)
    weights = torch.empty((int(blk[-1]),), dtype=torch.float32, device=dev)
    if blk[-1] == 0:
        return weights, blk
    po, go = _i32(pred_off, dev), _i32(gt_off, dev)
    bo = torch.from_numpy(blk[:-1].copy()).to(dev)
    _lib.check(_lib.lib().efg_det_eval_pair_weights_f32(
        _lib.ptr(pred_boxes.contiguous()), _lib.ptr(pred_labels.contiguous()), _lib.ptr(po),
        _lib.ptr(gt_boxes.contiguous()), _lib.ptr(gt_labels.contiguous()), _lib.ptr(go), _lib.ptr(bo), n_frames,
        int(np.diff(pred_off).max()), int(np.diff(gt_off).max()), *(float(t) for t in thresholds), _lib.ptr(weights),
        _lib.stream()))
    return weights, blk


def check_problems(problems):
    """The host-side size check of `prefix_assign`: raises, never truncates.  problems: host int [n, 6]."""
    max_pred, max_gt = limits()
    problems = np.asarray(problems).reshape(-1, 6)
    if len(problems) and problems[:, 2].max() > max_pred:
        raise RuntimeError("efg_amd det_eval: %d predictions of one class in one frame exceed the limit of %d"
                           % (problems[:, 2].max(), max_pred))
    if len(problems) and problems[:, 4].max() > max_gt:
        raise RuntimeError("efg_amd det_eval: %d ground truths of one class in one frame exceed the limit of %d"
                           % (problems[:, 4].max(), max_gt))
    return problems


def prefix_assign(weights, blk_off, pred_off, gt_off, problems, scores, pred_boxes, gt_boxes, gt_level):
    """One workgroup per row of `problems` (host int [n, 6]: frame, first prediction, predictions, first ground truth,
    ground truths, class 0..2).  The predictions of a problem are sorted by descending score.  Returns (counts int32
    [n, 101, 5], sums fp64 [n, 101, 3], problems on the device): at each score cutoff, the counts of the maximum-weight
    assignment between the predictions in play and the problem's ground truths."""
    problems = check_problems(problems)
    _lib.require_gpu(weights, scores, pred_boxes, gt_boxes, gt_level)
    assert scores.dtype == torch.float32 and gt_level.dtype == torch.int32
    dev, n = scores.device, len(problems)
    counts = torch.zeros((n, NUM_CUTOFFS, NUM_COUNTS), dtype=torch.int32, device=dev)
    sums = torch.zeros((n, NUM_CUTOFFS, NUM_SUMS), dtype=torch.float64, device=dev)
    prob = _i32(problems, dev)
    if n == 0:
        return counts, sums, prob
    po, go = _i32(pred_off, dev), _i32(gt_off, dev)
    bo = torch.from_numpy(np.ascontiguousarray(np.asarray(blk_off, dtype=np.int64)[: len(po) - 1])).to(dev)
    _lib.check(_lib.lib().efg_det_eval_assign_f32(
        _lib.ptr(weights), _lib.ptr(bo), _lib.ptr(po), _lib.ptr(go), _lib.ptr(prob), n, int(problems[:, 2].max()),
        int(problems[:, 4].max()), _lib.ptr(scores.contiguous()), _lib.ptr(pred_boxes.contiguous()),
        _lib.ptr(gt_boxes.contiguous()), _lib.ptr(gt_level.contiguous()), _lib.ptr(counts), _lib.ptr(sums), _lib.stream()))
    return counts, sums, prob


def accumulate(counts, sums, problems_dev, total_counts, total_sums):
    """total_counts int64 [3, 101, 5] and total_sums fp64 [3, 101, 3] += the problems of each class, in problem order."""
    _lib.require_gpu(counts, sums, problems_dev, total_counts, total_sums)
    assert total_counts.dtype == torch.int64 and total_counts.shape == (3, NUM_CUTOFFS, NUM_COUNTS)
    assert total_sums.dtype == torch.float64 and total_sums.shape == (3, NUM_CUTOFFS, NUM_SUMS)
    _lib.check(_lib.lib().efg_det_eval_accumulate(_lib.ptr(counts), _lib.ptr(sums), _lib.ptr(problems_dev),
                                                  counts.shape[0], _lib.ptr(total_counts), _lib.ptr(total_sums),
                                                  _lib.stream()))
