"""Tracking-evaluation kernels (csrc/track_eval.hip) -- thin wrappers over libefg_hip.so.

The layout is the detection evaluator's (operators/det_eval.py), tracks standing where predictions do: the tracks and
ground truths of the frames of one call are concatenated, frame f owns rows trk_off[f]:trk_off[f + 1] and
gt_off[f]:gt_off[f + 1] and a dense P_f x G_f block of the flat weight buffer, which `det_eval.pair_weights` writes.  A
problem is one class of one segment (a run of consecutive frames of one sequence).  Offsets, ranges and problems are host
arrays; everything else is on the device.  There is no CPU compute path here; the fp64 host formulation lives in
efg_amd/evaluator/waymo_track.py.
"""
import numpy as np
import torch

from .. import _lib
from .det_eval import IOU_THRESHOLDS, _i32, limits, pair_weights  # noqa: F401

# counts[..., :] = matches at level 1, level 2, tracks in play in no pair, unmatched ground truths of level <= 1, <= 2,
#                  mismatches at level 1, level 2, ground truths of level <= 1, <= 2
# sums[..., :] = sum of (1 - weight) over the matches of level <= 1, <= 2
NUM_COUNTS, NUM_SUMS = 9, 2
MAX_CUTOFFS = 101                # the kernel's limit (one launch row per cutoff; the library refuses more)


def check_ranges(ranges):
    """The host-side size check of `mot`: raises, never truncates.  ranges: host int [F, 3, 4] (first track, tracks, first
    ground truth, ground truths of every (frame, class))."""
    max_trk, max_gt = limits()
    ranges = np.asarray(ranges).reshape(-1, 3, 4)
    if ranges.size and ranges[:, :, 1].max() > max_trk:
        raise RuntimeError("efg_amd track_eval: %d tracks of one class in one frame exceed the limit of %d"
                           % (ranges[:, :, 1].max(), max_trk))
    if ranges.size and ranges[:, :, 3].max() > max_gt:
        raise RuntimeError("efg_amd track_eval: %d ground truths of one class in one frame exceed the limit of %d"
                           % (ranges[:, :, 3].max(), max_gt))
    return ranges


def check_cutoffs(cutoffs):
    """float32 [K], ascending, 1 <= K <= the kernel's limit: raises otherwise."""
    cutoffs = np.asarray(cutoffs, dtype=np.float32).reshape(-1)
    if not 1 <= len(cutoffs) <= MAX_CUTOFFS:
        raise ValueError("efg_amd track_eval: %d score cutoffs (1 to %d are accepted)" % (len(cutoffs), MAX_CUTOFFS))
    if not (np.isfinite(cutoffs).all() and (np.diff(cutoffs) > 0).all()):
        raise ValueError("efg_amd track_eval: the score cutoffs must be finite and ascending")
    return cutoffs


def mot(weights, blk_off, trk_off, gt_off, ranges, problems, scores, track_ids, gt_ids, gt_level, cutoffs, last):
    """One workgroup per (row of `problems`, cutoff).  ranges host int [F, 3, 4]; problems host int [n, 3] (first frame,
    end frame, class 0..2); scores fp32 [sum P], track_ids int32 [sum P], gt_ids int32 [sum G] (columns of `last`), gt_level
    int32 [sum G], cutoffs fp32 [K] and last int32 [K, capacity] on the device.  `last` is updated in place.  Returns
    (counts int32 [n, K, 9], sums fp64 [n, K, 2], problems on the device)."""
    ranges = check_ranges(ranges)                                      # before anything is launched
    problems = np.asarray(problems, dtype=np.int64).reshape(-1, 3)
    _lib.require_gpu(weights, scores, track_ids, gt_ids, gt_level, cutoffs, last)
    assert scores.dtype == torch.float32 and cutoffs.dtype == torch.float32
    assert track_ids.dtype == gt_ids.dtype == gt_level.dtype == last.dtype == torch.int32
    trk_off, gt_off = np.asarray(trk_off, dtype=np.int64), np.asarray(gt_off, dtype=np.int64)
    n_frames, n, k = len(trk_off) - 1, len(problems), cutoffs.shape[0]
    assert len(ranges) == n_frames and len(gt_off) == n_frames + 1
    assert trk_off[-1] == scores.shape[0] == track_ids.shape[0] and gt_off[-1] == gt_ids.shape[0] == gt_level.shape[0]
    assert last.dim() == 2 and last.shape[0] == k and last.is_contiguous()
    if n:
        assert problems[:, 0].min() >= 0 and problems[:, 1].max() <= n_frames and (problems[:, 0] <= problems[:, 1]).all()
        assert problems[:, 2].min() >= 0 and problems[:, 2].max() <= 2
    if n_frames:
        r = ranges.reshape(-1, 3, 4)
        assert (r[:, :, 0] >= trk_off[:-1, None]).all() and (r[:, :, 0] + r[:, :, 1] <= trk_off[1:, None]).all()
        assert (r[:, :, 2] >= gt_off[:-1, None]).all() and (r[:, :, 2] + r[:, :, 3] <= gt_off[1:, None]).all()
        assert (r[:, :, 1] >= 0).all() and (r[:, :, 3] >= 0).all()
    dev = scores.device
    counts = torch.zeros((n, k, NUM_COUNTS), dtype=torch.int32, device=dev)
    sums = torch.zeros((n, k, NUM_SUMS), dtype=torch.float64, device=dev)
    prob = _i32(problems, dev)
    if n == 0 or n_frames == 0:
        return counts, sums, prob
    to, go, rg = _i32(trk_off, dev), _i32(gt_off, dev), _i32(ranges.reshape(-1), dev)
    bo = torch.from_numpy(np.ascontiguousarray(np.asarray(blk_off, dtype=np.int64)[:n_frames])).to(dev)
    _lib.check(_lib.lib().efg_track_eval_mot_f32(
        _lib.ptr(weights), _lib.ptr(bo), _lib.ptr(to), _lib.ptr(go), _lib.ptr(rg), _lib.ptr(prob), n, n_frames,
        int(ranges[:, :, 1].max()), int(ranges[:, :, 3].max()), _lib.ptr(scores.contiguous()),
        _lib.ptr(track_ids.contiguous()), _lib.ptr(gt_ids.contiguous()), _lib.ptr(gt_level.contiguous()),
        _lib.ptr(cutoffs.contiguous()), k, _lib.ptr(last), last.shape[1], _lib.ptr(counts), _lib.ptr(sums), _lib.stream()))
    return counts, sums, prob


def accumulate(counts, sums, problems_dev, total_counts, total_sums):
    """total_counts int64 [3, K, 9] and total_sums fp64 [3, K, 2] += the problems of each class, in problem order."""
    _lib.require_gpu(counts, sums, problems_dev, total_counts, total_sums)
    k = counts.shape[1]
    assert total_counts.dtype == torch.int64 and total_counts.shape == (3, k, NUM_COUNTS)
    assert total_sums.dtype == torch.float64 and total_sums.shape == (3, k, NUM_SUMS)
    _lib.check(_lib.lib().efg_track_eval_accumulate(_lib.ptr(counts), _lib.ptr(sums), _lib.ptr(problems_dev),
                                                    counts.shape[0], k, _lib.ptr(total_counts), _lib.ptr(total_sums),
                                                    _lib.stream()))
