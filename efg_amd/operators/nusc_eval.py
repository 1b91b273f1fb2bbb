"""nuScenes detection-evaluation kernels (csrc/nusc_eval.hip) -- thin wrappers over libefg_hip.so.

(frame, class) CSR layout: the predictions and ground truths of the frames of one call are concatenated, boxes are fp32
[n, 9] = (x, y, z, l, w, h, yaw, vx, vy), and a row of `problems` (host int [n, 5]: first prediction, predictions, first
ground truth, ground truths, class) names one class of one frame, its predictions sorted by descending score.  The problem
table is built and checked on the host; everything else is on the device.  There is no CPU compute path here; the fp64 host
formulation lives in efg_amd/evaluator/nuscenes.py.
"""
import numpy as np
import torch

from .. import _lib

DIST_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)      # metres; the errors are those of the true positives at index TP_THRESHOLD
TP_THRESHOLD = 2
NUM_ERRORS = 5                              # trans, scale, orient, vel, attr
BOX_DIM = 9


def max_gt():
    """Ground truths one (frame, class) problem may hold."""
    return _lib.lib().efg_nusc_eval_max_gt()


def check_problems(problems, n_pred, n_gt):
    """The host-side check of `greedy_match`: raises, never truncates.  problems: host int [n, 5]."""
    problems = np.asarray(problems, dtype=np.int64).reshape(-1, 5)
    if len(problems):
        limit = max_gt()
        if problems[:, 3].max() > limit:
            raise RuntimeError("efg_amd nusc_eval: %d ground truths of one class in one frame exceed the limit of %d"
                               % (problems[:, 3].max(), limit))
        ok = ((problems[:, :4] >= 0).all() and (problems[:, 0] + problems[:, 1]).max() <= n_pred
              and (problems[:, 2] + problems[:, 3]).max() <= n_gt)
        if not ok:
            raise RuntimeError("efg_amd nusc_eval: a problem lies outside the %d predictions / %d ground truths of the call"
                               % (n_pred, n_gt))
    return problems


def greedy_match(pred_boxes, gt_boxes, problems, thresholds=DIST_THRESHOLDS):
    """pred_boxes [sum P, 9], gt_boxes [sum G, 9] fp32 on the device, problems host int [n, 5] -> match int32 [4, sum P]:
    per distance threshold the global ground-truth row a prediction took, or -1.  In score order a prediction takes the
    nearest ground truth of its problem that is still free at that threshold, if it is closer than the threshold (strictly;
    equal distances: the lowest row).  One launch, one workgroup per problem."""
    _lib.require_gpu(pred_boxes, gt_boxes)
    assert pred_boxes.shape[1:] == (BOX_DIM,) and gt_boxes.shape[1:] == (BOX_DIM,), "boxes must be (N, 9)"
    assert pred_boxes.dtype == gt_boxes.dtype == torch.float32
    assert len(thresholds) == 4
    n_pred, n_gt = pred_boxes.shape[0], gt_boxes.shape[0]
    problems = check_problems(problems, n_pred, n_gt)           # before anything is launched
    match = torch.full((4, n_pred), -1, dtype=torch.int32, device=pred_boxes.device)
    if n_pred == 0 or len(problems) == 0:
        return match
    prob = torch.from_numpy(np.ascontiguousarray(problems, dtype=np.int32)).to(pred_boxes.device)
    _lib.check(_lib.lib().efg_nusc_eval_match_f32(
        _lib.ptr(pred_boxes.contiguous()), _lib.ptr(gt_boxes.contiguous()), _lib.ptr(prob), len(problems),
        int(problems[:, 3].max()), n_pred, n_gt, *(float(t) for t in thresholds), _lib.ptr(match), _lib.stream()))
    return match


def match_errors(pred_boxes, pred_attr, pred_class, gt_boxes, gt_attr, match, barrier_class=-1):
    """-> (tp_bits int32 [sum P]: bit t set where match[t] >= 0, err fp64 [sum P, 5]: translation, scale, orientation,
    velocity and attribute error against the ground truth match[TP_THRESHOLD]; NaN where there is none, where its velocity
    is NaN (velocity) or its attribute code is < 0 (attribute)).  pred_attr / pred_class int32 [sum P], gt_attr int32
    [sum G]; the orientation error has period pi for pred_class == barrier_class.  One launch."""
    _lib.require_gpu(pred_boxes, pred_attr, pred_class, gt_boxes, gt_attr, match)
    assert pred_boxes.shape[1:] == (BOX_DIM,) and gt_boxes.shape[1:] == (BOX_DIM,), "boxes must be (N, 9)"
    assert pred_boxes.dtype == gt_boxes.dtype == torch.float32
    assert pred_attr.dtype == pred_class.dtype == gt_attr.dtype == match.dtype == torch.int32
    n_pred, n_gt = pred_boxes.shape[0], gt_boxes.shape[0]
    assert match.shape == (4, n_pred) and pred_attr.shape == pred_class.shape == (n_pred,) and gt_attr.shape == (n_gt,)
    tp_bits = torch.zeros((n_pred,), dtype=torch.int32, device=pred_boxes.device)
    err = torch.empty((n_pred, NUM_ERRORS), dtype=torch.float64, device=pred_boxes.device)
    if n_pred == 0:
        return tp_bits, err
    _lib.check(_lib.lib().efg_nusc_eval_errors_f32(
        _lib.ptr(pred_boxes.contiguous()), _lib.ptr(pred_attr.contiguous()), _lib.ptr(pred_class.contiguous()),
        _lib.ptr(gt_boxes.contiguous()), _lib.ptr(gt_attr.contiguous()), _lib.ptr(match.contiguous()), n_pred, n_gt,
        int(barrier_class), _lib.ptr(tp_bits), _lib.ptr(err), _lib.stream()))
    return tp_bits, err
