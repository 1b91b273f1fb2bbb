"""Waymo-protocol 3-D detection AP / APH (DESIGN.md "Detection evaluation"), streamed.

Stands where the reference pickles every prediction to rank 0 and shells out to a TensorFlow script
(efg/evaluator/waymo_evaluator.py:42-86, datasets/utils/waymo_eval.py): `process` turns a batch into counts at once and adds
them to running totals of fixed size, `evaluate` all-reduces those totals and computes the 12 numbers on the host in fp64.

Two paths over one preparation (masks, heading wrap, score rule, per-class descending-score order):
  * device: csrc/det_eval.hip through operators/det_eval.py -- pair weights, one prefix-incremental assignment per
    (frame, class), totals accumulated on the device;
  * host (CPU tensors or device="cpu"): the fp64 formulation -- detection3d.utils.rot_giou3d for the IoU, one
    scipy.optimize.linear_sum_assignment per (frame, class, cutoff).  It is the yardstick of the device path's tests.
"""
import math

import numpy as np
import torch

from ..operators import det_eval as ops
from .evaluator import DatasetEvaluator

CLASS_NAMES = ("VEHICLE", "PEDESTRIAN", "CYCLIST")       # labels 1, 2, 3
NUM_CUTOFFS = ops.NUM_CUTOFFS
_TWO_PI = 2.0 * math.pi
_HA_GRID = 2.0 ** 30


def score_cutoffs():
    """float32 [101]: 0.00, 0.01, ..., 0.99, 1.0 (waymo_eval.py:125-127), each rounded from its fp64 product."""
    return np.array([np.float32(0.01 * k) for k in range(100)] + [np.float32(1.0)], dtype=np.float32)


def heading_accuracy(yaw_a, yaw_b):
    """1 - (heading error folded to [0, pi]) / pi, in fp64, rounded to a multiple of 2^-30: sums of up to 2^23 such values
    are exact in fp64, so totals do not depend on the order frames were added in."""
    m = np.fmod(np.abs(np.asarray(yaw_a, np.float64) - np.asarray(yaw_b, np.float64)), _TWO_PI)
    acc = 1.0 - np.minimum(m, _TWO_PI - m) / math.pi
    return np.where(acc > 0.0, np.rint(acc * _HA_GRID) / _HA_GRID, 0.0)


def average_precision(num, tp, fp, fn):
    """fp64 [101] each (num = tp for AP, the heading-accuracy sum for APH).  A cutoff without predictions in play gives no
    point; points by ascending recall, the higher cutoff first among equals; precision made non-increasing from the right;
    AP = sum of (recall step) x precision."""
    num, tp, fp, fn = (np.asarray(a, np.float64) for a in (num, tp, fp, fn))
    if not ((tp + fn) > 0).any():
        return 0.0
    valid = ((tp + fp) > 0) & ((tp + fn) > 0)
    k = np.nonzero(valid)[0]
    if k.size == 0:
        return 0.0
    prec, rec = num[k] / (tp[k] + fp[k]), num[k] / (tp[k] + fn[k])
    order = np.lexsort((-k, rec))
    prec, rec = prec[order], rec[order]
    prec = np.maximum.accumulate(prec[::-1])[::-1]
    return float(np.sum(np.diff(np.concatenate(([0.0], rec))) * prec))


def _np(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.array(x, dtype=dtype)


def _wrap(yaw):
    two_pi = np.float32(_TWO_PI)
    return (yaw - np.floor(yaw / two_pi + np.float32(0.5)) * two_pi).astype(np.float32)


class WaymoDetEvaluator(DatasetEvaluator):
    """process(inputs, outputs): `outputs` is the models' list of {"scores", "labels", "boxes3d"}; `inputs` the matching
    list of targets -- a dict with "gt_boxes", "labels" and optionally "difficulty" (default 0) and "num_points_in_gt"
    (default: more than 5), either directly, under "annotations", or as the second element of a (data, info) pair."""

    def __init__(self, config=None, classes=CLASS_NAMES, distance_thresh=100, device=None):
        self.config = config
        unknown = [c for c in classes if c not in CLASS_NAMES]
        if unknown:
            raise ValueError("WaymoDetEvaluator: unknown classes %s (known: %s)" % (unknown, list(CLASS_NAMES)))
        self.classes = tuple(classes)
        self._class_on = np.array([False] + [c in self.classes for c in CLASS_NAMES])      # by label
        self.distance_thresh = float(distance_thresh)
        self.device = None if device is None else torch.device(device)
        self.thresholds = ops.IOU_THRESHOLDS
        self.reset()

    def reset(self):
        self._counts = None        # int64 [3, 101, 5]; created on the device of the first batch
        self._sums = None          # fp64 [3, 101, 3]
        self.min_threshold_margin = math.inf    # host path: the closest a same-class IoU came to its threshold

    # ---- preparation (shared by both paths) -------------------------------------------------------------------------
    @staticmethod
    def _target(item):
        if isinstance(item, (tuple, list)):
            item = item[1]
        return item.get("annotations", item)

    def _in_range(self, boxes):
        return np.hypot(boxes[:, 0].astype(np.float64), boxes[:, 1].astype(np.float64)) < self.distance_thresh + 0.5

    def _frame(self, target, output):
        pb = _np(output["boxes3d"], np.float32)
        pb = pb.reshape(-1, pb.shape[-1] if pb.ndim == 2 else 7)[:, [0, 1, 2, 3, 4, 5, -1]]
        ps, pl = _np(output["scores"], np.float32).reshape(-1), _np(output["labels"], np.int64).reshape(-1)
        keep = self._in_range(pb) & (pl >= 1) & (pl <= 3)
        keep[keep] = self._class_on[pl[keep]]
        pb, ps, pl, pi = pb[keep], ps[keep], pl[keep], np.nonzero(keep)[0]

        gb = _np(target["gt_boxes"], np.float32)
        gb = gb.reshape(-1, gb.shape[-1] if gb.ndim == 2 else 7)[:, [0, 1, 2, 3, 4, 5, -1]]
        gl = _np(target["labels"], np.int64).reshape(-1)
        diff = _np(target["difficulty"], np.int64).reshape(-1) if "difficulty" in target else np.zeros(len(gl), np.int64)
        npts = (_np(target["num_points_in_gt"], np.int64).reshape(-1) if "num_points_in_gt" in target
                else np.full(len(gl), 6, np.int64))
        level = np.where(diff == 0, np.where(npts > 5, 1, 2), diff)
        keep = self._in_range(gb) & (npts > 0) & (gl >= 1) & (gl <= 3)
        keep[keep] = self._class_on[gl[keep]]
        gb, gl, level, gi = gb[keep], gl[keep], level[keep], np.nonzero(keep)[0]
        pb[:, 6], gb[:, 6] = _wrap(pb[:, 6]), _wrap(gb[:, 6])
        # pi / gi: the rows of the output / target that the other arrays hold, through every mask and permutation
        return {"pb": pb, "ps": ps, "pl": pl, "pi": pi, "gb": gb, "gl": gl, "level": level.astype(np.int32), "gi": gi}

    def _prepare(self, inputs, outputs):
        frames = [self._frame(self._target(i), o) for i, o in zip(inputs, outputs)]
        scores = np.concatenate([f["ps"] for f in frames]) if frames else np.zeros(0, np.float32)
        if scores.size and np.nanmax(scores) > 1:      # waymo_eval.py:255-258, over the frames of this call
            for f in frames:
                f["ps"] = (1.0 / (1.0 + np.exp(-f["ps"].astype(np.float64)))).astype(np.float32)
        for f in frames:
            # class-major, descending score inside a class, the lower index first among equal scores
            ps = np.where(np.isnan(f["ps"]), -np.inf, f["ps"]).astype(np.float32)
            order = np.lexsort((np.arange(len(ps)), -ps, f["pl"]))
            f["pb"], f["ps"], f["pl"], f["pi"] = f["pb"][order], ps[order], f["pl"][order], f["pi"][order]
            order = np.argsort(f["gl"], kind="stable")
            f["gb"], f["gl"], f["level"], f["gi"] = f["gb"][order], f["gl"][order], f["level"][order], f["gi"][order]
        return frames

    def _device_of(self, outputs):
        if self.device is not None:
            return self.device
        for o in outputs:
            if isinstance(o["boxes3d"], torch.Tensor):
                return o["boxes3d"].device
        return torch.device("cpu")

    def process(self, inputs, outputs):
        dev = self._device_of(outputs)
        if self._counts is None:
            self._counts = torch.zeros((3, NUM_CUTOFFS, ops.NUM_COUNTS), dtype=torch.int64, device=dev)
            self._sums = torch.zeros((3, NUM_CUTOFFS, ops.NUM_SUMS), dtype=torch.float64, device=dev)
        frames = self._prepare(inputs, outputs)
        if not frames:
            return
        if self._counts.is_cuda:
            self._process_device(frames)
        else:
            self._process_host(frames)

    # ---- device path ------------------------------------------------------------------------------------------------
    def _process_device(self, frames):
        dev = self._counts.device
        pred_off = np.concatenate(([0], np.cumsum([len(f["ps"]) for f in frames])))
        gt_off = np.concatenate(([0], np.cumsum([len(f["gl"]) for f in frames])))
        problems = []
        for i, f in enumerate(frames):
            for c in range(3):
                p0, p1 = np.searchsorted(f["pl"], [c + 1, c + 2])
                g0, g1 = np.searchsorted(f["gl"], [c + 1, c + 2])
                problems.append((i, pred_off[i] + p0, p1 - p0, gt_off[i] + g0, g1 - g0, c))
        problems = ops.check_problems(np.array(problems, dtype=np.int64))     # before anything is launched

        def up(key, dtype, tail=()):
            return torch.from_numpy(np.concatenate([f[key] for f in frames]).astype(dtype).reshape((-1,) + tail)).to(dev)

        pb, gb = up("pb", np.float32, (7,)), up("gb", np.float32, (7,))
        weights, blk = ops.pair_weights(pb, up("pl", np.int32), pred_off, gb, up("gl", np.int32), gt_off, self.thresholds)
        counts, sums, prob = ops.prefix_assign(weights, blk, pred_off, gt_off, problems, up("ps", np.float32), pb, gb,
                                               up("level", np.int32))
        ops.accumulate(counts, sums, prob, self._counts, self._sums)

    # ---- host path: the fp64 formulation ------------------------------------------------------------------------------
    def _process_host(self, frames):
        from scipy.optimize import linear_sum_assignment

        from ..detection3d.utils import rot_giou3d

        cutoffs = score_cutoffs()
        counts, sums = self._counts.numpy(), self._sums.numpy()       # views: updated in place
        for f in frames:
            for c in range(3):
                p0, p1 = np.searchsorted(f["pl"], [c + 1, c + 2])
                g0, g1 = np.searchsorted(f["gl"], [c + 1, c + 2])
                pb, ps = f["pb"][p0:p1].astype(np.float64), f["ps"][p0:p1]
                gb, level = f["gb"][g0:g1].astype(np.float64), f["level"][g0:g1]
                w = np.zeros((p1 - p0, g1 - g0))
                if w.size:
                    iou = rot_giou3d(torch.from_numpy(pb)[:, None, :], torch.from_numpy(gb)[None, :, :],
                                     (1.0, 1.0, 1.0, 0.0))[1].numpy()
                    ok = np.isfinite(iou)
                    w = np.where(ok & (np.where(ok, iou, 0.0) >= self.thresholds[c]), iou, 0.0)
                    if ok.any():
                        self.min_threshold_margin = min(self.min_threshold_margin,
                                                        float(np.abs(iou[ok] - self.thresholds[c]).min()))
                done = None
                for k in range(NUM_CUTOFFS):
                    n = int(np.count_nonzero(ps >= cutoffs[k]))        # a prefix: the scores are sorted
                    if done is None or done[0] != n:
                        rows, cols = linear_sum_assignment(w[:n], maximize=True) if n and w.shape[1] else ((), ())
                        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
                        hit = w[rows, cols] > 0
                        rows, cols = rows[hit], cols[hit]
                        matched = np.zeros(g1 - g0, bool)
                        matched[cols] = True
                        acc = heading_accuracy(pb[rows, 6], gb[cols, 6])
                        l1, l2 = level[cols] <= 1, level[cols] <= 2
                        done = (n, np.array([l1.sum(), l2.sum(), n - len(rows), (~matched & (level <= 1)).sum(),
                                             (~matched & (level <= 2)).sum()], np.int64),
                                np.array([acc[l1].sum(), acc[l2].sum(), w[rows, cols].sum()]))
                    counts[c, k] += done[1]
                    sums[c, k] += done[2]

    # ---- summary ----------------------------------------------------------------------------------------------------------
    def totals(self):
        """(counts int64 [3, 101, 5], sums fp64 [3, 101, 3]) on the host, summed over the ranks of an initialised
        torch.distributed group.  Integers and grid-rounded heading accuracies: the sum does not depend on the order."""
        if self._counts is None:
            counts = torch.zeros((3, NUM_CUTOFFS, ops.NUM_COUNTS), dtype=torch.int64)
            sums = torch.zeros((3, NUM_CUTOFFS, ops.NUM_SUMS), dtype=torch.float64)
        else:
            counts, sums = self._counts.clone(), self._sums.clone()
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            if torch.distributed.get_backend() == "gloo":
                counts, sums = counts.cpu(), sums.cpu()
            torch.distributed.all_reduce(counts)
            torch.distributed.all_reduce(sums)
        return counts.cpu(), sums.cpu()

    def evaluate(self):
        counts, sums = (t.numpy() for t in self.totals())
        table = np.zeros((3, 2, NUM_CUTOFFS, 4))
        result = {}
        for c, name in enumerate(CLASS_NAMES):
            for lv in range(2):
                tp, fp, fn, ha = counts[c, :, lv], counts[c, :, 2], counts[c, :, 3 + lv], sums[c, :, lv]
                table[c, lv] = np.stack([tp, fp, fn, ha], -1)
                key = "OBJECT_TYPE_TYPE_%s_LEVEL_%d/" % (name, lv + 1)
                result[key + "AP"] = average_precision(tp, tp, fp, fn)
                result[key + "APH"] = average_precision(ha, tp, fp, fn)
        result["counts"] = torch.from_numpy(table)
        return result
