"""nuScenes detection protocol (DESIGN.md "nuScenes detection evaluation"): mAP, the five mean true-positive errors and NDS,
streamed.

Stands where the reference pickles every prediction to rank 0, rewrites each box through pyquaternion into a JSON file and
calls the devkit's `NuScenesEval` (efg/evaluator/nuscenes_evaluator.py); neither `nuscenes` nor `pyquaternion` exists here, so
the protocol (`detection_cvpr_2019`) is restated in DESIGN.md and implemented from that text.  `process` turns a batch into one
record per kept prediction -- score, class, a true-positive bit per distance threshold, five errors -- and `evaluate` gathers
the records in rank order and computes curves and scores on the host in fp64, with one function for both paths.

Two paths over one preparation (class ranges, the point-count mask, the 500-per-frame rule, per-class descending-score order,
attribute codes):
  * device: csrc/nusc_eval.hip through operators/nusc_eval.py -- one greedy-matching launch and one error launch per call,
    records kept on the device;
  * host (CPU tensors or device="cpu"): the fp64 formulation in numpy, a Python loop per prediction.  It is the yardstick of
    the device path's tests.
"""
import math
import operator

import numpy as np
import torch

from ..operators import nusc_eval as ops
from .evaluator import DatasetEvaluator

CLASS_NAMES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
               "traffic_cone")                                   # labels 1..10, as CenterHead.predict emits them
CLASS_RANGE = {"car": 50.0, "truck": 50.0, "bus": 50.0, "trailer": 50.0, "construction_vehicle": 50.0, "pedestrian": 40.0,
               "motorcycle": 40.0, "bicycle": 40.0, "traffic_cone": 30.0, "barrier": 30.0}
DIST_THRESHOLDS = ops.DIST_THRESHOLDS
TP_THRESHOLD = ops.TP_THRESHOLD                                  # the errors are those of the true positives at 2 m
MAX_PRED_PER_FRAME = 500
ERRORS = ("trans", "scale", "orient", "vel", "attr")
ERROR_KEYS = {"trans": "ATE", "scale": "ASE", "orient": "AOE", "vel": "AVE", "attr": "AAE"}
UNDEFINED = {"traffic_cone": ("orient", "vel", "attr"), "barrier": ("vel", "attr")}     # class -> errors that are NaN
MIN_RECALL, MIN_PRECISION, NUM_RECALLS = 0.1, 0.1, 101
MOVING_SPEED = 0.2
ATTR_MOVING = {"car": "vehicle.moving", "construction_vehicle": "vehicle.moving", "bus": "vehicle.moving",
               "truck": "vehicle.moving", "trailer": "vehicle.moving", "bicycle": "cycle.with_rider",
               "motorcycle": "cycle.with_rider"}
ATTR_STILL = {"pedestrian": "pedestrian.standing", "bus": "vehicle.stopped"}
_NO_GT_ATTR, _NO_PRED_ATTR = -1, -2                              # never equal: a prediction without attribute matches nothing


# ---- the fp64 formulation: matching and errors ----------------------------------------------------------------------------
def centre_distances(pred_xy, gt_xy):
    """fp64 [P, G]: sqrt(dx * dx + dy * dy) on the float32 centres, in this operation order (numpy does not contract)."""
    p, g = np.asarray(pred_xy, np.float32).astype(np.float64), np.asarray(gt_xy, np.float32).astype(np.float64)
    dx, dy = p[:, None, 0] - g[None, :, 0], p[:, None, 1] - g[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def greedy_match(dist, thresholds=DIST_THRESHOLDS):
    """dist fp64 [P, G], rows by descending score -> int64 [len(thresholds), P]: the column a prediction took, or -1.  In row
    order a prediction takes the nearest column not yet taken at this threshold if its distance is < the threshold; equal
    distances go to the lowest column; a NaN distance is never taken."""
    n_p, n_g = dist.shape
    out = np.full((len(thresholds), n_p), -1, np.int64)
    if n_g == 0:
        return out
    dist = np.where(np.isnan(dist), np.inf, dist)
    for t, thr in enumerate(thresholds):
        thr = float(np.float32(thr))
        free = np.zeros(n_g)
        for i in range(n_p):
            d = dist[i] + free                        # taken columns: + inf
            j = int(np.argmin(d))                     # the first of equal minima
            if d[j] < thr:
                out[t, i] = j
                free[j] = np.inf
    return out


def pair_errors(pred, pred_attr, gt, gt_attr, barrier):
    """The five errors of matched pairs, fp64 [n, 5].  pred / gt float32 [n, 9] = (x, y, z, l, w, h, yaw, vx, vy), attribute
    codes int [n] (gt < 0: none -> NaN), barrier bool [n]: orientation period pi instead of 2 pi."""
    p, g = np.asarray(pred, np.float32).astype(np.float64), np.asarray(gt, np.float32).astype(np.float64)
    err = np.full((len(p), len(ERRORS)), np.nan)
    if not len(p):
        return err
    with np.errstate(invalid="ignore", divide="ignore"):
        dx, dy = p[:, 0] - g[:, 0], p[:, 1] - g[:, 1]
        err[:, 0] = np.sqrt(dx * dx + dy * dy)
        inter = np.fmin(p[:, 3], g[:, 3]) * np.fmin(p[:, 4], g[:, 4]) * np.fmin(p[:, 5], g[:, 5])
        vol_p, vol_g = p[:, 3] * p[:, 4] * p[:, 5], g[:, 3] * g[:, 4] * g[:, 5]
        err[:, 1] = 1.0 - inter / (vol_p + vol_g - inter)
        period = np.where(np.asarray(barrier, bool), math.pi, 2.0 * math.pi)
        r = np.fmod(p[:, 6] - g[:, 6] + period / 2.0, period)
        r = np.where(r < 0.0, r + period, r)          # the floored remainder
        a = np.abs(r - period / 2.0)
        err[:, 2] = np.where(a > math.pi, 2.0 * math.pi - a, a)
        dvx, dvy = p[:, 7] - g[:, 7], p[:, 8] - g[:, 8]
        err[:, 3] = np.sqrt(dvx * dvx + dvy * dvy)
    pred_attr, gt_attr = np.asarray(pred_attr), np.asarray(gt_attr)
    err[:, 4] = np.where(gt_attr < 0, np.nan, (pred_attr != gt_attr).astype(np.float64))
    return err


# ---- the summary: curves and scores, one function for both paths --------------------------------------------------------------
def cummean(x):
    """NaN-aware cumulative mean; an all-NaN series gives ones."""
    x = np.asarray(x, np.float64)
    if np.isnan(x).all():
        return np.ones(len(x))
    total, count = np.nancumsum(x), np.cumsum(~np.isnan(x))
    return np.divide(total, count, out=np.zeros_like(total), where=count != 0)


def accumulate(score, tp, npos, err=None):
    """One class at one threshold.  score fp [n] sorted by descending score, tp bool [n], npos ground truths, err fp64 [n, 5]
    or None -> (precision [101], confidence [101], error series [5, 101] or None) on the recall grid linspace(0, 1, 101)."""
    tp = np.asarray(tp, bool)
    if npos == 0 or not tp.any():                     # the no-prediction curve
        return np.zeros(NUM_RECALLS), np.zeros(NUM_RECALLS), (None if err is None else np.ones((len(ERRORS), NUM_RECALLS)))
    score = np.asarray(score, np.float64)
    tpc, fpc = np.cumsum(tp).astype(np.float64), np.cumsum(~tp).astype(np.float64)
    prec, rec = tpc / (fpc + tpc), tpc / float(npos)
    grid = np.linspace(0, 1, NUM_RECALLS)
    prec = np.interp(grid, rec, prec, right=0)
    conf = np.interp(grid, rec, score, right=0)
    series = None
    if err is not None:
        tp_conf = score[tp]
        series = np.stack([np.interp(conf[::-1], tp_conf[::-1], cummean(err[tp, k])[::-1])[::-1] for k in range(len(ERRORS))])
    return prec, conf, series


def average_precision(prec):
    first = round(100 * MIN_RECALL) + 1
    return float(np.mean(np.maximum(np.asarray(prec, np.float64)[first:] - MIN_PRECISION, 0.0))) / (1.0 - MIN_PRECISION)


def tp_metric(series, conf):
    """Mean of an error series over recall indices 11 .. the last one with a confidence != 0; 1.0 if there is none."""
    first = round(100 * MIN_RECALL) + 1
    nz = np.nonzero(conf)[0]
    last = int(nz[-1]) if len(nz) else 0
    return 1.0 if last < first else float(np.mean(series[first:last + 1]))


def _nanmean(values):
    values = np.asarray(values, np.float64)
    ok = ~np.isnan(values)
    return float(values[ok].mean()) if ok.any() else math.nan


def nd_score(mean_ap, mean_errors):
    """NDS = (5 mAP + sum over the five mean errors of 1 - min(1, error)) / 10."""
    return (5.0 * mean_ap + sum(1.0 - min(1.0, e) for e in mean_errors)) / 10.0


def summarize(score, cls, tp_bits, err, npos, classes=CLASS_NAMES, thresholds=DIST_THRESHOLDS):
    """score fp32 [N], cls int [N] (index into `classes`), tp_bits int [N] (bit t: true positive at thresholds[t]), err fp64
    [N, 5], npos int [len(classes)], all in stream order -> the result dict of NuScenesDetEvaluator.evaluate()."""
    score, cls, tp_bits, err = np.asarray(score), np.asarray(cls), np.asarray(tp_bits), np.asarray(err, np.float64)
    result, aps, errors = {}, [], {e: [] for e in ERRORS}
    for c, name in enumerate(classes):
        rows = np.nonzero(cls == c)[0]
        rows = rows[np.argsort(-score[rows].astype(np.float64), kind="stable")]      # ties keep stream order
        s, bits, e = score[rows], tp_bits[rows], err[rows]
        class_ap = []
        for t, thr in enumerate(thresholds):
            prec, conf, series = accumulate(s, (bits >> t) & 1, int(npos[c]), e if t == TP_THRESHOLD else None)
            result["AP/%s/%s" % (name, thr)] = average_precision(prec)
            class_ap.append(result["AP/%s/%s" % (name, thr)])
            if t == TP_THRESHOLD:
                for k, key in enumerate(ERRORS):
                    value = math.nan if key in UNDEFINED.get(name, ()) else tp_metric(series[k], conf)
                    result["%s/%s" % (ERROR_KEYS[key], name)] = value
                    errors[key].append(value)
        result["AP/%s" % name] = float(np.mean(class_ap))
        aps.append(result["AP/%s" % name])
    result["mAP"] = float(np.mean(aps)) if aps else math.nan
    for key in ERRORS:
        result["m" + ERROR_KEYS[key]] = _nanmean(errors[key])
    result["NDS"] = nd_score(result["mAP"], [result["m" + ERROR_KEYS[key]] for key in ERRORS])
    return result


def _np(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.array(x, dtype=dtype)


def _boxes9(x, what):
    """[n, 7] (x, y, z, l, w, h, yaw) or [n, 9] (x, y, z, l, w, h, vx, vy, yaw) -> float32 [n, 9] (..., yaw, vx, vy); seven
    columns count as zero velocity."""
    b = _np(x, np.float32)
    b = b.reshape(-1, b.shape[-1] if b.ndim == 2 else 7)
    if b.shape[1] == 9:
        return np.ascontiguousarray(b[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]])
    if b.shape[1] == 7:
        return np.concatenate((b, np.zeros((len(b), 2), np.float32)), axis=1)
    raise ValueError("NuScenesDetEvaluator: %s with %d columns (7 or 9 expected)" % (what, b.shape[1]))


class NuScenesDetEvaluator(DatasetEvaluator):
    """process(inputs, outputs): `outputs` is the models' list of {"scores", "labels", "boxes3d"} (boxes [P, 9] with the
    velocity in columns 6:8, or [P, 7]); `inputs` the matching list of targets -- a dict with "gt_boxes" [G, 7 or 9], "labels"
    and optionally "num_points_in_gt", "attributes" (strings, '' = none) and "ego_xy", either directly, under "annotations",
    or as the second element of a (data, info) pair.  Labels are 1..len(classes), indices into `classes`.

    The default attribute of a class comes from `default_attributes` (class -> attribute) or, as the reference passes it,
    from meta["cls_attr_dist"] (class -> {attribute: count}, the most frequent one); a class without either has none."""

    def __init__(self, config=None, classes=CLASS_NAMES, meta=None, default_attributes=None, device=None):
        self.config = config
        if classes is CLASS_NAMES and config is not None:
            try:
                classes = tuple(config.dataset.classes)
            except (AttributeError, KeyError):
                pass
        unknown = [c for c in classes if c not in CLASS_RANGE]
        if unknown:
            raise ValueError("NuScenesDetEvaluator: unknown classes %s (known: %s)" % (unknown, list(CLASS_NAMES)))
        self.classes = tuple(classes)
        self.thresholds = DIST_THRESHOLDS
        self.device = None if device is None else torch.device(device)
        self._range = np.array([np.inf] + [CLASS_RANGE[c] for c in self.classes])          # by label
        self._barrier = self.classes.index("barrier") if "barrier" in self.classes else -1  # class index
        defaults = {}
        for name, dist in dict((meta or {}).get("cls_attr_dist", {})).items():
            items = list(dict(dist).items())
            if items:
                defaults[name] = max(items, key=operator.itemgetter(1))[0]
        defaults.update(default_attributes or {})
        self.default_attributes = {c: defaults.get(c, "") for c in self.classes}
        self._attr_codes = {}
        # by label: the attribute code of a prediction that moves / does not move
        self._attr_moving = np.array([_NO_PRED_ATTR] + [self._code(ATTR_MOVING.get(c, self.default_attributes[c]), True)
                                                        for c in self.classes])
        self._attr_still = np.array([_NO_PRED_ATTR] + [self._code(ATTR_STILL.get(c, self.default_attributes[c]), True)
                                                       for c in self.classes])
        self.reset()

    def reset(self):
        self._records = []         # per call: (score fp32 [P], class int32 [P], tp bits int32 [P], errors fp64 [P, 5])
        self._npos = np.zeros(len(self.classes), np.int64)
        self._dev = None           # the device of the first batch

    def _code(self, name, pred=False):
        if name is None or name == "":
            return _NO_PRED_ATTR if pred else _NO_GT_ATTR
        return self._attr_codes.setdefault(str(name), len(self._attr_codes))

    # ---- preparation (shared by both paths) -------------------------------------------------------------------------
    @staticmethod
    def _target(item):
        if isinstance(item, (tuple, list)):
            item = item[1]
        return item.get("annotations", item)

    def _in_range(self, boxes, labels, ego):
        dx, dy = boxes[:, 0].astype(np.float64) - ego[0], boxes[:, 1].astype(np.float64) - ego[1]
        return np.sqrt(dx * dx + dy * dy) < self._range[labels]

    def _labels(self, x, what):
        labels = _np(x, np.int64).reshape(-1)
        if labels.size and (labels.min() < 1 or labels.max() > len(self.classes)):
            raise ValueError("NuScenesDetEvaluator: %s labels outside 1..%d" % (what, len(self.classes)))
        return labels

    def _frame(self, target, output):
        ego = tuple(float(v) for v in _np(target.get("ego_xy", (0.0, 0.0)), np.float64).reshape(-1)[:2])
        pb, pl = _boxes9(output["boxes3d"], "boxes3d"), self._labels(output["labels"], "prediction")
        ps = _np(output["scores"], np.float32).reshape(-1)
        keep = self._in_range(pb, pl, ego)
        pb, ps, pl = pb[keep], ps[keep], pl[keep]
        if len(ps) > MAX_PRED_PER_FRAME:
            raise RuntimeError("NuScenesDetEvaluator: %d predictions in one frame (the protocol allows %d; nothing is "
                               "truncated)" % (len(ps), MAX_PRED_PER_FRAME))
        vx, vy = pb[:, 7].astype(np.float64), pb[:, 8].astype(np.float64)
        with np.errstate(invalid="ignore"):
            moving = np.sqrt(vx * vx + vy * vy) > MOVING_SPEED
        pa = np.where(moving, self._attr_moving[pl], self._attr_still[pl])

        gb, gl = _boxes9(target["gt_boxes"], "gt_boxes"), self._labels(target["labels"], "ground-truth")
        if "attributes" in target:
            ga = np.array([self._code(a) for a in target["attributes"]], np.int64).reshape(-1)
        else:
            ga = np.full(len(gl), _NO_GT_ATTR, np.int64)
        if not len(gb) == len(gl) == len(ga):
            raise ValueError("NuScenesDetEvaluator: %d gt_boxes, %d labels, %d attributes" % (len(gb), len(gl), len(ga)))
        keep = self._in_range(gb, gl, ego)
        if "num_points_in_gt" in target:
            keep &= _np(target["num_points_in_gt"], np.int64).reshape(-1) != 0
        gb, gl, ga = gb[keep], gl[keep], ga[keep]

        # class-major, descending score inside a class, the lower row first among equal scores
        ps = np.where(np.isnan(ps), -np.inf, ps).astype(np.float32)
        order = np.lexsort((np.arange(len(ps)), -ps, pl))
        pb, ps, pl, pa = pb[order], ps[order], pl[order], pa[order]
        order = np.argsort(gl, kind="stable")
        gb, gl, ga = gb[order], gl[order], ga[order]
        return {"pb": pb, "ps": ps, "pl": pl, "pa": pa.astype(np.int32), "gb": gb, "gl": gl, "ga": ga.astype(np.int32)}

    def _prepare(self, inputs, outputs):
        return [self._frame(self._target(i), o) for i, o in zip(inputs, outputs)]

    def problems(self, frames):
        """int64 [F * C, 5]: (first prediction, predictions, first ground truth, ground truths, class) of every class of
        every prepared frame, rows of the call's concatenation."""
        pred_off = np.concatenate(([0], np.cumsum([len(f["ps"]) for f in frames])))
        gt_off = np.concatenate(([0], np.cumsum([len(f["gl"]) for f in frames])))
        rows = []
        for i, f in enumerate(frames):
            for c in range(len(self.classes)):
                p0, p1 = np.searchsorted(f["pl"], [c + 1, c + 2])
                g0, g1 = np.searchsorted(f["gl"], [c + 1, c + 2])
                rows.append((pred_off[i] + p0, p1 - p0, gt_off[i] + g0, g1 - g0, c))
        return np.array(rows, dtype=np.int64).reshape(-1, 5)

    def _device_of(self, outputs):
        if self.device is not None:
            return self.device
        for o in outputs:
            if isinstance(o["boxes3d"], torch.Tensor):
                return o["boxes3d"].device
        return torch.device("cpu")

    def process(self, inputs, outputs):
        if self._dev is None:
            self._dev = self._device_of(outputs)
        frames = self._prepare(inputs, outputs)
        if not frames:
            return
        run = self.device_records(frames, self._dev) if self._dev.type == "cuda" else self.host_records(frames)
        for f in frames:
            self._npos += np.bincount(f["gl"] - 1, minlength=len(self.classes))
        self._records.append((run["score"], run["cls"], run["tp_bits"], run["err"]))

    # ---- device path ------------------------------------------------------------------------------------------------
    def device_records(self, frames, dev):
        """The records of one call on the device, with the kernel's `match` int32 [4, sum P] (global ground-truth rows)."""
        problems = ops.check_problems(self.problems(frames), sum(len(f["ps"]) for f in frames),
                                      sum(len(f["gl"]) for f in frames))            # before anything is uploaded or launched

        def up(key, dtype, tail=()):
            return torch.from_numpy(np.concatenate([f[key] for f in frames]).astype(dtype).reshape((-1,) + tail)).to(dev)

        pb, gb = up("pb", np.float32, (ops.BOX_DIM,)), up("gb", np.float32, (ops.BOX_DIM,))
        cls = torch.from_numpy((np.concatenate([f["pl"] for f in frames]) - 1).astype(np.int32)).to(dev)
        match = ops.greedy_match(pb, gb, problems, self.thresholds)
        tp_bits, err = ops.match_errors(pb, up("pa", np.int32), cls, gb, up("ga", np.int32), match, self._barrier)
        return {"score": up("ps", np.float32), "cls": cls, "tp_bits": tp_bits, "err": err, "match": match}

    # ---- host path: the fp64 formulation ------------------------------------------------------------------------------
    def host_records(self, frames):
        """The records of one call in fp64 numpy (as CPU tensors), with `match` int32 [4, sum P]."""
        problems = self.problems(frames)
        cat = {k: np.concatenate([f[k] for f in frames]) for k in ("pb", "ps", "pl", "pa", "gb", "ga")}
        n_pred = len(cat["ps"])
        match = np.full((len(self.thresholds), n_pred), -1, np.int32)
        for p0, n_p, g0, n_g, _ in problems:
            if n_p and n_g:
                local = greedy_match(centre_distances(cat["pb"][p0:p0 + n_p, :2], cat["gb"][g0:g0 + n_g, :2]), self.thresholds)
                match[:, p0:p0 + n_p] = np.where(local >= 0, local + g0, -1)
        tp_bits = np.zeros(n_pred, np.int32)
        for t in range(len(self.thresholds)):
            tp_bits |= (match[t] >= 0).astype(np.int32) << t
        err = np.full((n_pred, len(ERRORS)), np.nan)
        rows = np.nonzero(match[TP_THRESHOLD] >= 0)[0]
        cols = match[TP_THRESHOLD][rows]
        cls = (cat["pl"] - 1).astype(np.int32)
        err[rows] = pair_errors(cat["pb"][rows], cat["pa"][rows], cat["gb"][cols], cat["ga"][cols], cls[rows] == self._barrier)
        return {"score": torch.from_numpy(cat["ps"].astype(np.float32)), "cls": torch.from_numpy(cls),
                "tp_bits": torch.from_numpy(tp_bits), "err": torch.from_numpy(err), "match": torch.from_numpy(match)}

    # ---- summary ----------------------------------------------------------------------------------------------------------
    def records(self):
        """(score fp32 [N], class int64 [N], tp bits int64 [N], errors fp64 [N, 5], npos int64 [C]) on the host: this rank's
        records in stream order, or, in an initialised torch.distributed group, every rank's in rank order (a padded
        all_gather: the records differ in length) with npos summed."""
        dev = self._dev if self._dev is not None else torch.device("cpu")
        if self._records:
            parts = [torch.cat([r[k] for r in self._records]) for k in range(4)]
        else:
            parts = [torch.zeros(0, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                     torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros((0, len(ERRORS)), dtype=torch.float64, device=dev)]
        # one fp64 row per record: score, class, tp bits (exact in fp64), the five errors
        packed = torch.cat([parts[0].double()[:, None], parts[1].double()[:, None], parts[2].double()[:, None], parts[3]], dim=1)
        npos = torch.from_numpy(self._npos.copy())
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            dist = torch.distributed
            if dist.get_backend() == "gloo":
                packed = packed.cpu()
            else:
                packed = packed.to(torch.device("cuda", torch.cuda.current_device()))
            npos = npos.to(packed.device)
            lengths = [torch.zeros(1, dtype=torch.int64, device=packed.device) for _ in range(dist.get_world_size())]
            dist.all_gather(lengths, torch.tensor([packed.shape[0]], dtype=torch.int64, device=packed.device))
            longest = max(int(n) for n in lengths)
            padded = torch.zeros((longest, packed.shape[1]), dtype=torch.float64, device=packed.device)
            padded[:packed.shape[0]] = packed
            gathered = [torch.zeros_like(padded) for _ in lengths]
            dist.all_gather(gathered, padded)
            packed = torch.cat([g[:int(n)] for g, n in zip(gathered, lengths)])
            dist.all_reduce(npos)
        packed = packed.cpu().numpy()
        return (packed[:, 0].astype(np.float32), packed[:, 1].astype(np.int64), packed[:, 2].astype(np.int64),
                np.ascontiguousarray(packed[:, 3:]), npos.cpu().numpy())

    def evaluate(self):
        score, cls, tp_bits, err, npos = self.records()
        return summarize(score, cls, tp_bits, err, npos, self.classes, self.thresholds)


nuScenesDetEvaluator = NuScenesDetEvaluator      # the reference's name (efg/evaluator/nuscenes_evaluator.py:86)
