"""Waymo-protocol 3-D tracking MOTA / MOTP / MISS / MISMATCH / FP (DESIGN.md "Tracking evaluation"), streamed.

Stands where the reference serialises protobufs and shells out to `compute_tracking_metrics_main`
(playground/tracking.3d/waymo/trajectoryformer/*/track_evaluator.py): `process` takes the online tracker's frames
({"track_ids", "track_boxes3d", "track_scores", "track_labels"}) in sequence order, `evaluate` all-reduces totals of fixed
size and computes the 30 numbers on the host in fp64.

The preparation (masks, levels, score rule, class-major descending-score order) is WaymoDetEvaluator's, through its own
code; on top of it the track ids and the targets' `gt_ids` are carried through the same masks and permutations, and the
ground truths of a class are ordered by dense id (the order in which a gt_id first appeared in its sequence).  Two paths
over that preparation run one CLEAR MOT state machine per (sequence, class, score cutoff):
  * device: csrc/track_eval.hip through operators/track_eval.py -- the detection evaluator's pair weights, then one
    workgroup per (class, cutoff) that walks the buffered frames of the open sequence; the map `last` lives in a device
    table between flushes;
  * host (CPU tensors or device="cpu"): the fp64 formulation -- detection3d.utils.rot_giou3d for the IoU, a dict for
    `last`, scipy.optimize.linear_sum_assignment for the residual assignment (`clear_mot_frame`).  It is the yardstick of
    the device path's tests.
"""
import numpy as np
import torch

from ..operators import track_eval as ops
from .waymo import CLASS_NAMES, WaymoDetEvaluator, _np

COUNT_NAMES = ("match1", "match2", "fp", "miss1", "miss2", "mismatch1", "mismatch2", "gt1", "gt2")
METRICS = ("MOTA", "MOTP", "MISS", "MISMATCH", "FP")
_COST_GRID = 2.0 ** 30


def score_cutoffs():
    """float32 [11]: 0.0, 0.1, ..., 0.9, each rounded from its fp64 product, and 1.0."""
    return np.array([np.float32(0.1 * k) for k in range(10)] + [np.float32(1.0)], dtype=np.float32)


def match_cost(w):
    """1 - weight in fp64, rounded to a multiple of 2^-30: sums of up to 2^23 such values are exact in fp64, so totals do
    not depend on how frames were chunked or spread over ranks."""
    return np.rint((1.0 - np.asarray(w, np.float64)) * _COST_GRID) / _COST_GRID


def clear_mot_frame(w, scores, track_ids, gt_ids, level, cutoffs, last, carry_over=True, stats=None):
    """One frame of one class through the CLEAR MOT state machine, at every cutoff.

    w [P, G]: pair weights (0 = no edge), rows sorted by descending score; scores float32 [P]; track_ids [P] and gt_ids [G]:
    hashable ids (the evaluator passes dense ints), gt_ids sortable; level int [G]; cutoffs float32 [K]; last: K dicts
    gt id -> id of the track it was most recently matched to, updated in place.  carry_over=False skips step 1 (every
    pair then comes from the assignment: plain per-frame Hungarian matching).  stats: a dict whose "kept" (pairs carried over)
    and "conflicts" (carry-overs lost to a ground truth of lower id) are counted up; if it holds a set "pairs", the (row,
    column) of every pair of the call is added to it.
    Returns (counts int64 [K, 9] in the order of COUNT_NAMES, cost fp64 [K, 2])."""
    from scipy.optimize import linear_sum_assignment

    w = np.asarray(w, np.float64).reshape(len(track_ids), len(gt_ids))
    w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
    scores, level = np.asarray(scores, np.float32), np.asarray(level, np.int64)
    n_gt = len(gt_ids)
    counts, cost = np.zeros((len(cutoffs), 9), np.int64), np.zeros((len(cutoffs), 2), np.float64)
    by_id = sorted(range(n_gt), key=lambda g: gt_ids[g])
    for k, cut in enumerate(np.asarray(cutoffs, np.float32)):
        n = int(np.count_nonzero(scores >= cut))                 # a prefix: the scores are sorted
        row_of = {track_ids[r]: r for r in range(n)}
        prev = [last[k].get(gt_ids[g]) for g in range(n_gt)]
        row = np.full(n_gt, -1, np.int64)
        kept, taken = np.zeros(n_gt, bool), np.zeros(n, bool)
        if carry_over:
            for g in by_id:
                r = row_of.get(prev[g]) if prev[g] is not None else None
                if r is not None and w[r, g] > 0:
                    if not taken[r]:
                        row[g], kept[g], taken[r] = r, True, True
                    if stats is not None:
                        what = "kept" if kept[g] else "conflicts"
                        stats[what] = stats.get(what, 0) + 1
        rows, cols = np.nonzero(~taken)[0], np.nonzero(~kept)[0]
        if len(rows) and len(cols):
            sub = w[np.ix_(rows, cols)]
            for a, b in zip(*linear_sum_assignment(sub, maximize=True)):
                if sub[a, b] > 0:
                    row[cols[b]] = rows[a]
        matched = row >= 0
        new = matched & ~kept
        switch = np.array([new[g] and prev[g] is not None and prev[g] != track_ids[row[g]] for g in range(n_gt)], bool)
        term = np.zeros(n_gt)
        term[matched] = match_cost(w[row[matched], np.nonzero(matched)[0]])
        for lv in (1, 2):
            on = level <= lv
            counts[k, lv - 1] = (matched & on).sum()
            counts[k, 2 + lv] = (~matched & on).sum()
            counts[k, 4 + lv] = (switch & on).sum()
            counts[k, 6 + lv] = on.sum()
            cost[k, lv - 1] = term[matched & on].sum()
        counts[k, 2] = n - matched.sum()
        for g in np.nonzero(matched)[0]:
            last[k][gt_ids[g]] = track_ids[row[g]]
        if stats is not None and "pairs" in stats:
            stats["pairs"].update((int(row[g]), int(g)) for g in np.nonzero(matched)[0])
    return counts, cost


def summarize(counts, sums, cutoffs):
    """counts int64 [3, K, 9], sums fp64 [3, K, 2] -> the metrics at the cutoff of the highest MOTA (the lowest among
    equals), in fp64; `score_cutoff` fp64 [3, 2]: that cutoff."""
    counts, sums = np.asarray(counts, np.int64), np.asarray(sums, np.float64)
    result, chosen = {}, np.zeros((3, 2))
    for c, name in enumerate(CLASS_NAMES):
        for lv in range(2):
            match, fp = counts[c, :, lv].astype(np.float64), counts[c, :, 2].astype(np.float64)
            miss, mism = counts[c, :, 3 + lv].astype(np.float64), counts[c, :, 5 + lv].astype(np.float64)
            gt, cost = counts[c, :, 7 + lv].astype(np.float64), sums[c, :, lv]
            key = "OBJECT_TYPE_TYPE_%s_LEVEL_%d/" % (name, lv + 1)
            if not (gt > 0).any():
                result.update({key + m: 0.0 for m in METRICS})
                chosen[c, lv] = float(cutoffs[0])
                continue
            mota = 1.0 - (miss + fp + mism) / gt               # gt is the same at every cutoff
            k = int(np.argmax(mota))                            # the first of equal maxima
            chosen[c, lv] = float(cutoffs[k])
            result[key + "MOTA"] = float(mota[k])
            result[key + "MOTP"] = float(cost[k] / match[k]) if match[k] > 0 else 0.0
            result[key + "MISS"] = float(miss[k] / gt[k])
            result[key + "MISMATCH"] = float(mism[k] / gt[k])
            result[key + "FP"] = float(fp[k] / gt[k])
    result["score_cutoff"] = torch.from_numpy(chosen)
    return result


def class_ranges(f):
    """int64 [3, 4]: first track, tracks, first ground truth, ground truths of every class, inside a prepared frame."""
    p = np.searchsorted(f["pl"], [1, 2, 3, 4])
    g = np.searchsorted(f["gl"], [1, 2, 3, 4])
    return np.stack([p[:3], np.diff(p), g[:3], np.diff(g)], 1).astype(np.int64)


def device_mot(segments, cutoffs, thresholds, last, dev):
    """One launch over `segments`: [(prepared frames, first column)], each the consecutive frames of one sequence whose
    dense ground-truth ids stand in `last` (int32 [K, capacity] on the device, updated in place) from `first column` on.
    Returns a dict: counts int32 [3 S, K, 9] and sums fp64 [3 S, K, 2] (problem 3 s + c = class c of segment s), the
    problems on the device, and the launch's layout (weights, blk_off, trk_off, gt_off, ranges, problems on the host)."""
    frames = [f for seg, _ in segments for f in seg]
    trk_off = np.concatenate(([0], np.cumsum([len(f["ps"]) for f in frames]))).astype(np.int64)
    gt_off = np.concatenate(([0], np.cumsum([len(f["gl"]) for f in frames]))).astype(np.int64)
    ranges = np.stack([class_ranges(f) for f in frames]) if frames else np.zeros((0, 3, 4), np.int64)
    ranges[:, :, 0] += trk_off[:-1, None]
    ranges[:, :, 2] += gt_off[:-1, None]
    ops.check_ranges(ranges)                                     # before anything is launched
    problems, first = [], 0
    for seg, _ in segments:
        problems += [(first, first + len(seg), c) for c in range(3)]
        first += len(seg)
    problems = np.array(problems, dtype=np.int64).reshape(-1, 3)
    columns = np.concatenate([f["gd"] + col for seg, col in segments for f in seg] + [np.zeros(0, np.int64)])
    assert columns.size == 0 or (columns.min() >= 0 and columns.max() < last.shape[1])

    def up(key, dtype, tail=()):
        return torch.from_numpy(np.concatenate([f[key] for f in frames]).astype(dtype).reshape((-1,) + tail)).to(dev)

    weights, blk = ops.pair_weights(up("pb", np.float32, (7,)), up("pl", np.int32), trk_off, up("gb", np.float32, (7,)),
                                    up("gl", np.int32), gt_off, thresholds)
    counts, sums, prob = ops.mot(weights, blk, trk_off, gt_off, ranges, problems, up("ps", np.float32), up("td", np.int32),
                                 torch.from_numpy(columns.astype(np.int32)).to(dev), up("level", np.int32),
                                 torch.from_numpy(np.asarray(cutoffs, np.float32)).to(dev), last)
    return dict(counts=counts, sums=sums, prob=prob, weights=weights, blk_off=blk, trk_off=trk_off, gt_off=gt_off,
                ranges=ranges, problems=problems, frames=frames)


class WaymoTrackEvaluator(WaymoDetEvaluator):
    """process(inputs, outputs): `outputs` is the online tracker's list of {"track_ids", "track_boxes3d", "track_scores",
    "track_labels"}; `inputs` the matching list of (data, info) pairs (or info dicts): the frame's token
    "<sequence>_frame_<n>[.ext]" under info["token"] or info["metadata"]["token"], the targets as WaymoDetEvaluator reads
    them plus "gt_ids".  Frames of a sequence arrive in ascending n; a sequence that has been left is closed.  cutoffs: any
    ascending list of at most 101 scores (default `score_cutoffs()`); flush_frames: the frames of the open sequence that are
    buffered before they are evaluated (the result does not depend on it)."""

    def __init__(self, config=None, classes=CLASS_NAMES, distance_thresh=100, device=None, cutoffs=None, flush_frames=64,
                 carry_over=True):
        self.carry_over = bool(carry_over)        # False: host path only, plain per-frame Hungarian matching (for the tests)
        self.cutoffs = ops.check_cutoffs(score_cutoffs() if cutoffs is None else cutoffs)
        if int(flush_frames) < 1:
            raise ValueError("WaymoTrackEvaluator: flush_frames must be at least 1")
        self.flush_frames = int(flush_frames)
        super().__init__(config=config, classes=classes, distance_thresh=distance_thresh, device=device)

    def reset(self):
        super().reset()            # totals: int64 [3, K, 9] and fp64 [3, K, 2], created on the device of the first batch
        self.carry_stats = {"kept": 0, "conflicts": 0}      # host path: see clear_mot_frame
        self._closed = set()
        self._open(None)

    def _open(self, sequence):
        self._sequence, self._frame_no = sequence, -1
        self._gt_dense, self._trk_dense = {}, {}       # id -> order of first appearance in the open sequence
        self._buffer = []                              # prepared frames of the open sequence, not yet evaluated
        self._last = None                              # device: int32 [K, capacity]; host: K dicts

    # ---- preparation ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _token(item):
        info = item[1] if isinstance(item, (tuple, list)) else item
        token = info.get("token", None)
        if token is None:
            token = (info.get("metadata", None) or {}).get("token", None)
        sequence, sep, rest = str(token).rpartition("_frame_") if token is not None else ("", "", "")
        number = rest.split(".")[0]
        if not sep or not sequence or not number.isdigit():
            raise ValueError("WaymoTrackEvaluator: no frame token of the form '<sequence>_frame_<n>' (got %r)" % (token,))
        return sequence, int(number)

    @staticmethod
    def _ids(values, what, n):
        if isinstance(values, torch.Tensor):
            values = values.detach().cpu().numpy()
        values = np.asarray(values).reshape(-1).tolist()
        if len(values) != n:
            raise ValueError("WaymoTrackEvaluator: %d %s for %d boxes" % (len(values), what, n))
        if len(set(values)) != len(values):
            raise ValueError("WaymoTrackEvaluator: duplicate %s in one frame" % what)
        return values

    @staticmethod
    def _as_detections(output):
        if "track_ids" not in output:
            raise ValueError("WaymoTrackEvaluator: an output without track_ids")
        return {"boxes3d": output["track_boxes3d"], "scores": output["track_scores"], "labels": output["track_labels"]}

    def _alloc(self, dev):
        k = len(self.cutoffs)
        self._counts = torch.zeros((3, k, ops.NUM_COUNTS), dtype=torch.int64, device=dev)
        self._sums = torch.zeros((3, k, ops.NUM_SUMS), dtype=torch.float64, device=dev)

    def process(self, inputs, outputs):
        detections = [self._as_detections(o) for o in outputs]
        if self._counts is None:
            self._alloc(self._device_of(detections))
        frames = self._prepare(inputs, detections)
        for item, output, f in zip(inputs, outputs, frames):
            sequence, number = self._token(item)
            target = self._target(item)
            if "gt_ids" not in target:
                raise ValueError("WaymoTrackEvaluator: a target without gt_ids")
            track_ids = self._ids(output["track_ids"], "track_ids", len(_np(output["track_scores"], np.float32).reshape(-1)))
            gt_ids = self._ids(target["gt_ids"], "gt_ids", len(_np(target["labels"], np.int64).reshape(-1)))
            if self._counts.is_cuda:
                ops.check_ranges(class_ranges(f)[None])        # the kernel's limits: before anything is buffered or launched
            if sequence != self._sequence:
                if sequence in self._closed:
                    raise ValueError("WaymoTrackEvaluator: sequence %r was left and is closed" % sequence)
                self._flush()
                if self._sequence is not None:
                    self._closed.add(self._sequence)
                self._open(sequence)
            elif number <= self._frame_no:
                raise ValueError("WaymoTrackEvaluator: frame %d of %r after frame %d" % (number, sequence, self._frame_no))
            self._frame_no = number
            # dense ids in the order of first appearance (rows of the target / output as they came)
            for j in sorted(f["gi"]):
                self._gt_dense.setdefault(gt_ids[j], len(self._gt_dense))
            for j in sorted(f["pi"]):
                self._trk_dense.setdefault(track_ids[j], len(self._trk_dense))
            f["gd"] = np.array([self._gt_dense[gt_ids[j]] for j in f["gi"]], np.int64)
            f["td"] = np.array([self._trk_dense[track_ids[j]] for j in f["pi"]], np.int64)
            order = np.lexsort((f["gd"], f["gl"]))             # class-major, ascending dense id inside a class
            for key in ("gb", "gl", "level", "gi", "gd"):
                f[key] = f[key][order]
            self._buffer.append(f)
            if len(self._buffer) >= self.flush_frames:
                self._flush()

    def _flush(self):
        frames, self._buffer = self._buffer, []
        if not frames:
            return
        if self._counts.is_cuda:
            self._flush_device(frames)
        else:
            self._flush_host(frames)

    # ---- device path ------------------------------------------------------------------------------------------------------
    def _flush_device(self, frames):
        if not self.carry_over:
            raise RuntimeError("WaymoTrackEvaluator: carry_over=False exists on the host path only")
        dev, k, need = self._counts.device, len(self.cutoffs), len(self._gt_dense)
        if self._last is None:
            self._last = torch.full((k, max(need, 64)), -1, dtype=torch.int32, device=dev)
        elif need > self._last.shape[1]:                         # the sequence met more ids: grow by reallocation
            grown = torch.full((k, max(need, 2 * self._last.shape[1])), -1, dtype=torch.int32, device=dev)
            grown[:, :self._last.shape[1]] = self._last
            self._last = grown
        run = device_mot([(frames, 0)], self.cutoffs, self.thresholds, self._last, dev)
        ops.accumulate(run["counts"], run["sums"], run["prob"], self._counts, self._sums)

    # ---- host path: the fp64 formulation --------------------------------------------------------------------------------
    def host_weights(self, f, c):
        """fp64 [P_c, G_c]: the pair weights of class c (0..2) of a prepared frame under the exact fp64 IoU."""
        from ..detection3d.utils import rot_giou3d

        (p0, n_p, g0, n_g) = class_ranges(f)[c]
        pb, gb = f["pb"][p0:p0 + n_p].astype(np.float64), f["gb"][g0:g0 + n_g].astype(np.float64)
        w = np.zeros((n_p, n_g))
        if w.size:
            iou = rot_giou3d(torch.from_numpy(pb)[:, None, :], torch.from_numpy(gb)[None, :, :], (1.0, 1.0, 1.0, 0.0))[1].numpy()
            ok = np.isfinite(iou)
            w = np.where(ok & (np.where(ok, iou, 0.0) >= self.thresholds[c]), iou, 0.0)
            if ok.any():
                self.min_threshold_margin = min(self.min_threshold_margin, float(np.abs(iou[ok] - self.thresholds[c]).min()))
        return w

    def _flush_host(self, frames):
        if self._last is None:
            self._last = [{} for _ in self.cutoffs]
        counts, sums = self._counts.numpy(), self._sums.numpy()       # views: updated in place
        for f in frames:
            for c, (p0, n_p, g0, n_g) in enumerate(class_ranges(f)):
                got = clear_mot_frame(self.host_weights(f, c), f["ps"][p0:p0 + n_p], f["td"][p0:p0 + n_p].tolist(),
                                      f["gd"][g0:g0 + n_g].tolist(), f["level"][g0:g0 + n_g], self.cutoffs, self._last,
                                      carry_over=self.carry_over, stats=self.carry_stats)
                counts[c] += got[0]
                sums[c] += got[1]

    # ---- summary ------------------------------------------------------------------------------------------------------------
    def totals(self):
        """(counts int64 [3, K, 9], sums fp64 [3, K, 2]) on the host, summed over the ranks of an initialised
        torch.distributed group (whole sequences belong to one rank).  Integers and grid-rounded costs: the sum does not
        depend on the order."""
        if self._counts is None:
            self._alloc(torch.device("cpu"))
        self._flush()
        return super().totals()

    def evaluate(self):
        counts, sums = self.totals()
        result = summarize(counts.numpy(), sums.numpy(), self.cutoffs)
        result["counts"], result["cost"] = counts, sums
        return result
