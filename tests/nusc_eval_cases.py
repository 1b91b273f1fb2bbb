"""Inputs of the nuScenes-evaluation tests (test_nusc_eval_ref.py on the CPU, test_nusc_eval_gpu.py on the device): helpers
for the closed-form hand cases and the synthetic frames.  No test in here."""
import json
import math
import os

import numpy as np
import torch

CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
           "traffic_cone")
LABEL = {name: i + 1 for i, name in enumerate(CLASSES)}
SIZES = {"car": (4.6, 1.9, 1.7), "truck": (6.9, 2.5, 2.8), "construction_vehicle": (6.4, 2.8, 3.2), "bus": (11.0, 2.9, 3.5),
         "trailer": (12.3, 2.9, 3.9), "barrier": (0.5, 2.5, 1.0), "motorcycle": (2.1, 0.8, 1.5), "bicycle": (1.7, 0.6, 1.3),
         "pedestrian": (0.7, 0.7, 1.8), "traffic_cone": (0.4, 0.4, 1.1)}
GT_ATTRIBUTES = {"car": ("vehicle.moving", "vehicle.parked", "vehicle.stopped"),
                 "truck": ("vehicle.moving", "vehicle.parked", "vehicle.stopped"),
                 "construction_vehicle": ("vehicle.moving", "vehicle.parked"),
                 "bus": ("vehicle.moving", "vehicle.stopped"), "trailer": ("vehicle.moving", "vehicle.parked"),
                 "barrier": ("",), "motorcycle": ("cycle.with_rider", "cycle.without_rider"),
                 "bicycle": ("cycle.with_rider", "cycle.without_rider"),
                 "pedestrian": ("pedestrian.moving", "pedestrian.standing", "pedestrian.sitting_lying_down"),
                 "traffic_cone": ("",)}
SEEDS = (0, 1, 2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def meta():
    """The dataset's `meta` with the tests' own attribute counts (tests/golden/nusc_eval_attr_counts.json)."""
    with open(os.path.join(GOLDEN, "nusc_eval_attr_counts.json")) as f:
        return {"cls_attr_dist": json.load(f)}


def box(x, y=0.0, z=0.0, size=(4.0, 2.0, 1.5), yaw=0.0, vel=(0.0, 0.0)):
    """One box in the models' nine-column layout: x, y, z, l, w, h, vx, vy, yaw."""
    return [x, y, z, size[0], size[1], size[2], vel[0], vel[1], yaw]


def frame(preds, gts, dim=9, **extra):
    """preds: [(box, score, class name)], gts: [(box, class name[, attribute[, num_points]])] -> (input, output) as the
    loader and the models hand them to an evaluator; `extra` goes into the target (ego_xy)."""
    out = {"boxes3d": torch.tensor([p[0] for p in preds], dtype=torch.float32).reshape(-1, dim),
           "scores": torch.tensor([p[1] for p in preds], dtype=torch.float32),
           "labels": torch.tensor([LABEL[p[2]] for p in preds], dtype=torch.int64)}
    tgt = {"gt_boxes": np.array([g[0] for g in gts], dtype=np.float32).reshape(-1, dim),
           "labels": np.array([LABEL[g[1]] for g in gts], dtype=np.int64),
           "attributes": [g[2] if len(g) > 2 else "" for g in gts],
           "num_points_in_gt": np.array([g[3] if len(g) > 3 else 1 for g in gts], dtype=np.int64)}
    tgt.update(extra)
    return ({}, {"annotations": tgt}), out


def evaluator(device, **kw):
    from efg_amd.evaluator import NuScenesDetEvaluator

    kw.setdefault("meta", meta())
    return NuScenesDetEvaluator(device=device, **kw)


def run(frames, device, chunk=None, **kw):
    """The evaluator's result over `frames` ([(input, output)]), `chunk` frames per `process` call (default: all)."""
    ev = evaluator(device, **kw)
    ev.reset()
    chunk = chunk or max(len(frames), 1)
    for i in range(0, len(frames), chunk):
        ev.process([f[0] for f in frames[i:i + chunk]], [f[1] for f in frames[i:i + chunk]])
    return ev.evaluate(), ev


# ---- synthetic frames --------------------------------------------------------------------------------------------------------
def _gt(rng, name, xy, nan_vel=0.1, no_attr=0.2, min_points=0):
    size = np.array(SIZES[name]) * rng.uniform(0.9, 1.1, 3)
    vel = (math.nan, math.nan) if rng.random() < nan_vel else tuple(rng.normal(0, 1.5, 2) * (rng.random() < 0.6))
    attr = "" if rng.random() < no_attr else str(rng.choice(GT_ATTRIBUTES[name]))
    return (box(xy[0], xy[1], rng.normal(0.5, 0.1), size, rng.uniform(-math.pi, math.pi), vel), name, attr,
            int(rng.integers(min_points, 20)))


def _det(rng, g, name, jitter=0.3):
    b = g[0]
    vel = rng.normal(0, 1.5, 2) if math.isnan(b[6]) else (b[6] + rng.normal(0, 0.3), b[7] + rng.normal(0, 0.3))
    score = rng.uniform(0.02, 1.0)
    if rng.random() < 0.3:
        score = round(score, 2)                 # equal scores
    return (box(b[0] + rng.normal(0, jitter), b[1] + rng.normal(0, jitter), b[2] + rng.normal(0, 0.05),
                np.array(b[3:6]) * rng.uniform(0.9, 1.1, 3), b[8] + rng.normal(0, 0.2) + (math.pi if rng.random() < 0.1 else 0.0),
                vel), score, name)


def synthetic_frame(rng, n_obj, classes=CLASSES, dets=(0, 3), clutter=8, wrong=0.05, spread=3.0, extent=28.0, **gt_kw):
    """Clusters of `classes` objects `spread` metres wide, dets[0]..dets[1] jittered detections per object, `clutter`
    detections 0.3-5 m from an object, `wrong` of the labels replaced; some ground truths without points, with NaN
    velocities, with no attribute; objects up to `extent` m out, so some fall outside the 30 m classes' range."""
    gts, preds = [], []
    centres = rng.uniform(-extent, extent, (max(n_obj // 6, 1), 2))
    for _ in range(n_obj):
        name = str(rng.choice(classes))
        g = _gt(rng, name, centres[rng.integers(len(centres))] + rng.normal(0, spread, 2), **gt_kw)
        gts.append(g)
        for _ in range(int(rng.integers(dets[0], dets[1] + 1))):
            p = _det(rng, g, name, jitter=0.3 if rng.random() < 0.8 else 1.2)
            preds.append(p[:2] + (str(rng.choice(CLASSES)),) if rng.random() < wrong else p)
    for _ in range(clutter if gts else 0):
        g = gts[rng.integers(len(gts))]
        r, a = rng.uniform(0.3, 5.0), rng.uniform(0, 2 * math.pi)
        b = box(g[0][0] + r * math.cos(a), g[0][1] + r * math.sin(a), 0.5, SIZES[g[1]], rng.uniform(-math.pi, math.pi),
                tuple(rng.normal(0, 1.0, 2)))
        preds.append((b, rng.uniform(0.0, 0.4), g[1]))
    order = rng.permutation(len(preds))
    return frame([preds[i] for i in order], gts)


def single_class_frame(rng, name, n_gt, n_pred, spacing=1.5):
    """`n_gt` objects of one class on a jittered grid `spacing` metres apart around the ego point (all in range, all with
    points) and exactly `n_pred` detections of them: the grid is denser than the 2 m and 4 m thresholds, so what a
    prediction takes depends on what the better-scored ones took."""
    side = int(math.ceil(math.sqrt(n_gt)))
    gts = []
    for k in range(n_gt):
        xy = ((k % side) - (side - 1) / 2.0) * spacing + rng.normal(0, 0.2), ((k // side) - (side - 1) / 2.0) * spacing + rng.normal(0, 0.2)
        gts.append(_gt(rng, name, xy, min_points=1))
    preds = [_det(rng, gts[rng.integers(n_gt)], name, jitter=0.3 if rng.random() < 0.7 else 1.0) for _ in range(n_pred)]
    return frame(preds, gts)


def planted_frame():
    """An exact distance tie (a bicycle 1 m from two bicycles: the lower row wins) and an exact-threshold distance (a
    pedestrian exactly 2 m from its only ground truth: a false positive at 2 m, a true positive at 4 m)."""
    gts = [(box(10.0, 6.0, size=SIZES["bicycle"]), "bicycle", "cycle.with_rider"),
           (box(10.0, 4.0, size=SIZES["bicycle"]), "bicycle", ""),
           (box(-5.0, 0.0, size=SIZES["pedestrian"]), "pedestrian", "pedestrian.moving")]
    preds = [(box(10.0, 5.0, size=SIZES["bicycle"], vel=(1.0, 0.0)), 0.9, "bicycle"),
             (box(10.0, 5.25, size=SIZES["bicycle"]), 0.8, "bicycle"),
             (box(-3.0, 0.0, size=SIZES["pedestrian"]), 0.7, "pedestrian")]
    return frame(preds, gts)


def all_classes_frame(rng):
    """One object and one detection of every class, 6 m apart on a line through the ego point."""
    gts = [_gt(rng, name, (6.0 * i - 27.0, 1.0), nan_vel=0.0, no_attr=0.0, min_points=1) for i, name in enumerate(CLASSES)]
    return frame([_det(rng, g, g[1]) for g in gts], gts)


def device_test_frames(seed):
    """What tests/test_nusc_eval_gpu.py::test_frames_cover_the_shapes lists, in 15 frames."""
    rng = np.random.default_rng(seed)
    no_trailer = tuple(c for c in CLASSES if c != "trailer")
    frames = [synthetic_frame(rng, 30, no_trailer), synthetic_frame(rng, 40, no_trailer, dets=(0, 1), clutter=3),
              synthetic_frame(rng, 16, no_trailer, dets=(2, 3), clutter=20), synthetic_frame(rng, 24, no_trailer, spread=1.0)]
    none = synthetic_frame(rng, 12, no_trailer)
    frames.append((none[0], frame([], [])[1]))                                     # no predictions at all
    frames.append((frame([], [])[0], synthetic_frame(rng, 12, no_trailer)[1]))     # no ground truths at all
    frames.append(single_class_frame(rng, "pedestrian", 1, 6))
    frames.append(single_class_frame(rng, "car", 65, 90))
    frames.append(single_class_frame(rng, "pedestrian", 1024, 300))
    frames.append(single_class_frame(rng, "car", 40, 500, spacing=4.0))
    frames.append(all_classes_frame(rng))
    frames.append(planted_frame())
    # trailers: predictions in one frame, ground truths only in another
    frames.append(frame([_det(rng, _gt(rng, "trailer", (8.0, 3.0)), "trailer") for _ in range(3)], []))
    frames.append(frame([], [_gt(rng, "trailer", (8.0, 3.0), min_points=1), _gt(rng, "trailer", (-9.0, 2.0), min_points=1)]))
    frames.append(synthetic_frame(rng, 20, no_trailer))
    return frames


def too_many_ground_truths():
    rng = np.random.default_rng(0)
    return single_class_frame(rng, "pedestrian", 1025, 4, spacing=1.0)
