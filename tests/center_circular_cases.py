"""Inputs shared by tests/test_center_circular_ref.py (CPU) and tests/test_center_circular_gpu.py: the fixture made from
the reference's own code, hand cases with hand-written expectations, and the dyadic family.

Geometry of the hand cases and the dyadic family: out_size_factor 8, voxel 0.25, range origin -16, so a cell is 2 m and
x = ((ix + reg0) * 8) * 0.25 - 16.  With reg a multiple of 1/8 every fp32 operation of the centre and of the squared
distance is exact (multiples of 1/4 m below 2^7; squares and sums of multiples of 1/16 below 2^14), so two implementations
agree even where the squared distance EQUALS the radius."""
import os

import numpy as np
import torch

from conftest import GOLDEN

HEADS = ("hm", "reg", "height", "dim", "rot", "vel")
LOW_LOGIT = -10.0            # sigmoid = 4.5e-5: never a candidate


def post_process(min_radius, post_max=83, limit=(-16.0, -16.0, -4.0, 112.0, 112.0, 4.0), threshold=0.1):
    from efg_amd.config import to_attr

    return to_attr({"post_center_limit_range": list(limit),
                    "nms": {"nms_pre_max_size": 1000, "nms_post_max_size": post_max, "nms_iou_threshold": 0.2},
                    "score_threshold": threshold, "pc_range": [-16.0, -16.0], "out_size_factor": 8,
                    "voxel_size": [0.25, 0.25], "circular_nms": True, "min_radius": list(min_radius)})


def logit(p):
    p = np.asarray(p, dtype=np.float64)
    return np.log(p) - np.log1p(-p)


def to(preds_dicts, dev):
    return [{k: v.to(dev) for k, v in p.items()} for p in preds_dicts]


# ---- the fixture --------------------------------------------------------------------------------------------------
def fixture():
    """-> (preds_dicts on the CPU, post_process, num_classes, the reference's per-scene results in `predict`'s format)."""
    from efg_amd.config import to_attr

    g = dict(np.load(os.path.join(GOLDEN, "centerpoint_nusc_circle.npz"), allow_pickle=False))
    num_classes = [int(n) for n in g["num_classes"]]
    preds = [{k: torch.from_numpy(g["map::%d::%s" % (t, k)]) for k in HEADS} for t in range(len(num_classes))]
    pp = {"nms": {}}
    for key, v in g.items():
        parts = key.split("::")
        if parts[0] == "post_process":
            (pp["nms"] if parts[1] == "nms" else pp)[parts[-1]] = v.tolist()
    ref = [{"scores": torch.from_numpy(g["ref::scores::%d" % b]),
            "labels": torch.from_numpy(g["ref::label_preds::%d" % b]).long() + 1,
            "boxes3d": torch.from_numpy(g["ref::boxes::%d" % b])} for b in range(preds[0]["hm"].shape[0])]
    return preds, to_attr(pp), num_classes, ref


def same_results(got, want):
    """Kept lists and labels identical and in the same order; scores atol 1e-5, boxes atol 1e-4 (the tolerances of
    tests/test_centerpoint_golden.py::_check_inference)."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert set(g) >= {"scores", "labels", "boxes3d"}
        assert not g["scores"].is_cuda and not g["labels"].is_cuda and not g["boxes3d"].is_cuda
        assert g["labels"].dtype == torch.int64 and g["boxes3d"].dtype == g["scores"].dtype == torch.float32
        assert g["boxes3d"].shape == w["boxes3d"].shape, (i, g["boxes3d"].shape, w["boxes3d"].shape)
        assert torch.equal(g["labels"], w["labels"]), i
        ds = float((g["scores"] - w["scores"]).abs().max()) if len(w["scores"]) else 0.0
        db = float((g["boxes3d"] - w["boxes3d"]).abs().max()) if len(w["scores"]) else 0.0
        print("scene %d: %d boxes, largest score difference %.3e, box difference %.3e" % (i, len(w["scores"]), ds, db))
        assert ds <= 1e-5 and db <= 1e-4, (i, ds, db)


# ---- hand cases ---------------------------------------------------------------------------------------------------
def build(h, w, entries, ncls=1, batch=1, vel=True):
    """One task's maps, every cell quiet but `entries`: dicts {cell, score | logit, x, y[, z, cls, scene]} -- the centre
    (x, y) in metres is put there through reg, whatever the cell."""
    m = {"hm": torch.full((batch, ncls, h * w), LOW_LOGIT), "reg": torch.zeros(batch, 2, h * w),
         "height": torch.zeros(batch, 1, h * w), "dim": torch.zeros(batch, 3, h * w), "rot": torch.zeros(batch, 2, h * w)}
    m["rot"][:, 1] = 1.0
    if vel:
        m["vel"] = torch.zeros(batch, 2, h * w)
    for e in entries:
        b, cell = e.get("scene", 0), e["cell"]
        iy, ix = divmod(cell, w)
        m["hm"][b, e.get("cls", 0), cell] = float(e["logit"]) if "logit" in e else float(logit(e["score"]))
        m["reg"][b, 0, cell] = (e["x"] + 16.0) / 2.0 - ix
        m["reg"][b, 1, cell] = (e["y"] + 16.0) / 2.0 - iy
        m["height"][b, 0, cell] = e.get("z", 0.0)
    return {k: v.reshape(v.shape[:2] + (h, w)).contiguous() for k, v in m.items()}


def hand_cases():
    """-> {name: (preds_dicts, post_process, num_classes, expected: per scene the kept (x, y) in kept order)}"""
    cases = {}
    # A suppresses B (2.25 <= 4); B would have suppressed C (2.25 <= 4) but is gone; A does not reach C (9 > 4)
    e = [{"cell": 5, "score": 0.9, "x": 0.0, "y": 0.0}, {"cell": 9, "score": 0.8, "x": 1.5, "y": 0.0},
         {"cell": 2, "score": 0.7, "x": 3.0, "y": 0.0}]
    cases["chain"] = ([build(4, 4, e)], post_process([4.0]), [1], [[(0.0, 0.0), (3.0, 0.0)]])
    # the SQUARED distance against the radius: 0.4 m apart is 0.16 <= 0.175 (suppressed), 0.45 m apart is 0.2025 (kept)
    e = [{"cell": 0, "score": 0.9, "x": 0.0, "y": 0.0}, {"cell": 1, "score": 0.8, "x": 0.4, "y": 0.0},
         {"cell": 2, "score": 0.7, "x": 5.0, "y": 5.0}, {"cell": 3, "score": 0.6, "x": 5.45, "y": 5.0}]
    cases["squared"] = ([build(4, 4, e)], post_process([0.175]), [1], [[(0.0, 0.0), (5.0, 5.0), (5.45, 5.0)]])
    # equal scores go by cell index: cell 3 first (it suppresses cell 5 next to it), then cell 7; cell 12 scores higher
    e = [{"cell": 7, "logit": 0.25, "x": 20.0, "y": 0.0}, {"cell": 5, "logit": 0.25, "x": 1.0, "y": 0.0},
         {"cell": 3, "logit": 0.25, "x": 0.0, "y": 0.0}, {"cell": 12, "logit": 0.5, "x": 40.0, "y": 0.0}]
    cases["equal"] = ([build(4, 4, e)], post_process([4.0]), [1], [[(40.0, 0.0), (0.0, 0.0), (20.0, 0.0)]])
    # more survivors than post_max_size: the first five by score
    e = [{"cell": c, "score": 0.9 - 0.05 * k, "x": 8.0 * k, "y": 4.0} for k, c in enumerate((8, 1, 15, 4, 11, 2, 13, 6, 0))]
    cases["truncation"] = ([build(4, 4, e)], post_process([4.0], post_max=5), [1], [[(8.0 * k, 4.0) for k in range(5)]])
    cases["none"] = ([build(4, 4, [], batch=2)], post_process([4.0]), [1], [[], []])
    # range limits, inclusive: z exactly on either limit and x exactly on the upper one are inside; one ulp beyond in z
    # and the next x the decode can produce (one ulp below -16, two ulps above 56: x is an even multiple there) are outside
    up, down = float(np.nextafter(np.float32(4.0), np.float32(np.inf))), float(np.nextafter(np.float32(-4.0), np.float32(-np.inf)))
    e = [{"cell": 0, "score": 0.9, "x": 0.0, "y": 0.0, "z": 4.0}, {"cell": 1, "score": 0.85, "x": 10.0, "y": 0.0, "z": up},
         {"cell": 2, "score": 0.8, "x": 20.0, "y": 0.0, "z": -4.0}, {"cell": 3, "score": 0.75, "x": 30.0, "y": 0.0, "z": down},
         {"cell": 4, "score": 0.7, "x": 56.0, "y": 10.0}, {"cell": 5, "score": 0.65, "x": 56.0 + 2.0 ** -17, "y": 20.0},
         {"cell": 6, "score": 0.6, "x": -16.0, "y": 30.0}, {"cell": 7, "score": 0.55, "x": -16.0 - 2.0 ** -19, "y": 40.0}]
    lim = (-16.0, -16.0, -4.0, 56.0, 56.0, 4.0)
    cases["range"] = ([build(4, 4, e)], post_process([4.0], limit=lim), [1],
                      [[(0.0, 0.0), (20.0, 0.0), (56.0, 10.0), (-16.0, 30.0)]])
    return cases


def check_expected(got, expected):
    assert len(got) == len(expected)
    for g, want in zip(got, expected):
        xy = g["boxes3d"][:, :2].tolist()
        assert len(xy) == len(want), (xy, want)
        for a, b in zip(xy, want):
            assert abs(a[0] - b[0]) <= 1e-4 and abs(a[1] - b[1]) <= 1e-4, (xy, want)
        assert g["scores"].tolist() == sorted(g["scores"].tolist(), reverse=True)


# ---- the dyadic family ----------------------------------------------------------------------------------------------
# name: (batch, h, w, classes per task, radii, post_max, candidates per (scene, task) or None for every cell, vel)
DYADIC = {
    "16x16_few": (1, 16, 16, (1, 2, 2, 1, 2, 2), (4.0, 8.0, 16.0, 1.0, 0.5, 0.25), 83, 12, True),
    "12x20_b3": (3, 12, 20, (2, 1), (4.0, 1.0), 83, 120, True),
    "40x40_all": (1, 40, 40, (1,), (4.0,), 83, None, True),
    "7x9_odd": (1, 7, 9, (1, 2), (4.0, 2.0), 83, 40, True),
    "12x20_no_vel": (1, 12, 20, (2, 1), (4.0, 0.5), 20, 150, False),
    "16x16_three_class": (3, 16, 16, (3,), (4.0,), 83, 200, True),
}


def dyadic(name):
    """-> (preds_dicts on the CPU, post_process, num_classes).  reg from multiples of 1/8 in [0, 1) (distinct cells have
    distinct centres), pairs planted at squared distance exactly 4.0 (neighbouring cells with equal reg) next to the many
    the lattice has anyway; scores a permuted linspace, never near the threshold; heights multiples of 1/4, some outside
    and some exactly on the range limits (+-4) unless every cell is to be a candidate."""
    batch, h, w, classes, radii, post_max, n_cand, vel = DYADIC[name]
    rng = np.random.default_rng(sorted(DYADIC).index(name))
    cells = h * w
    preds = []
    for ncls in classes:
        m = {"reg": rng.integers(0, 8, (batch, 2, cells)) / 8.0, "dim": rng.integers(-8, 9, (batch, 3, cells)) / 8.0,
             "rot": rng.normal(0, 1, (batch, 2, cells)), "height": rng.integers(-16, 17, (batch, 1, cells)) / 4.0}
        if n_cand is None:
            top = np.stack([rng.permutation(np.linspace(0.2, 0.9, cells)) for _ in range(batch)])
        else:
            m["height"] = rng.integers(-20, 21, (batch, 1, cells)) / 4.0          # -5 .. 5: some beyond +-4, some on it
            top = np.stack([rng.permutation(np.concatenate([np.linspace(0.15, 0.95, n_cand),
                                                            np.linspace(0.01, 0.09, cells - n_cand)])) for _ in range(batch)])
        for b in range(batch):                                                # planted: equal reg in neighbouring cells
            for cell in rng.choice(cells - 1, max(cells // 8, 2), replace=False):
                if (cell + 1) % w:
                    m["reg"][b, :, cell + 1] = m["reg"][b, :, cell]
        win = rng.integers(0, ncls, (batch, cells))
        hm = np.repeat((logit(top) - 1.0)[:, None, :], ncls, axis=1)
        np.put_along_axis(hm, win[:, None, :], logit(top)[:, None, :], axis=1)
        m["hm"] = hm
        if vel:
            m["vel"] = rng.integers(-16, 17, (batch, 2, cells)) / 4.0
        preds.append({k: torch.from_numpy(v.reshape(v.shape[:2] + (h, w)).astype(np.float32)) for k, v in m.items()})
    return preds, post_process(radii, post_max=post_max), list(classes)
