"""Inputs of the per-element float64 tests of the sampling kernels of csrc/msda.hip (test_msda_fp64_ref.py on the CPU,
test_msda_fp64_gpu.py on the device): deterministic case builders (CPU generators, fixed seeds), the float64 reference of
each case (fp64_ref.sample_fp64, computed once per process) and the comparison.  No test in here.

A case is a dict: value [B, S, H, D], shapes [L, 2] int64, level_start [L] int64, loc [B, Lq, H, L, P, 2], attn [B, Lq, H, L, P]
(a softmax over L * P), grad_out [B, Lq, H * D], all float32 on the CPU, and `kind` (generic / grid / lattice), `regime`,
`exact`, `redrawn`.  Every sampling point whose float64 pixel coordinate lies within 1e-3 px of a cell boundary is drawn again
from the distribution of its case (`redrawn` = their share in the first draw); only those points move.  Both sides then
interpolate between the same four corners, which is what the first-order geometry allowance of sample_fp64 assumes.

Three kinds of cases:
    generic  msda_kernel<false> and msda_kernel<true>: loc uniform in [-0.3, 1.3] (61 % of the points have a coordinate outside
             [0, 1]) unless the case says otherwise; the shapes walk through the lanes-per-pair table (D = 4 .. 256), the tail of
             the XCD remap, 1 x N / N x 1 / 1 x 1 levels and the level cap
    grid     msda_bwd_grid_kernel<32> (L = 1, D = 32, Lq = S >= 1024, P = 9) on the smallest maps that reach it, in three
             sampling regimes: near (the query's own cell centre +- 3 cells; vertically at most 0.4 of the map height), mixed
             (the same with MIXED_SHARE of the points uniform in [-0.2, 1.2]) and free (all uniform in [-0.2, 1.2])
    lattice  loc = (k / 2) / side on power-of-two sides: every pixel coordinate is an exact multiple of 0.5 in fp32 and fp64
             (-1.5, -1, -0.5, 0, ..., side - 0.5, side and beyond), so the geometry allowance is 0 (geo_ulps = 0), nothing is
             redrawn, and the reference applies the kernels' whole-point inside rule (sample_fp64(reference_inside=True))."""
import functools

import torch

from fp64_ref import GEO_ULPS, assert_elementwise, log_uniform_signed, near_cell_boundary, sample_fp64

# The rounding constant of assert_elementwise for every tensor: the value tests/test_box_attention_fp64_full_gpu.py uses for
# the same op.  Largest err / bound over the cases of a kind, at this c:
#   fp32 CPU oracle (oracle.msda_forward / msda_backward, tests/test_msda_fp64_ref.py):
#     generic  out 0.081  grad_value 0.10   grad_loc 0.089  grad_attn 0.074
#     grid     out 0.095  grad_value 0.077  grad_loc 0.057  grad_attn 0.051
#     lattice  out 0.14   grad_value 0.27   grad_loc 0.053  grad_attn 0.048   (no geometry term)
#   MI355X, the kernels of csrc/msda.hip (tests/test_msda_fp64_gpu.py; per kernel in its docstring):
#     generic  out 0.081  grad_value 0.10   grad_loc 0.089  grad_attn 0.074
#     grid     out 0.095  grad_value 0.078  grad_loc 0.057  grad_attn 0.051
#     lattice  out 0.15   grad_value 0.27   grad_loc 0.066  grad_attn 0.073
C = 4
TENSORS = ("out", "grad_value", "grad_loc", "grad_attn")

TQ, R = 8, 4                 # msda_bwd_grid_kernel: 8 x 8 query tiles, 4 cells on each side: a 16 x 16 window
MIXED_SHARE = 0.15           # share of the points of a mixed-regime case that are drawn uniformly over the map
REGIMES = ("near", "mixed", "free")

CASES = {}


def _add(name, kind, dims, loc="uniform", grad="normal", regime=None, seed=None):
    b, lq, h, d, levels, p = dims
    CASES[name] = dict(name=name, kind=kind, b=b, lq=lq, h=h, d=d, levels=levels, p=p, loc=loc, grad=grad, regime=regime,
                       seed=1000 + len(CASES) if seed is None else seed)


# ---- generic kernel: (B, Lq, H, D, levels, P) ---------------------------------------------------------------------------
_add("remap_tail", "generic", (2, 37, 5, 32, [[9, 13]], 7))           # 370 pairs = 12 blocks: bid >= per << 3, t >= total
_add("four_levels", "generic", (2, 50, 4, 8, [[12, 10], [6, 5], [3, 3], [2, 1]], 4))       # the golden's shapes, fresh data
_add("thin_levels", "generic", (1, 23, 3, 12, [[7, 9], [1, 6], [5, 1], [1, 1]], 3))        # D = 12: lp = 4, one idle lane
_add("d20", "generic", (3, 11, 2, 20, [[5, 4], [3, 2]], 5))                                 # lp = 8, three idle lanes
_add("d256", "generic", (1, 9, 1, 256, [[4, 4]], 2))                                        # one pair per wave
_add("d4_p1", "generic", (2, 17, 7, 4, [[6, 6]], 1))                                        # lp = 1: no reduction
_add("log_grad", "generic", (2, 64, 3, 64, [[8, 8]], 9), grad="log_uniform")               # grad_out 1e-6 .. 1e2
_add("eight_levels", "generic", (2, 13, 2, 16, [[5, 7], [4, 4], [3, 5], [2, 3], [3, 1], [1, 2], [2, 2], [1, 1]], 2))
# pile-up: every loc within +-0.01 of (0.37, 0.61), so every point has the cell (14, 18) among its corners and one grad_value
# row per head takes an entry from each of the Lq * P points.  With Lq = 1200 = 30 * 40 = S the case meets the grid kernel's
# dispatch condition (queries from all over the map onto one cell: nearly every add takes the out-of-window global path);
# one more query (Lq = 1201 != S) keeps the same pile on the generic backward's global atomics.
_add("pile_up", "generic", (1, 1201, 2, 32, [[30, 40]], 4), loc="pile")
_add("pile_up_grid", "grid", (1, 1200, 2, 32, [[30, 40]], 4), loc="pile", regime="pile")
# ---- grid kernel: every map in every regime -----------------------------------------------------------------------------------
GRID_MAPS = {"32x32": (1, 1, 32, 32), "29x37": (2, 3, 29, 37), "3x400": (1, 2, 3, 400), "1x1024": (1, 1, 1, 1024)}   # B, H, h, w
for _m, (_b, _h, _hm, _wm) in GRID_MAPS.items():
    for _r in REGIMES:
        _add("grid_%s_%s" % (_m, _r), "grid", (_b, _hm * _wm, _h, 32, [[_hm, _wm]], 9), loc=_r, regime=_r)
# ---- exact lattice ----------------------------------------------------------------------------------------------------------------
_add("lattice", "lattice", (2, 41, 3, 8, [[8, 16], [4, 4], [1, 2]], 6), loc="lattice")
_add("lattice_grid", "lattice", (1, 1024, 2, 32, [[32, 32]], 6), loc="lattice_near")       # the same on the grid kernel

GENERIC = [n for n, c in CASES.items() if c["kind"] == "generic"]
GRID = [n for n, c in CASES.items() if c["kind"] == "grid"]
LATTICE = [n for n, c in CASES.items() if c["kind"] == "lattice"]
UNIFORM = [n for n in GENERIC if CASES[n]["loc"] == "uniform"]


def takes_grid_kernel(case):
    """The dispatch condition of box_attn_backward / efg_msda_backward_f32 for the LDS-window kernel."""
    s = case["value"].shape[1]
    return case["shapes"].shape[0] == 1 and case["value"].shape[3] == 32 and s == case["loc"].shape[1] and s >= 1024


# ---- geometry in float64 -------------------------------------------------------------------------------------------------------
def pixels(loc, shapes):
    """float64 pixel coordinates (px, py) [B, Lq, H, L, P] of the float32 locations: loc * side - 0.5."""
    side = shapes.to(torch.float64)
    l64 = loc.to(torch.float64)
    return l64[..., 0] * side[:, 1].view(1, 1, 1, -1, 1) - 0.5, l64[..., 1] * side[:, 0].view(1, 1, 1, -1, 1) - 0.5


def point_inside(px, py, shapes):
    """The kernels' rule for a whole point: px > -1 && py > -1 && px < W && py < H."""
    hl, wl = (shapes[:, i].to(torch.float64).view(1, 1, 1, -1, 1) for i in (0, 1))
    return (px > -1) & (py > -1) & (px < wl) & (py < hl)


def corners_in_range(px, py, shapes):
    """Number of the 4 bilinear corners of every point that lie on the map (0, 1, 2 or 4: it is a product of two counts)."""
    hl, wl = (shapes[:, i].to(torch.float64).view(1, 1, 1, -1, 1) for i in (0, 1))
    x0, y0 = torch.floor(px), torch.floor(py)
    nx = ((x0 >= 0) & (x0 < wl)).long() + ((x0 + 1 >= 0) & (x0 + 1 < wl)).long()
    ny = ((y0 >= 0) & (y0 < hl)).long() + ((y0 + 1 >= 0) & (y0 + 1 < hl)).long()
    return nx * ny


def out_of_window_share(px, py, hm, wm):
    """Share of the in-map corners outside the 16 x 16 window of their query's 8 x 8 tile (queries = the cells of the map)."""
    q = torch.arange(hm * wm)
    wx0 = ((q % wm) // TQ * TQ - R).view(1, -1, 1, 1, 1)
    wy0 = ((q // wm) // TQ * TQ - R).view(1, -1, 1, 1, 1)
    x0, y0 = torch.floor(px), torch.floor(py)
    n_in = n_out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            cx, cy = x0 + dx, y0 + dy
            inside = (cx >= 0) & (cx < wm) & (cy >= 0) & (cy < hm)
            away = (cx < wx0) | (cx > wx0 + TQ + 2 * R - 1) | (cy < wy0) | (cy > wy0 + TQ + 2 * R - 1)
            n_in += int(inside.sum())
            n_out += int((inside & away).sum())
    return n_out / n_in


# ---- builders ------------------------------------------------------------------------------------------------------------------
def _uniform(shape, lo, hi, gen):
    return torch.empty(shape, dtype=torch.float32).uniform_(lo, hi, generator=gen)


def _near(spec, gen):
    """The query's own cell centre + up to 3 cells (vertically at most 0.4 of the map height), as normalised locations."""
    b, lq, h, p = spec["b"], spec["lq"], spec["h"], spec["p"]
    hm, wm = spec["levels"][0]
    q = torch.arange(lq)
    qx, qy = (q % wm).view(1, lq, 1, 1, 1).double(), (q // wm).view(1, lq, 1, 1, 1).double()
    sx, sy = 3.0, min(3.0, 0.4 * hm)
    px = qx + _uniform((b, lq, h, 1, p), -sx, sx, gen).double()
    py = qy + _uniform((b, lq, h, 1, p), -sy, sy, gen).double()
    return torch.stack(((px + 0.5) / wm, (py + 0.5) / hm), dim=-1).float()


def _draw_loc(spec, gen):
    b, lq, h, p, levels = spec["b"], spec["lq"], spec["h"], spec["p"], spec["levels"]
    shape = (b, lq, h, len(levels), p, 2)
    kind = spec["loc"]
    if kind == "uniform":
        return _uniform(shape, -0.3, 1.3, gen)
    if kind == "pile":
        return torch.tensor([0.37, 0.61]) + _uniform(shape, -0.01, 0.01, gen)
    if kind == "free":
        return _uniform(shape, -0.2, 1.2, gen)
    if kind in ("near", "mixed"):
        loc = _near(spec, gen)
        if kind == "mixed":
            far = torch.rand(shape[:-1], generator=gen) < MIXED_SHARE
            loc = torch.where(far.unsqueeze(-1), _uniform(shape, -0.2, 1.2, gen), loc)
        return loc
    # lattices: loc = (k / 2) / side, k integer in [-4, 2 * side + 4]; side a power of two, so loc * side - 0.5 is exact
    loc = torch.empty(shape, dtype=torch.float64)
    for lv, (hl, wl) in enumerate(levels):
        for axis, side in ((0, wl), (1, hl)):
            assert side & (side - 1) == 0
            if kind == "lattice":
                k = torch.randint(-4, 2 * side + 5, shape[:3] + (p,), generator=gen)
            else:   # lattice_near: around the query's own cell (k = 2 q + 1 is its centre), +- 8 half cells
                q = torch.arange(lq)
                own = (q % wl if axis == 0 else q // wl).view(1, lq, 1, 1)
                k = (2 * own + 1 + torch.randint(-8, 9, shape[:3] + (p,), generator=gen)).clamp(-4, 2 * side + 4)
            loc[:, :, :, lv, :, axis] = (k.double() / 2) / side
    assert bool((loc.float().double() == loc).all())
    return loc.float()


@functools.lru_cache(maxsize=None)
def build(name):
    """The case `name` (see the module docstring).  Built once per process; nobody writes into its tensors."""
    spec = CASES[name]
    gen = torch.Generator().manual_seed(spec["seed"])
    b, lq, h, d, p = spec["b"], spec["lq"], spec["h"], spec["d"], spec["p"]
    shapes = torch.tensor(spec["levels"], dtype=torch.int64)
    cells = shapes[:, 0] * shapes[:, 1]
    level_start = torch.cumsum(cells, 0) - cells
    nl, s = len(spec["levels"]), int(cells.sum())
    value = torch.randn(b, s, h, d, generator=gen)
    attn = torch.softmax(torch.randn(b, lq, h, nl * p, generator=gen), -1).view(b, lq, h, nl, p).contiguous()
    if spec["grad"] == "log_uniform":
        grad_out = log_uniform_signed((b, lq, h * d), 1e-6, 1e2, gen)
    else:
        grad_out = torch.randn(b, lq, h * d, generator=gen)
    loc = _draw_loc(spec, gen)
    exact = spec["kind"] == "lattice"
    redrawn = 0.0
    if not exact:
        for trip in range(20):
            near = near_cell_boundary(*pixels(loc, shapes))
            if trip == 0:
                redrawn = float(near.float().mean())
            if not bool(near.any()):
                break
            loc = torch.where(near.unsqueeze(-1), _draw_loc(spec, gen), loc)
        else:
            raise AssertionError("%s: sampling points keep landing on cell boundaries" % name)
    return dict(name=name, kind=spec["kind"], regime=spec["regime"], exact=exact, redrawn=redrawn, value=value, shapes=shapes,
                level_start=level_start, loc=loc.contiguous(), attn=attn, grad_out=grad_out)


@functools.lru_cache(maxsize=None)
def mutation_case():
    """The d4_p1 shapes (one level, one point: an out element is ONE bilinear sample) with two changes that put small
    elements next to unit-scale ones: the last row of the map holds values of 1e-6, and every (batch, query, head) row of
    grad_out has its own log-uniform factor in [1e-6, 1e2]."""
    case = dict(build("d4_p1"))
    gen = torch.Generator().manual_seed(77)
    hm, wm = (int(v) for v in case["shapes"][0])
    value = case["value"].clone()
    value[:, (hm - 1) * wm:] *= 1e-6
    b, lq, hd = case["grad_out"].shape
    h = value.shape[2]
    factor = log_uniform_signed((b, lq, h, 1), 1e-6, 1e2, gen).abs()
    grad_out = (case["grad_out"].view(b, lq, h, -1) * factor).reshape(b, lq, hd).contiguous()
    case.update(name="mutation", value=value, grad_out=grad_out)
    return case


# ---- reference and comparison --------------------------------------------------------------------------------------------
def reference_of(case, reference_inside=None):
    """sample_fp64 of a case on the CPU: geo_ulps = 0 and the whole-point inside rule for the lattice cases."""
    exact = case["exact"]
    return sample_fp64(case["value"], case["shapes"], case["level_start"], case["loc"], case["attn"], case["grad_out"],
                       geo_ulps=0 if exact else GEO_ULPS, reference_inside=exact if reference_inside is None else reference_inside)


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(build(name))


def n_terms(case, ref, key):
    """Products per element: out 4 corners x L x P points; grad_attn and grad_loc 4 corners x D channels; grad_value the
    reference's count of (point, corner) entries of the row."""
    nl, p, d = case["loc"].shape[3], case["loc"].shape[4], case["value"].shape[3]
    return {"out": 4 * nl * p, "grad_attn": 4 * d, "grad_loc": 4 * d, "grad_value": ref["grad_value_n"]}[key]


def check(tag, case, ref, got, c=C):
    """assert_elementwise for every tensor of `got` (a dict over TENSORS or a part of them); prints and returns the err / bound
    ratios."""
    ratios = {}
    for k, g in got.items():
        ratios[k] = assert_elementwise("%s %s" % (tag, k), torch.as_tensor(g), ref[k], ref[k + "_mag"], n_terms(case, ref, k), c,
                                       ref[k + "_geo"])
    print("%s: err/bound %s" % (tag, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    return ratios
