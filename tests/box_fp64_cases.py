"""Inputs of the per-element float64 tests of the fused box attention of csrc/box_fused.hip (test_box_fp64_ref.py on the
CPU, test_box_fused_fp64_gpu.py on the device, and the geometry helpers of test_box_attention_fp64_full_gpu.py):
deterministic case builders (CPU generators, fixed seeds), an honest fp32 restatement of the op for the CPU, and the
comparison.  No test in here.

A case is a dict: value [B, S, H, D], shapes [L, 2] int64, starts [L] int64, ref [B, Lq, 7], offsets [B, Lq, H * L * nvar],
logits [B, Lq, H * L * P], kidx [P, 2], nvar (5 rotated, 4 not), grad_out [B, Lq, H * D], all float32 on the CPU, plus
`path` (the kernel family the host dispatch must choose: decoder / tile / window; `forward` for the forward-only cases),
`near` (share of the sampling points within 1e-3 px of a cell boundary in the first draw) and the conditions of the case
(`far`: bounds on the share of in-map corners outside the query tile's window; `sampling`: at least 40 % of the corners
are on the map).  Defaults: offsets ~ 0.5 randn, logits, value, grad_out ~ randn, kidx the module's lattice (`lattice`).
Every (query, head, level) with a sampling point within 1e-3 px of a cell boundary gets new offsets (`redraw_kinks`); a
case with hand-set offsets (gates) sets them again after every redraw.  "Grid" cases put query q on the centre of cell q
with a fixed box size; "free" cases draw ref ~ U(0, 1) with sizes 0.02 + 0.2 U.

Comparison: fp64_ref.assert_elementwise at c = 4 for every tensor (the constant of the msda and the full-size box tests),
with the `_geo` allowance of the reference plus fp64_ref.binned_sum_allowance on grad_value where the kernels bin
(decoder: every corner; tile: the far corners).  Largest err / bound per path at this c, and the measured conditions:

  honest fp32 on the CPU (box_attention_fp32: box_sampling_grid, softmax, F.grid_sample per level, autograd; no redraw needed):
    decoder  out 0.14   grad_value 0.15   grad_offsets 0.043  grad_logits 0.034
    tile     out 0.17   grad_value 0.12   grad_offsets 0.070  grad_logits 0.058
    window   out 0.15   grad_value 0.14   grad_offsets 0.082  grad_logits 0.087
    forward  out 0.065
  MI355X, the kernels of csrc/box_fused.hip (test_box_fused_fp64_gpu.py):
    decoder  out 0.14   grad_value 0.99   grad_offsets 0.043  grad_logits 0.034
    tile     out 0.17   grad_value 0.13   grad_offsets 0.068  grad_logits 0.059
    window   out 0.14   grad_value 0.14   grad_offsets 0.082  grad_logits 0.084
    forward  out 0.079
    (decoder grad_value: 0.15 without softmax_edges.  Its saturated softmax gives many corners a weight far below the unit
    2^-sh of the binned sums; a bin of one such entry is off by up to half a unit, which is exactly what binned_sum_allowance
    grants -- the allowance is the worst case of the rounding and this case attains it.)
  near-boundary share of the first draw: 0.00 % (one_query) .. 1.8 % (window_1x1024_p128_near; the strips are the highest
    because py has only one cell: 1.1 % on the tile strips, 0.6 .. 1.8 % on the window strips); 0.2 .. 0.5 % elsewhere
  far-corner share: FAR_MEASURED below, next to the condition of each case
  in-map corners: 0.43 (window_1x1024_*_far) .. 0.96; off_map 0.33 (62 % of its points are off the map)
"""
import functools
import math

import torch

from fp64_ref import assert_elementwise, binned_sum_allowance, box_attention_fp64, near_cell_boundary

C = 4
TENSORS = ("out", "grad_value", "grad_offsets", "grad_logits")
NEAR_MAX = 0.02              # largest share of near-boundary points in a first draw
IN_MAP_MIN = 0.40            # smallest share of in-map corners of a case that is there for its sampling
TILE = {"tile": (4, 8), "window": (8, 8)}   # query tile (rows, columns) of box_bwd_tile_*_kernel / box_bwd_kernel<32, true>
R = 4                        # cells of window on each side of a tile

def lattice(p):
    """The module's k x k lattice for P = k * k, else the first P rows of the ceil(sqrt(P)) lattice."""
    from efg_amd.detection3d.box_attention import _lattice

    k = math.isqrt(p)
    return _lattice(k) if k * k == p else _lattice(k + 1)[:p].contiguous()


def dispatch_path(l, s, lq, p):
    """The backward's choice in efg_box_attn_fused_backward_strided_f32 / BoxAttnFusedFunction.backward, from the shapes."""
    if l == 1 and s == lq and s >= 1024:
        return "tile" if l * p <= 32 else "window"
    return "decoder"


# ---- geometry in float64 -------------------------------------------------------------------------------------------------------
def pixels(ref, offsets, kidx, rot, shapes, nhead):
    """float64 pixel coordinates (px, py) [B, Q, H, L, P] of every sampling point; shapes: L rows of (h, w)."""
    from efg_amd.operators.box_attention_func import box_sampling_grid

    sides = torch.as_tensor(shapes).to(device=ref.device, dtype=torch.float64).reshape(-1, 2)
    nl = sides.shape[0]
    grid = box_sampling_grid(ref.double(), offsets.double(), kidx.double(), nhead, nl, rot)
    return grid[..., 0] * sides[:, 1].view(1, 1, 1, nl, 1) - 0.5, grid[..., 1] * sides[:, 0].view(1, 1, 1, nl, 1) - 0.5


def redraw_kinks(ref, offsets, kidx, rot, shapes, nhead, gen, fix=None, tries=100):
    """New offsets (in place) for every (query, head, level) with a sampling point within 1e-3 px of a cell boundary; `fix`
    (optional) puts hand-set offsets back after a redraw.  Returns the share of sampling points that were that close in the
    first draw.  (A small box on a level of one or two cells keeps its whole lattice within a few hundredths of a pixel: such
    a row can need tens of draws.)"""
    nvar = 5 if rot else 4
    b = ref.shape[0]
    nl = torch.as_tensor(shapes).reshape(-1, 2).shape[0]
    first = None
    for _ in range(tries):
        near = near_cell_boundary(*pixels(ref, offsets, kidx, rot, shapes, nhead))
        if first is None:
            first = float(near.float().mean())
        rows = near.any(-1)
        if not bool(rows.any()):
            return first
        off = offsets.view(b, -1, nhead, nl, nvar)
        off[rows] = (torch.randn(int(rows.sum()), nvar, generator=gen) * 0.5).to(off.device)
        if fix is not None:
            fix()
    raise AssertionError("sampling points keep landing on cell boundaries")


def _corner_counts(px, py, hm, wm, away_of=None):
    x0, y0 = torch.floor(px), torch.floor(py)
    n_in = n_away = 0
    for dy in (0, 1):
        for dx in (0, 1):
            cx, cy = x0 + dx, y0 + dy
            inside = (cx >= 0) & (cx < wm) & (cy >= 0) & (cy < hm)
            n_in += int(inside.sum())
            if away_of is not None:
                n_away += int((inside & away_of(cx, cy)).sum())
    return n_in, n_away


def out_of_window_share(px, py, hm, wm, tile=(4, 8)):
    """Share of the in-map corners outside the window of their query's tile (tile + R cells each side; queries = the cells of
    the map in row-major order).  px, py [B, Q, H, 1, P]."""
    tqy, tqx = tile
    q = torch.arange(hm * wm, device=px.device)
    wx0 = ((q % wm) // tqx * tqx - R).view(1, -1, 1, 1, 1)
    wy0 = ((q // wm) // tqy * tqy - R).view(1, -1, 1, 1, 1)
    n_in, n_out = _corner_counts(px, py, hm, wm, lambda cx, cy: (cx < wx0) | (cx > wx0 + tqx + 2 * R - 1) | (cy < wy0)
                                 | (cy > wy0 + tqy + 2 * R - 1))
    return n_out / n_in


def in_map_share(case):
    """Share of the 4 * (sampling points) bilinear corners that lie on their level's map."""
    px, py = case_pixels(case)
    n_in = 0
    for lv in range(case["shapes"].shape[0]):
        hl, wl = (int(v) for v in case["shapes"][lv])
        n_in += _corner_counts(px[:, :, :, lv], py[:, :, :, lv], hl, wl)[0]
    return n_in / (4 * px.numel())


def point_outside(case):
    """[B, Q, H, L, P] bool: the whole point is off its map by the kernels' rule (not px > -1 && py > -1 && px < W && py < H)."""
    px, py = case_pixels(case)
    hl, wl = (case["shapes"][:, i].to(torch.float64).view(1, 1, 1, -1, 1) for i in (0, 1))
    return ~((px > -1) & (py > -1) & (px < wl) & (py < hl))


def case_pixels(case):
    return pixels(case["ref"], case["offsets"], case["kidx"], case["nvar"] == 5, case["shapes"], case["value"].shape[2])


def far_share(case):
    hm, wm = (int(v) for v in case["shapes"][0])
    return out_of_window_share(*case_pixels(case), hm, wm, TILE[case["path"]])


# ---- the cases -----------------------------------------------------------------------------------------------------------------
CASES = {}
# measured far-corner shares (fp64 geometry of these builders), next to the asserted condition
FAR_MEASURED = {}


def _add(name, path, b, lq, h, levels, p, rot, d=32, size=None, special=None, far=None, sampling=True):
    """size None: free queries; (l, w): grid queries (Lq = the cells of the one level) with that box size."""
    CASES[name] = dict(name=name, path=path, b=b, lq=lq, h=h, d=d, levels=levels, p=p, rot=rot, size=size, special=special,
                       far=far, sampling=sampling, seed=4000 + len(CASES))


EIGHT = [[5, 7], [4, 4], [3, 5], [2, 3], [3, 1], [1, 2], [2, 2], [1, 1]]
FOUR = [[12, 10], [6, 5], [3, 3], [2, 1]]
# ---- decoder path: box_bwd_kernel<32, false> + bins
_add("three_levels", "decoder", 2, 37, 5, FOUR[:3], 9, True)          # 370 pairs = 12 blocks of 32: xcd_remap tail, t >= total
_add("four_levels_25", "decoder", 2, 50, 4, FOUR, 25, False)          # L * P = 100
_add("eight_levels_cap", "decoder", 1, 29, 2, EIGHT, 16, True)        # L = 8, L * P = 128, 32 * 128 == kSoftmaxLds
_add("below_grid_threshold", "decoder", 2, 1023, 2, [[31, 33]], 25, False, size=(0.1, 0.1))   # s == lq == 1023
_add("one_query", "decoder", 1, 1, 1, [[4, 4]], 25, True)
_add("gates", "decoder", 2, 64, 4, [[16, 16]], 25, True, special="gates")
_add("off_map", "decoder", 2, 64, 4, [[16, 16]], 25, True, special="off_map", sampling=False)
_add("softmax_edges", "decoder", 1, 64, 4, [[16, 16], [8, 8]], 9, False, special="softmax_edges")
DECODER = [n for n, c in CASES.items() if c["path"] == "decoder"]

# ---- tile path: box_bwd_tile_a_kernel + box_bwd_tile_b_kernel (L = 1, Lq = S >= 1024, P <= 32)
for _name, _b, _h, _hw, _size, _rot, _far, _meas in (
        ("tile_32x32_anchor", 1, 2, (32, 32), (0.1, 0.1), False, (0.0, 0.01), 0.000),
        ("tile_32x32_grown", 1, 2, (32, 32), (0.5, 0.5), False, (0.20, 1.01), 0.303),
        ("tile_33x32", 2, 3, (33, 32), (0.3, 0.3), True, (0.02, 0.30), 0.052),
        ("tile_1x1024", 1, 1, (1, 1024), (0.01, 0.5), True, (0.50, 1.01), 0.745),
        ("tile_1024x1", 1, 1, (1024, 1), (0.5, 0.01), True, (0.50, 1.01), 0.762),
        ("tile_5x205", 2, 2, (5, 205), (0.05, 0.6), False, (0.005, 0.10), 0.019),
        ("tile_32x32_free", 1, 2, (32, 32), None, True, (0.70, 1.01), 0.839)):
    _add(_name, "tile", _b, _hw[0] * _hw[1], _h, [list(_hw)], 25, _rot, size=_size, far=_far)
    FAR_MEASURED[_name] = _meas
for _p in (1, 9, 16, 31, 32):   # idle owners in the quads; 32 = PMAX
    _add("tile_33x32_p%d" % _p, "tile", 2, 33 * 32, 3, [[33, 32]], _p, True, size=(0.3, 0.3))
TILE_CASES = [n for n, c in CASES.items() if c["path"] == "tile"]

# ---- window path: box_bwd_kernel<32, true> (L = 1, Lq = S >= 1024, P > 32).  On the 1 x 1024 strip a rotated box of either
# size reaches tens of cells along x: both regimes are far there (measured 0.88 and 0.97 at 7 x 7)
for _p in (33, 49, 128):
    for _map, _b, _h, _hw in (("33x32", 1, 2, (33, 32)), ("1x1024", 1, 1, (1, 1024))):
        for _reg, _sz in (("near", 0.15), ("far", 0.6)):
            _far = (0.0, 0.01) if (_reg == "near" and _map == "33x32") else (0.20, 1.01)
            _add("window_%s_p%d_%s" % (_map, _p, _reg), "window", _b, _hw[0] * _hw[1], _h, [list(_hw)], _p, True,
                 size=(_sz, _sz), far=_far)
FAR_MEASURED.update({"window_33x32_p33_near": 0.000, "window_33x32_p33_far": 0.328, "window_1x1024_p33_near": 0.875,
                     "window_1x1024_p33_far": 0.966, "window_33x32_p49_near": 0.000, "window_33x32_p49_far": 0.355,
                     "window_1x1024_p49_near": 0.881, "window_1x1024_p49_far": 0.966, "window_33x32_p128_near": 0.000,
                     "window_33x32_p128_far": 0.321, "window_1x1024_p128_near": 0.873, "window_1x1024_p128_far": 0.964})
WINDOW = [n for n, c in CASES.items() if c["path"] == "window"]

# ---- forward only: D in 4 .. 256 (lanes per pair 1 .. 64; D = 12, 24: idle channel lanes that still own points)
TWO = [[9, 13], [4, 6]]
for _d, _p, _lv in ((4, 9, TWO[:1]), (8, 25, TWO[:1]), (12, 9, TWO), (16, 25, TWO), (24, 16, TWO[:1]), (64, 25, FOUR), (128, 49, TWO),
                    (256, 16, EIGHT)):
    _add("forward_d%d" % _d, "forward", 2, 37, 5, _lv, _p, True, d=_d)
FORWARD = [n for n, c in CASES.items() if c["path"] == "forward"]
BACKWARD = DECODER + TILE_CASES + WINDOW


def _special(spec, t, gen):
    """The hand-made parts of gates / off_map / softmax_edges; returns the function that sets hand-set offsets again."""
    b, lq, h, p, nl = spec["b"], spec["lq"], spec["h"], spec["p"], len(spec["levels"])
    q = torch.arange(lq).view(1, lq, 1)
    m = torch.arange(h).view(1, 1, h)
    if spec["special"] == "gates":
        # by (q + m) % 4: the length gate closed exactly at 0 (offset -8: size l + (-8 / 8) l = 0, gradient 0 by the w > 0 rule, as
        # torch.relu gives the reference) / closed below 0 / both gates closed (every point on the centre) / untouched
        group = ((q + m) % 4).expand(b, lq, h)
        t["ref"][:, 1::4, 3] *= -1                       # a quarter of the queries: negative length
        t["ref"][0, :8, 6] = 0.0                         # with offsets[4] = 0: ang == 0 on the rotated path

        def fix():
            off = t["offsets"].view(b, lq, h, nl, 5)
            off[..., 2][(group == 0).unsqueeze(-1).expand(b, lq, h, nl)] = -8.0
            off[..., 2][(group == 1).unsqueeze(-1).expand(b, lq, h, nl)] = -9.5
            both = (group == 2).unsqueeze(-1).expand(b, lq, h, nl)
            off[..., 2][both] = -8.5
            off[..., 3][both] = -8.5
            off[0, :8, :, :, 4] = 0.0
        fix()
        return fix
    if spec["special"] == "off_map":
        t["ref"][..., 0:2] = torch.rand(b, lq, 2, generator=gen) * 1.8 - 0.4
        return None
    # softmax_edges, by q % 3: logits x 30 (near one-hot) / all equal / one at +80 among the rest at -80
    lg = t["logits"].view(b, lq, h, nl * p)
    lg[:, 0::3] *= 30.0
    lg[:, 1::3] = 0.7
    hot = ((q + m) % (nl * p)).expand(b, lq, h)[:, 2::3]
    lg[:, 2::3] = -80.0
    lg[:, 2::3].scatter_(-1, hot.unsqueeze(-1), 80.0)
    return None


@functools.lru_cache(maxsize=None)
def build(name):
    """The case `name`.  Built once per process; nobody writes into its tensors."""
    spec = CASES[name]
    gen = torch.Generator().manual_seed(spec["seed"])
    b, lq, h, d, p, rot = spec["b"], spec["lq"], spec["h"], spec["d"], spec["p"], spec["rot"]
    shapes = torch.tensor(spec["levels"], dtype=torch.int64)
    cells = shapes[:, 0] * shapes[:, 1]
    starts = torch.cumsum(cells, 0) - cells
    nl, s, nvar = len(spec["levels"]), int(cells.sum()), 5 if rot else 4
    if spec["size"] is None:
        ref = torch.rand(b, lq, 7, generator=gen)
        ref[..., 3:5] = ref[..., 3:5] * 0.2 + 0.02
    else:
        hm, wm = spec["levels"][0]
        assert nl == 1 and lq == hm * wm
        ys, xs = torch.meshgrid(torch.arange(hm) + 0.5, torch.arange(wm) + 0.5, indexing="ij")
        ref = torch.zeros(b, lq, 7)
        ref[..., 0], ref[..., 1] = (xs / wm).reshape(-1), (ys / hm).reshape(-1)
        ref[..., 2] = ref[..., 5] = 0.5
        ref[..., 3], ref[..., 4] = spec["size"]
        if rot:
            ref[..., 6] = torch.rand(b, lq, generator=gen)
    t = dict(ref=ref, value=torch.randn(b, s, h, d, generator=gen), offsets=torch.randn(b, lq, h * nl * nvar, generator=gen) * 0.5,
             logits=torch.randn(b, lq, h * nl * p, generator=gen), grad_out=torch.randn(b, lq, h * d, generator=gen))
    fix = _special(spec, t, gen) if spec["special"] else None
    kidx = lattice(p)
    near = redraw_kinks(t["ref"], t["offsets"], kidx, rot, shapes, h, gen, fix)
    case = dict(name=name, path=spec["path"], far=spec["far"], sampling=spec["sampling"], special=spec["special"], near=near,
                shapes=shapes, starts=starts, kidx=kidx, nvar=nvar, **{k: v.contiguous() for k, v in t.items()})
    return case


# ---- an honest fp32 implementation -------------------------------------------------------------------------------------------
def box_attention_fp32(case, starts=None, softmax_per_level=False, drop_point=None, dtype=torch.float32):
    """The op from plain torch parts in `dtype`: box_sampling_grid, one softmax over L * P, F.grid_sample(align_corners=False,
    padding_mode="zeros") per level, torch autograd.  The keywords are the mutations of test_box_fp64_ref.py: other level
    starts, a softmax per level, one lattice point left out."""
    import torch.nn.functional as F

    from efg_amd.operators.box_attention_func import box_sampling_grid

    value, off, lg = (case[k].to(dtype).clone().requires_grad_(True) for k in ("value", "offsets", "logits"))
    b, s, h, d = value.shape
    lq, nl, p = case["ref"].shape[1], case["shapes"].shape[0], case["kidx"].shape[0]
    starts = case["starts"] if starts is None else starts
    grid = box_sampling_grid(case["ref"].to(dtype), off, case["kidx"].to(dtype), h, nl, case["nvar"] == 5)
    if softmax_per_level:
        attn = torch.softmax(lg.view(b, lq, h, nl, p), dim=-1)
    else:
        attn = torch.softmax(lg.view(b, lq, h, nl * p), dim=-1).view(b, lq, h, nl, p)
    if drop_point is not None:
        keep = torch.ones(p, dtype=dtype)
        keep[drop_point] = 0
        attn = attn * keep
    out = 0
    for lv in range(nl):
        hl, wl, st = int(case["shapes"][lv, 0]), int(case["shapes"][lv, 1]), int(starts[lv])
        vl = value[:, st:st + hl * wl].permute(0, 2, 3, 1).reshape(b * h, d, hl, wl)
        g = grid[:, :, :, lv].permute(0, 2, 1, 3, 4).reshape(b * h, lq, p, 2) * 2 - 1
        smp = F.grid_sample(vl, g, mode="bilinear", padding_mode="zeros", align_corners=False)    # [B * H, D, Lq, P]
        out = out + (smp * attn[:, :, :, lv].permute(0, 2, 1, 3).reshape(b * h, 1, lq, p)).sum(-1)
    out = out.view(b, h, d, lq).permute(0, 3, 1, 2).reshape(b, lq, h * d)
    out.backward(case["grad_out"].to(dtype))
    return {"out": out.detach(), "grad_value": value.grad, "grad_offsets": off.grad, "grad_logits": lg.grad}


# ---- reference and comparison --------------------------------------------------------------------------------------------------
def reference_of(case, grad_out=None, dev=None):
    """box_attention_fp64 of a case (on `dev`; with another grad_out)."""
    mv = (lambda x: x) if dev is None else (lambda x: x.to(dev))
    g = case["grad_out"] if grad_out is None else grad_out
    return box_attention_fp64(mv(case["value"]), mv(case["shapes"]), mv(case["starts"]), mv(case["ref"]), mv(case["offsets"]),
                              mv(case["logits"]), mv(case["kidx"]), case["nvar"], mv(g))


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(build(name))


def check(tag, case, ref, got, grad_out=None, bins=None, c=C):
    """assert_elementwise for every tensor of `got` (a dict over TENSORS or a part of them) against the reference `ref`;
    prints and returns the err / bound ratios.  `bins` (default: the case's path bins) adds binned_sum_allowance for the
    call's grad_out to grad_value."""
    bins = case["path"] in ("decoder", "tile") if bins is None else bins
    ratios = {}
    for k, g in got.items():
        geo = ref[k + "_geo"]
        if k == "grad_value" and bins:
            geo = geo + binned_sum_allowance(ref["grad_value_n"], case["grad_out"] if grad_out is None else grad_out)
        ratios[k] = assert_elementwise("%s %s" % (tag, k), g, ref[k], ref[k + "_mag"], ref[k + "_n"], c, geo)
    print("%s: err/bound %s" % (tag, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    return ratios
