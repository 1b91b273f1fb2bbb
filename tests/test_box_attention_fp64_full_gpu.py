"""GPU: the fused box attention (csrc/box_fused.hip) against the float64 op of tests/fp64_ref.py at production size --
B = 2, H = 8, D = 32, one level, the 5 x 5 lattice -- called through BoxAttnFusedFunction.apply in both forms (separate
logits; one shared projection, logits=None).  Encoder: the queries are the cells of a 188 x 188 map (and of a 101 x 147
map, sides not multiples of the 4 x 8 query tile): the tile backward, with the corners that leave a tile's 12 x 16
window binned.  Decoder: 1200 free rotated queries, every corner binned (box_bwd_kernel).  out, grad_value, grad_offsets
and grad_logits are checked element by element (fp64_ref.assert_elementwise, with the fp32-geometry term), so an element
far below its tensor's largest one is held to its own size.  One decoder case draws grad_out log-uniform over 1e-6 ... 1e2:
the binned sums are fixed-point integers at a unit set by the call's largest |grad_out|, and a grad_value row may differ
by at most its entries' rounding to that unit (fp64_ref.binned_sum_allowance, ~1e-13 of the largest |grad_out| per entry).

Sampling points whose fp64 pixel coordinate lies within 1e-3 px of a cell boundary get new offsets first (both sides then
interpolate between the same four corners; a few per cent of the (query, head) rows need it)."""
import pytest
import torch

from box_fp64_cases import out_of_window_share, pixels, redraw_kinks
from fp64_ref import assert_elementwise, binned_sum_allowance, box_attention_fp64, log_uniform_signed

pytestmark = pytest.mark.gpu

B, H, D, L, P = 2, 8, 32, 1, 25
ANCHOR = 0.025   # transformer._create_ref_windows: every BEV token's anchor box is l = w = 0.025 of the map
# rounding constants c of assert_elementwise per tensor (the geometry term dominates the sampling bounds).  Largest
# err / bound measured on MI355X: out 0.19, grad_value 0.28 (decoder bins), grad_offsets 0.081, grad_logits 0.075
C = {"out": 4, "grad_value": 4, "grad_offsets": 4, "grad_logits": 4}
MAPS = {"188x188": (188, 188), "101x147": (101, 147)}


def _lattice():
    from efg_amd.detection3d.box_attention import _lattice

    return _lattice(5)


def _run(dev, tag, hm, wm, ref, value, offsets, logits, kidx, nvar, gout, shared):
    from efg_amd.operators.box_attention_func import BoxAttnFusedFunction

    shapes = torch.tensor([[hm, wm]], device=dev)
    start = torch.zeros(1, dtype=torch.int64, device=dev)
    v = value.clone().requires_grad_(True)
    n_lg = H * L * P
    if shared:
        proj = torch.cat([logits, offsets], -1).requires_grad_(True)
        out = BoxAttnFusedFunction.apply(v, shapes, start, ref, proj, None, kidx, nvar)
        out.backward(gout)
        g_lg, g_off = proj.grad[..., :n_lg], proj.grad[..., n_lg:]
    else:
        o, lg = offsets.clone().requires_grad_(True), logits.clone().requires_grad_(True)
        out = BoxAttnFusedFunction.apply(v, shapes, start, ref, o, lg, kidx, nvar)
        out.backward(gout)
        g_lg, g_off = lg.grad, o.grad
    torch.cuda.synchronize()
    r = box_attention_fp64(value, shapes, start, ref, offsets, logits, kidx, nvar, gout)
    got = {"out": out, "grad_value": v.grad, "grad_offsets": g_off, "grad_logits": g_lg}
    # binned grad_value rows are exact fixed-point sums at a unit set by the call's largest |grad_out|: on top of the
    # element-wise bar, each row may be off by its entries' rounding to that unit (n * 2^-(sh+1), binned_sum_allowance)
    extra = {"grad_value": binned_sum_allowance(r["grad_value_n"], gout)}
    ratios = {k: assert_elementwise("%s %s" % (tag, k), got[k], r[k], r[k + "_mag"], r[k + "_n"], C[k],
                                    r[k + "_geo"] + extra.get(k, 0.0))
              for k in got}
    print("%s: err/bound %s" % (tag, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    return r, ratios


def _encoder_case(dev, hm, wm, regime, rot, gen):
    s = hm * wm
    ys, xs = torch.meshgrid(torch.arange(hm) + 0.5, torch.arange(wm) + 0.5, indexing="ij")
    ref = torch.zeros(B, s, 7)
    ref[..., 0], ref[..., 1] = (xs / wm).reshape(-1), (ys / hm).reshape(-1)
    ref[..., 2] = ref[..., 5] = 0.5
    if regime == "anchor":
        ref[..., 3] = ref[..., 4] = ANCHOR
    elif regime == "grown":   # 5x the anchors: most corners leave the window (3x: 24 % of them, measured in fp64)
        ref[..., 3] = ref[..., 4] = 5 * ANCHOR
    else:                     # heavy tail: Pareto sizes from the anchor up, ~3 % above half the map; boxes cross the edge
        size = ANCHOR * torch.rand(B, s, generator=gen).clamp_min(1e-6) ** (-1 / 1.2)
        ref[..., 3] = size.clamp_max(0.75)
        ref[..., 4] = (size * (0.5 + torch.rand(B, s, generator=gen))).clamp_max(0.75)
    if rot:
        ref[..., 6] = torch.rand(B, s, generator=gen)
    nvar = 5 if rot else 4
    value = torch.randn(B, s, H, D, generator=gen)
    offsets = torch.randn(B, s, H * L * nvar, generator=gen) * 0.5
    logits = torch.randn(B, s, H * L * P, generator=gen)
    gout = torch.randn(B, s, H * D, generator=gen)
    return tuple(t.to(dev) for t in (ref, value, offsets, logits, gout)) + (nvar,)


# (map, regime) -> (rotated, shared projection): both forms and both offset widths on each map
ENCODER = {("188x188", "anchor"): (False, False), ("188x188", "grown"): (False, True), ("188x188", "heavy"): (True, False),
           ("101x147", "anchor"): (False, True), ("101x147", "grown"): (True, False), ("101x147", "heavy"): (True, True)}


@pytest.mark.parametrize("map_name,regime", list(ENCODER))
def test_encoder_tile_path_against_fp64(dev, map_name, regime):
    hm, wm = MAPS[map_name]
    rot, shared = ENCODER[(map_name, regime)]
    gen = torch.Generator().manual_seed(100 + list(ENCODER).index((map_name, regime)))
    ref, value, offsets, logits, gout, nvar = _encoder_case(dev, hm, wm, regime, rot, gen)
    kidx = _lattice().to(dev)
    near = redraw_kinks(ref, offsets, kidx, rot, [[hm, wm]], H, gen)
    assert near < 0.01, near
    px, py = pixels(ref, offsets, kidx, rot, [[hm, wm]], H)
    share = out_of_window_share(px, py, hm, wm)
    print("%s %s: %.3f of the in-map corners outside their tile window, %.4f of the points redrawn" % (
        map_name, regime, share, near))
    # measured (fp64 geometry of these draws): anchor 0.000 / 0.000, grown 0.640 / 0.285 (rotated), heavy 0.189 / 0.105
    if regime == "anchor":
        assert share < 0.01          # anchor boxes stay inside the window
    elif regime == "grown":
        assert share >= (0.5 if map_name == "188x188" else 0.25)   # the binned path takes most / many corners
    else:
        assert 0.05 < share < 0.5    # a mix of both paths
    _run(dev, "encoder %s %s" % (map_name, regime), hm, wm, ref, value, offsets, logits, kidx, nvar, gout, shared)


@pytest.mark.parametrize("grad", ["normal", "log_uniform"])
def test_decoder_binned_path_against_fp64(dev, grad):
    """1200 free rotated queries on the 188 x 188 map: every corner goes through the bins (box_bin_reduce_kernel).  With
    grad_out log-uniform over 1e-6 ... 1e2 (random signs) most bins hold a handful of entries, many of them only small
    ones: the element-wise bar asks each bin's sum for fp32 accuracy relative to ITS products."""
    hm, wm = MAPS["188x188"]
    lq, nvar = 1200, 5
    gen = torch.Generator().manual_seed(17 if grad == "normal" else 19)
    ref = torch.rand(B, lq, 7, generator=gen)
    ref[..., 3:5] = ref[..., 3:5] * 0.2 + 0.02
    value = torch.randn(B, hm * wm, H, D, generator=gen)
    offsets = torch.randn(B, lq, H * L * nvar, generator=gen) * 0.5
    logits = torch.randn(B, lq, H * L * P, generator=gen)
    gout = (torch.randn(B, lq, H * D, generator=gen) if grad == "normal" else
            log_uniform_signed((B, lq, H * D), 1e-6, 1e2, gen))
    ref, value, offsets, logits, gout = (t.to(dev) for t in (ref, value, offsets, logits, gout))
    kidx = _lattice().to(dev)
    near = redraw_kinks(ref, offsets, kidx, True, [[hm, wm]], H, gen)
    assert near < 0.01, near
    _run(dev, "decoder %s" % grad, hm, wm, ref, value, offsets, logits, kidx, nvar, gout, shared=(grad == "normal"))
