"""CPU pins of the inputs and of the error bar of tests/test_box_fused_fp64_gpu.py, before a kernel is involved.

1. The conditions of every case hold: the share of near-boundary points of the first draw, the far-corner share of the tile
   and window cases, the share of in-map corners, the hand-made parts of gates / off_map / softmax_edges, and the host
   dispatch condition of the path the case names, re-derived from (l, s, lq, p): a change to the dispatch makes this test
   say so rather than silently testing another kernel.
2. An honest fp32 implementation from plain torch parts (box_fp64_cases.box_attention_fp32) meets the GPU test's bar on
   every case, so every bar is known to be attainable.  Largest err / bound per path: the docstring of box_fp64_cases.
3. The reference is sensitive: the level starts of another layout, a softmax per level, a dropped lattice point and relu'(0) = 1
   each fail the bar."""
import unittest.mock

import pytest
import torch

from box_fp64_cases import (BACKWARD, CASES, DECODER, FORWARD, IN_MAP_MIN, NEAR_MAX, TENSORS, TILE_CASES, WINDOW,
                            box_attention_fp32, build, case_pixels, check, dispatch_path, far_share, in_map_share, lattice,
                            point_outside, reference)
from fp64_ref import near_cell_boundary


# ---- 1. conditions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_is_well_formed(name):
    case, spec = build(name), CASES[name]
    b, s, h, d = case["value"].shape
    lq, nl, p, nvar = case["ref"].shape[1], case["shapes"].shape[0], case["kidx"].shape[0], case["nvar"]
    assert (b, lq, h, d, p) == tuple(spec[k] for k in ("b", "lq", "h", "d", "p"))
    assert s == int((case["shapes"][:, 0] * case["shapes"][:, 1]).sum()) and case["starts"][0] == 0
    assert case["offsets"].shape == (b, lq, h * nl * nvar) and case["logits"].shape == (b, lq, h * nl * p)
    assert case["grad_out"].shape == (b, lq, h * d) and case["ref"].shape == (b, lq, 7) and case["kidx"].shape == (p, 2)
    assert all(case[k].dtype == torch.float32 and case[k].is_contiguous()
               for k in ("value", "ref", "offsets", "logits", "kidx", "grad_out"))
    # the path the case is there for is the one the host code takes (forward-only cases have no backward: D != 32)
    if case["path"] == "forward":
        assert d != 32
    else:
        assert d == 32 and dispatch_path(nl, s, lq, p) == case["path"]
    assert nl <= 8 and nl * p <= 128 and (256 // max(1, _lanes(d))) * nl * p <= 4096      # inside the caps of check()
    print("%s: near %.4f" % (name, case["near"]))
    assert case["near"] < NEAR_MAX, case["near"]
    assert not bool(near_cell_boundary(*case_pixels(case)).any())
    share = in_map_share(case)
    print("%s: in-map corners %.3f" % (name, share))
    if case["sampling"]:
        assert share >= IN_MAP_MIN, share
    if case["far"] is not None:
        far = far_share(case)
        print("%s: far corners %.3f" % (name, far))
        assert case["far"][0] <= far < case["far"][1], far
    ref = reference(name)
    for k in TENSORS:
        assert bool((ref[k].abs() <= ref[k + "_mag"] * (1 + 1e-12) + 1e-300).all()), k
        assert bool((ref[k + "_geo"] >= 0).all())


def _lanes(d):
    lp = 1
    while lp * 4 < d:
        lp *= 2
    return lp


def test_paths_are_all_present():
    assert len(DECODER) == 8 and len(TILE_CASES) == 12 and len(WINDOW) == 12 and len(FORWARD) == 8
    assert sorted(CASES[n]["p"] for n in TILE_CASES if "_p" in n) == [1, 9, 16, 31, 32]
    assert {CASES[n]["p"] for n in WINDOW} == {33, 49, 128}
    assert [CASES[n]["d"] for n in FORWARD] == [4, 8, 12, 16, 24, 64, 128, 256]
    assert build("below_grid_threshold")["value"].shape[1] == 1023
    assert lattice(25).shape == (25, 2) and lattice(31).shape == (31, 2) and torch.equal(lattice(31), lattice(36)[:31])


def test_gates_case():
    case = build("gates")
    b, lq, _ = case["ref"].shape
    h = case["value"].shape[2]
    off = case["offsets"].view(b, lq, h, 5)
    q, m = torch.arange(lq).view(1, lq, 1), torch.arange(h).view(1, 1, h)
    group = ((q + m) % 4).expand(b, lq, h)
    assert bool((off[..., 2][group == 0] == -8.0).all()) and bool((off[..., 2][group == 1] == -9.5).all())
    assert bool((off[..., 2:4][group == 2] == -8.5).all())
    ref = case["ref"]
    assert int((ref[..., 3] < 0).sum()) == b * lq // 4
    assert bool((ref[0, :8, 6] == 0).all()) and bool((off[0, :8, :, 4] == 0).all())
    # in fp32, as the kernels evaluate it: the size at offset -8 is exactly 0; both gates closed put every point on the centre
    size = ref[..., 3].unsqueeze(-1) + off[..., 2] / 8 * ref[..., 3].unsqueeze(-1)
    assert bool((size[group == 0] == 0).all())
    px, py = case_pixels(case)
    both = (group == 2) & (ref[..., 3] > 0).unsqueeze(-1)
    assert bool(both.any()) and bool((px[both].amax(-1) == px[both].amin(-1)).all())
    open_by_sign = (group == 1) & (ref[..., 3] < 0).unsqueeze(-1)      # a negative length under a negative factor: open again
    assert bool(open_by_sign.any()) and bool((px[open_by_sign].amax(-1) > px[open_by_sign].amin(-1)).all())
    r = reference("gates")
    assert bool((r["grad_offsets"].view(b, lq, h, 5)[..., 2][group == 0] == 0).all())


def test_off_map_case():
    case = build("off_map")
    outside = point_outside(case)
    share = float(outside.float().mean())
    print("off_map: %.3f of the points outside the map" % share)
    assert share >= 0.20
    rows_out, rows_in = outside.all(-1).all(-1), (~outside).all(-1).all(-1)      # [B, Q, H]
    assert bool(rows_out.any()) and bool(rows_in.any())
    r = reference("off_map")
    b, lq, h = rows_out.shape
    for k in ("out", "grad_offsets", "grad_logits"):
        assert bool((r[k].view(b, lq, h, -1)[rows_out] == 0).all()), k


def test_softmax_edges_case():
    case = build("softmax_edges")
    b, lq, _ = case["logits"].shape
    lg = case["logits"].view(b, lq, 4, 18)
    assert bool((lg[:, 1::3] == lg[:, 1::3][..., :1]).all())
    hot = lg[:, 2::3]
    assert bool(((hot == 80).sum(-1) == 1).all()) and bool(((hot == -80).sum(-1) == 17).all())
    top = torch.softmax(lg[:, 0::3].double(), -1).amax(-1)
    assert float(top.median()) > 0.99


# ---- 2. an honest fp32 implementation meets the bar ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_honest_fp32_meets_the_bar(name):
    case = build(name)
    got = box_attention_fp32(case)
    if case["path"] == "forward":
        got = {"out": got["out"]}
    check("fp32 " + name, case, reference(name), got)


# ---- 3. the reference is sensitive -----------------------------------------------------------------------------------------------
def _fails(name, **mutation):
    case = build(name)
    with pytest.raises(AssertionError, match="elements outside"):
        check("mutated " + name, case, reference(name), box_attention_fp32(case, **mutation))


def test_levels_swapped_in_starts_fail():
    """The level starts of the reversed layout (the last level first): every level reads another level's cells."""
    case = build("three_levels")
    cells = (case["shapes"][:, 0] * case["shapes"][:, 1]).flip(0)
    _fails("three_levels", starts=(torch.cumsum(cells, 0) - cells).flip(0))


def test_softmax_per_level_fails():
    _fails("three_levels", softmax_per_level=True)
    _fails("eight_levels_cap", softmax_per_level=True)


def test_dropped_lattice_point_fails():
    for name in ("three_levels", "tile_33x32", "window_33x32_p49_near"):
        _fails(name, drop_point=CASES[name]["p"] - 1)


def test_relu_gradient_one_at_zero_fails():
    """clamp(min=0) passes the gradient at exactly 0, relu does not: the gates case has sizes of exactly 0."""
    with unittest.mock.patch("torch.relu", lambda x: x.clamp(min=0)):
        _fails("gates")
    check("fp32 gates", build("gates"), reference("gates"), box_attention_fp32(build("gates")))


def test_backward_cases_alternate_forms():
    """The GPU test alternates separate logits / shared projection over the backward cases: both forms on every path, the
    shared one among the multi-level cases."""
    shared = {n: i % 2 == 1 for i, n in enumerate(BACKWARD)}
    for names in (DECODER, TILE_CASES, WINDOW):
        assert {shared[n] for n in names} == {False, True}
    assert any(shared[n] for n in DECODER if len(CASES[n]["levels"]) > 1)
