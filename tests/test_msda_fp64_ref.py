"""CPU pins of the inputs and of the error bar of tests/test_msda_fp64_gpu.py, before a kernel is involved.

1. The fp32 CPU restatement of the op (oracle.msda_forward / msda_backward: the arithmetic of the CUDA reference, one
   rounding per operation) passes assert_elementwise against fp64_ref.sample_fp64 on every case at the GPU test's constant,
   so inputs and bar are sound and every bar is known to be attainable.
2. The numeric conditions on the inputs hold (share of redrawn points, share of points off the map, corner counts, window
   shares of the grid regimes, the pile-up count, the share of lattice points on the -1 line), so a case cannot hide a failure by
   not exercising what it is there for.
3. The lattice convention: at px == -1 or py == -1 exactly the kernels and the CUDA reference call the whole point outside;
   sample_fp64 takes the one-sided derivative of the weight-0 corner unless reference_inside=True.
4. Mutations that the absolute tolerances of tests/test_msda_gpu.py let through fail the bar."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from fp64_ref import assert_elementwise, near_cell_boundary, sample_fp64
from msda_fp64_cases import (C, CASES, GRID, LATTICE, TENSORS, UNIFORM, build, check, corners_in_range, mutation_case,
                             n_terms, out_of_window_share, pixels, point_inside, reference, reference_of, takes_grid_kernel)

MSDA_GOLDENS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "msda_*.npz")))


def run_oracle(oracle, case, value=None):
    """out, grad_value, grad_loc, grad_attn of the fp32 CPU oracle as float32 tensors."""
    v = (case["value"] if value is None else value).numpy()
    args = (v, case["shapes"].numpy(), case["level_start"].numpy(), case["loc"].numpy(), case["attn"].numpy())
    out = oracle.msda_forward(*args)
    gv, gl, ga = oracle.msda_backward(*args, case["grad_out"].numpy())
    return {k: torch.from_numpy(a) for k, a in (("out", out), ("grad_value", gv), ("grad_loc", gl), ("grad_attn", ga))}


# ---- 1. the oracle against the bar ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_oracle_passes_the_bar(oracle_mod, name):
    """Largest err / bound at c = 4 over the cases of a kind: see the comment at msda_fp64_cases.C."""
    case = build(name)
    ratios = check("oracle " + name, case, reference(name), run_oracle(oracle_mod, case))
    assert set(ratios) == set(TENSORS)


# ---- 2. conditions on the inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_is_well_formed(name):
    case = build(name)
    b, s, h, d = case["value"].shape
    lq, nl, p = case["loc"].shape[1], case["loc"].shape[3], case["loc"].shape[4]
    assert case["loc"].shape == (b, lq, h, nl, p, 2) and case["attn"].shape == (b, lq, h, nl, p)
    assert case["grad_out"].shape == (b, lq, h * d)
    assert s == int((case["shapes"][:, 0] * case["shapes"][:, 1]).sum())
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (case["value"], case["loc"], case["attn"], case["grad_out"]))
    torch.testing.assert_close(case["attn"].sum((-1, -2)), torch.ones(b, lq, h), rtol=0, atol=1e-6)
    px, py = pixels(case["loc"], case["shapes"])
    if case["exact"]:
        assert case["redrawn"] == 0.0
        assert bool((px * 2 == torch.round(px * 2)).all()) and bool((py * 2 == torch.round(py * 2)).all())
    else:
        # at most 2 % of the points were redrawn for nearness to a cell boundary (measured 0.1 .. 0.84 %, the largest on
        # d4_p1; 0 of the 18 points of d256), and none is near one now
        assert case["redrawn"] <= 0.02, case["redrawn"]
        assert not bool(near_cell_boundary(px, py).any())
    assert takes_grid_kernel(case) == (name in GRID or name == "lattice_grid")
    # the reference is the same kind of object for every case: magnitudes above the values
    ref = reference(name)
    for k in TENSORS:
        assert bool((ref[k].abs() <= ref[k + "_mag"] * (1 + 1e-12) + 1e-300).all()), k
        assert bool((ref[k + "_geo"] >= 0).all()) and (not case["exact"] or float(ref[k + "_geo"].max()) == 0.0)


@pytest.mark.parametrize("name", UNIFORM)
def test_uniform_cases_cover_the_map_edge(name):
    """Between 40 % and 80 % of the points have a coordinate outside [0, 1] (measured 59 .. 66 %; 1 - 1 / 1.6^2 = 61 % expected), and every
    case has a point off the map and points with exactly one, two and all four corners on it.  (Three corners cannot be in
    range: the count is the product of the columns in range, 0 .. 2, and the rows in range, 0 .. 2.)"""
    case = build(name)
    off = ((case["loc"] < 0) | (case["loc"] > 1)).any(-1).float().mean()
    assert 0.4 <= float(off) <= 0.8, float(off)
    px, py = pixels(case["loc"], case["shapes"])
    n = corners_in_range(px, py, case["shapes"])
    assert sorted(set(n.unique().tolist())) == [0, 1, 2, 4]
    assert bool((~point_inside(px, py, case["shapes"])).any())
    # off the map by the whole-point rule == no corner in range, because no point is near a boundary
    assert torch.equal(point_inside(px, py, case["shapes"]), n > 0)


@pytest.mark.parametrize("name", GRID)
def test_grid_regimes_split_between_window_and_global_path(name):
    """Share of the in-map corners outside the 16 x 16 window of the query's 8 x 8 tile, from the float64 geometry.  Measured:
        map      near    mixed   free
        32x32    0.000   0.080   0.814
        29x37    0.000   0.075   0.816
        3x400    0.000   0.105   0.961
        1x1024   0.000   0.112   0.983
    and 0.787 for pile_up_grid (queries from all over the 30 x 40 map onto one cell), held to the bound of the free regime."""
    case = build(name)
    hm, wm = (int(v) for v in case["shapes"][0])
    px, py = pixels(case["loc"], case["shapes"])
    share = out_of_window_share(px, py, hm, wm)
    print("%s: %.3f of the in-map corners outside the tile window, %.4f of the points redrawn" % (name, share, case["redrawn"]))
    if case["regime"] == "near":
        assert share < 0.01
    elif case["regime"] == "mixed":
        assert 0.05 < share < 0.5
    else:
        assert share >= 0.5
    if hm == 1:   # a one-row map: the vertical spread stays within 0.4 of the map height around the row's centre
        assert float(py.abs().max()) <= 0.4 + 1e-6 or case["regime"] != "near"


def test_pile_up_piles_up():
    """Every point of the pile-up case has the cell (14, 18) among its corners: 4800 entries in one grad_value row."""
    for name in ("pile_up", "pile_up_grid"):
        ref = reference(name)
        print("%s: largest grad_value_n %d" % (name, int(ref["grad_value_n"].max())))
        assert float(ref["grad_value_n"].max()) >= 2000          # measured: 4804 and 4800
    assert not takes_grid_kernel(build("pile_up")) and takes_grid_kernel(build("pile_up_grid"))


def _on_minus_one_line(case):
    px, py = pixels(case["loc"], case["shapes"])
    return (px == -1) | (py == -1)


def test_lattice_covers_the_minus_one_line():
    """Between 5 % and 20 % of the lattice points lie on px == -1 or py == -1 (measured 11.2 %)."""
    share = float(_on_minus_one_line(build("lattice")).float().mean())
    print("lattice: %.4f of the points on the -1 line" % share)
    assert 0.05 <= share <= 0.2
    assert bool(_on_minus_one_line(build("lattice_grid")).any())
    px, py = pixels(build("lattice")["loc"], build("lattice")["shapes"])
    for lv, (hl, wl) in enumerate(CASES["lattice"]["levels"]):   # -1.5, -1, -0.5, 0, side - 1, side - 0.5, side all occur
        for coord, side in ((px[:, :, :, lv], wl), (py[:, :, :, lv], hl)):
            assert {-1.5, -1.0, -0.5, 0.0, side - 1.0, side - 0.5, float(side)} <= set(coord.unique().tolist())


# ---- 3. the lattice convention -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LATTICE)
def test_lattice_convention_of_the_minus_one_line(oracle_mod, name):
    """On the -1 line the oracle (like the kernels and box_attn_kernel.cuh) writes exactly 0 everywhere; the default
    sample_fp64 has a one-sided derivative there and agrees with the oracle at every other point; with reference_inside=True
    all four tensors agree at every point (test_fp32_oracle_passes_the_bar)."""
    case = build(name)
    got = run_oracle(oracle_mod, case)
    line = _on_minus_one_line(case)
    assert bool((got["grad_loc"][line] == 0).all()) and bool((got["grad_attn"][line] == 0).all())
    plain = reference_of(case, reference_inside=False)
    assert bool((plain["grad_loc"][line] != 0).any()), "the per-corner rule has a one-sided derivative on the line"
    differs = (plain["grad_loc"] != reference(name)["grad_loc"]).any(-1)
    assert bool(differs.any()) and not bool((differs & ~line).any())
    for k in ("out", "grad_value", "grad_attn"):      # weight 0: nothing but grad_loc sees the corner
        assert torch.equal(plain[k], reference(name)[k]), k
    off = ~line
    assert_elementwise(name + " grad_loc off the line", got["grad_loc"][off], plain["grad_loc"][off], plain["grad_loc_mag"][off],
                       n_terms(case, plain, "grad_loc"), C, plain["grad_loc_geo"][off])


@pytest.mark.parametrize("golden_name", MSDA_GOLDENS)
def test_reference_inside_does_not_move_the_goldens(golden_name):
    """No sampling point of the three goldens sits on the -1 line (asserted), so sample_fp64 returns the same bits with the
    keyword on and off."""
    g = golden(golden_name)
    t = {k: torch.from_numpy(g[k]) for k in ("value", "shapes", "level_start", "loc", "attn", "grad_out")}
    px, py = pixels(t["loc"], t["shapes"])
    assert not bool(((px == -1) | (py == -1)).any())
    args = (t["value"].double(), t["shapes"], t["level_start"], t["loc"].double(), t["attn"].double(), t["grad_out"].double())
    off, on = sample_fp64(*args), sample_fp64(*args, reference_inside=True)
    assert off.keys() == on.keys()
    for k in off:
        assert torch.equal(off[k], on[k]), k
    np.testing.assert_allclose(on["grad_loc"].numpy(), g["grad_loc"].astype(np.float64), rtol=1e-9, atol=1e-12 * float(np.abs(g["grad_loc"]).max()))


# ---- 4. the bar has teeth ------------------------------------------------------------------------------------------------------
def _old_tolerance_passes(got, ref64, atol=1e-4):
    return np.allclose(got.double().numpy(), ref64.numpy(), rtol=1e-4, atol=atol)


def test_bar_catches_a_dropped_corner_in_a_small_row(oracle_mod):
    """The last row of the map holds values of 1e-6.  A result computed without that row (its corners dropped: the row zeroed
    on the tested side only) is 100 % wrong in every out element sampled below the last row's centres; it passes atol = 1e-4
    (and the forward's 1e-5) and fails the bar."""
    case = mutation_case()
    ref = reference_of(case)
    good = run_oracle(oracle_mod, case)
    check("mutation case, unchanged", case, ref, good)
    hm, wm = (int(v) for v in case["shapes"][0])
    dropped = case["value"].clone()
    dropped[:, (hm - 1) * wm:] = 0
    bad = run_oracle(oracle_mod, case, value=dropped)
    assert not torch.equal(bad["out"], good["out"])
    assert _old_tolerance_passes(bad["out"], ref["out"], atol=1e-5), "a dropped corner must pass atol = 1e-4 for this test to mean anything"
    with pytest.raises(AssertionError, match="out: .* elements outside"):
        check("dropped corner (passes atol = 1e-4)", case, ref, {"out": bad["out"]})
    with pytest.raises(AssertionError, match="elements outside"):
        check("dropped corner (passes atol = 1e-4)", case, ref, {"grad_loc": bad["grad_loc"]})


def test_bar_catches_a_sign_flip_of_a_small_grad_loc_element(oracle_mod):
    """One grad_loc element below 1e-4 of the tensor's largest, with the wrong sign: passes atol = 1e-4, fails the bar at the
    helper's cap c = 16."""
    case = mutation_case()
    ref = reference_of(case)
    good = run_oracle(oracle_mod, case)
    r, mag, geo = ref["grad_loc"], ref["grad_loc_mag"], ref["grad_loc_geo"]
    # well conditioned, below 1e-4 of the largest, and small enough for 2 |element| to stay under atol = 1e-4
    quiet = (geo < 1e-4 * r.abs()) & (mag < 4 * r.abs()) & (r.abs() < 1e-4 * r.abs().max()) & (r.abs() < 4e-5) & (r != 0)
    assert bool(quiet.any())
    flat = torch.where(quiet, r.abs(), torch.zeros_like(r)).reshape(-1)
    i = int(torch.argmax(flat))
    bad = good["grad_loc"].clone()
    bad.view(-1)[i] = -bad.view(-1)[i]
    assert _old_tolerance_passes(bad, r), "a flipped element of %.3g (largest %.3g) must pass atol = 1e-4 for this test to mean anything" % (
        float(flat[i]), float(r.abs().max()))
    with pytest.raises(AssertionError, match="1 of"):
        check("sign flip (passes atol = 1e-4)", case, ref, {"grad_loc": bad}, c=16)
