"""GPU: every arm of the fused box attention (csrc/box_fused.hip) against the float64 op of tests/fp64_ref.py, element by
element, on the small cases of tests/box_fp64_cases.py (conditions and an honest fp32 implementation: test_box_fp64_ref.py):

  decoder  box_bwd_kernel<32, false> + the bins: several levels up to the caps L = 8, L * P = 128, s == lq below the grid
           threshold, one query, closed relu gates, boxes off the map, saturated and flat softmax
  tile     box_bwd_tile_a/b_kernel at P = 1 .. 32 and on maps where the launch geometry matters (strips, W < 8, H < 4, sides one
           past a tile multiple, queries that are not on their cells)
  window   box_bwd_kernel<32, true> (P > 32), which no other test launches
  forward  box_fwd_kernel at D = 4 .. 256 (scalar and quad-DPP body, idle channel lanes)

through BoxAttnFusedFunction.apply in both forms (separate logits; one shared projection, logits=None), alternating over the
cases.  Then the refusals of the host code's check(), empty calls, and properties of the backward: equal bits run to run,
grad_out scaled by 2^-60 and 2^60 (the fixed-point scale of box_bin_reduce_kernel moves with the call's largest |grad_out|
and nothing else may), grad_out == 0 and one +inf in grad_out (the reduce kernel's non-finite arm).

Found by test_empty_calls: with B = 0 or Lq = 0 the host code returned before anything wrote the workspace's overflow word,
and BoxAttnFusedFunction.backward then read it uninitialised (EFG_CHECK_BINS=1) and could report overflowed bins; the host
code now zeroes the word on that path too."""
import functools

import pytest
import torch

from box_fp64_cases import (BACKWARD, FORWARD, NEAR_MAX, build, check, far_share, lattice, point_outside, reference_of)
from efg_amd.operators import box_attention_func
from efg_amd.operators.box_attention_func import BoxAttnFusedFunction

pytestmark = pytest.mark.gpu

assert box_attention_func._CHECK_BINS, "the tests read the bins' overflow word after every backward (EFG_CHECK_BINS=1)"

SHARED = {n: i % 2 == 1 for i, n in enumerate(BACKWARD + FORWARD)}   # the form of each case: both forms on every path
INPUTS = ("value", "shapes", "starts", "ref", "offsets", "logits", "kidx")


def _apply(t, nvar, shared, grad_out=None):
    """out (and, with grad_out, the three gradients) of BoxAttnFusedFunction on the device tensors `t`."""
    n_lg = t["logits"].shape[-1]
    if grad_out is None:
        with torch.no_grad():
            proj = torch.cat([t["logits"], t["offsets"]], -1) if shared else t["offsets"]
            return {"out": BoxAttnFusedFunction.apply(t["value"], t["shapes"], t["starts"], t["ref"], proj,
                                                      None if shared else t["logits"], t["kidx"], nvar)}
    v = t["value"].clone().requires_grad_(True)
    if shared:
        proj = torch.cat([t["logits"], t["offsets"]], -1).requires_grad_(True)
        out = BoxAttnFusedFunction.apply(v, t["shapes"], t["starts"], t["ref"], proj, None, t["kidx"], nvar)
        out.backward(grad_out)
        g_lg, g_off = proj.grad[..., :n_lg], proj.grad[..., n_lg:]
    else:
        o, lg = t["offsets"].clone().requires_grad_(True), t["logits"].clone().requires_grad_(True)
        out = BoxAttnFusedFunction.apply(v, t["shapes"], t["starts"], t["ref"], o, lg, t["kidx"], nvar)
        out.backward(grad_out)
        g_lg, g_off = lg.grad, o.grad
    torch.cuda.synchronize()
    return {"out": out.detach(), "grad_value": v.grad, "grad_offsets": g_off, "grad_logits": g_lg}


@functools.lru_cache(maxsize=None)
def _on(name, dev):
    case = build(name)
    return {k: case[k].to(dev) for k in INPUTS + ("grad_out",)}


def _run(name, dev, grad_out=None, forward_only=False):
    t = _on(name, dev)
    return _apply(t, build(name)["nvar"], SHARED[name], None if forward_only else (t["grad_out"] if grad_out is None else grad_out))


@functools.lru_cache(maxsize=None)
def _reference(name, dev, scale=1.0):
    """The float64 reference of a case on the device, computed once (grad_out x `scale`)."""
    return reference_of(build(name), _on(name, dev)["grad_out"] * scale, dev)


# ---- every path against fp64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BACKWARD)
def test_backward_paths_against_fp64(dev, name):
    """Largest err / bound per path on MI355X: the docstring of box_fp64_cases."""
    case = build(name)
    assert case["near"] < NEAR_MAX, case["near"]
    if case["far"] is not None:
        assert case["far"][0] <= far_share(case) < case["far"][1]
    got = _run(name, dev)
    r = _reference(name, dev)
    check("%s %s" % (case["path"], name), case, r, got)
    if name == "off_map":   # a (query, head) whose every point is off the map: its out row and its gradients are exactly 0
        rows = point_outside(case).all(-1).all(-1).to(dev)
        b, lq, h = rows.shape
        assert bool(rows.any())
        for k in ("out", "grad_offsets", "grad_logits"):
            assert bool((got[k].reshape(b, lq, h, -1)[rows] == 0).all()), k
    if name == "gates":     # the gate closed at exactly 0 passes no gradient
        b, lq, h = case["ref"].shape[0], case["ref"].shape[1], case["value"].shape[2]
        closed = (case["offsets"].view(b, lq, h, 5)[..., 2] == -8.0).to(dev)
        assert bool((got["grad_offsets"].reshape(b, lq, h, 5)[..., 2][closed] == 0).all())


@pytest.mark.parametrize("name", FORWARD)
def test_forward_head_dims_against_fp64(dev, name):
    case = build(name)
    assert case["near"] < NEAR_MAX, case["near"]
    check("forward %s" % name, case, _reference(name, dev), _run(name, dev, forward_only=True))


# ---- refusals and empty calls ------------------------------------------------------------------------------------------------
def _tiny(dev, d=32, p=25, nl=1, nvar=5, b=1, lq=3, h=2):
    """Well-formed inputs of any shape on levels of 2 x 2 cells."""
    t = dict(value=torch.randn(b, 4 * nl, h, d), shapes=torch.tensor([[2, 2]] * nl), starts=torch.arange(nl) * 4,
             ref=torch.rand(b, lq, 7), offsets=torch.randn(b, lq, h * nl * nvar), logits=torch.randn(b, lq, h * nl * p),
             kidx=lattice(p))
    return {k: v.to(dev) for k, v in t.items()}


REFUSED = {"forward_d4_p25": dict(d=4, p=25), "points_129": dict(p=129), "levels_9": dict(nl=9, p=1), "d6": dict(d=6),
           "d260": dict(d=260), "num_var_3": dict(nvar=3)}


@pytest.mark.parametrize("name", list(REFUSED))
def test_forward_refusals(dev, name):
    kw = REFUSED[name]
    t = _tiny(dev, **kw)
    with pytest.raises(RuntimeError, match="box_attn_fused"):
        _apply(t, kw.get("nvar", 5), shared=False)


def test_backward_refuses_other_head_dims(dev):
    t = _tiny(dev, d=64)
    with pytest.raises(RuntimeError, match="head dim 32 only"):
        _apply(t, 5, shared=False, grad_out=torch.randn(1, 3, 2 * 64, device=dev))


@pytest.mark.parametrize("which", ["b0", "lq0"])
@pytest.mark.parametrize("shared", [False, True])
def test_empty_calls(dev, which, shared):
    """B = 0 and Lq = 0: empty out, empty or zero gradients, no error (see the module docstring)."""
    t = _tiny(dev, b=0) if which == "b0" else _tiny(dev, lq=0)
    b, lq = t["ref"].shape[:2]
    # scratch memory that is not zero, for the allocator to hand to the backward's workspace
    junk = torch.full((1 << 16,), -1, dtype=torch.int32, device=dev)
    del junk
    got = _apply(t, 5, shared, grad_out=torch.zeros(b, lq, 64, device=dev))
    assert got["out"].shape == (b, lq, 64)
    assert got["grad_value"].shape == t["value"].shape and not bool(got["grad_value"].any())
    assert got["grad_offsets"].shape == t["offsets"].shape and got["grad_logits"].shape == t["logits"].shape


# ---- properties ------------------------------------------------------------------------------------------------------------------
PROPERTY_CASES = ("three_levels", "tile_33x32")


@pytest.mark.parametrize("name", PROPERTY_CASES + ("tile_33x32_p32",))
def test_backward_is_reproducible(dev, name):
    """Decoder bins and coloured tile launches: two identical passes give the same bits.  (Not the window path: it flushes
    with float atomics.)"""
    a, b = _run(name, dev), _run(name, dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", PROPERTY_CASES)
def test_grad_out_scaled_by_powers_of_two(dev, name):
    """grad_out x 2^k, k = -60, 0, 60: every tensor meets the bar at each k, and the binned grad_value (decoder: every corner;
    tile: the far corners, next to exact power-of-two scalings of the fp32 products of the window) is the k = 0 result times 2^k
    bit for bit: the scaling is exact in every product and only moves ex / sh of box_bin_reduce_kernel."""
    case = build(name)
    base = _on(name, dev)["grad_out"]
    got = {}
    for k in (-60, 0, 60):
        g = base * 2.0 ** k
        got[k] = _run(name, dev, grad_out=g)
        check("%s x 2^%d" % (name, k), case, _reference(name, dev, 2.0 ** k), got[k], grad_out=g)
    for k in (-60, 60):
        assert torch.equal(got[k]["grad_value"] * 2.0 ** -k, got[0]["grad_value"]), k
        assert torch.equal(got[k]["out"], got[0]["out"])


@pytest.mark.parametrize("name", PROPERTY_CASES)
def test_zero_grad_out(dev, name):
    got = _run(name, dev, grad_out=torch.zeros_like(_on(name, dev)["grad_out"]))
    for k in ("grad_value", "grad_offsets", "grad_logits"):
        assert bool(torch.isfinite(got[k]).all()) and not bool(got[k].any()), k


def test_one_inf_in_grad_out(dev):
    """One +inf in one (query, head) row of grad_out on the decoder path: box_bin_reduce_kernel takes its non-finite arm (plain
    fp32 sums in list order).  The grad_value elements that element reaches -- where two finite float64 runs with 0 and 1 in its
    place differ -- are non-finite; every other one, and the offsets / logits gradients of every other row, meet the bar
    against the reference with 0 in its place (no bin allowance: nothing is rounded to the fixed-point unit on this arm)."""
    name, (bi, qi, mi, ch) = "three_levels", (0, 5, 2, 7)
    case = build(name)
    h, d = case["value"].shape[2:]
    g = {v: case["grad_out"].clone() for v in (0.0, 1.0, float("inf"))}
    for v, t in g.items():
        t[bi, qi, mi * d + ch] = v
    # the two finite references on the CPU: its index_add_ sums in a fixed order, so they differ only where the element reaches
    r0, r1 = reference_of(case, g[0.0]), reference_of(case, g[1.0])
    touched = r0["grad_value"] != r1["grad_value"]
    assert (touched.sum((0, 1, 2)) > 0).tolist() == [c == ch for c in range(d)]     # channel `ch` of cells of head `mi`
    got = {k: v.cpu() for k, v in _run(name, dev, grad_out=g[float("inf")].to(dev)).items()}
    assert not bool(torch.isfinite(got["grad_value"][touched]).any())
    b, lq = case["ref"].shape[:2]
    rows = {"grad_value": touched}
    for k in ("grad_offsets", "grad_logits"):
        hit = torch.zeros(b, lq, h, r0[k].shape[-1] // h, dtype=torch.bool)
        hit[bi, qi, mi] = True
        rows[k] = hit.reshape(r0[k].shape)
    rest = {k: torch.where(rows[k], r0[k].float(), got[k]) for k in rows}
    rest["out"] = got["out"]
    check("one inf", case, r0, rest, bins=False)
