"""GPU: the sampling kernels of csrc/msda.hip -- msda_kernel<false>, msda_kernel<true> and the LDS-window backward
msda_bwd_grid_kernel<32> -- against the float64 op of tests/fp64_ref.py (sample_fp64), element by element: out, grad_value,
grad_loc and grad_attn each satisfy |got - ref| <= c sqrt(n) 2^-24 |terms| + geometry (fp64_ref.assert_elementwise), so an element
far below its tensor's largest one is held to its own size.  The cases, their conditions and the constant c = 4 are those of
tests/msda_fp64_cases.py; tests/test_msda_fp64_ref.py holds the fp32 CPU oracle to the same bars on the same inputs.

The kernels are called through box_attn_forward / box_attn_backward (one case also through MSDeformAttnFunction.apply), and
once more through the C ABI itself with grad_loc and grad_attn pre-filled with NaN: the backward must WRITE every element, 0
for a point off the map.

Largest err / bound at c = 4 measured on MI355X, per kernel and tensor:
    msda_kernel<false>         out 0.15 (lattice_grid, no geometry term), 0.095 otherwise
    msda_kernel<true>          grad_value 0.27 (lattice), 0.10 otherwise; grad_loc 0.089; grad_attn 0.074
    msda_bwd_grid_kernel<32>   grad_value 0.26 (lattice_grid), 0.078 otherwise; grad_loc 0.057; grad_attn 0.051
The pile-up rows (4800 entries each) stand at 0.0094 on the generic backward's global atomics and 0.0069 on the grid kernel.
The fp32 CPU oracle's figures on the same cases are next to msda_fp64_cases.C: the kernels are not further from float64 than
a plain fp32 evaluation is."""
import pytest
import torch

from msda_fp64_cases import CASES, GRID, build, check, pixels, point_inside, reference, takes_grid_kernel

pytestmark = pytest.mark.gpu

GRID_KERNEL, GENERIC_BWD, FWD = "msda_bwd_grid_kernel<32>", "msda_kernel<true>", "msda_kernel<false>"


def _on(dev, case):
    return tuple(case[k].to(dev) for k in ("value", "shapes", "level_start", "loc", "attn", "grad_out"))


def _launched(fn):
    """Run fn() with the launch records of efg_amd._prof on; returns (result, the kernel names the wrappers attributed)."""
    from efg_amd import _prof

    _prof.enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
        names = sorted(_prof.summary())
    finally:
        _prof.enable(False)
    return res, names


def _abi_backward(value, shapes, start, loc, attn, gout, fill):
    """efg_msda_backward_f32 itself, with grad_loc / grad_attn pre-filled with `fill` (grad_value is accumulated into: zeros)."""
    from efg_amd import _lib as L

    b, s, h, d = value.shape
    lq, nl, p = loc.shape[1], shapes.shape[0], loc.shape[4]
    gv = torch.zeros_like(value)
    gl, ga = torch.full_like(loc, fill), torch.full_like(attn, fill)
    rc = L.lib().efg_msda_backward_f32(L.ptr(value), L.ptr(shapes), L.ptr(start), L.ptr(loc), L.ptr(attn), L.ptr(gout), b, s, h, d,
                                       nl, lq, p, L.ptr(gv), L.ptr(gl), L.ptr(ga), L.stream())
    torch.cuda.synchronize()
    return rc, gv, gl, ga


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_fp64(dev, name):
    from efg_amd.operators.box_attention_func import box_attn_backward, box_attn_forward

    case, ref = build(name), reference(name)
    value, shapes, start, loc, attn, gout = _on(dev, case)
    out, fwd_names = _launched(lambda: box_attn_forward(value, shapes, start, loc, attn, 64))
    (gv, gl, ga), bwd_names = _launched(lambda: box_attn_backward(value, shapes, start, loc, attn, gout, 64))
    # dispatch: a later change of the condition cannot silently move a case to the other kernel
    grid = name in GRID or name == "lattice_grid"
    assert takes_grid_kernel(case) == grid
    assert fwd_names == [FWD] and bwd_names == [GRID_KERNEL if grid else GENERIC_BWD], (fwd_names, bwd_names)
    check(name, case, ref, {"out": out.cpu(), "grad_value": gv.cpu(), "grad_loc": gl.cpu(), "grad_attn": ga.cpu()})
    # every element of grad_loc / grad_attn is written, a point off the map as exactly 0
    rc, gv2, gl2, ga2 = _abi_backward(value, shapes, start, loc, attn, gout, float("nan"))
    assert rc == 0
    assert bool(torch.isfinite(gl2).all()) and bool(torch.isfinite(ga2).all()), "the backward left elements unwritten"
    off_map = ~point_inside(*pixels(case["loc"], case["shapes"]), case["shapes"])
    assert bool(off_map.any()) or CASES[name]["loc"] in ("near", "pile")
    assert bool((gl2.cpu()[off_map] == 0).all()) and bool((ga2.cpu()[off_map] == 0).all())
    assert torch.equal(gl2, gl) and torch.equal(ga2, ga)      # no atomics behind these two: the same bits as the wrapper's
    check(name + " (C ABI)", case, ref, {"grad_value": gv2.cpu()})


def test_through_msdeform_attn_function(dev):
    """The four-level case through MSDeformAttnFunction.apply and autograd: the same kernels, the same bars."""
    from efg_amd.operators.ms_deform_attn import MSDeformAttnFunction

    name = "four_levels"
    case, ref = build(name), reference(name)
    value, shapes, start, loc, attn, gout = _on(dev, case)
    value, loc, attn = (t.requires_grad_(True) for t in (value, loc, attn))
    out = MSDeformAttnFunction.apply(value, shapes, start, loc, attn, 64)
    out.backward(gout)
    check(name + " MSDeformAttnFunction", case, ref, {"out": out.detach().cpu(), "grad_value": value.grad.cpu(), "grad_loc": loc.grad.cpu(),
                                                      "grad_attn": attn.grad.cpu()})


@pytest.mark.parametrize("b,lq", [(2, 0), (0, 5)])
def test_empty_calls(dev, b, lq):
    """Lq = 0 and B = 0: empty outputs, an all-zero grad_value, no error."""
    from efg_amd.operators.box_attention_func import box_attn_backward, box_attn_forward

    h, d, p = 3, 8, 4
    shapes = torch.tensor([[4, 5]], device=dev)
    start = torch.zeros(1, dtype=torch.int64, device=dev)
    value = torch.randn(b, 20, h, d, device=dev)
    loc = torch.rand(b, lq, h, 1, p, 2, device=dev)
    attn = torch.rand(b, lq, h, 1, p, device=dev)
    out = box_attn_forward(value, shapes, start, loc, attn, 64)
    assert out.shape == (b, lq, h * d)
    gv, gl, ga = box_attn_backward(value, shapes, start, loc, attn, torch.randn(b, lq, h * d, device=dev), 64)
    torch.cuda.synchronize()
    assert gv.shape == value.shape and gl.shape == loc.shape and ga.shape == attn.shape
    assert bool((gv == 0).all())


@pytest.mark.parametrize("nl,d,message", [(9, 8, "msda: at most 8 levels"),
                                          (1, 260, "msda: head dim must be a multiple of 4 in [4,256], got 260"),
                                          (1, 6, "msda: head dim must be a multiple of 4 in [4,256], got 6")],
                         ids=["L9", "D260", "D6"])
def test_refused_calls_leave_the_outputs_alone(dev, nl, d, message):
    """L = 9, D = 260 and D = 6 are refused with check_dims' message, through the wrappers (RuntimeError) and at the C ABI, where
    the pre-filled output buffers keep every element."""
    import re

    from efg_amd import _lib as L
    from efg_amd.operators.box_attention_func import box_attn_backward, box_attn_forward

    b, lq, h, p = 1, 3, 2, 2
    shapes = torch.tensor([[2, 2]] * nl, device=dev)
    start = torch.arange(nl, device=dev) * 4
    value = torch.randn(b, 4 * nl, h, d, device=dev)
    loc = torch.rand(b, lq, h, nl, p, 2, device=dev)
    attn = torch.rand(b, lq, h, nl, p, device=dev)
    gout = torch.randn(b, lq, h * d, device=dev)
    with pytest.raises(RuntimeError, match=re.escape(message)):
        box_attn_forward(value, shapes, start, loc, attn, 64)
    with pytest.raises(RuntimeError, match=re.escape(message)):
        box_attn_backward(value, shapes, start, loc, attn, gout, 64)
    out = torch.full((b, lq, h * d), 7.0, device=dev)
    rc = L.lib().efg_msda_forward_f32(L.ptr(value), L.ptr(shapes), L.ptr(start), L.ptr(loc), L.ptr(attn), b, 4 * nl, h, d, nl, lq, p,
                                      L.ptr(out), L.stream())
    assert rc != 0 and message in L.lib().efg_last_error().decode()
    rc, gv, gl, ga = _abi_backward(value, shapes, start, loc, attn, gout, 7.0)
    assert rc != 0 and message in L.lib().efg_last_error().decode()
    assert bool((out == 7.0).all()) and bool((gl == 7.0).all()) and bool((ga == 7.0).all()) and bool((gv == 0).all())
