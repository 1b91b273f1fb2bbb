"""CPU pins of tests/fp64_ref.py, the float64 references of the full-size GPU tests: the hand-written sampling against the
reference's own `ms_deform_attn_core_pytorch` results (tests/golden/msda_*.npz) and against autograd through float64
grid_sample, the independent rulebook + products against dense float64 conv3d for every geometry of
tests/test_spconv_dense_gpu.py, and the element-wise error bar itself."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden
from fp64_ref import (assert_elementwise, box_attention_fp64, independent_rulebook, near_cell_boundary, sample_fp64,
                      spconv_fp64)
from test_spconv_dense_gpu import GEOMS, _dense_reference, _random_sparse

MSDA_CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "msda_*.npz")))


@pytest.mark.parametrize("case", MSDA_CASES)
def test_sampling_reproduces_the_reference_core(case):
    g = golden(case)
    t = {k: torch.from_numpy(g[k]) for k in ("value", "shapes", "level_start", "loc", "attn", "grad_out")}
    r = sample_fp64(t["value"].double(), t["shapes"], t["level_start"], t["loc"].double(), t["attn"].double(),
                    t["grad_out"].double())
    for key, want in (("out", "out_fp64"), ("grad_value", "grad_value"), ("grad_loc", "grad_loc"), ("grad_attn", "grad_attn")):
        w = g[want].astype(np.float64)
        got = r[key].numpy()
        assert got.shape == w.shape, (key, got.shape, w.shape)
        np.testing.assert_allclose(got, w, rtol=1e-9, atol=1e-12 * max(float(np.abs(w).max()), 1.0), err_msg=key)
        assert bool((r[key].abs() <= r[key + "_mag"] * (1 + 1e-12) + 1e-300).all()), key + ": magnitude below |value|"


def _box_case(rot, gen, hm=11, wm=13, q=40, h=2, d=4, k=5):
    nvar = 5 if rot else 4
    axis = (torch.arange(k, dtype=torch.float64) - (k - 1) / 2) / k
    kidx = torch.stack((axis.repeat(k), axis.repeat_interleave(k)), dim=-1)
    ref = torch.rand(2, q, 7, generator=gen, dtype=torch.float64)
    ref[..., 3:5] = ref[..., 3:5] * 0.6 + 0.05          # some boxes reach past the map edge
    value = torch.randn(2, hm * wm, h, d, generator=gen, dtype=torch.float64)
    offsets = torch.randn(2, q, h * nvar, generator=gen, dtype=torch.float64) * 0.5
    logits = torch.randn(2, q, h * k * k, generator=gen, dtype=torch.float64)
    gout = torch.randn(2, q, h * d, generator=gen, dtype=torch.float64)
    return kidx, ref, value, offsets, logits, gout, nvar


@pytest.mark.parametrize("rot", [False, True])
def test_box_attention_equals_autograd_through_grid_sample(rot):
    """The whole op (geometry, softmax, hand-written sampling + its hand-written backward, magnitudes carried back through
    the geometry by forward-mode Jacobians) against float64 autograd through F.grid_sample(align_corners=False)."""
    from efg_amd.operators.box_attention_func import box_sampling_grid

    gen = torch.Generator().manual_seed(7 + rot)
    kidx, ref, value, offsets, logits, gout, nvar = _box_case(rot, gen)
    hm, wm, h, d = 11, 13, value.shape[2], value.shape[3]
    shapes, start = torch.tensor([[hm, wm]]), torch.zeros(1, dtype=torch.int64)
    r = box_attention_fp64(value, shapes, start, ref, offsets, logits, kidx, nvar, gout, chunk=16)

    v, o, lg = (t.clone().requires_grad_(True) for t in (value, offsets, logits))
    grid = box_sampling_grid(ref, o, kidx, h, 1, rot)[:, :, :, 0]                          # [B, Q, H, P, 2]
    attn = torch.softmax(lg.view(2, -1, h, 25), -1)
    vm = v.permute(0, 2, 3, 1).reshape(2 * h, d, hm, wm)
    gs = F.grid_sample(vm, (grid * 2 - 1).permute(0, 2, 1, 3, 4).reshape(2 * h, -1, 25, 2), mode="bilinear",
                       padding_mode="zeros", align_corners=False)                          # [B*H, D, Q, P]
    out = (gs.view(2, h, d, -1, 25) * attn.permute(0, 2, 1, 3).unsqueeze(2)).sum(-1)       # [B, H, D, Q]
    out = out.permute(0, 3, 1, 2).reshape(2, -1, h * d)
    out.backward(gout)
    px, py = r["px"], r["py"]
    assert not bool(near_cell_boundary(px, py, 1e-9).any())   # (one-sided derivatives would be a convention)
    for key, want in (("out", out), ("grad_value", v.grad), ("grad_offsets", o.grad), ("grad_logits", lg.grad)):
        w = want.detach()
        np.testing.assert_allclose(r[key].numpy(), w.numpy(), rtol=1e-9, atol=1e-12 * float(w.abs().max()), err_msg=key)
        assert bool((r[key].abs() <= r[key + "_mag"] * (1 + 1e-9) + 1e-300).all()), key + ": magnitude below |value|"
    assert float(r["out_geo"].max()) > 0 and float(r["grad_offsets_geo"].max()) > 0


@pytest.mark.parametrize("geom", list(GEOMS))
def test_rulebook_and_products_equal_dense_conv3d(geom):
    """independent_rulebook + spconv_fp64 == float64 F.conv3d on the densified tensor (sites, row order, forward, both
    gradients) for every geometry the GPU dense test covers."""
    ks, st, pd, subm = GEOMS[geom]
    rng = np.random.default_rng(len(geom))
    batch, shape, cin, cout = 2, (9, 20, 22), 12, 8
    idx, feat = _random_sparse(rng, batch, shape, 1800, cin)
    w5 = (rng.standard_normal((cout, *ks, cin)) / np.sqrt(cin * np.prod(ks))).astype(np.float32)
    o_idx, o_feat, gin, gw, go, oshape = _dense_reference(
        idx, feat, w5, None, batch, shape, ks, st, pd, subm,
        lambda s: np.random.default_rng(1).standard_normal(s).astype(np.float32))
    out_idx, out_shape, pairs = independent_rulebook(torch.from_numpy(idx), list(shape), ks, st, pd, subm)
    assert out_shape == (list(shape) if subm else oshape)
    assert np.array_equal(out_idx.numpy(), o_idx)
    r = spconv_fp64(torch.from_numpy(feat), torch.from_numpy(w5), torch.from_numpy(go), pairs, len(out_idx))
    for key, want in (("y", o_feat), ("dx", gin), ("dw", gw.reshape(cout, -1, cin))):
        np.testing.assert_allclose(r[key].numpy(), want, rtol=1e-10, atol=1e-12, err_msg=key)
        assert bool((r[key].abs() <= r[key + "_mag"] * (1 + 1e-12)).all()), key
    assert int(r["n_dw"].sum()) == sum(len(i) for i, _ in pairs) > 0


def test_error_bar_holds_fp32_and_catches_a_small_wrong_element():
    """An fp32 matrix product passes at c = 1; one element of 1e-7 of the tensor's largest with the wrong sign fails,
    though it is far below any bar relative to the tensor max."""
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(64, 300, generator=gen)
    b = torch.randn(300, 48, generator=gen)
    a[0] *= 1e-7   # row 0 of the product is tiny
    ref = a.double() @ b.double()
    mag = a.double().abs() @ b.double().abs()
    got = a @ b
    assert assert_elementwise("fp32 matmul", got, ref, mag, 300, 1) < 1
    bad = got.clone()
    bad[0, 5] = -bad[0, 5]
    assert float((bad.double() - ref).abs().max()) < 1e-6 * float(ref.abs().max())
    with pytest.raises(AssertionError, match=r"worst at \(0, 5\)"):
        assert_elementwise("sign flip", bad, ref, mag, 300, 16)
