"""GPU: the sparse convolution (csrc/spconv_tiles.hip, spconv_wgt.hip) against the float64 reference of tests/fp64_ref.py,
which shares nothing with it (rulebook from torch.sort / searchsorted, products as float64 matmuls), at full scene size:
two 180k-point scenes voxelized as the trainer does, every distinct (kernel, stride, padding, cin, cout) of the ConQueR
res18 backbone and of CenterPoint's SpMiddleResNetFHD at the level the model runs it.  Output sites bit-exact; forward,
data gradient and weight gradient element by element within c * sqrt(n) * 2^-24 * sum |terms|.  Also: the main +
shortcut pair launches, and a child process with stream-K on every eligible shape (EFG_TILE_STREAMK=2)."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from fp64_ref import assert_elementwise, independent_rulebook, spconv_fp64

pytestmark = pytest.mark.gpu

K3, S1, S2, P1 = (3, 3, 3), (1, 1, 1), (2, 2, 2), (1, 1, 1)
ZK, ZS = (3, 1, 1), (2, 1, 1)                    # the z-collapsing heads
# Levels: 0 = the voxel grid [41, 1504, 1504] of two scenes; 1..4 = the k3 s2 p1 chain (res18 stem conv and stage
# downsamplings; SpMiddleResNetFHD conv2 / conv3 are the same geometry); "3c" = CenterPoint's conv4, k3 s2 p(0, 1, 1)
# from level 2.  (sparse_net.py: SparseBasicStem, SparseBasicResBlock, SparseResNet, SparseBasicBlock, SpMiddleResNetFHD;
# configs: res18 stem width 16, stem_out 32, res1_out 64 -> 64 / 128 / 256, 5 voxel features.)  A tuple both models run
# at different levels is listed once.
# (name, level, kernel, stride, padding, subm, cin, cout)
CASES = [
    ("res18 stem conv 5-16", 0, K3, S2, P1, False, 5, 16),
    ("res18 stem subm 16-32", 1, K3, S1, P1, True, 16, 32),
    ("res18 res2 down 32-64 (= fhd conv3 down)", 1, K3, S2, P1, False, 32, 64),
    ("res18 res2 subm 64-64 (= fhd conv3 blocks)", 2, K3, S1, P1, True, 64, 64),
    ("res18 res3 down 64-128", 2, K3, S2, P1, False, 64, 128),
    ("res18 res3 subm 128-128 (fhd conv4 blocks: level 3c)", 3, K3, S1, P1, True, 128, 128),
    ("res18 res4 down 128-256", 3, K3, S2, P1, False, 128, 256),
    ("res18 res4 subm 256-256", 4, K3, S1, P1, True, 256, 256),
    ("res18 res2_out 64-64", 2, ZK, ZS, (1, 0, 0), False, 64, 64),
    ("res18 res3_out 128-128", 3, ZK, ZS, (1, 0, 0), False, 128, 128),
    ("res18 res4_out 256-256", 4, ZK, ZS, (1, 0, 0), False, 256, 256),
    ("fhd conv_input 5-16", 0, K3, S1, P1, True, 5, 16),
    ("fhd conv1 subm 16-16 (res18 stem: level 1)", 0, K3, S1, P1, True, 16, 16),
    ("fhd conv2 down 16-32", 0, K3, S2, P1, False, 16, 32),
    ("fhd conv2 subm 32-32", 1, K3, S1, P1, True, 32, 32),
    ("fhd conv4 down 64-128", 2, K3, S2, (0, 1, 1), False, 64, 128),
    ("fhd extra_conv 128-128", "3c", ZK, ZS, (0, 0, 0), False, 128, 128),
]
NAMES = [c[0] for c in CASES]
# rounding constants c of assert_elementwise.  Largest err / bound measured on MI355X with these constants: forward 0.43
# (conv_small_kernel on the 5 raw voxel features), data gradient 0.23, weight gradient 0.012
C_FWD, C_DGRAD, C_WGRAD = 4, 4, 2


def _levels(dev):
    from efg_amd.data.synthetic import PC_RANGE, VOXEL_SIZE, make_scene
    from efg_amd.operators import voxelize_batch

    pts = [torch.from_numpy(make_scene(2000 + i, n_points=180000)[0]).to(dev) for i in range(2)]
    vox = voxelize_batch(pts, VOXEL_SIZE, PC_RANGE, 5, 120000)
    lv = {0: (vox["coordinates"].int().contiguous(), [41, 1504, 1504], vox["voxel_mean"].float().contiguous())}
    for i in range(1, 5):
        idx, shp, _ = independent_rulebook(lv[i - 1][0], lv[i - 1][1], K3, S2, P1, False)
        lv[i] = (idx, shp, None)
    idx, shp, _ = independent_rulebook(lv[2][0], lv[2][1], K3, S2, (0, 1, 1), False)
    lv["3c"] = (idx, shp, None)
    return lv


@pytest.fixture(scope="module")
def levels(dev):
    lv = _levels(dev)
    rows = [lv[i][0].shape[0] for i in range(5)]
    assert rows[1] > 100000 and rows[0] > rows[1], rows   # the ~117k-row levels of a real scene pair
    return lv


def _check_case(dev, lv, name, expect_streamk=False):
    """One layer shape: HIP forward + backward against spconv_fp64 over independent_rulebook; returns the ratios."""
    import efg_amd.spconv as spconv
    from efg_amd.spconv import core

    _, level, ks, st, pd, subm, cin, cout = CASES[NAMES.index(name)]
    idx, shape, feat0 = lv[level]
    torch.manual_seed(cin * 1000 + cout + len(name))
    conv = (spconv.SubMConv3d(cin, cout, ks, padding=pd, bias=False, indice_key="k") if subm else
            spconv.SparseConv3d(cin, cout, ks, st, padding=pd, bias=False)).to(dev)
    feat = feat0 if feat0 is not None and feat0.shape[1] == cin else torch.randn(idx.shape[0], cin, device=dev)
    x = spconv.SparseConvTensor(feat.clone().requires_grad_(True), idx, list(shape), 2)
    y = conv(x)
    go = torch.randn(y.features.shape, device=dev)
    y.features.backward(go)
    torch.cuda.synchronize()
    rb = conv._rulebook(x)[0]
    out_idx, out_shape, pairs = independent_rulebook(idx, shape, ks, st, pd, subm)
    assert list(y.spatial_shape) == out_shape
    assert torch.equal(y.indices, out_idx), "%s: output sites / row order differ from the independent rulebook" % name
    ref = spconv_fp64(feat, conv.weight, go, pairs, out_idx.shape[0])
    kvol = math.prod(ks)
    ratios = {
        "fwd": assert_elementwise(name + " forward", y.features, ref["y"], ref["y_mag"], ref["n_y"], C_FWD),
        "dgrad": assert_elementwise(name + " dgrad", x.features.grad, ref["dx"], ref["dx_mag"], ref["n_dx"], C_DGRAD),
        "wgrad": assert_elementwise(name + " wgrad", conv.weight.grad.reshape(cout, kvol, cin), ref["dw"], ref["dw_mag"],
                                    ref["n_dw"], C_WGRAD),
    }
    # the path that ran: the forward kernel the library picks for this shape, the plan-walking wgrad where it applies
    fwd_kernel = core._tile_kernel_name(cin, cout, kvol, rb.m_in, rb.m_out)
    tiled_wgrad = (cin, cout) in rb._wgrad_sched
    assert tiled_wgrad == core._wgrad_tiled(cin, cout, kvol, rb.m_out, rb.m_in)
    if expect_streamk:   # EFG_TILE_STREAMK=2: stream-K takes every launch with 4 n-tiles per wave and split-K over 4 waves
        assert fwd_kernel == "conv_tile_kernel<4>" and kvol >= 8, (name, fwd_kernel)
    print("%-52s rows %7d -> %7d  %-24s wgrad %-5s  err/bound fwd %.3g dgrad %.3g wgrad %.3g" % (
        name, rb.m_in, rb.m_out, fwd_kernel, "tiled" if tiled_wgrad else "table", ratios["fwd"], ratios["dgrad"],
        ratios["wgrad"]))
    return fwd_kernel, tiled_wgrad, ratios


# the forward kernel the library runs for each shape (asserted, so a change of dispatch is noticed); the weight gradient
# of every shape here is the plan-walking kernel (spconv_wgt.hip)
SMALL = ("res18 stem conv 5-16", "res18 stem subm 16-32", "fhd conv_input 5-16", "fhd conv1 subm 16-16 (res18 stem: level 1)",
         "fhd conv2 down 16-32")


@pytest.mark.parametrize("name", NAMES)
def test_layer_against_fp64(dev, levels, name):
    fwd_kernel, tiled_wgrad, _ = _check_case(dev, levels, name)
    want = ("conv_small_kernel" if name in SMALL else
            "conv_tile_kernel<2>" if name == "fhd conv2 subm 32-32" else "conv_tile_kernel<4>")
    assert fwd_kernel.startswith(want) and tiled_wgrad, (name, fwd_kernel, tiled_wgrad)


def test_main_and_shortcut_pair_against_fp64(dev, levels):
    """res18 res2's first block: the strided main and shortcut convolutions over ONE rulebook through the convolution
    nodes of spconv.conv_pair_bn_act -- both products in one launch, the joint data gradient (the two gradients summed
    inside the kernel), both weight gradients in one launch + fold."""
    import efg_amd.spconv as spconv
    from efg_amd.spconv import core

    idx, shape, _ = levels[1]
    cin, cout = 32, 64
    torch.manual_seed(5)
    conv_a = spconv.SparseConv3d(cin, cout, 3, 2, padding=1, bias=False).to(dev)
    conv_b = spconv.SparseConv3d(cin, cout, 3, 2, padding=1, bias=False).to(dev)
    feat = torch.randn(idx.shape[0], cin, device=dev)
    x = spconv.SparseConvTensor(feat, idx, list(shape), 2)
    rb, geom = conv_a._rulebook(x)
    wa = conv_a.weight.detach().reshape(cout, rb.kvol, cin).contiguous()
    wb = conv_b.weight.detach().reshape(cout, rb.kvol, cin).contiguous()
    assert core._pair_ok(rb, wa, wb, cin, cout) and core._wgrad_tiled(cin, cout, rb.kvol, rb.m_out, rb.m_in)
    ya, yb = core._conv_forward_pair(feat, wa, wb, rb, conv_a.weight, conv_b.weight)
    go_a, go_b = torch.randn_like(ya), torch.randn_like(yb)
    dx = core._conv_dgrad_pair(go_a, go_b, wa, wb, rb, conv_a.weight, conv_b.weight)
    rb.prepare_wgrad(cin, cout)
    gwa, gwb = core._conv_wgrad_pair(feat, go_a, go_b, rb)
    torch.cuda.synchronize()
    out_idx, _, pairs = independent_rulebook(idx, shape, K3, S2, P1, False)
    assert torch.equal(geom[0], out_idx)
    ra = spconv_fp64(feat, wa, go_a, pairs, out_idx.shape[0])
    rbb = spconv_fp64(feat, wb, go_b, pairs, out_idx.shape[0])
    r = [assert_elementwise("pair forward a", ya, ra["y"], ra["y_mag"], ra["n_y"], C_FWD),
         assert_elementwise("pair forward b", yb, rbb["y"], rbb["y_mag"], rbb["n_y"], C_FWD),
         assert_elementwise("pair joint dgrad", dx, ra["dx"] + rbb["dx"], ra["dx_mag"] + rbb["dx_mag"],
                            ra["n_dx"] + rbb["n_dx"], C_DGRAD),
         assert_elementwise("pair wgrad a", gwa, ra["dw"], ra["dw_mag"], ra["n_dw"], C_WGRAD),
         assert_elementwise("pair wgrad b", gwb, rbb["dw"], rbb["dw_mag"], rbb["n_dw"], C_WGRAD)]
    print("pair 32-64: err/bound fwd a %.3g b %.3g, joint dgrad %.3g, wgrad a %.3g b %.3g" % tuple(r))


STREAMK_CASES = [c[0] for c in CASES if c[7] >= 64 and math.prod(c[2]) >= 8]

_CHILD = r"""
import sys, torch
sys.path[:0] = [%(root)r, %(tests)r]
import test_spconv_fp64_full_gpu as t
dev = torch.device("cuda:0")
lv = t._levels(dev)
for name in t.STREAMK_CASES:
    t._check_case(dev, lv, name, expect_streamk=True)
torch.cuda.synchronize()
print("CHILD_OK")
"""


def test_streamk_every_eligible_shape_against_fp64():
    """EFG_TILE_STREAMK=2 (the library reads it once, hence a child process): stream-K shares on every shape with
    64+ output channels and a 3x3x3 window, the strided ones included, against the same fp64 reference."""
    env = dict(os.environ, EFG_TILE_STREAMK="2", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert len(STREAMK_CASES) >= 6
