"""GPU: the BEV scatter kernel and its gather (bit-exact copies), P = 0, an empty scene, bit-reproducibility of the fused reader,
the composition fall-back for what the fused layer does not cover, and the limits that raise before anything is launched."""
import pytest
import torch

import pillar_fp64_cases as C

pytestmark = pytest.mark.gpu


def _scatter_case(dev, coors, batch, nx, ny, channels=64, seed=0):
    from efg_amd.modeling.readers import PointPillarsScatter

    gen = torch.Generator().manual_seed(seed)
    coors = torch.tensor(coors, dtype=torch.int32).reshape(-1, 4).to(dev)
    feats = torch.randn(coors.shape[0], channels, generator=gen).to(dev)
    dcanvas = torch.randn(batch, channels, ny, nx, generator=gen).to(dev)
    mod = PointPillarsScatter(num_input_features=channels)
    a, b = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    got = mod(a, coors, batch, [nx, ny])
    want = mod.forward_composition(b, coors, batch, [nx, ny])
    assert tuple(got.shape) == tuple(want.shape) == (batch, channels, ny, nx)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got, want), "the scatter is a copy"
    got.backward(dcanvas)
    want.backward(dcanvas)
    assert torch.equal(a.grad, b.grad), "the gather is a copy"
    return got


def test_scatter_corners_of_an_oblong_grid(dev):
    nx, ny = 12, 8
    coors = [[0, 0, 0, 0], [0, 0, ny - 1, nx - 1], [1, 0, 0, nx - 1], [1, 0, ny - 1, 0], [1, 0, 3, 7], [0, 0, 7, 3], [0, 0, 3, 7]]
    got = _scatter_case(dev, coors, 2, nx, ny)
    assert int((got != 0).any(1).sum()) == len(coors)


def test_scatter_empty_middle_scene_other_widths_and_many_pillars(dev):
    nx, ny = 5, 9
    got = _scatter_case(dev, [[0, 0, 1, 1], [0, 0, 8, 4], [2, 0, 0, 0], [2, 0, 8, 0], [2, 0, 4, 4]], 3, nx, ny)
    assert not bool(got[1].any()) and bool(got[0].any()) and bool(got[2].any())
    _scatter_case(dev, [[0, 0, 2, 3], [0, 0, 0, 4]], 1, nx, ny, channels=40)          # C not a multiple of 64
    _scatter_case(dev, [[0, 0, 2, 3], [0, 0, 0, 4]], 1, nx, ny, channels=130)
    cells = torch.randperm(2 * 120 * 100, generator=torch.Generator().manual_seed(1))[:9001]     # more pillars than grid waves
    coors = torch.stack([cells // 12000, torch.zeros_like(cells), (cells % 12000) // 100, cells % 100], 1).tolist()
    _scatter_case(dev, coors, 2, 100, 120)


def test_no_pillars_at_all(dev):
    from efg_amd.modeling.readers import PillarFeatureNet, PointPillarsScatter
    from efg_amd.operators.pillars import pillar_features

    net = PillarFeatureNet(num_input_features=5, num_filters=(64,)).to(dev).train()
    voxels = torch.zeros(0, 20, 5, device=dev)
    counts, coors = torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, 4, dtype=torch.int32, device=dev)
    assert net.usable(voxels)
    out = net(voxels, counts, coors)
    assert tuple(out.shape) == (0, 64)
    layer = net.pfn_layers[0]
    out2, index = pillar_features(voxels, counts, coors, layer.linear.weight, layer.norm, 0.2, 0.2, 0.1, 0.1, return_index=True)
    assert tuple(index.shape) == (0, 64) and index.dtype == torch.uint8
    out2.sum().backward()
    assert not bool(layer.linear.weight.grad.any()) and int(layer.norm.num_batches_tracked) == 0
    canvas = PointPillarsScatter()(out, coors, 2, [6, 4])
    assert tuple(canvas.shape) == (2, 64, 4, 6) and not bool(canvas.any())


def test_two_runs_agree_in_every_bit(dev):
    """Forward + backward of the largest case twice -- and of a 3001-pillar batch that fills more than one workgroup per
    segment of the finishing launches -- : outputs, index, statistics and gradients are equal, not close."""
    from test_pillar_fp64_gpu import run_fused

    family, n, f, with_distance = "plain", 32, 6, True
    case = C.make_case(family, n, f, with_distance)
    a, b = run_fused(case, dev), run_fused(case, dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    big = dict(case)
    reps = 231                                                     # 13 * 231 = 3003 pillars, 751 tiles
    big["voxels"] = case["voxels"].repeat(reps, 1, 1) + 0.001 * torch.arange(13 * reps).view(-1, 1, 1) * (case["voxels"].repeat(reps, 1, 1) != 0)
    big["num_points"], big["coors"] = case["num_points"].repeat(reps), case["coors"].repeat(reps, 1)
    big["dy"] = torch.randn(13 * reps, 64, generator=torch.Generator().manual_seed(5))
    a, b = run_fused(big, dev), run_fused(big, dev)
    for k in a:
        assert torch.equal(a[k], b[k]), "3003 pillars: " + k
    assert bool(torch.isfinite(a["dweight"]).all()) and bool(a["dweight"].any())


def _two_sides(dev, net_args, voxels, counts, coors, dy):
    """The same module and weights on the GPU and on the CPU: (out, grads) of both."""
    import copy

    from efg_amd.modeling.readers import PillarFeatureNet

    torch.manual_seed(3)
    cpu = PillarFeatureNet(**net_args).train()
    for m in cpu.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.3)
    gpu = copy.deepcopy(cpu).to(dev)
    res = []
    for net, d in ((gpu, dev), (cpu, torch.device("cpu"))):
        out = net(voxels.to(d), counts.to(d), coors.to(d))
        out.backward(dy.to(d))
        res.append((out.detach().cpu(), {k: p.grad.cpu() for k, p in net.named_parameters()},
                    {k: b.cpu() for k, b in net.named_buffers()}))
    return gpu, res


def test_two_layer_net_takes_the_composition_and_matches_the_cpu(dev):
    case = C.make_case("plain", 20, 5, False)
    args = dict(num_input_features=5, num_filters=(32, 64), voxel_size=(0.5, 0.5, 4.0), pc_range=(-4.0, -4.0, -3.0, 4.0, 4.0, 1.0))
    gpu, (g, c) = _two_sides(dev, args, case["voxels"], case["num_points"], case["coors"], case["dy"])
    assert not gpu.usable(case["voxels"].to(dev))
    assert float((g[0] - c[0]).abs().max()) <= 1e-4 * max(1.0, float(c[0].abs().max()))
    for k in c[1]:
        scale = max(float(c[1][k].abs().max()), 1e-6)
        assert float((g[1][k] - c[1][k]).abs().max()) <= 1e-3 * scale, k
    for k in c[2]:
        assert float((g[2][k].double() - c[2][k].double()).abs().max()) <= 1e-4 * max(1.0, float(c[2][k].double().abs().max())), k


def test_what_the_fused_layer_does_not_cover_falls_back_or_raises(dev):
    from efg_amd.modeling.readers import PillarFeatureNet
    from efg_amd.operators.pillars import pillar_features, pillar_scatter, usable

    bn = torch.nn.BatchNorm1d(64).to(dev)
    w = torch.rand(64, 10, device=dev)
    ok = torch.rand(4, 20, 5, device=dev)
    counts, coors = torch.ones(4, dtype=torch.int32, device=dev), torch.zeros(4, 4, dtype=torch.int32, device=dev)
    assert usable(ok, w, bn) and not usable(ok, w, bn, with_distance=True)
    assert not usable(torch.rand(4, 65, 5, device=dev), w, bn)                          # N > 64
    assert not usable(torch.rand(4, 20, 12, device=dev), torch.rand(64, 17, device=dev), bn)   # Cin > 16
    assert not usable(ok, torch.rand(32, 10, device=dev), torch.nn.BatchNorm1d(32).to(dev))     # not 64 channels
    assert not usable(ok.double(), w.double(), bn) and not usable(ok.cpu(), w.cpu(), torch.nn.BatchNorm1d(64))
    assert not usable(ok, w, torch.nn.BatchNorm1d(64, momentum=None).to(dev))
    assert not usable(ok, w, torch.nn.BatchNorm1d(64, affine=False).to(dev))
    with pytest.raises(ValueError, match="N = 65"):
        pillar_features(torch.rand(4, 65, 5, device=dev), counts, coors, w, bn, 0.2, 0.2, 0.1, 0.1)
    with pytest.raises(ValueError, match="Cin = 17"):
        pillar_features(torch.rand(4, 20, 12, device=dev), counts, coors, torch.rand(64, 17, device=dev), bn, 0.2, 0.2, 0.1, 0.1)
    with pytest.raises(ValueError, match="Linear"):
        pillar_features(ok, counts, coors, torch.rand(32, 10, device=dev), bn, 0.2, 0.2, 0.1, 0.1)
    with pytest.raises(ValueError, match="coors"):
        pillar_scatter(torch.rand(4, 64, device=dev), coors[:3], 1, 4, 4)
    # a 65-row batch still runs: through the composition
    net = PillarFeatureNet(num_input_features=5).to(dev).train()
    wide = torch.rand(4, 65, 5, device=dev)
    assert not net.usable(wide) and tuple(net(wide, counts, coors).shape) == (4, 64)
    # the C ABI refuses the same limits on its own
    from efg_amd import _lib as L

    rc = L.lib().efg_pillar_forward_f32(None, None, None, None, None, None, None, None, None, 0.1, 1e-5, 4, 65, 5, 0, 64, 0.2, 0.2,
                                        0.1, 0.1, 1, None, None, None, None, None, 0, 0, None)
    assert rc == -1 and b"N = 65" in L.lib().efg_last_error()
