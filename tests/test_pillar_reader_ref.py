"""CPU: our PointPillars reader (efg_amd/modeling/readers/pillar_encoder.py), on its PyTorch-composition path, against the
REFERENCE's own module: tests/golden/pillar_reader.npz is produced by scripts/make_golden_pillars.py from
efg/modeling/readers/pillar_encoder.py imported in place -- training and eval mode, forward + backward from a fixed dy, the
running statistics after the step, the scattered canvas.  Tolerances: the project's kernel-golden ones, 1e-5 for forward outputs
and statistics, 1e-4 for gradients.  Also: a reference state dict loads with strict=True, the final `.squeeze()`, the
reference's import names."""
import numpy as np
import pytest
import torch

from conftest import golden

FWD_TOL, GRAD_TOL = 1e-5, 1e-4


def build(g, device):
    """(PillarFeatureNet, PointPillarsScatter) with the golden's weights, loaded by the REFERENCE's state-dict names."""
    from efg_amd.modeling.readers import PillarFeatureNet, PointPillarsScatter

    f = g["in::voxels"].shape[2]
    net = PillarFeatureNet(num_input_features=f, num_filters=(64,), with_distance=False,
                           voxel_size=tuple(g["voxel_size"].tolist()), pc_range=tuple(g["pc_range"].tolist()), norm="BN1d")
    state = {"pfn_layers.0.linear.weight": g["in::weight"], "pfn_layers.0.norm.weight": g["in::gamma"],
             "pfn_layers.0.norm.bias": g["in::beta"], "pfn_layers.0.norm.running_mean": g["in::running_mean"],
             "pfn_layers.0.norm.running_var": g["in::running_var"],
             "pfn_layers.0.norm.num_batches_tracked": np.array(0, np.int64)}
    assert sorted(state) == [str(k) for k in g["state_keys"]] == sorted(net.state_dict())     # the reference module's own names
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return net.to(device), PointPillarsScatter(num_input_features=64)


def close(name, got, want, tol):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want, rtol=tol, atol=tol, err_msg=name)


def check_against_golden(g, device, expect_fused):
    t = {k[4:]: torch.from_numpy(v).to(device) for k, v in g.items() if k.startswith("in::")}
    grid, batch = g["grid"].tolist(), int(g["batch_size"])
    for mode in ("train", "eval"):
        net, scatter = build(g, device)
        net.train(mode == "train")
        assert net.usable(t["voxels"]) == expect_fused
        out = net(t["voxels"], t["num_points"], t["coors"])
        out.backward(t["dy"])
        layer = net.pfn_layers[0]
        close(mode + " out", out, g[mode + "::out"], FWD_TOL)
        for k, p in (("dweight", layer.linear.weight), ("dgamma", layer.norm.weight), ("dbeta", layer.norm.bias)):
            close("%s %s" % (mode, k), p.grad, g["%s::%s" % (mode, k)], GRAD_TOL)
        if mode == "train":
            close("running_mean", layer.norm.running_mean, g["train::running_mean"], FWD_TOL)
            close("running_var", layer.norm.running_var, g["train::running_var"], FWD_TOL)
            assert int(layer.norm.num_batches_tracked) == int(g["train::num_batches_tracked"]) == 1
            canvas = scatter(out.detach(), t["coors"], batch, grid)
            assert tuple(canvas.shape) == g["train::canvas"].shape == (batch, 64, grid[1], grid[0])
            close("canvas", canvas, g["train::canvas"], FWD_TOL)
            # the canvas holds the features themselves: a copy, so a transposed or shifted scatter cannot hide in a tolerance
            rows = canvas.permute(0, 2, 3, 1)[t["coors"][:, 0].long(), t["coors"][:, 2].long(), t["coors"][:, 3].long()]
            assert torch.equal(rows, out.detach()) and int((canvas != 0).sum()) == int((out != 0).sum())
        else:
            assert torch.equal(layer.norm.running_mean.cpu(), torch.from_numpy(g["in::running_mean"]))
            assert int(layer.norm.num_batches_tracked) == 0


def test_composition_against_the_reference_golden():
    check_against_golden(golden("pillar_reader.npz"), torch.device("cpu"), expect_fused=False)


def test_state_dict_names_are_the_reference_ones():
    from efg_amd.modeling.readers import PillarFeatureNet

    net = PillarFeatureNet(num_input_features=5, num_filters=(32, 64), with_distance=True)
    names = set(net.state_dict())
    for i, (cin, units) in enumerate(((11, 16), (32, 64))):
        assert tuple(net.state_dict()["pfn_layers.%d.linear.weight" % i].shape) == (units, cin)
        for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            assert "pfn_layers.%d.norm.%s" % (i, k) in names
    assert len(names) == 12 and not any(k.endswith("linear.bias") for k in names)
    assert net.x_offset == 0.2 / 2 + 0 and net.y_offset == 0.2 / 2 - 40


def test_squeeze_and_two_layer_shapes():
    from efg_amd.modeling.readers import PillarFeatureNet

    torch.manual_seed(0)
    net = PillarFeatureNet(num_input_features=4, num_filters=(64,)).eval()
    coors = torch.tensor([[0, 0, 1, 2], [0, 0, 3, 1], [1, 0, 0, 0]], dtype=torch.int32)
    voxels, counts = torch.rand(3, 6, 4), torch.tensor([6, 2, 1], dtype=torch.int32)
    assert tuple(net(voxels, counts, coors).shape) == (3, 64)
    assert tuple(net(voxels[:1], counts[:1], coors[:1]).shape) == (64,)        # the reference's final .squeeze()
    two = PillarFeatureNet(num_input_features=4, num_filters=(32, 64)).eval()
    assert tuple(two(voxels, counts, coors).shape) == (3, 64)
    # a padded row is zero after decoration whatever it holds
    dirty = voxels.clone()
    dirty[1, 2:] = 1e6
    dirty[2, 1:, 3:] = float("inf")
    clean = voxels.clone()
    clean[1, 2:, 3:] = 0
    clean[1, 2:, :3] = 1e6                          # xyz of padded rows enter the cluster mean, as in the reference
    clean[2, 1:, 3:] = 0
    assert torch.equal(net.decorate(dirty, counts, coors), net.decorate(clean, counts, coors))
    assert bool((net.decorate(dirty, counts, coors)[1, 2:] == 0).all())


def test_reference_import_names():
    from efg_amd import compat

    compat.install()
    from efg.modeling.readers import PillarFeatureNet as ByPackage
    from efg.modeling.readers.pillar_encoder import PFNLayer, PillarFeatureNet, PointPillarsScatter

    import efg_amd.modeling.readers as ours

    assert PillarFeatureNet is ours.PillarFeatureNet is ByPackage and PFNLayer is ours.PFNLayer
    assert PointPillarsScatter is ours.PointPillarsScatter


def test_operators_refuse_cpu_tensors():
    from efg_amd.operators.pillars import pillar_features, pillar_scatter

    bn = torch.nn.BatchNorm1d(64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pillar_features(torch.rand(2, 4, 4), torch.ones(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32),
                        torch.rand(64, 9), bn, 0.2, 0.2, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pillar_scatter(torch.rand(2, 64), torch.zeros(2, 4, dtype=torch.int32), 1, 4, 4)
