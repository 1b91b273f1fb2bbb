"""Inputs of the per-element float64 tests of the PointPillars reader (tests/test_pillar_fp64_ref.py on the CPU,
tests/test_pillar_fp64_gpu.py on the GPU): CPU generators with fixed seeds, so both see the same numbers.

Shapes: P = 3 x 4 + 1 pillars (the kernels' workgroup takes 4 pillars: three full tiles, then a tail tile with one wave busy),
N in {20, 32}, F in {4, 5, 6} with and without the distance column (Cin = 9 .. 12), two scenes, counts 1, 2, N - 1, N first
and random ones after.  Families:
    plain            points uniform inside their pillar, a 16 x 16 grid of 0.5 m pillars around the origin
    offset           the cloud centred at (70, -60, 1), 0.1 m spread inside a pillar
    scales           plain, every weight row times its own log-uniform factor in [1e-3, 1e3]
    padded-wins      channels 0..15: relu(bn(0)) of a padded row beats every real row; channels 16..31: every value is 0
    garbage-padding  plain, rows >= count filled with 1e6 (they move the cluster mean, which the reference sums over ALL
                     rows, and nothing else: they are zero after decoration)
    duplicates       every third pillar holds one point count times: the lowest row wins
A case is a condition on the INPUTS: none of its selected pre-ReLU values may be a ReLU tie (within 16 x its own bar of
zero, in float64).  `make_case` takes the first seed that meets it; the CPU test asserts it and prints the seed."""
import math

import torch

from pillar_fp64_ref import pillar_fp64

FAMILIES = ("plain", "offset", "scales", "padded-wins", "garbage-padding", "duplicates")
TILE = 4                       # pillars per workgroup (csrc/pillars.hip)
P = 3 * TILE + 1
ROWS = (20, 32)
FEATURES = ((4, False), (4, True), (5, False), (5, True), (6, False), (6, True))
CHANNELS = 64
GRID = 16
VOXEL = 0.5
MOMENTUM, EPS = 0.1, 1e-3
_CACHE = {}


def cases():
    """(family, n, f, with_distance): every family at every feature layout, the two N in turn."""
    out = []
    for fi, family in enumerate(FAMILIES):
        for li, (f, dist) in enumerate(FEATURES):
            out.append((family, ROWS[(fi + li) % 2], f, dist))
    return out


def _generate(family, n, f, with_distance, seed):
    gen = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=gen)      # noqa: E731
    randn = lambda *s: torch.randn(*s, generator=gen)    # noqa: E731
    origin = (66.0, -64.0, -1.0) if family == "offset" else (-4.0, -4.0, -3.0)
    cells = torch.randperm(2 * GRID * GRID, generator=gen)[:P].sort().values
    b, rest = cells // (GRID * GRID), cells % (GRID * GRID)
    coors = torch.stack([b, torch.zeros_like(b), rest // GRID, rest % GRID], 1).int()
    counts = torch.tensor([1, 2, n - 1, n] + [int(v) for v in torch.randint(1, n + 1, (P - 4,), generator=gen)], dtype=torch.int32)
    cx = origin[0] + (coors[:, 3].float() + 0.5) * VOXEL
    cy = origin[1] + (coors[:, 2].float() + 0.5) * VOXEL
    voxels = torch.zeros(P, n, f)
    if family == "offset":
        spread = (0.1 * randn(P, n, 2)).clamp(-0.24, 0.24)
    else:
        spread = (rand(P, n, 2) - 0.5) * VOXEL * 0.98
    voxels[:, :, 0] = cx.view(P, 1) + spread[:, :, 0]
    voxels[:, :, 1] = cy.view(P, 1) + spread[:, :, 1]
    voxels[:, :, 2] = origin[2] + 4.0 * rand(P, n)
    voxels[:, :, 3:] = 0.2 + 0.8 * rand(P, n, f - 3)
    if family == "duplicates":
        voxels[::3] = voxels[::3, :1].expand(-1, n, -1)
    real = torch.arange(n).view(1, n) < counts.view(P, 1)
    voxels = torch.where(real.unsqueeze(-1), voxels, torch.full((), 1e6 if family == "garbage-padding" else 0.0))
    cin = f + 5 + (1 if with_distance else 0)
    weight = 0.5 * randn(CHANNELS, cin)
    gamma, beta = 0.5 + rand(CHANNELS), 0.3 * randn(CHANNELS)
    if family == "scales":
        factor = torch.exp(torch.empty(CHANNELS, 1, dtype=torch.float64).uniform_(math.log(1e-3), math.log(1e3), generator=gen))
        weight = (weight * factor).float()
    if family == "padded-wins":
        weight[:16] = 0.0
        weight[:16, 3] = 0.5 + rand(16)        # x > 0 for every real row, 0 for a padded one ...
        gamma[:16] = -(0.5 + rand(16))         # ... and z falls with x: the padded row is the largest
        beta[:16] = 1.0
        beta[16:32] = -10.0                    # every z < 0: the whole channel is 0 after the ReLU
    return dict(family=family, seed=seed, n=n, f=f, with_distance=with_distance, voxels=voxels, num_points=counts, coors=coors,
                weight=weight, gamma=gamma, beta=beta, running_mean=0.1 * randn(CHANNELS), running_var=0.5 + rand(CHANNELS),
                dy=randn(P, CHANNELS), vx=VOXEL, vy=VOXEL, x_offset=VOXEL / 2 + origin[0], y_offset=VOXEL / 2 + origin[1],
                momentum=MOMENTUM, eps=EPS)


def reference(case, dy=None, index=None):
    return pillar_fp64(case["voxels"], case["num_points"], case["coors"], case["weight"], case["gamma"], case["beta"],
                       case["running_mean"], case["running_var"], case["momentum"], case["eps"], case["vx"], case["vy"],
                       case["x_offset"], case["y_offset"], case["with_distance"], dy=dy, index=index)


def make_case(family, n, f, with_distance):
    """The case of the first seed without a ReLU tie (cached: the forward reference is computed once and shared)."""
    key = (family, n, f, with_distance)
    if key not in _CACHE:
        base = 1000 * FAMILIES.index(family) + 100 * f + 10 * int(with_distance) + n
        for seed in range(base, base + 50):
            case = _generate(family, n, f, with_distance, seed)
            fwd = reference(case)
            if fwd["ties"] == 0:
                case["forward_ref"] = fwd
                _CACHE[key] = case
                break
        else:
            raise AssertionError("no seed without a ReLU tie for %s" % (key,))
    return _CACHE[key]


def build_net(case, device):
    """Our PillarFeatureNet with the case's weights and statistics, in training mode."""
    from efg_amd.modeling.readers import PillarFeatureNet

    origin_x, origin_y = case["x_offset"] - case["vx"] / 2, case["y_offset"] - case["vy"] / 2
    net = PillarFeatureNet(num_input_features=case["f"], num_filters=(CHANNELS,), with_distance=case["with_distance"],
                           voxel_size=(case["vx"], case["vy"], 4.0), pc_range=(origin_x, origin_y, -3, 0, 0, 1))
    net.x_offset, net.y_offset = case["x_offset"], case["y_offset"]
    layer = net.pfn_layers[0]
    layer.norm.momentum, layer.norm.eps = case["momentum"], case["eps"]
    with torch.no_grad():
        layer.linear.weight.copy_(case["weight"])
        layer.norm.weight.copy_(case["gamma"])
        layer.norm.bias.copy_(case["beta"])
        layer.norm.running_mean.copy_(case["running_mean"])
        layer.norm.running_var.copy_(case["running_var"])
    return net.to(device).train()


OUTPUTS = ("out", "index", "dweight", "dgamma", "dbeta", "running_mean", "running_var")


def figures(case, got):
    """err / bound at c = 1 of every output of an fp32 implementation (`got`: out, index [P, C], dweight, dgamma, dbeta and the
    running statistics after the step) against the float64 reference evaluated at ITS index.  -> (figures, reference)"""
    from pillar_fp64_ref import U32, index_terms

    ref = reference(case, dy=case["dy"], index=got["index"].cpu())
    value, best, mag, cond = index_terms(got["index"].cpu(), ref)
    fig = {"index": float(((value - best).abs() / (math.sqrt(ref["out_n"]) * U32 * mag + cond + 1e-30)).max())}
    for k in OUTPUTS:
        if k == "index":
            continue
        n = torch.as_tensor(ref[k + "_n"], dtype=torch.float64).clamp_min(1.0)
        err = (got[k].detach().cpu().to(torch.float64) - ref[k]).abs()
        fig[k] = float((err / (torch.sqrt(n) * U32 * ref[k + "_mag"] + ref[k + "_cond"] + 1e-30)).max())
    return fig, ref


def check(name, case, got, consts):
    """Print the figures, then assert every output within its bar at the constants `consts`.  Returns the figures."""
    from pillar_fp64_ref import assert_elementwise, check_index

    fig, ref = figures(case, got)
    print("%s: err / bound at c = 1: %s" % (name, "  ".join("%s %.3g" % kv for kv in fig.items())))
    check_index(name + " index", got["index"].cpu(), ref, consts["index"])
    for k in OUTPUTS:
        if k != "index":
            assert_elementwise("%s %s" % (name, k), got[k].cpu(), ref[k], ref[k + "_mag"], ref[k + "_n"], consts[k],
                               geo64=ref[k + "_cond"])
    return fig


def composition(case, device="cpu"):
    """The fp32 PyTorch composition (the reference's formulation: our module's composition path, written out so that the
    arg-max is at hand): out, index, the three gradients from the case's dy, the running statistics after the step."""
    net = build_net(case, device)
    layer = net.pfn_layers[0]
    dev = torch.device(device)
    dec = net.decorate(case["voxels"].to(dev), case["num_points"].to(dev), case["coors"].to(dev))
    x = layer.linear(dec)
    x = layer.norm(x.permute(0, 2, 1).contiguous()).permute(0, 2, 1).contiguous()
    out, index = torch.max(torch.relu(x), dim=1)
    out.backward(case["dy"].to(dev))
    assert int(layer.norm.num_batches_tracked) == 1
    return dict(out=out.detach(), index=index, dweight=layer.linear.weight.grad, dgamma=layer.norm.weight.grad,
                dbeta=layer.norm.bias.grad, running_mean=layer.norm.running_mean.clone(), running_var=layer.norm.running_var.clone())
