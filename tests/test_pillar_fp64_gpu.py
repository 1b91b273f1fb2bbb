"""GPU: the fused PointPillars reader (csrc/pillars.hip) against the float64 reference of tests/pillar_fp64_ref.py, element by
element, on every output: |got - ref| <= c * sqrt(n) * 2^-24 * |terms| + cond (the terms: pillar_fp64_ref.py; `cond` is
batchnorm_fp64's own allowance for the rounded mean and rstd).  The backward reference is evaluated at the KERNEL's index, and the
index check holds the float64 value at that row to the bar of the float64 maximum.

The constants c are measured, not chosen: tests/test_pillar_fp64_ref.py runs the fp32 PyTorch composition on the CPU over the
same inputs against the same reference and records the worst err / bound at c = 1 per family and output (FIG below);
c = min(16, 4 x figure) rounded up to a power of two and at least 1, the rule of tests/test_norm_fp64_gpu.py.

Cases, shapes and input families: tests/pillar_fp64_cases.py."""
import math

import pytest
import torch

import pillar_fp64_cases as C

pytestmark = pytest.mark.gpu

# worst err / bound at c = 1 of the fp32 PyTorch composition on the CPU, per family over its six cases
# (printed by tests/test_pillar_fp64_ref.py::test_composition_figures, which also asserts that they are still what it measures)
FIG = {
    "plain": dict(out=0.14, index=0.0, dweight=0.10, dgamma=0.02, dbeta=0.07, running_mean=0.03, running_var=0.07),
    "offset": dict(out=0.20, index=0.0, dweight=0.23, dgamma=0.04, dbeta=0.08, running_mean=0.02, running_var=0.01),
    "scales": dict(out=0.14, index=0.0, dweight=0.19, dgamma=0.02, dbeta=0.12, running_mean=0.11, running_var=0.11),
    "padded-wins": dict(out=0.14, index=0.0, dweight=0.11, dgamma=0.02, dbeta=0.11, running_mean=0.04, running_var=0.09),
    "garbage-padding": dict(out=0.85, index=0.17, dweight=0.81, dgamma=0.12, dbeta=0.10, running_mean=0.04, running_var=0.04),
    "duplicates": dict(out=0.15, index=0.0, dweight=0.29, dgamma=0.03, dbeta=0.12, running_mean=0.03, running_var=0.07),
}


def bar_constant(figure):
    """min(16, 4 x figure), rounded up to a power of two and at least 1."""
    return 2.0 ** math.ceil(math.log2(max(1.0, min(16.0, 4.0 * figure))))


CONSTS = {family: {k: bar_constant(v) for k, v in fig.items()} for family, fig in FIG.items()}


def run_fused(case, dev, max_blocks=0, voxels=None):
    """Forward + backward of the fused path on the case: the outputs `pillar_fp64_cases.check` takes."""
    from efg_amd.operators.pillars import pillar_features

    net = C.build_net(case, dev)
    layer = net.pfn_layers[0]
    voxels = (case["voxels"] if voxels is None else voxels).to(dev)
    assert net.usable(voxels)
    out, index = pillar_features(voxels, case["num_points"].to(dev), case["coors"].to(dev), layer.linear.weight, layer.norm,
                                 net.vx, net.vy, net.x_offset, net.y_offset, case["with_distance"], return_index=True,
                                 max_blocks=max_blocks)
    out.backward(case["dy"].to(dev))
    torch.cuda.synchronize()
    assert int(layer.norm.num_batches_tracked) == 1 and index.dtype == torch.uint8
    return dict(out=out.detach(), index=index, dweight=layer.linear.weight.grad, dgamma=layer.norm.weight.grad,
                dbeta=layer.norm.bias.grad, running_mean=layer.norm.running_mean.clone(), running_var=layer.norm.running_var.clone())


@pytest.mark.parametrize("family,n,f,with_distance", C.cases())
def test_fused_reader_against_fp64(dev, family, n, f, with_distance):
    case = C.make_case(family, n, f, with_distance)
    got = run_fused(case, dev)
    C.check("%s N=%d F=%d dist=%d" % (family, n, f, with_distance), case, got, CONSTS[family])
    index, counts = got["index"].cpu().long(), case["num_points"].long()
    if family == "padded-wins":
        padded = counts < n
        assert bool((index[padded, :16] == counts[padded].view(-1, 1)).all()), "the first padded row stands for the padded rows"
        assert bool((index[~padded, :16] < n).all())
        assert bool((got["out"].cpu()[:, 16:32] == 0).all()) and bool((index[:, 16:32] == 0).all())
        assert bool((got["dweight"].cpu()[16:32] == 0).all()) and bool((got["dbeta"].cpu()[16:32] == 0).all())
    if family == "duplicates":
        dup = index[::3]
        assert bool(((dup == 0) | (dup == counts[::3].view(-1, 1))).all()), "identical rows: the lowest one wins"


def test_looped_grid_against_fp64(dev):
    """Two workgroups loop over the four tiles: the same bars."""
    family, n, f, with_distance = C.cases()[0]
    case = C.make_case(family, n, f, with_distance)
    C.check("looped grid", case, run_fused(case, dev, max_blocks=2), CONSTS[family])


def test_garbage_outside_xyz_changes_nothing(dev):
    """Padded rows are masked after decoration whatever they hold: 1e6 in their columns >= 3 (which no mean reads) leaves every
    output as it is with zeros there, bit for bit.  (In the xyz columns padded rows move the cluster mean, as in the reference,
    which sums over all rows: the garbage-padding family above.)"""
    family, n, f, with_distance = "plain", 20, 5, True
    case = C.make_case(family, n, f, with_distance)
    real = (torch.arange(n).view(1, n) < case["num_points"].view(-1, 1)).unsqueeze(-1)
    dirty = case["voxels"].clone()
    dirty[:, :, 3:] = torch.where(real, dirty[:, :, 3:], torch.full((), 1e6))
    a, b = run_fused(case, dev), run_fused(case, dev, voxels=dirty)
    for k in a:
        assert torch.equal(a[k], b[k]), k
