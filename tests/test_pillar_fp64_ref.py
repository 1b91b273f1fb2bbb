"""CPU pins of the float64 reference of the PointPillars reader (tests/pillar_fp64_ref.py), and the place where the constants of
tests/test_pillar_fp64_gpu.py are fixed.

1. The reference equals the module's PyTorch composition evaluated in float64 with autograd, to 1e-10 of its terms.
2. The SAME composition in fp32 -- the reference's formulation, what the kernels replace -- is held against the reference on the
   CPU.  The worst err / bound at c = 1 per family and output is printed; the figures are recorded in FIG of the GPU test file,
   from which its constants follow as c = min(16, 4 x figure) rounded up to a power of two and at least 1; the test asserts that
   the composition passes at those constants.
3. No case holds a ReLU tie: a selected pre-ReLU value within 16 x its bar of zero.  This is a condition on the inputs;
   `pillar_fp64_cases.make_case` takes the first seed that meets it, and the seed is printed."""
import pytest
import torch

import pillar_fp64_cases as C
from test_pillar_fp64_gpu import CONSTS, FIG, bar_constant


def _family_cases(family):
    return [c for c in C.cases() if c[0] == family]


@pytest.mark.parametrize("family", C.FAMILIES)
def test_no_relu_ties_and_every_boundary_is_crossed(family):
    for _, n, f, with_distance in _family_cases(family):
        case = C.make_case(family, n, f, with_distance)
        fwd = case["forward_ref"]
        print("%s N=%d F=%d dist=%d: seed %d" % (family, n, f, with_distance, case["seed"]))
        assert fwd["ties"] == 0
        counts = case["num_points"].tolist()
        assert counts[:4] == [1, 2, n - 1, n] and len(counts) == 3 * C.TILE + 1 and min(counts) >= 1
        assert sorted(set(case["coors"][:, 0].tolist())) == [0, 1]
        keys = case["coors"][:, 0] * 1000 + case["coors"][:, 2] * C.GRID + case["coors"][:, 3]
        assert len(set(keys.tolist())) == len(keys), "pillar coordinates are unique per scene"
        if family == "padded-wins":
            padded = case["num_points"].long() < n
            arg = fwd["argmax"]
            assert bool((arg[padded, :16] == case["num_points"].long()[padded].view(-1, 1)).all())
            assert bool((fwd["out"][:, 16:32] == 0).all()) and bool((fwd["out"][:, 32:] > 0).any())


@pytest.mark.parametrize("family", C.FAMILIES)
def test_reference_equals_the_float64_composition(family):
    _, n, f, with_distance = _family_cases(family)[0]
    case = C.make_case(family, n, f, with_distance)
    case64 = {k: (v.double() if torch.is_tensor(v) and v.dtype == torch.float32 else v) for k, v in case.items()}
    net = C.build_net(case, "cpu").double()
    layer = net.pfn_layers[0]
    dec = net.decorate(case64["voxels"], case["num_points"], case["coors"])
    x = layer.norm(layer.linear(dec).permute(0, 2, 1).contiguous()).permute(0, 2, 1)
    out, index = torch.max(torch.relu(x), dim=1)
    out.backward(case64["dy"])
    ref = C.reference(case, dy=case["dy"], index=index)
    got = dict(out=out.detach(), dweight=layer.linear.weight.grad, dgamma=layer.norm.weight.grad, dbeta=layer.norm.bias.grad,
               running_mean=layer.norm.running_mean, running_var=layer.norm.running_var)
    for k, g in got.items():
        bad = (g - ref[k]).abs() > 1e-10 * ref[k + "_mag"] + 2.0 ** -29 * ref[k + "_cond"] + 1e-300
        assert not bool(bad.any()), "%s %s: worst %.3g" % (family, k, float((g - ref[k]).abs().max()))
        assert bool((ref[k].abs() <= ref[k + "_mag"] * (1 + 1e-9) + 1e-300).all()), "%s %s: magnitude below |value|" % (family, k)


@pytest.mark.parametrize("family", C.FAMILIES)
def test_composition_figures(family):
    worst = {}
    for _, n, f, with_distance in _family_cases(family):
        case = C.make_case(family, n, f, with_distance)
        fig = C.check("%s N=%d F=%d dist=%d fp32 composition" % (family, n, f, with_distance), case, C.composition(case),
                      CONSTS[family])
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("%s: fp32 composition, worst err / bound at c = 1: %s" % (family, ", ".join("%s=%.2f" % kv for kv in sorted(worst.items()))))
    assert set(worst) == set(FIG[family]) == set(CONSTS[family])
    for k, v in worst.items():
        assert CONSTS[family][k] == bar_constant(FIG[family][k]) and 1 <= CONSTS[family][k] <= 16
