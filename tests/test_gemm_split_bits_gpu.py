"""GPU: the two split-bf16 GEMM arms (csrc/gemm_split_bf16.h as csrc/gemm_bf16x3.hip and csrc/gemm_bf16x6.hip) compute, bit
for bit, what the two hand-written programs they replaced computed.

tests/golden/gemm_split_bits.json holds the SHA-256 of every output of scripts/record_gemm_split_bits.py as the build of
commit 7172bf6 (two separate sources) produced them on an MI355X; the same script builds the inputs (integer arithmetic on
torch.arange, not bf16-representable, rows and columns asymmetric) and runs the cases here.  Forward at m, k, n =
130, 36, 132 (two row tiles, two column blocks, two K steps, each with a ragged tail): bias + ReLU, neither, a row-strided
view (lda > k), an overlapping-row view (lda < k), and the packed buffers of pack_linear and of pack_linear_both; weight
gradient at 200 x 132 x 36 (seven 32-row chunks: the unrolled and the tail loop of the reduce) and 33 x 8 x 4.

A hash that moves means the split, the product order, the K-step / tile / chunk order or a packed layout changed.  The
fixture is not re-recorded to follow the code."""
import importlib
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["packed_forward", "packed_dgrad", "packed_both_forward", "packed_both_dgrad", "forward_bias_relu", "forward_plain",
         "forward_row_strided", "forward_overlapping_rows", "wgrad_200_132_36", "wgrad_33_8_4"]


def _recorder():
    spec = importlib.util.spec_from_file_location("record_gemm_split_bits",
                                                  os.path.join(ROOT, "scripts", "record_gemm_split_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "gemm_split_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    """{arm: {case: sha256}}: every case run once for the module."""
    R = _recorder()
    return {arm: {name: R.sha(t) for name, t in R.cases(importlib.import_module("efg_amd.operators.gemm_" + arm)).items()}
            for arm in R.ARMS}


@pytest.mark.parametrize("arm", ["bf16x3", "bf16x6"])
def test_every_recorded_case_is_computed(arm, recorded, computed):
    assert sorted(recorded[arm]) == sorted(CASES) == sorted(computed[arm])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("arm", ["bf16x3", "bf16x6"])
def test_bits_match_the_two_source_build(arm, case, recorded, computed):
    print("%s %s: recorded %s computed %s" % (arm, case, recorded[arm][case], computed[arm][case]))
    assert computed[arm][case] == recorded[arm][case]


@pytest.mark.parametrize("arm", ["bf16x3", "bf16x6"])
def test_the_cases_tell_the_arms_and_the_layouts_apart(arm, recorded):
    """What the fixture is worth: no two different cases share a hash (a transposed weight, a dropped bias or ReLU, another
    row stride each give other bytes), the two packers agree, and no case of one arm equals the other arm's."""
    r = recorded[arm]
    assert r["packed_forward"] == r["packed_both_forward"] and r["packed_dgrad"] == r["packed_both_dgrad"]
    distinct = [c for c in CASES if not c.startswith("packed_both")]
    assert len({r[c] for c in distinct}) == len(distinct)
    other = recorded["bf16x6" if arm == "bf16x3" else "bf16x3"]
    assert not set(r.values()) & set(other.values())
