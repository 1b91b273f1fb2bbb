"""GPU: the encoder's tiled box-attention backward (csrc/box_fused.hip: box_bwd_tile_a_kernel + box_bwd_tile_b_kernel and the
binned far corners) computes bit for bit what the build of commit 6fe29a6 computed -- in both of the forms that build held,
the two kernels and the one kernel (box_bwd_tile_kernel, EFG_BOX_SPLIT=0) that has since been deleted.

tests/golden/box_bwd_bits.json holds the SHA-256 of grad_value, grad_offsets and grad_logits (one matrix where offsets and
logits share a projection) of scripts/record_box_bwd_bits.py as that build produced them on an MI355X; the recorder wrote the
file only after the one-kernel and the two-kernel form had given equal hashes for every output.  The same script builds the
inputs (integer arithmetic on torch.arange) and runs the cases here, through BoxAttnFusedFunction with 8 heads of 32 channels
and the 5 x 5 lattice, a dropped bin entry raising: `near` (2 x 44 x 52, no corner leaves its tile's window; 77 tiles on 64
workgroups), `rot` (rotated boxes, the shared matrix of row stride 240, 1 % of the corners binned), `big` (61 % binned) and
`wide` (1 x 90 x 142: 72, 72 and 63 tiles per colour class of pass B on 64 workgroups).

The softmax goes through expf, and `rot` through cosf and sinf, of the device library: the fixture belongs to the ROCm release
it names.  A hash that moves means an operation, its order, a guard or a corner's bin changed.  The fixture is not re-recorded
to follow the code."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEPARATE, SHARED = ["grad_value", "grad_offsets", "grad_logits"], ["grad_value", "grad_logits_offsets"]
OUTPUTS = {"near": SEPARATE, "rot": SHARED, "big": SHARED, "wide": SEPARATE}
ALL = [(c, o) for c in OUTPUTS for o in OUTPUTS[c]]


def _recorder():
    spec = importlib.util.spec_from_file_location("record_box_bwd_bits", os.path.join(ROOT, "scripts", "record_box_bwd_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "box_bwd_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    """{case: {output: sha256}}: every case run once for the module."""
    return _recorder().hashes()


def test_every_recorded_case_is_computed(recorded, computed):
    assert recorded["recorded_at"] == "6fe29a6" and recorded["rocm"]
    want = sorted("%s/%s" % co for co in ALL)
    assert sorted("%s/%s" % (c, o) for c in recorded["hashes"] for o in recorded["hashes"][c]) == want
    assert sorted("%s/%s" % (c, o) for c in computed for o in computed[c]) == want
    assert sorted(recorded["far_corner_share"]) == sorted(OUTPUTS)


@pytest.mark.parametrize("case,output", ALL, ids=["%s-%s" % co for co in ALL])
def test_bits_match_the_one_kernel_build(case, output, recorded, computed):
    print("%s %s: recorded %s (ROCm %s) computed %s (ROCm %s)" % (case, output, recorded["hashes"][case][output], recorded["rocm"],
                                                                 computed[case][output], torch.version.hip))
    assert computed[case][output] == recorded["hashes"][case][output]


def test_the_cases_tell_each_other_apart(recorded):
    """What the fixture is worth: no two outputs of any two cases share a hash."""
    flat = [recorded["hashes"][c][o] for c, o in ALL]
    assert len(set(flat)) == len(ALL)
