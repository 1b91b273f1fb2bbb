"""GPU: the matching-cost, box-loss and paired rotated-GIoU kernels, as templates over one GIoU source (csrc/giou3d.h in
csrc/det_loss.hip and csrc/rot_giou.hip), compute bit for bit what the two copies they replaced computed.

tests/golden/det_loss_bits.json holds the SHA-256 of every output of scripts/record_det_loss_bits.py as the build of commit
066a8e9 (the axis-aligned kernels in det_loss.hip, their rotated copies in rot_giou.hip) produced them on an MI355X; the same
script builds the inputs (integer arithmetic on torch.arange) and runs the cases here, each for the axis-aligned GIoU, the
rotated one in the code frame and the rotated one in the metric frame: the match cost at (L, B, Q, C, G) = (2, 2, 70, 3, 5)
(1400 entries: six 256-thread blocks, the last ragged) and at (1, 2, 70, 3, 17) with an all-zero last target column; the
box-loss sums and gradient at L, B, Q, G = 3, 2, 200, 9 with 1 pair and with 1100 (the 1024-thread workgroup's loop runs
twice, ragged; three pairs are unmatched columns); the paired forward and backward at n = 65.

The match cost goes through expf, powf and logf of the device library: the fixture belongs to the ROCm release it names.
A hash that moves means an operation, its order, the reduction tree or a guard changed.  The fixture is not re-recorded to
follow the code."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ["aligned", "rotated_code", "rotated_metric"]
CASES = ["match_cost_2_2_70_3_5", "match_cost_padded_1_2_70_3_17", "box_loss_sums_n1", "box_loss_grad_n1", "box_loss_sums_n1100",
         "box_loss_grad_n1100"]
PAIRED = ["paired_giou_n65", "paired_iou_n65", "paired_grad_a_n65", "paired_grad_b_n65"]
ALL = [(v, c) for v in VARIANTS for c in CASES + (PAIRED if v != "aligned" else [])]


def _recorder():
    spec = importlib.util.spec_from_file_location("record_det_loss_bits", os.path.join(ROOT, "scripts", "record_det_loss_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "det_loss_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    """{variant: {case: sha256}}: every case run once for the module; torch's global generators handed on as found."""
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state_all()
    try:
        return _recorder().hashes()
    finally:
        torch.set_rng_state(cpu)
        torch.cuda.set_rng_state_all(gpu)


def test_every_recorded_case_is_computed(recorded, computed):
    assert recorded["recorded_at"] == "066a8e9" and recorded["rocm"]
    want = sorted("%s/%s" % vc for vc in ALL)
    assert sorted("%s/%s" % (v, c) for v in recorded["hashes"] for c in recorded["hashes"][v]) == want
    assert sorted("%s/%s" % (v, c) for v in computed for c in computed[v]) == want


@pytest.mark.parametrize("variant,case", ALL, ids=["%s-%s" % vc for vc in ALL])
def test_bits_match_the_two_copy_build(variant, case, recorded, computed):
    print("%s %s: recorded %s (ROCm %s) computed %s (ROCm %s)" % (variant, case, recorded["hashes"][variant][case], recorded["rocm"],
                                                                 computed[variant][case], torch.version.hip))
    assert computed[variant][case] == recorded["hashes"][variant][case]


def test_the_cases_tell_the_forms_and_the_frames_apart(recorded):
    """What the fixture is worth: no two different cases share a hash -- the axis-aligned form, the rotated form and its two
    frames each give other bytes for every case (columns 0 and 2 of the sums are common, column 1 and the gradient are not)."""
    flat = [recorded["hashes"][v][c] for v, c in ALL]
    assert len(set(flat)) == len(ALL)
    for c in CASES:
        assert recorded["hashes"]["aligned"][c] not in (recorded["hashes"]["rotated_code"][c], recorded["hashes"]["rotated_metric"][c])
