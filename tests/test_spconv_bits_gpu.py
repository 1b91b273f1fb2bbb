"""GPU: the tiled sparse convolution (csrc/spconv_tiles.hip: the 13 instantiations of conv_tile_kernel the launch rule reaches,
the 5 of conv_small_kernel), the weight packer and the weight gradients (csrc/spconv_wgt.hip, the table kernels of
csrc/spconv_conv.hip) compute bit for bit what the build of commit 3bebb20 computed -- the last one whose tile kernel had the
V4 parameter and was compiled in 24 instantiations.

tests/golden/spconv_bits.json holds the SHA-256 of y, dx and (where the case has one) dw of scripts/record_spconv_bits.py as
that build produced them on an MI355X.  The same script builds the inputs (integer arithmetic on torch.arange; the sites of
tests/test_spconv_streamk_gpu.py at 44989 and at 498 sites), asserts per case that the library's launch rule picks the
instantiation the case is for, and runs the five configurations (default, EFG_TILE_STREAMK=0, =2, EFG_GEMM_ARM=bf16x3 with
stream-K 0 and 2) in one child process each, one after the other.

Every sum has a fixed order, so a hash that moves means an operation, its order, the dealing of the steps to the waves or
the cut of a stream-K item list changed.  A stream-K launch is (workgroups per CU) x CUs workgroups and the cuts follow that
number: on a device with the recorded CU count no case may be left out; on any other only the stream-K cases are skipped,
each with its reason.  A late stream-K share (efg_spconv_streamk_fallbacks != 0) changes the order of a sum too and is reported
as that, not as a hash mismatch.  The fixture is not re-recorded to follow the code."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_spconv_bits", os.path.join(ROOT, "scripts", "record_spconv_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
ALL = [(g, c, o) for g, (_, cases) in REC.CONFIGS.items() for c in cases for o in REC.outputs(cases[c])]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "spconv_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    """({config: {case: {output: sha256}}}, {config: late shares}, CUs): every configuration run once for the module."""
    return REC.hashes()


def test_every_recorded_case_is_computed(recorded, computed):
    assert recorded["recorded_at"] == "3bebb20" and recorded["rocm"] and recorded["cus"] > 0
    want = sorted("%s/%s/%s" % gco for gco in ALL)
    assert len(want) == 75
    assert sorted("%s/%s/%s" % (g, c, o) for g, cs in recorded["hashes"].items() for c in cs for o in cs[c]) == want
    assert sorted("%s/%s/%s" % (g, c, o) for g, cs in computed[0].items() for c in cs for o in cs[c]) == want


def test_no_streamk_share_was_late(computed):
    late = {g: n for g, n in computed[1].items() if n}
    assert not late, "stream-K shares arrived late and their units were recomputed in another order of the sum: %s" % late


@pytest.mark.parametrize("config,case,output", ALL, ids=["%s-%s-%s" % gco for gco in ALL])
def test_bits_match_the_parent_build(config, case, output, recorded, computed):
    got, late, cus = computed
    c = REC.CONFIGS[config][1][case]
    if cus != recorded["cus"] and REC.is_streamk(c):
        pytest.skip("stream-K case (%s / %s): the fixture's cuts are those of %d CUs, this device has %d" % (
            c["fwd"], c["dgrad"], recorded["cus"], cus))
    print("%s %s %s: recorded %s computed %s (%d CUs)" % (config, case, output, recorded["hashes"][config][case][output],
                                                           got[config][case][output], cus))
    assert not late[config], "a stream-K share was late in configuration %s: the order of a sum is not the recorded one" % config
    assert got[config][case][output] == recorded["hashes"][config][case][output]


def test_the_cases_tell_each_other_apart(recorded):
    """What the fixture is worth: no two outputs of any two cases share a hash."""
    flat = [recorded["hashes"][g][c][o] for g, c, o in ALL]
    assert len(set(flat)) == len(ALL)
