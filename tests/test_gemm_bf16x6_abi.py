"""CPU: the C ABI of the fp32-equivalent split-precision arm (csrc/gemm_bf16x6.hip) -- the header declares its six symbols,
the built library exports them, efg_amd/_lib.py lists them with the signatures of their bf16 x 3 twins, and the host-side size
functions answer without a device."""
import os
import re

import pytest

from conftest import ROOT

SYMBOLS = ["efg_gemm_bf16x6_pack_bytes", "efg_gemm_bf16x6_pack_f32", "efg_gemm_bf16x6_pack_linear_f32", "efg_gemm_bf16x6_f32",
           "efg_gemm_bf16x6_wgrad_workspace_bytes", "efg_gemm_bf16x6_wgrad_f32"]


@pytest.fixture(scope="module")
def lib():
    from efg_amd import _lib, build

    build.build()
    return _lib.lib()


def test_the_six_symbols_are_declared_exported_and_listed(lib):
    from efg_amd import _lib

    header = open(os.path.join(ROOT, "include", "efg_hip.h")).read()
    declared = set(re.findall(r"\b(efg_[a-z0-9_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared, name + " is not declared in include/efg_hip.h"
        assert hasattr(lib, name), "libefg_hip.so does not export " + name
        assert name in _lib.EXPORTED_SYMBOLS, name + " is missing from efg_amd/_lib.py"
        # argument for argument the x3 function
        assert _lib._SIGS[name] == _lib._SIGS[name.replace("bf16x6", "bf16x3")], name


def test_header_arguments_mirror_the_x3_declarations():
    header = open(os.path.join(ROOT, "include", "efg_hip.h")).read()

    def decl(name):
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()

    for name in SYMBOLS:
        assert decl(name) == decl(name.replace("bf16x6", "bf16x3")), name


def test_sizes_on_the_host(lib):
    # three pieces of 2 bytes per element of the padded [k to 32][n to 128] matrix: 1.5 x the x3 buffer
    assert lib.efg_gemm_bf16x6_pack_bytes(256, 256) == 256 * 256 * 6
    assert lib.efg_gemm_bf16x6_pack_bytes(200, 7) == 224 * 128 * 6
    assert 2 * lib.efg_gemm_bf16x6_pack_bytes(1024, 200) == 3 * lib.efg_gemm_bf16x3_pack_bytes(1024, 200)
    assert lib.efg_gemm_bf16x6_pack_bytes(0, 4) == 0
    ws = lib.efg_gemm_bf16x6_wgrad_workspace_bytes(70688, 256, 256)
    assert ws > 0 and ws % (256 * 256 * 4) == 0      # whole partial matrices, one per row chunk
    assert lib.efg_gemm_bf16x6_wgrad_workspace_bytes(0, 256, 256) == 0
