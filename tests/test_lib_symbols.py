"""CPU: the C-ABI library builds, loads and exports every symbol include/efg_hip.h declares (no
compute calls without a GPU), and argument validation works on the host side."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from efg_amd import _lib, build

    build.build()
    return _lib.lib()


def test_header_symbols_are_exported(lib):
    from efg_amd import _lib

    header = open(os.path.join(ROOT, "include", "efg_hip.h")).read()
    declared = set(re.findall(r"\b(efg_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), "libefg_hip.so does not export " + name
    assert declared == set(_lib.EXPORTED_SYMBOLS), declared ^ set(_lib.EXPORTED_SYMBOLS)


def test_version_and_error_channel(lib):
    assert lib.efg_version().decode().startswith("efg_hip")
    assert b"gfx950" in lib.efg_version()
    # host-side validation: bad arguments are rejected before any device work
    vs, cr = (ctypes.c_float * 3)(0.1, 0.1, 0.15), (ctypes.c_float * 6)(-75.2, -75.2, -2.0, 75.2, 75.2, 4.0)
    assert lib.efg_hard_voxelize_workspace_bytes(1000, 1, 5, 0, 10, vs, cr) == 0
    assert lib.efg_hard_voxelize_workspace_bytes(1000, 1, 2, 5, 10, vs, cr) == 0
    assert lib.efg_hard_voxelize_workspace_bytes(180000, 2, 5, 5, 120000, vs, cr) > 0
    assert lib.efg_spconv_packed_weight_bytes(64, 27, 64, 0) >= 27 * 64 * 64 * 4
    assert lib.efg_spconv_wgrad_workspace_bytes(100000, 64, 64, 27) > 0
    # a sparse-convolution window has at most 31 offsets: one limit for the plan, the tiles and both weight gradients
    assert lib.efg_spconv_tile_plan_bytes(1000, 32) == 0
    assert lib.efg_spconv_wgrad_tiled_ok(64, 64, 32) == 0
    shp = (ctypes.c_int * 3)(41, 1504, 1504)
    assert lib.efg_spconv_index_bytes(2, shp) == ((2 * 41 * 1504 * 1504 + 31) // 32) * 8
    big = (ctypes.c_int * 3)(4100, 1504, 1504)
    assert lib.efg_spconv_index_bytes(2, big) == 0  # >= 2^32 cells is refused
    assert b"2^32" in lib.efg_last_error()
    rc = lib.efg_msda_forward_f32(None, None, None, None, None, 1, 4, 2, 6, 1, 1, 1, None, None)  # d % 4 != 0
    assert rc == -1 and b"head dim" in lib.efg_last_error()


def test_missing_library_fails_loudly(monkeypatch):
    from efg_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_LIB_PATH", "/nonexistent/libefg_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def _c_kind(decl):
    """'ptr' | 'int' | 'int64_t' | 'size_t' | 'float' of a C return type or parameter declaration."""
    if "*" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    assert words and words[0] in ("int", "int64_t", "size_t", "float"), "unclassified C type: %r" % decl
    return words[0]


def _ctypes_kind(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    return {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_float: "float"}[t]


def test_header_prototypes_match_the_ctypes_signatures():
    """Every prototype of include/efg_hip.h against _lib._SIGS, return type and argument by argument (pointer, int, int64_t,
    size_t or float): the two are kept by hand, and a call through a wrong argtypes list passes garbage without an error.
    Declarations only: no built library."""
    from efg_amd import _lib

    header = open(os.path.join(ROOT, "include", "efg_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    protos = re.findall(r"([\w\s\*]+?)\b(efg_\w+)\s*\(([^)]*)\)\s*;", header)
    assert len(protos) >= 100 and len({name for _, name, _ in protos}) == len(protos)
    declared = {}
    for ret, name, params in protos:
        params = [p for p in (q.strip() for q in params.split(",")) if p and p != "void"]
        declared[name] = (_c_kind(ret), [_c_kind(p) for p in params])
    bound = {name: (_ctypes_kind(res), [_ctypes_kind(a) for a in args]) for name, (res, args) in _lib._SIGS.items()}
    assert sorted(declared) == sorted(bound)
    wrong = {name: (declared[name], bound[name]) for name in declared if declared[name] != bound[name]}
    assert not wrong, wrong
