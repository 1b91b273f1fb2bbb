"""The bits of the tiled sparse convolution (csrc/spconv_tiles.hip: conv_tile_kernel in its 13 reachable instantiations,
conv_small_kernel in its 5), of the weight packer and of the weight gradients (csrc/spconv_wgt.hip, the table kernels of
csrc/spconv_conv.hip) on fixed inputs.  GPU box.

  python scripts/record_spconv_bits.py            print the SHA-256 of every case's outputs, compare with the fixture
  python scripts/record_spconv_bits.py --write    and write them to tests/golden/spconv_bits.json

tests/golden/spconv_bits.json was written ONCE, on an MI355X, by the kernels of commit 3bebb20 -- the last build whose tile
kernel still carried the V4 template parameter, 24 instantiations and the knock-out sites of conv_small_kernel -- loaded
into this script through EFG_HIP_LIB_AB (that build's csrc + include compiled to efg_amd/lib/libefg_hip_parent.so).
tests/test_spconv_bits_gpu.py holds later builds to it: every sum here has a fixed order, so a hash that moves means an
operation, its order, the dealing of the steps to the waves or the cut of a stream-K item list changed.  The fixture is not
re-recorded to follow the code.

A stream-K launch is as many workgroups as the device holds at once (occupancy x CUs), and that number sets where the item
list is cut and therefore the order of a straddling unit's sum: the stream-K hashes belong to the CU count the fixture names
("cus") and to 4 (R = 2) / 5 (R = 1) workgroups per CU.  Everything else is independent of the device's size.

Inputs are integer arithmetic on torch.arange (no random generator for features, weights or gradients).  The sites are those
of tests/test_spconv_streamk_gpu.py (default_rng(5), 2 scenes, grid 12 x 160 x 160) in two sizes: G, 60000 draws per scene
(44989 sites, 2811 row tiles: fills a stream-K launch, units straddle cuts) and g, 600 draws (498 sites, 31 tiles: fewer items
than workgroups, the surplus workgroups leave).

The library reads EFG_TILE_STREAMK once, so each configuration (CONFIGS) is one child process, one after the other, each
under its own time limit; the run stops at the first that fails.  Every case hashes y (forward), dx (data gradient) and, where
the case says so, dw.  Before a case runs, the child asserts that the library's own launch rule (efg_spconv_small_ok,
efg_spconv_tile_shape, plus the stream-K / bf16x3 conditions of run_tiles) picks the instantiation the case is for: a later
change of the rule fails loudly instead of silently testing something else."""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "spconv_bits.json")
RECORDED_AT = "3bebb20"
SHAPE, BATCH = (12, 160, 160), 2
SITES = {"G": (60000, 44989), "g": (600, 498)}      # draws per scene, sites
_MOD = 16777213                                      # the largest prime under 2^24: v / 2^24 is an exact fp32 number
CHILD_TIMEOUT = 240

K3, S1, S2, P1 = (3, 3, 3), (1, 1, 1), (2, 2, 2), (1, 1, 1)
HK, HS, HP = (3, 1, 1), (2, 1, 1), (0, 0, 0)        # the z-collapsing heads


def T(nt, r, ks, mode):
    return "tile<%d,%d,%d,%d>" % (nt, r, ks, mode)


def S(c16, nt, vec):
    return "small<%d,%d,%d>" % (c16, nt, vec)


def case(cin, cout, geo, fwd, dgrad, kind="subm", bias=False, dw=None, pair=False):
    """kind: subm | down (k3 s2 p1) | head (k(3,1,1) s(2,1,1)); dw: None | "tiled" | "table"; fwd / dgrad: the instantiation."""
    return dict(cin=cin, cout=cout, geo=geo, kind=kind, bias=bias, dw=dw, pair=pair, fwd=fwd, dgrad=dgrad)


# config -> (environment, {case name: case})
CONFIGS = {
    "default": ({}, {
        "subm64_G": case(64, 64, "G", T(4, 2, 4, 2), T(4, 2, 4, 2), bias=True, dw="tiled"),
        "subm64_g": case(64, 64, "g", T(4, 2, 4, 2), T(4, 2, 4, 2), bias=True),
        "subm128_G": case(128, 128, "G", T(4, 2, 4, 2), T(4, 2, 4, 2), dw="tiled"),
        "subm256_G": case(256, 256, "G", T(4, 2, 4, 2), T(4, 2, 4, 2)),
        "down128_256_G": case(128, 256, "G", T(4, 1, 4, 2), T(4, 1, 4, 2), kind="down"),
        "down64_128_G": case(64, 128, "G", T(4, 1, 4, 0), T(4, 1, 4, 0), kind="down", dw="tiled"),
        "subm32_G": case(32, 32, "G", T(2, 1, 4, 0), T(2, 1, 4, 0)),
        "subm64_16_G": case(64, 16, "G", T(1, 1, 4, 0), T(4, 1, 4, 2)),
        "head64_G": case(64, 64, "G", T(4, 1, 1, 0), T(4, 1, 1, 0), kind="head"),
        "head128_G": case(128, 128, "G", T(4, 1, 1, 0), T(4, 1, 1, 0), kind="head"),
        "head64_32_G": case(64, 32, "G", T(2, 1, 1, 0), T(4, 1, 1, 0), kind="head"),
        "head64_16_G": case(64, 16, "G", T(1, 1, 1, 0), T(4, 1, 1, 0), kind="head"),
        "down5_16_G": case(5, 16, "G", S(1, 1, 0), S(1, 1, 1), kind="down"),
        "down4_32_G": case(4, 32, "G", S(1, 2, 0), S(2, 1, 1), kind="down"),
        "subm16_G": case(16, 16, "G", S(1, 1, 1), S(1, 1, 1)),
        "subm16_32_G": case(16, 32, "G", S(1, 2, 1), S(2, 1, 1)),
        "pair64_128_G": case(64, 128, "G", T(4, 1, 4, 0), T(4, 1, 4, 0), kind="down", dw="tiled", pair=True),
        "table_subm64_G": case(64, 64, "G", T(4, 2, 4, 2), T(4, 2, 4, 2), dw="table"),
        "table_subm16_G": case(16, 16, "G", S(1, 1, 1), S(1, 1, 1), dw="table"),
        "table_subm16_32_G": case(16, 32, "G", S(1, 2, 1), S(2, 1, 1), dw="table"),
        "table_down5_16_G": case(5, 16, "G", S(1, 1, 0), S(1, 1, 1), kind="down", dw="table"),
    }),
    "streamk0": ({"EFG_TILE_STREAMK": "0"}, {
        "subm64_G": case(64, 64, "G", T(4, 1, 4, 0), T(4, 1, 4, 0)),
        "subm128_G": case(128, 128, "G", T(4, 2, 4, 0), T(4, 2, 4, 0)),
        "subm256_G": case(256, 256, "G", T(4, 2, 4, 0), T(4, 2, 4, 0)),
    }),
    "streamk2": ({"EFG_TILE_STREAMK": "2"}, {
        "down64_128_G": case(64, 128, "G", T(4, 1, 4, 2), T(4, 1, 4, 2), kind="down"),
        "pair64_128_G": case(64, 128, "G", T(4, 1, 4, 2), T(4, 1, 4, 2), kind="down", pair=True),
    }),
    "bf16x3_streamk0": ({"EFG_TILE_STREAMK": "0", "EFG_GEMM_ARM": "bf16x3"}, {
        "subm64_G": case(64, 64, "G", T(4, 1, 4, 4), T(4, 1, 4, 4)),
        "subm128_G": case(128, 128, "G", T(4, 2, 4, 4), T(4, 2, 4, 4)),
        "down128_256_G": case(128, 256, "G", T(4, 1, 4, 4), T(4, 1, 4, 4), kind="down"),
    }),
    "bf16x3_streamk2": ({"EFG_TILE_STREAMK": "2", "EFG_GEMM_ARM": "bf16x3"}, {
        "subm64_G": case(64, 64, "G", T(4, 2, 4, 6), T(4, 2, 4, 6)),
        "subm128_G": case(128, 128, "G", T(4, 2, 4, 6), T(4, 2, 4, 6)),
        "down128_256_G": case(128, 256, "G", T(4, 1, 4, 6), T(4, 1, 4, 6), kind="down"),
    }),
}
_SWITCHES = ("EFG_TILE_STREAMK", "EFG_TILE_SK_POLLS", "EFG_GEMM_ARM", "EFG_CONV_ARM", "EFG_CONV_SMALL", "EFG_CONV_PAIR",
             "EFG_WGRAD_TILED")


def outputs(c):
    """Names of the tensors a case hashes."""
    if c["pair"]:
        return ["y_a", "y_b", "dx"] + (["dw_a", "dw_b"] if c["dw"] else [])
    return ["y", "dx"] + (["dw"] if c["dw"] else [])


def is_streamk(c):
    """Does a hash of the case depend on the number of resident workgroups?"""
    return any(int(c[d][:-1].split(",")[3]) & 2 for d in ("fwd", "dgrad") if c[d].startswith("tile"))


def unit(shape, salt):
    """fp32 host tensor of `shape`, values in [0, 1)."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    v = (i * i * 7919 + i * 104729 + (i % 7) * 15485863 + salt * 1299709 + 12345) % _MOD
    return (v.to(torch.float32) * 2.0 ** -24).view(shape)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def sites(draws):
    """int32 [m, 4] (b, z, y, x): clustered sites (a few planes + blobs), the generator of tests/test_spconv_streamk_gpu.py."""
    rng = np.random.default_rng(5)
    pts = []
    for b in range(BATCH):
        z = rng.integers(0, SHAPE[0], draws)
        y = rng.integers(0, SHAPE[1], draws)
        x = rng.integers(0, SHAPE[2], draws)
        keep = (z < 3) | ((x + y) % 7 == 0) | (rng.random(draws) < 0.08)
        pts.append(np.stack([np.full(keep.sum(), b), z[keep], y[keep], x[keep]], 1))
    return np.unique(np.concatenate(pts), axis=0).astype(np.int32)


def kernel_label(cin, cout, kvol, m_in, m_out, arm_on):
    """The instantiation run_tiles launches for this convolution, from the library's own rule."""
    from efg_amd import _lib as L

    lib = L.lib()
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    bf3 = bool(arm_on and lib.efg_spconv_tile_bf16x3_ok(cin, cout, kvol, m_in, m_out))
    if not bf3 and lib.efg_spconv_small_ok(cin, cout, kvol, ctypes.byref(a), ctypes.byref(b)):
        return S(a.value, b.value, int(cin > 8))
    L.check(lib.efg_spconv_tile_shape(cin, cout, kvol, m_in, m_out, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    nt, r, ks = a.value, b.value, c.value
    # MODE is a COPY of the rule in run_tiles (csrc/spconv_tiles.hip: the stream-K eligibility below `sk_env`, bf3 from the flag
    # word); the library has no query for it.  Not copied: a launch under graph capture never runs stream-K (nothing here captures).
    sk = int(os.environ.get("EFG_TILE_STREAMK", "1"))
    streamk = sk and nt == 4 and ks == 4 and (sk == 2 or m_in == m_out or (cin >= 128 and cout >= 128))
    return T(nt, r, ks, (2 if streamk else 0) | (4 if bf3 else 0))


def run_case(name, c, salt, dev, geo):
    """{output: tensor} of one case, through the functions of efg_amd/spconv/core.py that call the library."""
    import efg_amd.spconv as spconv
    from efg_amd.operators import linear as lin
    from efg_amd.spconv import core

    cin, cout = c["cin"], c["cout"]
    idx = geo[c["geo"]]
    x = spconv.SparseConvTensor(torch.zeros(idx.shape[0], 1, device=dev), idx, list(SHAPE), BATCH)
    if c["kind"] == "subm":
        conv = spconv.SubMConv3d(cin, cout, 3, padding=1, bias=False, indice_key="k")
    elif c["kind"] == "down":
        conv = spconv.SparseConv3d(cin, cout, K3, S2, padding=P1, bias=False)
    else:
        conv = spconv.SparseConv3d(cin, cout, HK, HS, padding=HP, bias=False)
    rb, _ = conv._rulebook(x)
    kvol = rb.kvol
    arm = bool(lin._ARM_BF16X3)
    got = (kernel_label(cin, cout, kvol, rb.m_in, rb.m_out, arm), kernel_label(cout, cin, kvol, rb.m_out, rb.m_in, arm))
    assert got == (c["fwd"], c["dgrad"]), "case %s is for %s / %s, the library's rule picks %s / %s" % (
        name, c["fwd"], c["dgrad"], got[0], got[1])
    feat = (unit((rb.m_in, cin), salt + 1) * 2 - 1).to(dev)
    go = (unit((rb.m_out, cout), salt + 2) * 2 - 1).to(dev)
    w = ((unit((cout, kvol, cin), salt + 3) * 2 - 1) * 0.25).to(dev)
    bias = (unit((cout,), salt + 4) * 2 - 1).to(dev) if c["bias"] else None
    table = c["dw"] == "table"
    if table:      # the table kernels of csrc/spconv_conv.hip instead of the plan-walking weight gradient
        os.environ["EFG_WGRAD_TILED"] = "0"
        core._WGT_OK.clear()
    try:
        if c["pair"]:
            wb = ((unit((cout, kvol, cin), salt + 5) * 2 - 1) * 0.25).to(dev)
            gob = (unit((rb.m_out, cout), salt + 6) * 2 - 1).to(dev)
            assert core._pair_ok(rb, w, wb, cin, cout) and core._wgrad_tiled(cin, cout, kvol, rb.m_out, rb.m_in)
            out = {}
            out["y_a"], out["y_b"] = core._conv_forward_pair(feat, w, wb, rb, None, None)
            out["dx"] = core._conv_dgrad_pair(go, gob, w, wb, rb, None, None)
            if c["dw"]:
                out["dw_a"], out["dw_b"] = core._conv_wgrad_pair(feat, go, gob, rb)
            return out
        out = {"y": core._conv_forward(feat, w, bias, rb), "dx": core._conv_dgrad(go, w, rb)}
        if c["dw"]:
            assert core._wgrad_tiled(cin, cout, kvol, rb.m_out, rb.m_in) == (not table), name
            out["dw"] = core._conv_wgrad(feat, go, rb)
        return out
    finally:
        if table:
            del os.environ["EFG_WGRAD_TILED"]
            core._WGT_OK.clear()


def child(config):
    """One configuration in this process: prints one JSON line {"hashes", "fallbacks", "cus"}."""
    sys.path.insert(0, ROOT)
    from efg_amd import _lib as L

    dev = torch.device("cuda:0")
    geo = {}
    for g, (draws, m) in SITES.items():
        idx = sites(draws)
        assert idx.shape[0] == m, (g, idx.shape[0])
        geo[g] = torch.from_numpy(idx).to(dev)
    cases = CONFIGS[config][1]
    hashes = {}
    for n, name in enumerate(sorted(cases)):
        out = run_case(name, cases[name], 10000 * list(CONFIGS).index(config) + 100 * (1 + n), dev, geo)
        assert sorted(out) == sorted(outputs(cases[name]))
        hashes[name] = {k: sha(t) for k, t in out.items()}
    torch.cuda.synchronize()
    count = ctypes.c_int64()
    L.check(L.lib().efg_spconv_streamk_fallbacks(ctypes.byref(count), 0))
    print("CHILD_RESULT " + json.dumps({"hashes": hashes, "fallbacks": count.value,
                                        "cus": torch.cuda.get_device_properties(0).multi_processor_count}))


def hashes():
    """({config: {case: {output: sha256}}}, {config: late shares}, CUs): one child per configuration, stopping at the first
    that fails."""
    out, late, cus = {}, {}, None
    for config, (env, _) in CONFIGS.items():
        e = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
        e.update(env)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config], capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT, cwd=ROOT, env=e)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD_RESULT ")]
        if r.returncode != 0 or len(lines) != 1:
            raise RuntimeError("configuration %s failed (exit %d):\n%s\n%s" % (config, r.returncode, r.stdout[-1000:], r.stderr[-3000:]))
        res = json.loads(lines[0][len("CHILD_RESULT "):])
        out[config], late[config], cus = res["hashes"], res["fallbacks"], res["cus"]
    return out, late, cus


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write tests/golden/spconv_bits.json (see the module docstring)")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_spconv_bits.py runs the kernels: no device found")
    if args.child:
        child(args.child)
        return 0
    got, late, cus = hashes()
    doc = {"recorded_at": RECORDED_AT, "rocm": torch.version.hip, "cus": cus, "hashes": got}
    print(json.dumps(doc, indent=1))
    print("late stream-K shares (efg_spconv_streamk_fallbacks): %s" % json.dumps(late))
    if any(late.values()):
        raise SystemExit("a stream-K share arrived late: the order of a sum is not the recorded one; nothing written or compared")
    if args.write:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    elif os.path.exists(args.out):
        with open(args.out) as f:
            want = json.load(f)
        bad = [(g, c, k) for g in got for c in got[g] for k in got[g][c] if want["hashes"].get(g, {}).get(c, {}).get(k) != got[g][c][k]]
        print("differs from %s (recorded on %d CUs, here %d): %s" % (os.path.relpath(args.out, ROOT), want["cus"], cus, bad or "nothing"))
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
