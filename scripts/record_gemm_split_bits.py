"""The bits of the split-bf16 GEMM arms (operators/gemm_bf16x3.py, operators/gemm_bf16x6.py) on fixed inputs.  GPU box.

  python scripts/record_gemm_split_bits.py            print the SHA-256 of every case's output bytes
  python scripts/record_gemm_split_bits.py --write    and write them to tests/golden/gemm_split_bits.json

tests/golden/gemm_split_bits.json was written ONCE, by the build of the commit before the two arms became one source
(7172bf6: csrc/gemm_bf16x3.hip and csrc/gemm_bf16x6.hip as two hand-written programs), and
tests/test_gemm_split_bits_gpu.py holds every later build to it: same split, same product order, same K-step, tile and
chunk order, same packed bytes.  A change that moves a hash changed the arithmetic or a layout; the fixture is not
re-recorded to follow it.

Inputs are integer arithmetic on torch.arange (no random generator: nothing here depends on a library's stream of
numbers): 24-bit integers scaled by a power of two, so most values need all three bf16 pieces, with different
row and column coefficients, so a transposed operand is another matrix."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_split_bits.json")
ARMS = ("bf16x3", "bf16x6")

_MOD = 16777213    # the largest prime under 2^24: every value below is an exact fp32 number with up to 24 significand bits


def matrix(rows, cols, salt):
    """[rows, cols] fp32 on the host, values in (-1, 1)."""
    i = torch.arange(rows, dtype=torch.int64).view(-1, 1)
    j = torch.arange(cols, dtype=torch.int64).view(1, -1)
    v = (i * i * 7919 + i * 104729 + j * j * 15485863 + j * 32452843 + i * j * 611953 + salt * 1299709 + 12345) % _MOD
    x = (v - _MOD // 2).to(torch.float32) * 2.0 ** -23
    # what the cases are for: the third piece of the split is there, and the matrix is not its own transpose
    p0 = x.bfloat16().float()
    p1 = (x - p0).bfloat16().float()
    assert float(((x - p0) - p1 != 0).float().mean()) > 0.75
    if rows > 1 and cols > 1:
        assert x[0, 1] != x[1, 0]
    return x


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def cases(G):
    """{case: output tensor} of one arm's module G, on the smallest shapes that reach every branch of its kernels."""
    dev = torch.device("cuda")
    out = {}
    # forward: two row tiles, two column blocks, two K steps, a ragged tail on each
    m, k, n = 130, 36, 132
    a = matrix(m, k, 1).to(dev)
    w = matrix(n, k, 2).to(dev)            # an nn.Linear weight [out, in]
    b = matrix(1, n, 3).view(n).to(dev)
    fwd, dgr = G.pack_linear(w, transposed=False), G.pack_linear(w, transposed=True)
    out["packed_forward"], out["packed_dgrad"] = fwd, dgr
    out["packed_both_forward"], out["packed_both_dgrad"] = G.pack_linear_both(w)
    out["forward_bias_relu"] = G.gemm(a, fwd, n, bias=b, relu=True)
    out["forward_plain"] = G.gemm(a, fwd, n)
    wide = matrix(m, k + 16, 4).to(dev)
    out["forward_row_strided"] = G.gemm(wide[:, 8:8 + k], fwd, n, bias=b)                       # lda = k + 16 > k
    c = k // 3
    flat = matrix(1, m * c + k, 5).view(-1).to(dev)
    out["forward_overlapping_rows"] = G.gemm(flat.as_strided((m, k), (c, 1), 0), fwd, n, bias=b)  # lda = k / 3 < k
    # weight gradient: seven 32-row chunks (the 4-unrolled and the tail loop of the reduce), then the smallest shape
    for m, n, k in ((200, 132, 36), (33, 8, 4)):
        g = matrix(m, n, 6).to(dev)
        x = matrix(m, k, 7).to(dev)
        out["wgrad_%d_%d_%d" % (m, n, k)] = G.wgrad(g, x)
    torch.cuda.synchronize()
    return out


def hashes():
    import importlib

    sys.path.insert(0, ROOT)
    return {arm: {name: sha(t) for name, t in cases(importlib.import_module("efg_amd.operators.gemm_" + arm)).items()}
            for arm in ARMS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write tests/golden/gemm_split_bits.json (see the module docstring)")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_gemm_split_bits.py runs the kernels: no device found")
    got = hashes()
    print(json.dumps(got, indent=1))
    if args.write:
        with open(args.out, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
    elif os.path.exists(args.out):
        with open(args.out) as f:
            want = json.load(f)
        bad = [(arm, name) for arm in ARMS for name in got[arm] if want[arm].get(name) != got[arm][name]]
        print("differs from %s: %s" % (os.path.relpath(args.out, ROOT), bad or "nothing"))
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
