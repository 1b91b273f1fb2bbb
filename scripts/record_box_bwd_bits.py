"""The bits of the encoder's tiled box-attention backward (csrc/box_fused.hip: box_bwd_tile_a_kernel, box_bwd_tile_b_kernel,
the binned far corners) on fixed inputs.  GPU box.

  python scripts/record_box_bwd_bits.py            print the SHA-256 of every case's gradients, compare with the fixture
  python scripts/record_box_bwd_bits.py --write    and write them to tests/golden/box_bwd_bits.json

tests/golden/box_bwd_bits.json was written ONCE, by the build of commit 6fe29a6, the last one that held the backward a third
time as ONE kernel (box_bwd_tile_kernel, behind EFG_BOX_SPLIT=0).  --write runs every case under EFG_BOX_SPLIT=0 and under
EFG_BOX_SPLIT=1 (that build reads the switch per call) and refuses to write unless the two forms give the same hash for every
output: what tests/test_box_fused_gpu.py::test_split_backward_bits_equal_one_kernel asserted, made once, on that build.  Later
builds have no such switch; tests/test_box_bwd_bits_gpu.py holds them to the fixture: same operations in the same order, same
guards, the same corners in the same bins.  A change that moves a hash changed the arithmetic; the fixture is not re-recorded
to follow it.  The softmax goes through expf, and `rot` through cosf and sinf, of the device library, so the fixture belongs
to the ROCm release it names ("rocm").

Everything goes through operators.box_attention_func.BoxAttnFusedFunction, not through Box3dAttention, whose Linear layers
run GEMM arms that are not the subject.  heads = 8, d = 32, one level, the 5 x 5 lattice.  Inputs are integer arithmetic on
torch.arange (no random generator, no module weights); queries are the cells of the map, anchors square with a side of `size`
of the map.  The offsets of a case are uniform in its own per-column range (`lo`, `hi`: dx, dy, dl, dw, dangle), chosen so
that the share of bilinear corners outside the 12 x 16 window of their query's 4 x 8 tile -- computed on the CPU from
box_sampling_grid, over the corners that lie on the map -- is what the case is for:

  near   2 x 44 x 52, size 0.08, separate offsets / logits    share 0: the pure window path; 77 tiles on a 64-workgroup launch,
                                                               so pass A strides over tiles
  rot    same map, 5 variables, ONE shared matrix (stride 240) 0 < share < 0.2: rotation (anchor angle in [0, 1) turns), strided
                                                               rows, a few binned corners
  big    same map, size 0.4, shared matrix (stride 232)        share > 0.5: most corners binned
  wide   1 x 90 x 142, size 0.08, separate                     share 0; 23 x 18 tiles put 72, 72 and 63 tiles into the colour
                                                               classes of pass B against its 64-workgroup launch: its tile loop
                                                               runs twice in some classes and once in others.  0.08 of 142 cells
                                                               is 11.4 cells, whose lattice would leave the window, so the size
                                                               offsets are negative here (boxes of 0.5 to 0.75 of their anchor)
All four maps are ragged in x (52 and 142 are no multiple of 8), `wide` in y too (90 = 22 * 4 + 2)."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "box_bwd_bits.json")
RECORDED_AT = "6fe29a6"
HEADS, D, KSIZE = 8, 32, 5
P = KSIZE * KSIZE
TQY, TQX, R = 4, 8, 4              # csrc/box_fused.hip: the query tile and the halo of its window
_MOD = 16777213                    # the largest prime under 2^24: v / 2^24 is an exact fp32 number

# case -> batch, map, anchor side, per-column offset range, one shared [logits | offsets] matrix, the far-corner share it must have
CASES = {
    "near": dict(b=2, hw=(44, 52), size=0.08, lo=(-1, -1, -1, -1), hi=(1, 1, 1, 1), shared=False, share=lambda f: f == 0.0),
    "rot": dict(b=2, hw=(44, 52), size=0.08, lo=(-4, -4, 0, 0, -1), hi=(4, 4, 10, 10, 1), shared=True, share=lambda f: 0.0 < f < 0.2),
    "big": dict(b=2, hw=(44, 52), size=0.4, lo=(-1, -1, 0, 0), hi=(1, 1, 4, 4), shared=True, share=lambda f: f > 0.5),
    "wide": dict(b=1, hw=(90, 142), size=0.08, lo=(-0.25, -0.25, -4, -4), hi=(0.25, 0.25, -2, -2), shared=False,
                 share=lambda f: f == 0.0),
}


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


def lattice():
    k = torch.arange(-(KSIZE // 2), KSIZE // 2 + 1, dtype=torch.float32) / KSIZE
    ky, kx = torch.meshgrid(k, k, indexing="ij")
    return torch.stack((kx, ky), -1).reshape(-1, 2).contiguous()


def inputs(name):
    """Host tensors of one case: value, shapes, start, ref, offsets [b, S, heads * nvar], logits [b, S, heads * P], lattice,
    grad_out."""
    c = CASES[name]
    salt = 100 * (1 + sorted(CASES).index(name))
    b, (H, W), nvar = c["b"], c["hw"], len(c["lo"])
    S = H * W
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    ref = torch.zeros(b, S, 7)
    ref[..., 0], ref[..., 1] = (xs / W).reshape(-1), (ys / H).reshape(-1)
    ref[..., 2] = ref[..., 5] = 0.5
    ref[..., 3] = ref[..., 4] = c["size"]
    if nvar == 5:
        ref[..., 6] = unit((b, S), salt + 1)
    lo, hi = torch.tensor(c["lo"], dtype=torch.float32), torch.tensor(c["hi"], dtype=torch.float32)
    offsets = (lo + unit((b, S, HEADS, nvar), salt + 2) * (hi - lo)).view(b, S, HEADS * nvar)
    logits = unit((b, S, HEADS * P), salt + 3) * 6 - 3
    value = unit((b, S, HEADS, D), salt + 4) * 2 - 1
    gout = unit((b, S, HEADS * D), salt + 5) * 2 - 1
    return value, torch.tensor([[H, W]]), torch.zeros(1, dtype=torch.int64), ref, offsets, logits, lattice(), gout


def far_share(name):
    """Share of the bilinear corners on the map that lie outside the window of their query's tile (CPU)."""
    from efg_amd.operators.box_attention_func import box_sampling_grid

    c = CASES[name]
    (H, W), nvar = c["hw"], len(c["lo"])
    _, _, _, ref, offsets, _, kidx, _ = inputs(name)
    grid = box_sampling_grid(ref, offsets, kidx, HEADS, 1, nvar == 5)       # [b, S, heads, 1, P, 2]
    px, py = grid[..., 0] * W - 0.5, grid[..., 1] * H - 0.5
    inside = (py > -1) & (px > -1) & (py < H) & (px < W)
    q = torch.arange(H * W)
    wx0 = ((q % W) // TQX * TQX - R).view(1, -1, 1, 1, 1)
    wy0 = ((q // W) // TQY * TQY - R).view(1, -1, 1, 1, 1)
    on_map = far = 0
    for dy in (0, 1):
        for dx in (0, 1):
            cy, cx = torch.floor(py) + dy, torch.floor(px) + dx
            ok = inside & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
            in_win = (cy >= wy0) & (cy < wy0 + TQY + 2 * R) & (cx >= wx0) & (cx < wx0 + TQX + 2 * R)
            on_map += int(ok.sum())
            far += int((ok & ~in_win).sum())
    return far / on_map


def run(name, dev):
    """{output: gradient tensor} of one case."""
    from efg_amd.operators.box_attention_func import BoxAttnFusedFunction

    c = CASES[name]
    nvar = len(c["lo"])
    value, shapes, start, ref, offsets, logits, kidx, gout = (t.to(dev) for t in inputs(name))
    value.requires_grad_(True)
    if c["shared"]:
        lo = torch.cat((logits, offsets), -1).contiguous().requires_grad_(True)
        assert lo.shape[-1] == HEADS * (P + nvar)
        BoxAttnFusedFunction.apply(value, shapes, start, ref, lo, None, kidx, nvar).backward(gout)
        return {"grad_value": value.grad, "grad_logits_offsets": lo.grad}
    offsets.requires_grad_(True)
    logits.requires_grad_(True)
    BoxAttnFusedFunction.apply(value, shapes, start, ref, offsets, logits, kidx, nvar).backward(gout)
    return {"grad_value": value.grad, "grad_offsets": offsets.grad, "grad_logits": logits.grad}


def hashes():
    """{case: {output: sha256}}; a binned entry that does not fit its bin raises (box_attention_func._CHECK_BINS)."""
    import efg_amd.operators.box_attention_func as baf

    dev = torch.device("cuda")
    old, baf._CHECK_BINS = baf._CHECK_BINS, True
    try:
        out = {name: {k: sha(t) for k, t in run(name, dev).items()} for name in CASES}
        torch.cuda.synchronize()
        return out
    finally:
        baf._CHECK_BINS = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write tests/golden/box_bwd_bits.json (see the module docstring)")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    shares = {name: far_share(name) for name in CASES}
    print("far-corner shares: %s" % json.dumps(shares))
    for name, f in shares.items():
        assert CASES[name]["share"](f), "case %s: far-corner share %.4f is not what the case is for" % (name, f)
    if not torch.cuda.is_available():
        raise SystemExit("record_box_bwd_bits.py runs the kernels: no device found")
    if args.write:
        forms = {}
        for split in ("0", "1"):     # the one-kernel form, then the two-kernel form
            os.environ["EFG_BOX_SPLIT"] = split
            forms[split] = hashes()
        del os.environ["EFG_BOX_SPLIT"]
        if forms["0"] != forms["1"]:
            print(json.dumps(forms, indent=1))
            raise SystemExit("the one-kernel and the two-kernel form differ: nothing written")
        print("EFG_BOX_SPLIT=0 and EFG_BOX_SPLIT=1 give the same hashes")
    got = {"recorded_at": RECORDED_AT, "rocm": torch.version.hip, "far_corner_share": shares, "hashes": hashes()}
    print(json.dumps(got, indent=1))
    if args.write:
        assert got["hashes"] == forms["1"]
        with open(args.out, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
    elif os.path.exists(args.out):
        with open(args.out) as f:
            want = json.load(f)["hashes"]
        bad = [(c, k) for c in got["hashes"] for k in got["hashes"][c] if want.get(c, {}).get(k) != got["hashes"][c][k]]
        print("differs from %s: %s" % (os.path.relpath(args.out, ROOT), bad or "nothing"))
        return 1 if bad else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
