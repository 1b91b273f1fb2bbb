"""Inputs of the per-element float64 tests of the attention kernels of csrc/attention.hip (test_attention_fp64_ref.py on the CPU,
test_attention_fp64_gpu.py on the device): named, seeded case builders (CPU generators), the float64 reference of each case
(fp64_ref.attention_fp64, computed once per process) and the comparison.  No test in here.

A case is a dict: q, grad_out [B, Sq, H, D] and k, v [B, Sk, H, D] float32 on the CPU (the memory order of the kernels' operands;
`bhsd` gives the [B, H, S, D] views the reference takes), mask bool [S, S] (True = not attended) or None, scale = 1 / sqrt(D), and
`kind`: short_self / short_cross (attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel: D = 64, at most 128 tokens) or long
(attn_long_*_kernel: D = 32, any length, optional mask).

Value families:
    normal       randn * 1.5 (grad_out randn), the inputs of tests/test_attention_gpu.py
    head_scales  q, k log-uniform in [0.05, 4]; v and grad_out log-uniform in [0.1, 10] times a per-head factor from
                 {1, 1e-6, 1e2, 1e-3} (v) and {1, 1e-6, 1e-3, 1e2} (grad_out): head 1 is 1e-6 of head 0 in both
    sharp        q, k randn * 6: rows are near one-hot, most exponents lie below -126 (the flush to zero)
    offset       randn * 1.5 plus one shared vector of length 30 on q and k: every logit carries 900 * scale (112 or 159) that the
                 max / log-sum-exp subtraction has to cancel
    zero_q       q = 0: uniform probabilities over the allowed keys
    twin_keys    keys and values 2 i + 1 are copies of 2 i

Lengths of the short kernels (waves own 32 queries or keys, tiles are 16 wide): every tile edge from 1 to 128 for self-attention,
six (sq, sk) pairs for cross-attention.  Lengths of the long kernels (a wave owns 16 queries, a workgroup 64, key blocks are 128
wide, mask words 32): every edge from 1 to 333.  The masks of the long cases are described at `MASKS`; the CPU test asserts
each structural property, so a later edit cannot quietly turn one into another random mask."""
import functools
import math

import torch

from fp64_ref import assert_elementwise, attention_fp64, log_uniform_signed

# The rounding constant of assert_elementwise for every tensor: the value of the msda and norm suites.  It multiplies the
# conditioning allowance too (see `check_against`).  COMPOSITE_WORST: the largest err / bound at this c of the fp32 torch composite
# (matmul / softmax / autograd in fp32, tests/test_attention_fp64_ref.py, which printed these figures) per group of cases --
# the kernels a case runs on (short: 64-wide heads, at most 128 tokens; long: 32-wide heads) and `normal` (the unmasked cases of
# the normal family) or `other` (the other families and every masked case).  The MI355X figures of the kernels are in the
# docstring of tests/test_attention_fp64_gpu.py.
C = 4
COMPOSITE_WORST = {"short normal": dict(out=0.174, lse=0.233, dq=0.133, dk=0.107, dv=0.163),
                   "short other": dict(out=0.260, lse=0.209, dq=0.172, dk=0.185, dv=0.360),
                   "long normal": dict(out=0.143, lse=0.184, dq=0.088, dk=0.093, dv=0.161),
                   "long other": dict(out=0.261, lse=0.237, dq=0.159, dk=0.182, dv=0.293)}
TENSORS = ("out", "lse", "dq", "dk", "dv")
V_HEAD_SCALES = (1.0, 1e-6, 1e2, 1e-3)
G_HEAD_SCALES = (1.0, 1e-6, 1e-3, 1e2)
SMALL_HEAD = 1              # the head at 1e-6 of head 0 in the head_scales family
FAMILIES = ("normal", "head_scales", "sharp", "offset", "zero_q", "twin_keys")

SELF_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 65, 100, 127, 128)
CROSS_LENGTHS = ((1, 128), (5, 77), (128, 16), (33, 1), (17, 127), (65, 31))
LONG_LENGTHS = (1, 5, 63, 64, 65, 127, 128, 129, 257, 333)
WAVE_Q, GROUP_Q, KEY_BLOCK = 16, 64, 128      # attn_long_*: queries per wave and per workgroup, keys per block

# name -> (s, dead rows).  True = not attended.
#   dn_blocks      groups A = [0, 128), B = [128, 256), C = [256, 320): A sees A, B sees A and B, C sees B and C.  Every (16-query
#                  wave x 128-key block) tile is fully allowed or fully forbidden; blocks 0 and 1 lie inside the sequence, so
#                  the allowed ones take the `plain` path WITH a mask present, and C's block 0 is forbidden before its first
#                  allowed key (the m_new == -inf branch)
#   late_start     10 % random holes; queries >= 256 see no key below 128
#   last_key_only  every query sees only key s - 1: key 128 at s = 129 (bit 0 of word 4, alone in the ragged second block) and
#                  key 127 at s = 128 (the last bit of the last word of the only block)
#   bit31, bit32   the only allowed key is 31 (word 0 = 0x7fffffff) / 32 (word 0 = 0xffffffff: the sign bit of the packed int32)
#   half_random    50 % random
#   dead_rows      10 % random holes and six queries with no allowed key, each in a wave with live queries; 332 lies in the last,
#                  ragged workgroup (queries 320 .. 332)
MASKS = {"dn_blocks": (320, ()), "late_start": (333, ()), "last_key_only": (129, ()), "last_key_only_128": (128, ()),
         "bit31": (129, ()), "bit32": (129, ()), "half_random": (333, ()), "dead_rows": (333, (3, 17, 64, 200, 255, 332))}

CASES = {}


def _add(name, kind, b, h, sq, sk, family="normal", mask=None):
    CASES[name] = dict(name=name, kind=kind, b=b, h=h, sq=sq, sk=sk, d=32 if kind == "long" else 64, family=family, mask=mask,
                       seed=4000 + len(CASES))


for _s in SELF_LENGTHS:
    _add("self_%d" % _s, "short_self", 2, 2, _s, _s)
for _sq, _sk in CROSS_LENGTHS:
    _add("cross_%dx%d" % (_sq, _sk), "short_cross", 2, 2, _sq, _sk)
for _f in FAMILIES[1:]:
    for _s in (128, 33):
        _add("self_%d_%s" % (_s, _f), "short_self", 1 if _f != "head_scales" else 2, 4 if _f == "head_scales" else 2, _s, _s, _f)
    _add("cross_17x127_%s" % _f, "short_cross", 1, 4 if _f == "head_scales" else 2, 17, 127, _f)
for _s in LONG_LENGTHS:
    _add("long_%d" % _s, "long", 2 if _s < 200 else 1, 3, _s, _s)
for _f in FAMILIES[1:]:
    for _s in (128, 333):
        _add("long_%d_%s" % (_s, _f), "long", 1, 4 if _f == "head_scales" else 2, _s, _s, _f)
for _m, (_s, _) in MASKS.items():
    _add("long_%s" % _m, "long", 2, 2, _s, _s, mask=_m)
_add("long_dead_rows_head_scales", "long", 1, 4, 333, 333, "head_scales", mask="dead_rows")
_add("long_dn_blocks_sharp", "long", 1, 2, 320, 320, "sharp", mask="dn_blocks")

SHORT_SELF = [n for n, c in CASES.items() if c["kind"] == "short_self"]
SHORT_CROSS = [n for n, c in CASES.items() if c["kind"] == "short_cross"]
LONG = [n for n, c in CASES.items() if c["kind"] == "long"]
NORMAL = [n for n, c in CASES.items() if c["family"] == "normal"]


def group_of(name):
    """The row of COMPOSITE_WORST (and of the measured table of the GPU test) a case belongs to."""
    spec = CASES[name]
    return "%s %s" % ("long" if spec["kind"] == "long" else "short",
                      "normal" if spec["family"] == "normal" and not spec["mask"] else "other")


def make_mask(name, gen):
    s, dead = MASKS[name]
    if name == "dn_blocks":
        grp = torch.arange(s) // KEY_BLOCK
        return ~((grp[:, None] == grp[None, :]) | (grp[:, None] == grp[None, :] + 1))
    if name in ("late_start", "dead_rows"):
        mask = torch.rand(s, s, generator=gen) < 0.1
        mask[torch.arange(s), torch.arange(s)] = False
        if name == "late_start":
            mask[256:, :KEY_BLOCK] = True
        for r in dead:
            mask[r] = True
        return mask
    if name == "half_random":
        return torch.rand(s, s, generator=gen) < 0.5
    only = {"last_key_only": s - 1, "last_key_only_128": s - 1, "bit31": 31, "bit32": 32}[name]
    mask = torch.ones(s, s, dtype=torch.bool)
    mask[:, only] = False
    return mask


def mask_words(mask):
    """The bit rule of the kernels, written out: word key >> 5 of a query's row holds bit key & 31 = 1 for a key that is NOT
    attended; [S][ceil(S / 32)] Python ints in [0, 2^32)."""
    s = mask.shape[1]
    rows = []
    for r in mask.tolist():
        words = [0] * ((s + 31) // 32)
        for key, bit in enumerate(r):
            if bit:
                words[key >> 5] |= 1 << (key & 31)
        rows.append(words)
    return rows


@functools.lru_cache(maxsize=None)
def build(name):
    """The case `name` (see the module docstring).  Built once per process; nobody writes into its tensors."""
    spec = CASES[name]
    gen = torch.Generator().manual_seed(spec["seed"])
    b, h, sq, sk, d, fam = spec["b"], spec["h"], spec["sq"], spec["sk"], spec["d"], spec["family"]
    qs, ks = (b, sq, h, d), (b, sk, h, d)
    if fam == "head_scales":
        q, k = log_uniform_signed(qs, 0.05, 4.0, gen), log_uniform_signed(ks, 0.05, 4.0, gen)
        v = log_uniform_signed(ks, 0.1, 10.0, gen) * torch.tensor(V_HEAD_SCALES[:h]).view(1, 1, h, 1)
        go = log_uniform_signed(qs, 0.1, 10.0, gen) * torch.tensor(G_HEAD_SCALES[:h]).view(1, 1, h, 1)
    else:
        mul = 6.0 if fam == "sharp" else 1.5
        q, k = torch.randn(qs, generator=gen) * mul, torch.randn(ks, generator=gen) * mul
        v, go = torch.randn(ks, generator=gen) * 1.5, torch.randn(qs, generator=gen)
        if fam == "offset":
            unit = torch.randn(d, generator=gen)
            unit = 30.0 * unit / unit.norm()
            q, k = q + unit, k + unit
        elif fam == "zero_q":
            q = torch.zeros(qs)
        elif fam == "twin_keys":
            k[:, 1::2] = k[:, 0:2 * (sk // 2):2]
            v[:, 1::2] = v[:, 0:2 * (sk // 2):2]
    mask = make_mask(spec["mask"], gen) if spec["mask"] else None
    return dict(name=name, kind=spec["kind"], family=fam, q=q.contiguous(), k=k.contiguous(), v=v.contiguous(),
                grad_out=go.contiguous(), mask=mask, scale=1.0 / math.sqrt(d), heads=h)


def bhsd(t):
    """[B, S, H, D] -> the [B, H, S, D] view."""
    return t.permute(0, 2, 1, 3)


def reference_of(case):
    return attention_fp64(bhsd(case["q"]), bhsd(case["k"]), bhsd(case["v"]), bhsd(case["grad_out"]), case["scale"], case["mask"])


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(build(name))


def check_against(tag, ref, got, c=C):
    """assert_elementwise for every tensor of `got` (a dict over TENSORS or a part of them; out, dq, dk, dv as [B, H, S, D], lse
    as [B, H, Sq]).  The bar of an element is c (sqrt(n) 2^-24 |terms| + cond): attention_fp64's `_cond` is a root-sum-square like
    the first term, so it carries the same constant (the section comment in fp64_ref.py).  lse of a query with no allowed key must
    be -inf exactly and is left out of the bar.  Prints and returns the err / bound ratios."""
    ratios = {}
    for key, g in got.items():
        g = torch.as_tensor(g).detach().cpu()
        r64, cond = ref[key], ref[key + "_cond"]
        if key == "lse":
            dead = ~ref["live"]
            if bool(dead.any()):
                assert bool((g[:, :, dead] == -math.inf).all()), "%s lse: a query with no allowed key must have lse = -inf" % tag
                g, r64 = g.clone(), r64.clone()
                g[:, :, dead] = 0
                r64[:, :, dead] = 0
        ratios[key] = assert_elementwise("%s %s" % (tag, key), g, r64, ref[key + "_mag"], ref[key + "_n"], c, c * cond)
    print("%s: err/bound %s" % (tag, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    return ratios


def check(name, got, c=C, tag=""):
    """`got` against the reference of the case `name`; `tag` is appended to the name in messages."""
    return check_against(name + tag, reference(name), got, c)
