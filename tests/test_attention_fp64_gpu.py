"""GPU: the six kernels of csrc/attention.hip -- attn_fwd_kernel, attn_bwd_dq_kernel, attn_bwd_dkv_kernel (at most 128 tokens,
64-wide heads) and attn_long_fwd_kernel, attn_long_bwd_dq_kernel, attn_long_bwd_dkv_kernel (any length, 32-wide heads, bit-packed
mask) -- against the float64 op of tests/fp64_ref.py (attention_fp64), element by element: out, lse, dq, dk and dv each satisfy
|got - ref| <= c (sqrt(n) 2^-24 |terms| + cond) (fp64_ref.assert_elementwise), so a head 1e-6 of its neighbour is held to its own
size.  The cases, the masks and the constant c = 4 are those of tests/attention_fp64_cases.py; tests/test_attention_fp64_ref.py
holds the fp32 torch composite to the same bars on the same inputs.

Every case runs through the wrappers (_SelfAttention.apply, cross_attention_kv, long_self_attention with pack_mask) and once more
through the C ABI, which also returns the log-sum-exp.  At the C ABI the operands are also laid out with padded rows (row stride
heads * D + 8 floats, one spare row per batch, every padding float NaN on the way in and on the way out).

Largest err / bound at c = 4 measured on MI355X, per kernel and tensor (`normal`: the unmasked cases of the normal family;
`other`: the other families and every masked case), next to the fp32 torch composite's figure on the same cases:
                                               normal                      other
    attn_fwd_kernel           out   0.20   (composite 0.17)    0.31   (0.26)   self_33_offset
                              lse   0.24   (0.23)              0.27   (0.21)   self_33_offset
    attn_bwd_dq_kernel        dq    0.13   (0.13)              0.21   (0.17)   self_128_offset
    attn_bwd_dkv_kernel       dk    0.14   (0.11)              0.22   (0.19)   self_33_offset
                              dv    0.20   (0.16)              0.36   (0.36)   self_33_offset
    attn_long_fwd_kernel      out   0.14   (0.14)              0.20   (0.26)   long_333_twin_keys
                              lse   0.18   (0.18)              0.29   (0.24)   long_dn_blocks_sharp
    attn_long_bwd_dq_kernel   dq    0.11   (0.088)             0.17   (0.16)   long_333_twin_keys
    attn_long_bwd_dkv_kernel  dk    0.11   (0.093)             0.14   (0.18)   long_128_offset
                              dv    0.17   (0.16)              0.29   (0.29)   long_128_offset
(the last column names the case of the `other` figure).  No kernel needs more than 0.36 of the bar, and each stands within a
factor of 1.3 of the plain fp32 evaluation's figure; the `offset` family, whose logits of 112 .. 159 put the rounding of the folded
scale * log2(e) and of the dK / dV kernel's recomputed S on show, is the worst of both."""
import math

import pytest
import torch

import attention_fp64_cases as AC
from attention_fp64_cases import CASES, MASKS, bhsd, build, check, reference

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _split(t, heads):
    """[B, S, H * D] -> the [B, H, S, D] view."""
    b, s, c = t.shape
    return bhsd(t.reshape(b, s, heads, c // heads))


def _flat(t):
    b, s, h, d = t.shape
    return t.reshape(b, s, h * d)


def _through_wrapper(case, dev):
    """out, dq, dk, dv [B, H, S, D] of the case through the autograd wrappers of efg_amd.operators.attention."""
    from efg_amd.operators import attention as A

    h = case["heads"]
    q, k, v, go = (_flat(case[n]).to(dev) for n in ("q", "k", "v", "grad_out"))
    if case["kind"] == "short_self":
        qkv = torch.cat([q, k, v], -1).requires_grad_(True)
        assert A.fused(qkv, h)
        out = A._SelfAttention.apply(qkv, h)
        out.backward(go)
        grads = qkv.grad.chunk(3, -1)
    elif case["kind"] == "short_cross":
        q = q.requires_grad_(True)
        kv = torch.cat([k, v], -1).requires_grad_(True)
        assert A.fused_cross(q, kv, h)
        out = A.cross_attention_kv(q, kv, h)
        out.backward(go)
        grads = (q.grad,) + tuple(kv.grad.chunk(2, -1))
    else:
        qk = torch.cat([q, k], -1).requires_grad_(True)
        v = v.requires_grad_(True)
        assert A.fused_long(v, h)
        bits = A.pack_mask(None if case["mask"] is None else case["mask"].to(dev))
        out = A.long_self_attention(qk, v, bits, h)
        out.backward(go)
        grads = tuple(qk.grad.chunk(2, -1)) + (v.grad,)
    torch.cuda.synchronize()
    return dict(out=_split(out.detach(), h), dq=_split(grads[0], h), dk=_split(grads[1], h), dv=_split(grads[2], h))


def _padded(t, pad, dev):
    """[B, S, H, D] -> a [B, S + 1, H * D + pad] buffer (pad = 0: [B, S, H * D]) holding t, every other float NaN."""
    b, s, h, d = t.shape
    if not pad:
        return _flat(t).to(dev).contiguous()
    buf = torch.full((b, s + 1, h * d + pad), NAN, device=dev)
    buf[:, :s, :h * d] = _flat(t).to(dev)
    return buf


def _through_abi(case, dev, pad=0):
    """The C ABI itself on separate q / k / v buffers with `pad` spare floats per row (and one spare row per batch when pad > 0);
    dq / dk / dv buffers of the same layout pre-filled with NaN.  Returns out [B, Sq, C], lse [B, H, Sq] and the three gradient
    BUFFERS."""
    from efg_amd import _lib as L
    from efg_amd.operators.attention import pack_mask

    h, scale = case["heads"], case["scale"]
    b, sq, _, d = case["q"].shape
    sk = case["k"].shape[1]
    qb, kb, vb = (_padded(case[n], pad, dev) for n in ("q", "k", "v"))
    go = _flat(case["grad_out"]).to(dev).contiguous()
    out = torch.full((b, sq, h * d), NAN, device=dev)
    lse = torch.full((b, h, sq), NAN, device=dev)
    dq, dk, dv = (torch.full_like(t, NAN) for t in (qb, kb, vb))
    strides = lambda t: (t.stride(0), t.stride(1))   # noqa: E731
    lib = L.lib()
    if case["kind"] == "long":
        bits = pack_mask(None if case["mask"] is None else case["mask"].to(dev))
        words = 0 if bits is None else bits.shape[1]
        ops = (qb.data_ptr(), *strides(qb), kb.data_ptr(), *strides(kb), vb.data_ptr(), *strides(vb), L.ptr(bits), words)
        L.check(lib.efg_attention_long_fwd_f32(*ops, b, sq, h, scale, L.ptr(out), L.ptr(lse), L.stream()))
        ws = torch.empty_like(lse)
        L.check(lib.efg_attention_long_bwd_f32(*ops, L.ptr(out), L.ptr(lse), L.ptr(go), b, sq, h, scale, dq.data_ptr(), dk.data_ptr(),
                                               dv.data_ptr(), L.ptr(ws), L.stream()))
    else:
        assert strides(kb) == strides(vb)
        ops = (qb.data_ptr(), *strides(qb), kb.data_ptr(), vb.data_ptr(), *strides(kb))
        L.check(lib.efg_attention_fwd_f32(*ops, b, sq, sk, h, scale, L.ptr(out), L.ptr(lse), L.stream()))
        L.check(lib.efg_attention_bwd_f32(*ops, L.ptr(out), L.ptr(lse), L.ptr(go), b, sq, sk, h, scale, dq.data_ptr(), dk.data_ptr(),
                                          dv.data_ptr(), L.stream()))
    torch.cuda.synchronize()
    return out, lse, dq, dk, dv


def _inner(buf, like):
    """The (b, row < seq, h, d) part of a gradient buffer as [B, H, S, D], and the rest of the buffer (the padding floats)."""
    b, s, h, d = like.shape
    part = bhsd(buf[:, :s, :h * d].reshape(b, s, h, d))
    rest = torch.ones_like(buf, dtype=torch.bool)
    rest[:, :s, :h * d] = False
    return part, buf[rest]


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_fp64(dev, name):
    case = build(name)
    got = _through_wrapper(case, dev)
    check(name, got)
    out, lse, dq, dk, dv = _through_abi(case, dev)
    h = case["heads"]
    assert torch.equal(_split(out, h), got["out"]), "the C ABI's out differs from the wrapper's"
    check(name, {"lse": lse}, tag=" (C ABI)")      # -inf exactly for a query with no allowed key
    for key, buf in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.equal(_split(buf, h), got[key]), key
    if case["mask"] is not None and MASKS[CASES[name]["mask"]][0] <= 129:
        from efg_amd.operators.attention import pack_mask

        words = (pack_mask(case["mask"].to(dev)).cpu().to(torch.int64) & 0xFFFFFFFF).tolist()
        assert words == AC.mask_words(case["mask"])


@pytest.mark.parametrize("name", ["long_dead_rows", "long_dead_rows_head_scales"])
def test_queries_without_an_allowed_key(dev, name):
    """out and dq of such a query are exactly 0 and WRITTEN (the buffers start as NaN), lse is -inf, every gradient is finite, and
    dk / dv stand within the bars of a reference to which these queries contribute nothing."""
    case, ref = build(name), reference(name)
    dead = ~ref["live"]
    assert int(dead.sum()) == len(MASKS["dead_rows"][1])
    out, lse, dq, dk, dv = _through_abi(case, dev)
    h = case["heads"]
    out, dq, dk, dv = (_split(t, h).cpu() for t in (out, dq, dk, dv))
    for t in (out, dq, dk, dv):
        assert bool(torch.isfinite(t).all())
    assert bool((out[:, :, dead] == 0).all()) and bool((dq[:, :, dead] == 0).all())
    assert bool((lse.cpu()[:, :, dead] == -math.inf).all()) and bool(torch.isfinite(lse.cpu()[:, :, ~dead]).all())
    check(name, dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), tag=" (C ABI)")
    wrapped = _through_wrapper(case, dev)
    assert bool((wrapped["out"].cpu()[:, :, dead] == 0).all()) and bool((wrapped["dq"].cpu()[:, :, dead] == 0).all())
    for t in wrapped.values():
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("name", ["self_33", "cross_17x127", "cross_65x31", "long_late_start", "long_65"])
def test_padded_strides(dev, name):
    """Row stride heads * D + 8 floats, batch stride one row more than needed: every (b, row < seq, h, d) element is written and
    within the bars, every padding float of dq / dk / dv is still NaN, and the results have the bits of the contiguous call."""
    case = build(name)
    plain = _through_abi(case, dev)
    out, lse, dq, dk, dv = _through_abi(case, dev, pad=8)
    assert dq.stride(1) == case["heads"] * case["q"].shape[3] + 8 and dq.stride(0) == (case["q"].shape[1] + 1) * dq.stride(1)
    h = case["heads"]
    got = dict(out=_split(out, h), lse=lse)
    for key, buf, like in (("dq", dq, case["q"]), ("dk", dk, case["k"]), ("dv", dv, case["v"])):
        got[key], rest = _inner(buf, like)
        assert rest.numel() > 0 and bool(torch.isnan(rest).all()), "%s: a padding float was written" % key
        assert bool(torch.isfinite(got[key]).all()), "%s: an element of the sub-array was not written" % key
    check(name, got, tag=" (padded)")
    assert torch.equal(out, plain[0]) and torch.equal(lse, plain[1])
    for key, buf in zip(("dq", "dk", "dv"), plain[2:]):
        assert torch.equal(got[key], _split(buf, h)), key


@pytest.mark.parametrize("name", ["long_half_random", "self_100"])
def test_two_calls_give_the_same_bits(dev, name):
    case = build(name)
    first, second = _through_abi(case, dev), _through_abi(case, dev)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("what,message", [("batch_heads", "batch x heads must be < 65536"),
                                          ("mask_words", "mask rows need ceil(s / 32) words"),
                                          ("stride", "strides must be multiples of 4 floats")])
def test_refused_long_calls_leave_the_outputs_alone(dev, what, message):
    """batch * heads = 65536, mask_words = ceil(s / 32) - 1 and a row stride of 6 floats: non-zero, check_long's message in
    efg_last_error(), and the pre-filled outputs keep every element.  The buffers have the full size of the call all the same."""
    from efg_amd import _lib as L

    b, s, h = (65536, 1, 1) if what == "batch_heads" else (1, 65, 2)
    c = h * 32
    q, k, v, go = (torch.randn(b, s, c, device=dev) for _ in range(4))
    words = (s + 31) // 32
    bits = torch.zeros(s, words, dtype=torch.int32, device=dev)
    row = 6 if what == "stride" else c
    ops = (L.ptr(q), s * c, row, L.ptr(k), s * c, c, L.ptr(v), s * c, c, L.ptr(bits), words - 1 if what == "mask_words" else words)
    out, lse = torch.full((b, s, c), 7.0, device=dev), torch.full((b, h, s), 7.0, device=dev)
    lib = L.lib()
    rc = lib.efg_attention_long_fwd_f32(*ops, b, s, h, 32 ** -0.5, L.ptr(out), L.ptr(lse), L.stream())
    assert rc != 0 and message in lib.efg_last_error().decode()
    assert "attention_long_fwd" in lib.efg_last_error().decode()
    dq, dk, dv, ws = (torch.full_like(t, 7.0) for t in (q, k, v, lse))
    rc = lib.efg_attention_long_bwd_f32(*ops, L.ptr(out), L.ptr(lse), L.ptr(go), b, s, h, 32 ** -0.5, L.ptr(dq), L.ptr(dk), L.ptr(dv),
                                        L.ptr(ws), L.stream())
    assert rc != 0 and message in lib.efg_last_error().decode()
    assert "attention_long_bwd" in lib.efg_last_error().decode()
    torch.cuda.synchronize()
    for t in (out, lse, dq, dk, dv, ws):
        assert bool((t == 7.0).all())
