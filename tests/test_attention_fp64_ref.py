"""CPU: the float64 attention reference (fp64_ref.attention_fp64) and the cases of attention_fp64_cases.py, without a GPU.

    - the reference against hand-computed values and against float64 autograd of the same formula;
    - the cases are what their names say (mask structure, small heads, near one-hot rows);
    - the fp32 torch composite (matmul / softmax / autograd in fp32 on the case's inputs) passes every bar, and in the `normal`
      family its worst err / bound per tensor stays inside [0.02, 0.5]: the bars are neither vacuous nor razor-thin;
    - mutants of the composite that the max-norm criterion of tests/test_attention_gpu.py lets through fail the per-element bar."""
import math

import pytest
import torch

import attention_fp64_cases as AC
from attention_fp64_cases import CASES, MASKS, bhsd, build, check, reference
from fp64_ref import attention_fp64


# ---- the fp32 composite and the max-norm criterion of test_attention_gpu.py ----------------------------------------------------
def composite(case, dtype=torch.float32, scale_mul=1.0, mask="case"):
    """matmul / softmax / autograd in `dtype` on the case's inputs; a query with no allowed key gives zeros (the kernels'
    convention) and lse = -inf.  Returns out, lse, dq, dk, dv as [B, H, S, D] / [B, H, Sq]."""
    q, k, v = (bhsd(case[n]).to(dtype).detach().clone().requires_grad_(True) for n in ("q", "k", "v"))
    mask = case["mask"] if isinstance(mask, str) else mask
    logits = (q @ k.transpose(-1, -2)) * torch.tensor(case["scale"] * scale_mul, dtype=dtype)
    if mask is not None:
        logits = logits.masked_fill(mask, -math.inf)
    lse = torch.logsumexp(logits, -1)
    if mask is not None and bool(mask.all(1).any()):
        dead = mask.all(1).view(1, 1, -1, 1)
        p = torch.softmax(torch.where(dead, torch.zeros((), dtype=dtype), logits), -1) * (~dead).to(dtype)
    else:
        p = torch.softmax(logits, -1)
    out = p @ v
    out.backward(bhsd(case["grad_out"]).to(dtype))
    return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def old_criterion(case, got, comp, ref):
    """The assertions of tests/test_attention_gpu.py on the tensors it compares: out, and the gradients of the packed operands
    (qkv; q and kv; qk and v) -- max |got - ref| / max |ref| <= max(4 x the composite's, 2e-6 for out, 5e-6 for gradients).
    Returns the list of tensors that fail it."""
    groups = {"short_self": [("out",), ("dq", "dk", "dv")], "short_cross": [("out",), ("dq",), ("dk", "dv")],
              "long": [("out",), ("dq", "dk"), ("dv",)]}[case["kind"]]

    def err(side, keys):
        a = torch.cat([side[k].double().reshape(-1) for k in keys])
        r = torch.cat([ref[k].reshape(-1) for k in keys])
        return float((a - r).abs().max() / r.abs().max().clamp_min(1e-30))

    return [keys for keys in groups if not err(got, keys) <= max(4 * err(comp, keys), 2e-6 if keys == ("out",) else 5e-6)]


_COMPOSITES = {}


def composite_of(name):
    if name not in _COMPOSITES:
        _COMPOSITES[name] = composite(build(name))
    return _COMPOSITES[name]


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    """2 queries x 3 keys x d = 4, scale 1, pair (0, 2) masked.  Logits: query 0 -> (ln 2, 0, masked), query 1 -> (0, 0, ln 3), so
    p = [[2/3, 1/3, 0], [1/5, 1/5, 3/5]] and lse = (ln 3, ln 5)."""
    ln2, ln3 = math.log(2.0), math.log(3.0)
    q = torch.tensor([[ln2, 0, 0, 0], [0, ln3, 0, 0]], dtype=torch.float64).view(1, 1, 2, 4)
    k = torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0], [5, 1, 0, 0]], dtype=torch.float64).view(1, 1, 3, 4)
    v = torch.tensor([[3, 0, 15, 1], [6, 3, 0, 1], [100, 5, 10, 1]], dtype=torch.float64).view(1, 1, 3, 4)
    go = torch.tensor([[3, 0, 0, 1], [0, 5, 0, 1]], dtype=torch.float64).view(1, 1, 2, 4)
    mask = torch.tensor([[False, False, True], [False, False, False]])
    ref = attention_fp64(q, k, v, go, 1.0, mask)
    close = lambda a, b: torch.testing.assert_close(a.reshape(-1), torch.tensor(b, dtype=torch.float64), rtol=1e-14, atol=1e-14)   # noqa: E731
    # out_0 = 2/3 v_0 + 1/3 v_1 = (4, 1, 10, 1); out_1 = 1/5 v_0 + 1/5 v_1 + 3/5 v_2 = (61.8, 3.6, 9, 1)
    close(ref["out"], [4, 1, 10, 1, 61.8, 3.6, 9, 1])
    close(ref["lse"], [ln3, math.log(5.0)])
    # dv_j = sum_i p_ij dO_i: dv_0 = 2/3 (3,0,0,1) + 1/5 (0,5,0,1); dv_1 = 1/3 (3,0,0,1) + 1/5 (0,5,0,1); dv_2 = 3/5 (0,5,0,1)
    close(ref["dv"], [2, 1, 0, 2 / 3 + 0.2, 1, 1, 0, 1 / 3 + 0.2, 0, 3, 0, 0.6])
    # dP_0 = (10, 19, -), D_0 = 13, dS_0 = (2/3 (-3), 1/3 (6), 0) = (-2, 2, 0): dq_0 = -2 k_0 + 2 k_1 = (-2, 0, 0, 0)
    # dP_1 = (1, 16, 26), D_1 = 19, dS_1 = (1/5 (-18), 1/5 (-3), 3/5 (7)) = (-3.6, -0.6, 4.2): dq_1 = -3.6 k_0 + 4.2 k_2
    close(ref["dq"], [-2, 0, 0, 0, -3.6 + 21, 4.2, 0, 0])
    # dk_j = sum_i dS_ij q_i: dk_0 = -2 q_0 - 3.6 q_1, dk_1 = 2 q_0 - 0.6 q_1, dk_2 = 4.2 q_1
    close(ref["dk"], [-2 * ln2, -3.6 * ln3, 0, 0, 2 * ln2, -0.6 * ln3, 0, 0, 0, 4.2 * ln3, 0, 0])
    assert ref["out_n"].reshape(-1).tolist() == [2, 3] and ref["dv_n"].reshape(-1).tolist() == [2, 2, 1]
    # the masked pair carries no allowance, and every allowance is of the order of 2^-24 of its element
    for key in ("out", "dq", "dk", "dv"):
        assert bool((ref[key + "_cond"] <= 1e-5 * ref[key + "_mag"] + 1e-300).all())
        assert bool((ref[key + "_mag"] >= ref[key].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("name", ["cross_17x127", "long_dead_rows"])
def test_reference_matches_float64_autograd(name):
    case, ref = build(name), reference(name)
    auto = composite(case, torch.float64)
    for key in ("out", "dq", "dk", "dv"):
        torch.testing.assert_close(ref[key], auto[key], rtol=1e-11, atol=1e-13)
    live = ref["live"]
    torch.testing.assert_close(ref["lse"][:, :, live], auto["lse"][:, :, live], rtol=1e-12, atol=1e-12)
    assert bool((auto["lse"][:, :, ~live] == -math.inf).all()) and bool((ref["lse"][:, :, ~live] == -math.inf).all())


def test_dead_rows_contribute_nothing():
    """out, dq of a dead query are exactly 0 in the reference, and dk / dv equal those of the sequence without the dead queries'
    grad_out."""
    case, ref = build("long_dead_rows"), reference("long_dead_rows")
    dead = ~ref["live"]
    assert int(dead.sum()) == len(MASKS["dead_rows"][1])
    assert bool((ref["out"][:, :, dead] == 0).all()) and bool((ref["dq"][:, :, dead] == 0).all())
    go = case["grad_out"].clone()
    go[:, dead] = 0
    other = attention_fp64(bhsd(case["q"]), bhsd(case["k"]), bhsd(case["v"]), bhsd(go), case["scale"], case["mask"])
    assert torch.equal(other["dk"], ref["dk"]) and torch.equal(other["dv"], ref["dv"])


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def test_case_list():
    assert [CASES[n]["sq"] for n in AC.SHORT_SELF if CASES[n]["family"] == "normal"] == list(AC.SELF_LENGTHS)
    assert [(CASES[n]["sq"], CASES[n]["sk"]) for n in AC.SHORT_CROSS if CASES[n]["family"] == "normal"] == list(AC.CROSS_LENGTHS)
    assert [CASES[n]["sq"] for n in AC.LONG if CASES[n]["family"] == "normal" and not CASES[n]["mask"]] == list(AC.LONG_LENGTHS)
    for fam in AC.FAMILIES[1:]:
        for kind in ("short_self", "long"):
            lengths = {CASES[n]["sq"] for n in CASES if CASES[n]["family"] == fam and CASES[n]["kind"] == kind and not CASES[n]["mask"]}
            assert 128 in lengths and any(s % 16 for s in lengths), (fam, kind)
    for name, spec in CASES.items():
        assert 1 <= spec["b"] <= 3 and 1 <= spec["h"] <= 4
        assert spec["kind"] == "long" or (spec["sq"] <= 128 and spec["sk"] <= 128)
        assert (spec["mask"] is None) or MASKS[spec["mask"]][0] == spec["sq"]


def _mask(name):
    return build("long_" + name)["mask"]


def test_mask_dn_blocks():
    mask = _mask("dn_blocks")
    s = mask.shape[0]
    assert not bool(mask.diagonal().any())
    tiles = {"plain": 0, "forbidden": 0, "late": 0}
    for w0 in range(0, s, AC.WAVE_Q):
        seen = False
        for k0 in range(0, s, AC.KEY_BLOCK):
            tile = mask[w0:w0 + AC.WAVE_Q, k0:k0 + AC.KEY_BLOCK]
            assert bool(tile.all()) or not bool(tile.any()), "tile (%d, %d) is mixed" % (w0, k0)
            if bool(tile.all()):
                tiles["forbidden"] += 1
                tiles["late"] += not seen          # a forbidden block BEFORE the wave's first allowed key
            else:
                seen = True
                tiles["plain"] += k0 + AC.KEY_BLOCK <= s   # no mask bit, block inside the sequence: the kernels' fast path
    assert tiles["plain"] >= 8 and tiles["forbidden"] >= 8 and tiles["late"] >= 4, tiles


def test_mask_late_start_and_half_random():
    mask = _mask("late_start")
    assert mask.shape == (333, 333) and bool(mask[256:, :128].all()) and not bool(mask.all(1).any())
    assert not bool(mask[:256, :128].all(1).any())              # the others do see the first block
    frac = float(mask[:256].float().mean())
    assert 0.08 < frac < 0.12
    half = _mask("half_random")
    assert half.shape == (333, 333) and 0.48 < float(half.float().mean()) < 0.52 and not bool(half.all(1).any())


@pytest.mark.parametrize("name,key", [("last_key_only", 128), ("last_key_only_128", 127), ("bit31", 31), ("bit32", 32)])
def test_mask_single_key(name, key):
    mask = _mask(name)
    s = MASKS[name][0]
    assert mask.shape == (s, s)
    assert bool((~mask).sum(1).eq(1).all()) and not bool(mask[:, key].any())
    if name.startswith("last_key_only"):
        assert key == s - 1
    words = AC.mask_words(mask)
    full = 0xFFFFFFFF
    expect = [full] * ((s + 31) // 32)
    expect[-1] = (1 << (s - 32 * (len(expect) - 1))) - 1         # bits of keys >= s stay 0
    expect[key >> 5] &= ~(1 << (key & 31)) & full
    assert all(row == expect for row in words)
    if name == "bit31":
        assert expect[0] == 0x7FFFFFFF
    if name == "bit32":
        assert expect[0] == full and expect[1] == 0xFFFFFFFE      # word 0 is -1 as the int32 pack_mask stores


def test_mask_dead_rows():
    mask = _mask("dead_rows")
    s, dead = MASKS["dead_rows"]
    assert mask.shape == (s, s)
    assert torch.nonzero(mask.all(1)).flatten().tolist() == list(dead)
    for r in dead:
        wave = mask[r // AC.WAVE_Q * AC.WAVE_Q:(r // AC.WAVE_Q + 1) * AC.WAVE_Q]
        assert not bool(wave.all(1).all()), "query %d has no live query in its wave" % r
    assert s % AC.GROUP_Q and any(r >= s // AC.GROUP_Q * AC.GROUP_Q for r in dead)     # one in the last, ragged workgroup
    assert bool(torch.equal(build("long_dead_rows_head_scales")["mask"].all(1), mask.all(1)))


def test_value_families():
    for name in ("self_128_head_scales", "cross_17x127_head_scales", "long_dead_rows_head_scales"):
        case = build(name)
        for key in ("v", "grad_out"):
            per_head = case[key].abs().amax((0, 1, 3))
            assert float(per_head[AC.SMALL_HEAD]) <= 1e-5 * float(per_head.max()), (name, key)
        assert 0.05 <= float(case["q"].abs().min()) and float(case["q"].abs().max()) <= 4.0
    for name in ("self_128_sharp", "long_333_sharp"):
        ref = reference(name)
        p_max = torch.exp(bhsd(build(name)["q"]).double() @ bhsd(build(name)["k"]).double().transpose(-1, -2) * build(name)["scale"]
                          - ref["lse"].unsqueeze(-1)).amax(-1)
        assert float((p_max > 1 - 1e-6).float().mean()) > 0.1, name
    case = build("long_128_offset")
    logits = bhsd(case["q"]).double() @ bhsd(case["k"]).double().transpose(-1, -2) * case["scale"]
    assert float(logits.min()) > 100
    assert not bool(build("self_33_zero_q")["q"].any())
    twin = build("self_33_twin_keys")
    assert torch.equal(twin["k"][:, 1::2], twin["k"][:, 0:32:2]) and torch.equal(twin["v"][:, 1::2], twin["v"][:, 0:32:2])


# ---- the composite within the bars ---------------------------------------------------------------------------------------------
COMPOSITE_LOW, COMPOSITE_HIGH = 0.02, 0.5


def test_composite_within_the_bars():
    worst = {grp: dict.fromkeys(AC.TENSORS, 0.0) for grp in AC.COMPOSITE_WORST}
    for name in CASES:
        ratios = check(name, composite_of(name))
        for key, r in ratios.items():
            worst[AC.group_of(name)][key] = max(worst[AC.group_of(name)][key], r)
    for grp, row in worst.items():
        print("composite %-12s %s" % (grp, "  ".join("%s %.3g" % kv for kv in row.items())))
    for grp, row in worst.items():
        for key in AC.TENSORS:
            if grp.endswith("normal"):
                assert COMPOSITE_LOW <= row[key] <= COMPOSITE_HIGH, (grp, key, row[key])
                assert COMPOSITE_LOW <= AC.COMPOSITE_WORST[grp][key] <= COMPOSITE_HIGH
            # the table is what this test printed when it was written; another BLAS may round differently, but not by 2x
            assert row[key] <= 2 * AC.COMPOSITE_WORST[grp][key] <= 1.0, (grp, key, row[key])


# ---- the bar catches what the max-norm criterion lets through ------------------------------------------------------------------
def _fails_check(name, got):
    with pytest.raises(AssertionError, match="outside c="):
        check(name, got)


def test_mutant_last_key_ignored_in_the_small_head():
    name = "self_128_head_scales"
    case, ref, comp = build(name), reference(name), composite_of(name)
    mask = torch.zeros(128, 128, dtype=torch.bool)
    mask[:, 127] = True
    wrong = composite(case, mask=mask)
    got = {k: v.clone() for k, v in comp.items()}
    for key in got:
        got[key][:, AC.SMALL_HEAD] = wrong[key][:, AC.SMALL_HEAD]
    got_old = {k: got[k] for k in ("out", "dq", "dk", "dv")}
    assert old_criterion(case, got_old, comp, ref) == []
    for key in ("out", "dq", "dk", "dv"):
        _fails_check(name, {key: got[key]})


def test_mutant_dk_sign_flipped_for_one_key_of_the_small_head():
    name = "self_128_head_scales"
    case, ref, comp = build(name), reference(name), composite_of(name)
    got = {k: v.clone() for k, v in comp.items()}
    got["dk"][:, AC.SMALL_HEAD, 77] *= -1
    assert old_criterion(case, got, comp, ref) == []
    _fails_check(name, {"dk": got["dk"]})


def test_mutant_dead_row_returns_the_mean_of_v():
    name = "long_dead_rows_head_scales"
    case, ref, comp = build(name), reference(name), composite_of(name)
    got = {k: v.clone() for k, v in comp.items()}
    row = MASKS["dead_rows"][1][-1]
    got["out"][:, AC.SMALL_HEAD, row] = bhsd(case["v"])[:, AC.SMALL_HEAD].mean(1)
    assert old_criterion(case, got, comp, ref) == []
    _fails_check(name, {"out": got["out"]})


def test_mutant_scale_off_by_2_to_the_minus_16():
    """No claim about the old criterion here: a relative error of 2^-16 in the scale moves every logit by 2^-16 |s|, several times
    what the allowance grants a logit of this size.  Measured when this was written: err / bound 3.5 (out) at 2^-16 and 1.75 at
    2^-17; the lse bar still catches 2^-18 (3.0) and 2^-19 (1.5)."""
    name = "self_128"
    wrong = composite(build(name), scale_mul=1 + 2.0 ** -16)
    with pytest.raises(AssertionError, match="outside c="):
        check(name, wrong)
    check(name, composite_of(name))
