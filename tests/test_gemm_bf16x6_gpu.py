"""GPU: the fp32-equivalent split-precision arm (EFG_GEMM_ARM=bf16x6, csrc/gemm_bf16x6.hip) against fp64 products, measured on
the scale of the LIBRARY's fp32 product on the same tensors.

Error of a result c of a . b:  e(c) = |c - c64| / (|a|_64 . |b|_64) element-wise, as a max and as an rms; c64 is the fp64
product formed here and e32 is the same figure for torch.addmm / mm in fp32.  The bar, on every case:
    max e6 <= max(2 max e32, 2^-23)   and   rms e6 <= max(2 rms e32, 2^-25)
The factor 2 is headroom for the MFMA chain's accumulation order (a CPU emulation of the split sits at 0.4-1.03 of e32), the
floors are one output ulp: no fp32 result beats them, and they keep tiny shapes from dividing by a near-zero e32."""
import pytest
import torch
from conftest import force_proposals

pytestmark = pytest.mark.gpu

FLOOR_MAX, FLOOR_RMS = 2.0 ** -23, 2.0 ** -25


def _err(c, c64, den):
    e = (c.double() - c64).abs() / den
    return float(e.max()), float(e.square().mean().sqrt())


def _assert_fp32_equivalent(e6, e32, what=""):
    print("%s  x6 max %.3e rms %.3e | fp32 max %.3e rms %.3e | ratios %.2f %.2f"
          % (what, e6[0], e6[1], e32[0], e32[1], e6[0] / max(e32[0], 1e-300), e6[1] / max(e32[1], 1e-300)))
    assert e6[0] <= max(2 * e32[0], FLOOR_MAX), (what, e6, e32)
    assert e6[1] <= max(2 * e32[1], FLOOR_RMS), (what, e6, e32)


def _forward_case(a, w, b, also_x3):
    """a [m, k], w [n, k] (an nn.Linear weight), b [n]: y = a w^T + b on the x6 arm, the library and (also_x3) the x3 arm."""
    from efg_amd.operators import gemm_bf16x3 as G3
    from efg_amd.operators import gemm_bf16x6 as G6

    n = w.shape[0]
    c64 = a.double() @ w.double().t() + b.double()
    den = a.double().abs() @ w.double().abs().t()
    out = G6.gemm(a, G6.pack_linear(w, transposed=False), n, bias=b)
    e6, e32 = _err(out, c64, den), _err(torch.addmm(b, a, w.t()), c64, den)
    _assert_fp32_equivalent(e6, e32, "forward %s x %s" % (tuple(a.shape), tuple(w.shape)))
    if also_x3:
        e3 = _err(G3.gemm(a, G3.pack_linear(w, transposed=False), n, bias=b), c64, den)
        print("   x3 max %.3e rms %.3e" % e3)
        assert e6[1] < e3[1] / 4, (e6, e3)     # a build that drops the third piece lands on x3's error
    return out


@pytest.mark.parametrize("m,k,n", [(128, 32, 128), (70688, 256, 256), (4097, 256, 1024), (3001, 1024, 256), (2049, 256, 200),
                                   (777, 200, 256), (1500, 256, 32), (640, 32, 256), (5, 64, 7)])
def test_forward_is_fp32_equivalent(m, k, n):
    g = torch.Generator().manual_seed(m + k + n)
    a = torch.randn(m, k, generator=g).cuda()
    w = (torch.randn(n, k, generator=g) / k ** 0.5).cuda()     # nn.Linear weight [out, in]
    b = torch.randn(n, generator=g).cuda()
    _forward_case(a, w, b, also_x3=k >= 256)


def test_forward_with_log_normally_scaled_operands():
    """Every element carries its own scale exp(4 z): sums dominated by a few terms, fifteen decades of dynamic range."""
    g = torch.Generator().manual_seed(44)
    a = (torch.randn(4096, 256, generator=g) * torch.exp(4 * torch.randn(4096, 256, generator=g))).cuda()
    w = (torch.randn(256, 256, generator=g) * torch.exp(4 * torch.randn(256, 256, generator=g))).cuda()
    b = torch.randn(256, generator=g).cuda()
    _forward_case(a, w, b, also_x3=True)


def test_bias_relu_epilogue_strided_rows_and_data_gradient_packing():
    from efg_amd.operators import gemm_bf16x6 as G

    g = torch.Generator().manual_seed(5)
    # data-gradient packing: dx = dy W with W [out, in] = [200, 256]
    dy = torch.randn(1000, 200, generator=g).cuda()
    w = torch.randn(200, 256, generator=g).cuda()
    b = torch.randn(256, generator=g).cuda()
    packed = G.pack_linear(w, transposed=True)
    c64, den = dy.double() @ w.double(), dy.double().abs() @ w.double().abs()
    out = G.gemm(dy, packed, 256)
    _assert_fp32_equivalent(_err(out, c64, den), _err(dy @ w, c64, den), "dgrad 1000 x 200 -> 256")
    assert torch.equal(G.pack_linear_both(w)[1], packed)                      # the one-launch packer writes the same images
    assert torch.equal(G.pack_linear_both(w)[0], G.pack_linear(w, transposed=False))
    out_b = G.gemm(dy, packed, 256, bias=b)
    assert torch.equal(G.gemm(dy, packed, 256, bias=b, relu=True), out_b.clamp_min(0))
    assert torch.equal(G.gemm(dy, packed, 256, relu=True), out.clamp_min(0))
    # strided A rows: row stride 512, 16-byte aligned start
    wide = torch.randn(1000, 512, generator=g).cuda()
    view = wide[:, 128:384]
    w2 = torch.randn(64, 256, generator=g).cuda()
    b2 = torch.randn(64, generator=g).cuda()
    p2 = G.pack_linear(w2, transposed=False)
    c64 = view.double() @ w2.double().t() + b2.double()
    den = view.double().abs() @ w2.double().abs().t()
    out2 = G.gemm(view, p2, 64, bias=b2)
    _assert_fp32_equivalent(_err(out2, c64, den), _err(torch.addmm(b2, view, w2.t()), c64, den), "strided rows")
    assert torch.equal(out2, G.gemm(view.contiguous(), p2, 64, bias=b2))
    assert torch.equal(G.gemm(view, p2, 64, bias=b2, relu=True), out2.clamp_min(0))


@pytest.mark.parametrize("m,n,k", [(70688, 256, 256), (9000, 1024, 256), (9000, 256, 1024), (4097, 200, 256), (4097, 32, 256),
                                   (31, 256, 256), (33, 8, 4)])
def test_weight_gradient_is_fp32_equivalent(m, n, k):
    from efg_amd.operators import gemm_bf16x6 as G

    gen = torch.Generator().manual_seed(m + n + k)
    g = torch.randn(m, n, generator=gen).cuda()
    x = torch.randn(m, k, generator=gen).cuda()
    c64, den = g.double().t() @ x.double(), g.double().abs().t() @ x.double().abs()
    out = G.wgrad(g, x)
    assert out.shape == (n, k)
    _assert_fp32_equivalent(_err(out, c64, den), _err(g.t() @ x, c64, den), "wgrad %d rows -> %d x %d" % (m, n, k))
    assert torch.equal(out, G.wgrad(g, x))      # fixed summation order: run-to-run identical


def test_bad_arguments_are_refused_before_any_launch():
    from efg_amd import _lib

    lib = _lib.lib()
    a = torch.randn(64, 64).cuda()
    w = torch.randn(64, 64).cuda()
    packed = torch.empty(lib.efg_gemm_bf16x6_pack_bytes(64, 64), dtype=torch.uint8, device="cuda")
    assert lib.efg_gemm_bf16x6_pack_f32(_lib.ptr(w), 1, 64, 64, 64, _lib.ptr(packed), _lib.stream()) == 0
    c = torch.full((64, 64), 7.0).cuda()
    # k % 4 != 0
    assert lib.efg_gemm_bf16x6_f32(a.data_ptr(), 64, 62, 64, _lib.ptr(packed), 64, None, 0, _lib.ptr(c), 64, _lib.stream()) != 0
    assert b"multiple of 4" in lib.efg_last_error()
    # rows 4 bytes off a 16-byte boundary
    assert lib.efg_gemm_bf16x6_f32(a.data_ptr() + 4, 63, 60, 64, _lib.ptr(packed), 64, None, 0, _lib.ptr(c), 64,
                                   _lib.stream()) != 0
    assert b"16-byte aligned" in lib.efg_last_error()
    assert lib.efg_gemm_bf16x6_pack_f32(_lib.ptr(w), 1, 64, 0, 64, _lib.ptr(packed), _lib.stream()) != 0
    assert b"gemm_bf16x6 pack" in lib.efg_last_error()
    # weight gradient: workspace one byte short, then misaligned rows and n % 4 != 0
    dw = torch.full((64, 64), 7.0).cuda()
    need = lib.efg_gemm_bf16x6_wgrad_workspace_bytes(64, 64, 64)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    args = (64, 64, 64, _lib.ptr(dw), _lib.ptr(ws))
    assert lib.efg_gemm_bf16x6_wgrad_f32(a.data_ptr(), 64, w.data_ptr(), 64, *args, need - 1, _lib.stream()) != 0
    assert b"workspace too small" in lib.efg_last_error()
    assert lib.efg_gemm_bf16x6_wgrad_f32(a.data_ptr() + 4, 64, w.data_ptr(), 64, *args, need, _lib.stream()) != 0
    assert b"16-byte aligned" in lib.efg_last_error()
    assert lib.efg_gemm_bf16x6_wgrad_f32(a.data_ptr(), 64, w.data_ptr(), 64, 64, 62, 64, _lib.ptr(dw), _lib.ptr(ws), need,
                                         _lib.stream()) != 0
    assert b"multiples of 4" in lib.efg_last_error()
    torch.cuda.synchronize()
    assert bool((c == 7.0).all()) and bool((dw == 7.0).all())      # nothing was launched
    # and the same call with good arguments goes through
    assert lib.efg_gemm_bf16x6_wgrad_f32(a.data_ptr(), 64, w.data_ptr(), 64, *args, need, _lib.stream()) == 0


def test_linear_on_the_x6_arm_follows_the_optimizer(monkeypatch):
    """lin.Linear(256, 256) on 20 000 rows with the x6 switch on: output and weight gradient at fp32's error over three fused
    AdamW steps (the weights are split anew on every call, so the products follow the in-place update)."""
    from efg_amd.operators import gemm_bf16x6 as G6
    from efg_amd.operators import linear as lin

    monkeypatch.setattr(lin, "_ARM_BF16X3", False)
    monkeypatch.setattr(lin, "_ARM_BF16X6", True)
    calls = []
    real, real_w = G6.gemm, G6.wgrad
    monkeypatch.setattr(G6, "gemm", lambda *a, **k: (calls.append("gemm"), real(*a, **k))[1])
    monkeypatch.setattr(G6, "wgrad", lambda *a, **k: (calls.append("wgrad"), real_w(*a, **k))[1])
    g = torch.Generator().manual_seed(11)
    layer = lin.Linear(256, 256).cuda()
    opt = torch.optim.AdamW(layer.parameters(), lr=0.05, fused=True)
    x = torch.randn(20000, 256, generator=g).cuda()
    for it in range(3):
        w, b = layer.weight.detach().clone(), layer.bias.detach().clone()
        y = layer(x)
        grads = []
        y.register_hook(grads.append)
        c64, den = x.double() @ w.double().t() + b.double(), x.double().abs() @ w.double().abs().t()
        _assert_fp32_equivalent(_err(y.detach(), c64, den), _err(torch.addmm(b, x, w.t()), c64, den), "Linear step %d: y" % it)
        y.square().mean().backward()
        gy = grads[0]
        c64, den = gy.double().t() @ x.double(), gy.double().abs().t() @ x.double().abs()
        _assert_fp32_equivalent(_err(layer.weight.grad, c64, den), _err(gy.t() @ x, c64, den), "Linear step %d: dW" % it)
        opt.step()
        opt.zero_grad(set_to_none=True)
        assert not torch.equal(layer.weight.detach(), w)
    assert calls.count("gemm") == 3 and calls.count("wgrad") == 3, calls     # (x has no gradient: no data-gradient product)


def test_x3_wins_when_both_switches_are_on(monkeypatch):
    from efg_amd.operators import gemm_bf16x3 as G3
    from efg_amd.operators import gemm_bf16x6 as G6
    from efg_amd.operators import linear as lin

    monkeypatch.setattr(lin, "_ARM_BF16X3", True)
    monkeypatch.setattr(lin, "_ARM_BF16X6", True)
    calls = []
    for mod, tag in ((G3, "x3"), (G6, "x6")):
        for name in ("gemm", "wgrad", "pack_linear_both"):
            real = getattr(mod, name)
            monkeypatch.setattr(mod, name, lambda *a, _real=real, _t=tag + "." + name, **k: (calls.append(_t), _real(*a, **k))[1])
    layer = lin.Linear(256, 256).cuda()
    x = torch.randn(20000, 256).cuda().requires_grad_(True)
    layer(x).square().mean().backward()
    assert calls.count("x3.gemm") == 2 and calls.count("x3.wgrad") == 1, calls
    assert not [c for c in calls if c.startswith("x6")], calls


def test_x6_passes_the_parity_gate_on_a_full_size_conquer_step(monkeypatch):
    """The project's gate for an arm (tests/test_gemm_bf16x3_gpu.py), three full-size ConQueR steps with forced proposals:
    exact fp32, x3, x6.  x6 against fp32: encoder logits within 1e-4, every loss term within 1e-4 relative, gradient norm
    within 5e-4 relative; its logits closer to fp32's than x3's; and the x6 products, not the x3 ones, actually ran."""
    import numpy as np

    from efg_amd.engine import Trainer, synthetic_batch
    from efg_amd.operators import gemm_bf16x3 as G3
    from efg_amd.operators import gemm_bf16x6 as G6
    from efg_amd.operators import linear as lin

    dev = torch.device("cuda:0")
    calls = {"x3": [], "x6": []}
    wcalls = {"x3": [], "x6": []}
    for mod, tag in ((G3, "x3"), (G6, "x6")):
        real, real_w = mod.gemm, mod.wgrad
        monkeypatch.setattr(mod, "gemm", lambda *a, _r=real, _t=tag, **k: (calls[_t].append(a[0].shape), _r(*a, **k))[1])
        monkeypatch.setattr(mod, "wgrad", lambda *a, _r=real_w, _t=tag, **k: (wcalls[_t].append(a[0].shape), _r(*a, **k))[1])

    def step(x3, x6, forced):
        monkeypatch.setattr(lin, "_ARM_BF16X3", x3)
        monkeypatch.setattr(lin, "_ARM_BF16X6", x6)
        np.random.seed(3)
        tr = Trainer(device=dev, overrides={"model.transformer.num_queries": 900}, seed=0, ddp=False)
        tr.model.noise_generator = torch.Generator().manual_seed(4321)
        seen = {}
        force_proposals(tr.model.transformer, forced)
        tr.model.transformer.register_forward_hook(lambda mod, inp, out: seen.update(
            topk=mod.enc_outputs["topk_indexes"].detach().cpu()[..., 0], logits=mod.enc_outputs["pred_logits"].detach().cpu()))
        losses, _ = tr.step(synthetic_batch(1000, 2, n_points=180000, device=dev))
        out = {k: float(v.detach()) for k, v in losses.items()}
        norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum().cpu() for p in tr.model.parameters() if p.grad is not None)))
        tr.close()
        return out, norm, seen

    ref, ref_norm, ref_seen = step(False, False, None)
    assert not calls["x3"] and not calls["x6"]
    _, _, x3_seen = step(True, False, ref_seen["topk"])
    assert calls["x3"] and not calls["x6"] and not wcalls["x6"]
    n3, nw3 = len(calls["x3"]), len(wcalls["x3"])
    arm, arm_norm, arm_seen = step(False, True, ref_seen["topk"])
    assert len(calls["x3"]) == n3 and len(wcalls["x3"]) == nw3          # the x3 module was not called during the x6 step
    assert len(calls["x6"]) >= 30 and all(s[0] >= 16384 for s in calls["x6"]), len(calls["x6"])
    assert len(wcalls["x6"]) >= 15, len(wcalls["x6"])
    d6 = float((arm_seen["logits"] - ref_seen["logits"]).abs().max())
    d3 = float((x3_seen["logits"] - ref_seen["logits"]).abs().max())
    print("max |logit - fp32 logit|: x6 %.3e, x3 %.3e; gradient norm fp32 %.9g x6 %.9g" % (d6, d3, ref_norm, arm_norm))
    assert d6 < 1e-4
    for k in ref:
        assert arm[k] == pytest.approx(ref[k], rel=1e-4, abs=1e-6), k
    assert arm_norm == pytest.approx(ref_norm, rel=5e-4)
    assert d6 < d3, (d6, d3)


def test_conv3x3_on_the_x6_arm_matches_the_fp32_convolution(monkeypatch):
    """operators/conv2d.py:Conv3x3ArmFunction with the x6 products against F.conv2d in fp64 -- forward, data, weight and bias
    gradient, each error (max |diff| / max |ref|) no more than twice that of the exact-fp32 conv3x3 path on the same tensors,
    with a floor of 2^-23."""
    import torch.nn.functional as F

    from efg_amd.operators import gemm_bf16x3 as G3
    from efg_amd.operators import gemm_bf16x6 as G6
    from efg_amd.operators import linear as lin
    from efg_amd.operators.conv2d import conv3x3, conv3x3_arm

    monkeypatch.setattr(lin, "_ARM_BF16X3", False)
    monkeypatch.setattr(lin, "_ARM_BF16X6", True)
    calls = []
    for mod, tag in ((G3, "x3"), (G6, "x6")):
        for name in ("gemm", "wgrad"):
            real = getattr(mod, name)
            monkeypatch.setattr(mod, name, lambda *a, _real=real, _t=tag, **k: (calls.append(_t), _real(*a, **k))[1])
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(2, 64, 37, 29, generator=g).to(dev)
    w0 = (torch.randn(128, 64, 3, 3, generator=g) * 0.05).to(dev)
    b0 = torch.randn(128, generator=g).to(dev)
    up = None
    results = {}
    for name, fn, dt in (("fp64", lambda x, w, b: F.conv2d(x, w, b, padding=1), torch.float64), ("x6", conv3x3_arm, torch.float32),
                         ("fp32", conv3x3, torch.float32)):
        if name == "fp32":
            monkeypatch.setattr(lin, "_ARM_BF16X6", False)      # the exact path: weight_grad must not take the arm
        x, w, b = (t.detach().to(dt).requires_grad_(True) for t in (x0, w0, b0))
        y = fn(x, w, b)
        if up is None:
            up = torch.randn(y.shape, generator=g).to(dev)
        (y * up.to(dt)).sum().backward()
        results[name] = (y.detach(), x.grad, w.grad, b.grad)
    assert calls.count("x6") == 9 and "x3" not in calls, calls     # 3 products per pass: forward, data and weight gradient

    def rel(a, ref):
        return float((a.double() - ref).abs().max() / ref.abs().max())

    for i, what in enumerate(("y", "dx", "dw", "db")):
        e6, e32 = rel(results["x6"][i], results["fp64"][i]), rel(results["fp32"][i], results["fp64"][i])
        print("conv3x3 %s: x6 %.3e fp32 %.3e" % (what, e6, e32))
        assert e6 <= max(2 * e32, FLOOR_MAX), (what, e6, e32)
