"""The measurement behind the fp32-equivalent split-precision arm (EFG_GEMM_ARM=bf16x6, csrc/gemm_bf16x6.hip).  GPU box.

  python scripts/gemm_bf16x6_report.py [--out profiles] [--skip-step] [--skip-ops]

writes
  <out>/gemm_bf16x6_step.json  ms per step of ONE Trainer at the headline workload (ConQueR, 2 x 180k points, 900 queries,
                               EFG_DETERMINISTIC=1 as bench.py sets it) with exact fp32, the x3 arm and the x6 arm switched in
                               turn (the switches are read at call time; the reason bench.py gives for timing its own arm on
                               the same trainer holds here), in alternating rounds; and the (rows, in, out) of every product
                               that reaches operators/linear.py:LinearFunction with >= 16 384 rows in one step.
  <out>/gemm_bf16x6_ops.txt    forward, data-gradient and weight-gradient product of those shapes: library fp32 / x3 / x6 in
                               us (HIP events, one process, un-profiled, arms interleaved in rounds, >= 50 launches each after
                               warm-up) and each one's error against an fp64 product, e = |c - c64| / (|a| . |b|), max / rms.

bench.py labels a run under EFG_GEMM_ARM=bf16x6 `dtype: f32` (it knows the x3 switch only): x6 timings are quoted from here."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("EFG_DETERMINISTIC", "1")

# (rows, in, out) of the encoder's Linear layers; the step adds whatever else reaches LinearFunction (the BEV 1 x 1 convolutions)
STEP_SHAPES = [(70688, 256, 256), (70688, 256, 1024), (70688, 256, 200), (70688, 1024, 256)]
ROUNDS, PER_ROUND, WARM = 6, 10, 5


def interleaved_us(fns):
    """{name: callable} -> {name: (median, min, max) us per launch over ROUNDS rounds of PER_ROUND launches}, the arms taking
    turns inside every round."""
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(PER_ROUND):
                fn()
            e1.record()
            torch.cuda.synchronize()
            got[name].append(e0.elapsed_time(e1) / PER_ROUND * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def err(c, c64, den):
    e = (c.double() - c64).abs() / den
    return float(e.max()), float(e.square().mean().sqrt())


def set_arm(lin, name):
    lin._ARM_BF16X3, lin._ARM_BF16X6 = name == "x3", name == "x6"


def step_report(args):
    import numpy as np

    from efg_amd.engine import Trainer, synthetic_batch
    from efg_amd.operators import linear as lin

    dev = torch.device("cuda:0")
    np.random.seed(0)
    trainer = Trainer(device=dev, overrides={"model.transformer.num_queries": 900}, seed=0)
    pool = [synthetic_batch(2000 + 100 * p, 2, n_points=180000, device=dev) for p in range(2)]
    arms = ("fp32", "x3", "x6")
    times = {a: [] for a in arms}
    for a in arms:                      # lazy initialisation of every arm's kernels and library solutions: start-up, not a step
        set_arm(lin, a)
        for w in range(3):
            trainer.step(pool[w % 2])
    torch.cuda.synchronize()
    for _ in range(args.step_rounds):
        for a in arms:
            set_arm(lin, a)
            for w in range(2):
                trainer.step(pool[w % 2])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.steps):
                trainer.step(pool[s % 2])
            torch.cuda.synchronize()
            times[a].append(1000.0 * (time.perf_counter() - t0) / args.steps)
    # one more exact-fp32 step with a recorder in front of LinearFunction: the long products of the step
    set_arm(lin, "fp32")
    seen = {}
    real = lin.LinearFunction.forward

    def recording(ctx, x, weight, bias, relu=False):
        rows = x.numel() // x.shape[-1]
        if rows >= lin._FUSED_MIN_ROWS:
            key = (rows, weight.shape[1], weight.shape[0])
            seen[key] = seen.get(key, 0) + 1
        return real(ctx, x, weight, bias, relu)

    lin.LinearFunction.forward = staticmethod(recording)
    try:
        trainer.step(pool[0])
        torch.cuda.synchronize()
    finally:
        lin.LinearFunction.forward = staticmethod(real)
    # (the fused encoder layer of detection3d/encoder_layer.py makes the encoder's own products without LinearFunction in
    # the exact-fp32 step; under either arm it steps aside and they all come through it)
    set_arm(lin, "x6")
    seen_arm = {}
    seen, seen_fp32 = seen_arm, seen
    lin.LinearFunction.forward = staticmethod(recording)
    try:
        trainer.step(pool[0])
        torch.cuda.synchronize()
    finally:
        lin.LinearFunction.forward = staticmethod(real)
        set_arm(lin, "fp32")
    trainer.close()
    out = {
        "workload": "ConQueR train step, 2 scenes x 180k points, 900 queries, EFG_DETERMINISTIC=1, one Trainer, one process",
        "method": "%d alternating rounds of %d steps per arm after 2 warm-up steps, host clock around a device synchronise"
                  % (args.step_rounds, args.steps),
        "ms_per_step": {a: {"median": round(statistics.median(v), 3), "rounds": [round(t, 3) for t in v]} for a, v in times.items()},
        "labels": {"fp32": "exact fp32 (both switches off: the headline path)", "x3": "_ARM_BF16X3 (EFG_GEMM_ARM=bf16x3)",
                   "x6": "_ARM_BF16X6 (EFG_GEMM_ARM=bf16x6)"},
        "long_products_through_LinearFunction": {
            "exact_fp32_step": [{"rows": k[0], "in": k[1], "out": k[2], "calls": n} for k, n in sorted(seen_fp32.items())],
            "x6_step": [{"rows": k[0], "in": k[1], "out": k[2], "calls": n} for k, n in sorted(seen_arm.items())]},
        "device": torch.cuda.get_device_name(0),
    }
    return out, sorted(set(seen_fp32) | set(seen_arm))


def ops_report(shapes, lines):
    from efg_amd.engine import use_tuned_gemms
    from efg_amd.operators import gemm_bf16x3 as G3
    from efg_amd.operators import gemm_bf16x6 as G6
    from efg_amd.operators import linear as lin

    use_tuned_gemms()
    set_arm(lin, "fp32")
    dev = torch.device("cuda:0")
    lines.append("us per launch: median (min-max) of %d rounds x %d launches, arms interleaved; error vs fp64: max / rms of "
                 "|c - c64| / (|a| . |b|)" % (ROUNDS, PER_ROUND))
    lines.append("device: %s" % torch.cuda.get_device_name(0))
    fmt_t = lambda t: "%7.1f (%6.1f-%6.1f)" % t
    fmt_e = lambda e: "%.1e / %.1e" % e
    for m, k, n in shapes:
        g = torch.Generator().manual_seed(m + k + n)
        x = torch.randn(m, k, generator=g).to(dev)
        w = (torch.randn(n, k, generator=g) / k ** 0.5).to(dev)
        b = torch.randn(n, generator=g).to(dev)
        gy = torch.randn(m, n, generator=g).to(dev)
        lines.append("")
        lines.append("%d rows, %d -> %d" % (m, k, n))
        p3f, p3d = G3.pack_linear_both(w)
        p6f, p6d = G6.pack_linear_both(w)
        cases = [
            ("forward  y = x W^T + b", x, w.t(), b,
             {"fp32": lambda: torch.addmm(b, x, w.t()), "x3": lambda: G3.gemm(x, p3f, n, bias=b), "x6": lambda: G6.gemm(x, p6f, n, bias=b)}),
            ("data     dx = dy W", gy, w, None,
             {"fp32": lambda: gy.mm(w), "x3": lambda: G3.gemm(gy, p3d, k), "x6": lambda: G6.gemm(gy, p6d, k)}),
            ("weight   dW = dy^T x", gy.t(), x, None,
             {"fp32": lambda: lin.weight_grad(x, gy), "x3": lambda: G3.wgrad(gy, x), "x6": lambda: G6.wgrad(gy, x)}),
        ]
        total = {"fp32": 0.0, "x3": 0.0, "x6": 0.0}
        for what, a_op, b_op, bias, fns in cases:
            c64 = a_op.double() @ b_op.double()
            den = a_op.double().abs() @ b_op.double().abs()
            if bias is not None:
                c64 += bias.double()
            errs = {name: err(fn(), c64, den) for name, fn in fns.items()}
            del c64, den
            t = interleaved_us(fns)
            for name in total:
                total[name] += t[name][0]
            lines.append("  %-24s fp32 %s  x3 %s  x6 %s us   err fp32 %s  x3 %s  x6 %s   x6/fp32 time %.2f"
                         % (what, fmt_t(t["fp32"]), fmt_t(t["x3"]), fmt_t(t["x6"]), fmt_e(errs["fp32"]), fmt_e(errs["x3"]),
                            fmt_e(errs["x6"]), t["x6"][0] / t["fp32"][0]))
        t = interleaved_us({"x3": lambda: G3.pack_linear_both(w), "x6": lambda: G6.pack_linear_both(w)})
        total["x3"] += t["x3"][0]
        total["x6"] += t["x6"][0]
        lines.append("  %-24s fp32    --                 x3 %s  x6 %s us   (both layouts, one launch per forward)"
                     % ("pack W", fmt_t(t["x3"]), fmt_t(t["x6"])))
        lines.append("  %-24s fp32 %7.1f  x3 %7.1f  x6 %7.1f us   x6/fp32 %.2f"
                     % ("layer (3 products + pack)", total["fp32"], total["x3"], total["x6"], total["x6"] / total["fp32"]))
        del x, w, b, gy
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-ops", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_bf16x6_report.py measures on the GPU: no device found")
    os.makedirs(args.out, exist_ok=True)
    shapes = list(STEP_SHAPES)
    if not args.skip_step:
        rep, seen = step_report(args)
        with open(os.path.join(args.out, "gemm_bf16x6_step.json"), "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")
        print(json.dumps(rep["ms_per_step"]))
        shapes += [s for s in seen if s not in shapes and s[1] % 4 == 0 and s[2] % 4 == 0]
    if not args.skip_ops:
        lines = []
        try:
            ops_report(shapes, lines)
        finally:
            with open(os.path.join(args.out, "gemm_bf16x6_ops.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        print("\n".join(lines))


if __name__ == "__main__":
    main()
