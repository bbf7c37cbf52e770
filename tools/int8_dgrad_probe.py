"""Probe (GPU): the LLM.int8 input gradient grad[rows, N] @ W[N, K] on one Llama-2-7B weight, bf16, W ~ CB * SCB / 127.
Arms, interleaved round by round after a warm-up and a clock ramp, each timed by device events around HIP-graph replays
of `reps` back-to-back calls (no host time in the figure):
  (a) the expression MatMul8bitLt.backward used before: torch.matmul(G, CB.to(dtype).mul_(SCB / 127)) (a fresh [N, K]
      weight per call in three launches, the library's NN GEMM);
  (b) F.int8_linear_dgrad(_route="hgemm"): the transposing int8 dequantise into the weight workspace + k_hgemm;
  (c) the dequantise alone on the same weight: the torch expression ([N, K]) against k_dequantize_int8_t ([K, N]).
Per arm: best and median of the rounds and the spread (max - min) / median; (b) / (a) and transposed / torch ratios.
The verdict per row count is the static rule's criterion: "hgemm" only where (b)'s median is below (a)'s by more than
the larger spread of the two arms.  (b) is checked against (a)'s product at the GEMM tolerance, the transposed
dequantise bit for bit, before any timing.

    python tools/int8_dgrad_probe.py --weight 4096,11008 [--rows 4096,256,16] [--rounds 7] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitsandbytes-sycl_amd")]
import python_src_quants.functional as F  # noqa: E402


def timed(fn, reps):
    """us per call: 5 replays of a graph of `reps` calls between two events (the graph was replayed once before)."""
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(reps):
            fn()
    gr.replay()
    torch.cuda.synchronize()

    def run():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(5):
            gr.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / (5 * reps)
    return run


def summary(xs):
    med = statistics.median(xs)
    return min(xs), med, (max(xs) - min(xs)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weight", default="4096,4096", help="N,K of the weight (out_features, in_features)")
    ap.add_argument("--rows", default="4096,256,16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    args = ap.parse_args()
    N, K = (int(v) for v in args.weight.split(","))
    rows_list = [int(v) for v in args.rows.split(",")]
    assert torch.cuda.is_available(), "int8_dgrad_probe needs a GPU"
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1)
    W = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.float16)
    CB, _, SCB, _, _ = F.double_quant(W)
    del W
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# weight [{N}, {K}] int8 rows + fp32 row absmax, bf16; {torch.cuda.get_device_name(0)}; "
        f"{args.rounds} interleaved rounds; us per call (best / median / spread)")

    # (c) the dequantise alone
    Wt = torch.empty((K, N), dtype=dtype, device=dev)
    assert F._dequant_int8_t_launch(CB, SCB, Wt) == 0
    torch.cuda.synchronize()
    assert torch.equal(Wt.view(torch.int16), F._int8_weight_16(CB, SCB, dtype).t().contiguous().view(torch.int16)), \
        "transposed dequantise differs"
    t0 = time.time()
    while time.time() - t0 < 0.5:          # clock ramp
        F._dequant_int8_t_launch(CB, SCB, Wt)
    torch.cuda.synchronize()
    arms = {"torch": timed(lambda: F._int8_weight_16(CB, SCB, dtype), 20),
            "transposed": timed(lambda: F._dequant_int8_t_launch(CB, SCB, Wt), 20)}
    res = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, run in arms.items():
            res[k].append(run())
    s_, t_ = summary(res["torch"]), summary(res["transposed"])
    gbytes = N * K * 3.0 / 1e3             # 1 B read + 2 B written per weight, in kB -> GB/s with us
    for name, r in (("torch", s_), ("transposed", t_)):
        say(f"(c) dequantise {name:10s} {r[0]:8.2f} / {r[1]:8.2f} us / {100 * r[2]:4.1f} %   "
            f"{gbytes / r[1]:7.1f} GB/s of the kernel's traffic at the median")
    say(f"(c) transposed / torch = {t_[1] / s_[1]:.3f} (medians), {t_[0] / s_[0]:.3f} (best)")
    del arms, Wt

    for rows in rows_list:
        G = torch.randn(rows, N, device=dev, generator=g).to(dtype)

        def arm_a():
            return torch.matmul(G, F._int8_weight_16(CB, SCB, dtype))

        out = torch.empty((rows, K), dtype=dtype, device=dev)

        def arm_b():
            return F.int8_linear_dgrad(G, CB, SCB, out=out, _route="hgemm")

        ya, yb = arm_a().double(), arm_b().double()
        rms = ya.pow(2).mean().sqrt()
        assert ((yb - ya).abs() <= 4e-2 * rms + 4e-2 * ya.abs()).all(), "arms (a) and (b) disagree"
        del ya, yb
        reps = 10 if rows >= 1024 else 20
        arms = {"a": timed(arm_a, reps), "b": timed(arm_b, reps)}
        res = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, run in arms.items():
                res[k].append(run())
        a_, b_ = summary(res["a"]), summary(res["b"])
        flop = 2.0 * rows * N * K
        verdict = "hgemm" if b_[1] < a_[1] * (1.0 - max(a_[2], b_[2])) else "library"
        say(f"rows {rows:5d}  (a) torch dequantise + torch.matmul {a_[0]:8.2f} / {a_[1]:8.2f} us / {100 * a_[2]:4.1f} %   "
            f"(b) int8_linear_dgrad hgemm {b_[0]:8.2f} / {b_[1]:8.2f} us / {100 * b_[2]:4.1f} %   "
            f"(b)/(a) = {b_[1] / a_[1]:.3f} (medians), {b_[0] / a_[0]:.3f} (best)   "
            f"(b) {flop / b_[1] / 1e6:.1f} TFLOP/s   -> {verdict}")
        del arms, G, out
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
