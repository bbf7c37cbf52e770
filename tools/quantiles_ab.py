"""A/B (GPU): F.estimate_quantiles (csrc/quantiles.hip: one read of A, a 4096-key sort per workgroup) against a torch
restatement on the same GPU, at n = 2^24 for fp32 and fp16, one process, arms alternated.

The restatement is A[:B * 4096].view(B, 4096).sort(dim=1), a gather at the 256 indices and the mean over the B blocks
(fp32 mean: its last bits differ from the fixed-order fp64 sum; the largest difference is reported, not compared).
Both arms run eagerly between two device events over a window of at least --window seconds, rotating through more than
256 MB of distinct inputs so that the Infinity Cache does not serve them; REPS repetitions per arm, alternating, give
the spread.  Reported per dtype: each arm's median time and spread, the ratio, and our achieved read rate n *
sizeof(T) / time as a share of the 8.0 TB/s specified peak.  The histogram (n = 2^20 adds into 256 x 256 bins) has no
counterpart; its time is recorded beside them.  Writes profiles/quantiles_ab.json.

Usage: python tools/quantiles_ab.py [--n 16777216] [--window 0.3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitsandbytes-sycl_amd"), os.path.join(ROOT, "tests")]
import python_src_quants.functional as F  # noqa: E402
import quantile_helpers as qh  # noqa: E402

PEAK_SPEC_TBS = 8.0
ROTATE_BYTES = 256 * 2 ** 20
REPS = 5


def window_ms(calls, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        for c in calls:
            c()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def ab(arms, window_s):
    """arms: {name: [calls]}; {name: [us per call] * REPS}, arms alternated within every repetition."""
    iters = {}
    for name, calls in arms.items():
        window_ms(calls, 1)                                              # warm-up
        iters[name] = max(2, int(window_s * 1e3 / max(window_ms(calls, 1), 1e-3)) + 1)
    res = {name: [] for name in arms}
    for _ in range(REPS):
        for name, calls in arms.items():
            res[name].append(window_ms(calls, iters[name]) * 1e3 / iters[name] / len(calls))
    return res


def summarise(ts):
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2 ** 24)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantiles_ab.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    n, blocks = args.n, args.n // qh.BLOCK
    idx = torch.from_numpy(qh.quantile_indices(qh.BLOCK, 1 / 512)).to(dev)
    table = []
    for dtype in (torch.float32, torch.float16):
        size = torch.empty(0, dtype=dtype).element_size()
        copies = ROTATE_BYTES // (n * size) + 2
        As = [torch.randn(n, device=dev, generator=gen).to(dtype) for _ in range(copies)]
        outs = {"ours": torch.empty(256, device=dev), "torch": None}

        def ours(A):
            return lambda: F.estimate_quantiles(A, out=outs["ours"])

        def restated(A):
            def run():
                s = A[:blocks * qh.BLOCK].view(blocks, qh.BLOCK).sort(dim=1).values
                outs["torch"] = s[:, idx].float().mean(dim=0)
            return run

        arms = {"ours": [ours(A) for A in As], "torch": [restated(A) for A in As]}
        res = ab(arms, args.window)                # both arms end on the last input
        diff = float((outs["ours"] - outs["torch"]).abs().max())
        mine, theirs = summarise(res["ours"]), summarise(res["torch"])
        rate = n * size / (mine["median_us"] * 1e-6)
        row = {"op": "estimate_quantiles", "dtype": str(dtype), "n": n, "copies": copies, "ours": mine, "torch": theirs,
               "torch_over_ours": theirs["median_us"] / mine["median_us"], "read_TBs": rate / 1e12,
               "share_of_8.0TBs": rate / (PEAK_SPEC_TBS * 1e12), "max_abs_diff": diff,
               "ours_wins_beyond_spread": mine["max_us"] < theirs["min_us"]}
        table.append(row)
        print(f"{str(dtype):14s} n={n}: ours {mine['median_us']:8.1f} us [{mine['min_us']:.1f}..{mine['max_us']:.1f}]  "
              f"torch {theirs['median_us']:8.1f} us [{theirs['min_us']:.1f}..{theirs['max_us']:.1f}]  ratio "
              f"{row['torch_over_ours']:.2f}  {rate / 1e12:.2f} TB/s = {row['share_of_8.0TBs'] * 100:.1f} % of 8.0 TB/s  "
              f"max |diff| {diff:.3g}", flush=True)
        del As, arms
        torch.cuda.empty_cache()
    m = 2 ** 20
    i1, i2 = (torch.randint(0, 256, (m,), device=dev, generator=gen, dtype=torch.int32) for _ in range(2))
    src = torch.ones(m, device=dev)
    hist = torch.zeros(256, 256, device=dev)
    res = ab({"histogram": [lambda: F.histogram_scatter_add_2d(hist, i1, i2, src)]}, args.window)
    row = {"op": "histogram_scatter_add_2d", "n": m, "bins": [256, 256], "ours": summarise(res["histogram"])}
    table.append(row)
    print(f"histogram_scatter_add_2d n={m}: {row['ours']['median_us']:.1f} us "
          f"[{row['ours']['min_us']:.1f}..{row['ours']['max_us']:.1f}]", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "window_s": args.window,
                   "peak_spec_TBs": PEAK_SPEC_TBS, "table": table}, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
