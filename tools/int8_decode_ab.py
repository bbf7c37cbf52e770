"""A/B (GPU): the LLM.int8 decode step on the weight-streaming kernel (igemv8.hip, cigemv_set_mode(1)) against the tile
kernels it replaces (cigemv_set_mode(-1)), same build, one process, arms alternated.

For 1, 2, 4, 8, 16 and 32 activation rows and the weights [N, K] 11008 x 4096, 4096 x 11008, 4096 x 4096 and
8192 x 28672:
  * "product": F.igemmlt_dequant(CA, CB, SCA, SCB) alone under both modes;
  * "forward": F.int8_row_quant + F.igemmlt_dequant under mode -1 against F.int8_linear_rows (one launch) under mode 1;
each once with one weight replayed (hot: the Infinity Cache serves a stream that fits in it) and once rotating through
more than 256 MB of distinct weights (HBM).  The calls of one arm are captured into a HIP graph (one call per weight
copy) and replayed between two device events, so the host's call overhead is not in the figure; the replay count is
calibrated to a window of at least 0.2 s, and each arm is measured REPS times, alternating with the other, so the
spread is known.  Both routes' outputs are compared with torch.equal at every timed shape; a mismatch ends the run with
exit status 1.

Per table row: each route's median time and spread, the algorithmic bytes N*K + rows*K + 2*rows*N + 4*N, and the new
route's share of the HBM bound (8.0 TB/s specified peak; 6.29 TB/s is what a float4 copy reaches on this part).
Writes profiles/int8_decode_ab.json.

With --threshold T (> 0) the A/B is the outlier forward instead: the whole Linear8bitLt forward (threshold T, stored
int8 weight, fp16 bias) with fused_outlier_decode off (double_quant with its host synchronisations, whole-column zeroing,
igemmlt_dequant, fp16 outlier matmul) against the same layer with the flag on (one launch, igemv8_outlier.hip,
cigemv_set_mode(1)), on the same shapes and rows, weights rotating through HBM.  The activations are randn (sigma 1)
with --outlier-cols C columns (default 8) given one value of magnitude 8..60 each.  The unfused forward synchronises
with the host, so both arms run eagerly between two device events (host time included, as a caller sees it); the
fused arm is also replayed as a HIP graph ("fused_graph": its device time alone).  The two arms round differently (the
fused one once): their largest difference is reported, not compared.  Writes profiles/int8_outlier_decode_ab.json.
A second fused arm, "prefill", is the layer with fused_outlier_prefill on (int8_outlier_prefill.hip: the outlier columns
found on the device around the int8 GEMM, any row count), eager and as a graph ("prefill_graph"); the decode arm runs
only at 1..32 rows, where its kernel exists.  With every row count above 32 (--rows 64,256,1024,4096) the run is flag off
against flag on for the prefill and writes profiles/int8_outlier_prefill_ab.json.

Usage: python tools/int8_decode_ab.py [--rows 1,2,...] [--shapes 11008x4096,...] [--out FILE] [--window 0.2]
                                      [--threshold T [--outlier-cols C]]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitsandbytes-sycl_amd")]
import python_src_quants.functional as F  # noqa: E402

PEAK_SPEC_TBS = 8.0
PEAK_COPY_TBS = 6.29
ROTATE_BYTES = 256 * 2 ** 20
REPS = 3


def capture(calls):
    for c in calls:      # warm-up: workspaces and allocator pools grow here, not inside the capture
        c()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in calls:
            c()
    g.replay()
    torch.cuda.synchronize()
    return g


def window_ms(g, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def ab(arms, ncalls, window_s):
    """arms: {name: graph}; returns {name: [us per call] * REPS}, arms alternated within every repetition."""
    iters = {}
    for name, g in arms.items():
        ms = max(window_ms(g, 3) / 3, 1e-3)
        iters[name] = max(3, int(window_s * 1e3 / ms) + 1)
    res = {name: [] for name in arms}
    for _ in range(REPS):
        for name, g in arms.items():
            res[name].append(window_ms(g, iters[name]) * 1e3 / iters[name] / ncalls)
    return res


def summarise(ts):
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}


def eager_window_ms(calls, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        for c in calls:
            c()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def make_layer(CB, SCB, bias, threshold, fused, prefill=False):
    """A Linear8bitLt around an already quantised weight (CB, SCB are shared, not copied)."""
    from python_src_quants.nn import Int8Params, Linear8bitLt
    n, k = CB.shape
    lin = Linear8bitLt(16, 16, bias=True, has_fp16_weights=False, threshold=threshold, fused_outlier_decode=fused,
                       fused_outlier_prefill=prefill)
    lin.in_features, lin.out_features = k, n
    lin.weight = Int8Params(CB, requires_grad=False, has_fp16_weights=False, CB=CB, SCB=SCB)
    lin.bias = torch.nn.Parameter(bias, requires_grad=False)
    return lin.eval()


def main_outlier(args, rows_list, shapes):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    lib = F.lib
    table = []
    prev_mode = lib.cigemv_set_mode(1)
    try:
        for n, k in shapes:
            copies = ROTATE_BYTES // (n * k) + 2          # > 256 MB of distinct weights
            CBs = [torch.randint(-128, 128, (n, k), device=dev, dtype=torch.int8, generator=gen) for _ in range(copies)]
            SCB = torch.rand(n, device=dev, generator=gen) + 0.5
            bias = torch.randn(n, device=dev, generator=gen).half()
            layers = {arm: [make_layer(CB, SCB, bias, args.threshold, arm == "fused", arm == "prefill") for CB in CBs]
                      for arm in ("unfused", "fused", "prefill")}
            for rows in rows_list:
                A = torch.randn(rows, k, device=dev, generator=gen).clamp_(-5, 5).half()
                cols = torch.randperm(k, device=dev, generator=gen)[:args.outlier_cols]
                for i, c in enumerate(cols.tolist()):
                    A[i % rows, c] = (8.0 + (i * 13) % 53) * (1 if i % 2 == 0 else -1)
                outs = {}

                def arm_calls(arm):
                    def call(lin):
                        def run():
                            outs[arm] = lin(A)
                        return run
                    return [call(lin) for lin in layers[arm]]

                # the decode arm where its kernel exists: beyond 32 rows that layer is the unfused one
                fused_arms = (["fused"] if rows <= F.IGEMV_MAX_ROWS else []) + ["prefill"]
                calls = {arm: arm_calls(arm) for arm in ["unfused"] + fused_arms}
                with torch.no_grad():
                    for arm in calls:                     # warm-up; both end on the last weight
                        for c in calls[arm]:
                            c()
                    torch.cuda.synchronize()
                    diff = {arm: float((outs["unfused"].float() - outs[arm].float()).abs().max()) for arm in fused_arms}
                    scale = float(outs["unfused"].float().abs().max())
                    iters = {}
                    for arm in calls:
                        ms = max(eager_window_ms(calls[arm], 1), 1e-3)
                        iters[arm] = max(2, int(args.window * 1e3 / ms) + 1)
                    res = {arm: [] for arm in list(calls) + [a + "_graph" for a in fused_arms]}
                    for _ in range(REPS):
                        for arm in calls:
                            res[arm].append(eager_window_ms(calls[arm], iters[arm]) * 1e3 / iters[arm] / copies)
                        # captured anew after the eager windows: on an MI355X a graph of the prefill layer forward
                        # (its tensors allocated in the graph's pool) that was instantiated BEFORE the unfused forward
                        # ran replayed about ten times slower from then on (758 against 74 us per call at 1024 rows
                        # on 4096 x 4096); a fresh capture does not (cause not found)
                        for arm in fused_arms:
                            g = capture(calls[arm])
                            g_iters = max(3, int(args.window * 1e3 / max(window_ms(g, 3) / 3, 1e-3)) + 1)
                            res[arm + "_graph"].append(window_ms(g, g_iters) * 1e3 / g_iters / copies)
                            del g
                row = {"n": n, "k": k, "rows": rows, "copies": copies, "threshold": args.threshold,
                       "outlier_cols": args.outlier_cols, "max_abs_out": scale,
                       **{arm: summarise(ts) for arm, ts in res.items()}}
                line = (f"{n:5d} x {k:5d} rows {rows:4d} thr {args.threshold:g} cols {args.outlier_cols}: unfused "
                        f"{row['unfused']['median_us']:8.2f} us [{row['unfused']['min_us']:.2f}.."
                        f"{row['unfused']['max_us']:.2f}]")
                for arm in fused_arms:
                    # a fused forward wins when even its slowest repetition beats the unfused forward's fastest
                    row[arm + "_wins_beyond_spread"] = row[arm]["max_us"] < row["unfused"]["min_us"]
                    row["max_abs_diff" if arm == "fused" else arm + "_max_abs_diff"] = diff[arm]
                    line += (f"  {arm} {row[arm]['median_us']:8.2f} us [{row[arm]['min_us']:.2f}.."
                             f"{row[arm]['max_us']:.2f}]  {arm} graph {row[arm + '_graph']['median_us']:8.2f} us  "
                             f"max |diff| {diff[arm]:.4g} of {scale:.4g}")
                table.append(row)
                print(line, flush=True)
            del CBs, layers
            torch.cuda.empty_cache()
    finally:
        lib.cigemv_set_mode(prev_mode)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "window_s": args.window,
                   "threshold": args.threshold, "outlier_cols": args.outlier_cols, "table": table}, f, indent=1)
    print(f"wrote {args.out}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,2,4,8,16,32")
    ap.add_argument("--shapes", default="11008x4096,4096x11008,4096x4096,8192x28672")
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--outlier-cols", type=int, default=8)
    args = ap.parse_args()
    rows_list = [int(r) for r in args.rows.split(",")]
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.out is None:
        name = "int8_decode_ab.json"
        if args.threshold > 0.0:
            prefill_only = min(rows_list) > F.IGEMV_MAX_ROWS
            name = "int8_outlier_prefill_ab.json" if prefill_only else "int8_outlier_decode_ab.json"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.threshold > 0.0:
        return main_outlier(args, rows_list, shapes)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(7)
    lib = F.lib
    table, mismatches = [], 0
    prev_mode = lib.cigemv_set_mode(0)
    try:
        for n, k in shapes:
            copies = ROTATE_BYTES // (n * k) + 2          # > 256 MB of distinct weights
            CBs = [torch.randint(-128, 128, (n, k), device=dev, dtype=torch.int8, generator=gen) for _ in range(copies)]
            SCB = torch.rand(n, device=dev, generator=gen) + 0.5
            bias = torch.randn(n, device=dev, generator=gen).half()
            for rows in rows_list:
                A = (torch.randn(rows, k, device=dev, generator=gen) * 3).half()
                CA, SCA = F.int8_row_quant(A)
                outs = {a: torch.empty(rows, n, device=dev, dtype=torch.float16) for a in ("old", "new")}
                nbytes = n * k + rows * k + 2 * rows * n + 4 * n

                def product(arm, CB):
                    return lambda: F.igemmlt_dequant(CA, CB, SCA, SCB, bias=bias, out=outs[arm])

                def forward_old(CB):
                    def run():
                        ca, sca = F.int8_row_quant(A)
                        F.igemmlt_dequant(ca, CB, sca, SCB, bias=bias, out=outs["old"])
                    return run

                def forward_new(CB):
                    return lambda: F.int8_linear_rows(A, CB, SCB, bias=bias, out=outs["new"])

                for step in ("product", "forward"):
                    for residency, ws in (("hot", [CBs[0]] * copies), ("hbm", CBs)):
                        lib.cigemv_set_mode(-1)
                        g_old = capture([product("old", w) if step == "product" else forward_old(w) for w in ws])
                        lib.cigemv_set_mode(1)
                        g_new = capture([product("new", w) if step == "product" else forward_new(w) for w in ws])
                        # both graphs end on the last weight of the list: the outputs must be the same bytes
                        g_old.replay()
                        g_new.replay()
                        torch.cuda.synchronize()
                        equal = bool(torch.equal(outs["old"], outs["new"]))
                        mismatches += 0 if equal else 1
                        r = ab({"old": g_old, "new": g_new}, len(ws), args.window)
                        old, new = summarise(r["old"]), summarise(r["new"])
                        row = {"n": n, "k": k, "rows": rows, "step": step, "residency": residency, "copies": len(ws),
                               "old": old, "new": new, "equal": equal, "bytes": nbytes,
                               "new_share_of_8.0TBs": nbytes / (new["median_us"] * 1e-6) / (PEAK_SPEC_TBS * 1e12),
                               "new_share_of_6.29TBs": nbytes / (new["median_us"] * 1e-6) / (PEAK_COPY_TBS * 1e12),
                               # the new route wins when even its slowest repetition beats the old route's fastest
                               "new_wins_beyond_spread": new["max_us"] < old["min_us"]}
                        table.append(row)
                        print(f"{n:5d} x {k:5d} rows {rows:2d} {step:8s} {residency:3s}: old {old['median_us']:8.2f} us "
                              f"[{old['min_us']:.2f}..{old['max_us']:.2f}]  new {new['median_us']:8.2f} us "
                              f"[{new['min_us']:.2f}..{new['max_us']:.2f}]  {row['new_share_of_8.0TBs'] * 100:5.1f} % of "
                              f"8.0 TB/s  equal={equal}", flush=True)
                        del g_old, g_new
            del CBs
            torch.cuda.empty_cache()
    finally:
        lib.cigemv_set_mode(prev_mode)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": REPS, "window_s": args.window,
                   "peak_spec_TBs": PEAK_SPEC_TBS, "peak_copy_TBs": PEAK_COPY_TBS, "mismatches": mismatches,
                   "table": table}, f, indent=1)
    print(f"wrote {args.out}; mismatches: {mismatches}")
    return 1 if mismatches else 0


if __name__ == "__main__":
    sys.exit(main())
