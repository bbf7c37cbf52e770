"""One fp32 Adam step with 8-bit state at 2^27 elements: the global-max path (F.optimizer_update_8bit, three
launches) beside the blockwise path (F.optimizer_update_8bit_blockwise, one launch), same process, interleaved.

Each round times `--iters` consecutive steps of one path between two device events, then the same for the
other; the per-step times of all rounds are reported with their median, and the achieved bytes/s from the
traffic the algorithm needs (blockwise 16 B/element: g, p read + write, two state bytes read + write; global
max 22 B/element: the precondition reads g and the two state bytes once more).

    python tools/optim_static8_ab.py [--log2n 27] [--rounds 9] [--iters 100] [--warmup 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "bitsandbytes-sycl_amd")):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch  # noqa: E402

import python_src_quants.functional as F  # noqa: E402

BYTES = {"blockwise": 16, "global_max": 22}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    n = 1 << args.log2n
    gen = torch.Generator(device=dev).manual_seed(0)
    g = torch.randn(n, device=dev, generator=gen) * 0.01
    q1, q2 = F.create_dynamic_map(signed=True).to(dev), F.create_dynamic_map(signed=False).to(dev)

    def codes():
        return torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)

    bw = dict(p=torch.randn(n, device=dev, generator=gen) * 0.1, s=codes(),
              a=[torch.zeros((n + 2047) // 2048, device=dev) for _ in range(2)], step=0)
    gm = dict(p=bw["p"].clone(), s=codes(), m=[torch.zeros(1, device=dev) for _ in range(4)], step=0)

    def blockwise():
        bw["step"] += 1
        F.optimizer_update_8bit_blockwise("adam", g, bw["p"], bw["s"][0], bw["s"][1], 0.9, 0.999, 1e-8, bw["step"], 1e-3,
                                          q1, q2, bw["a"][0], bw["a"][1], 0.0)

    def global_max():
        gm["step"] += 1
        m = gm["m"]
        F.optimizer_update_8bit("adam", g, gm["p"], gm["s"][0], gm["s"][1], 0.9, 0.999, 1e-8, gm["step"], 1e-3, q1, q2,
                                m[0], m[1], m[2], m[3], 0.0)
        gm["m"] = [m[2], m[3], m[0], m[1]]

    paths = {"blockwise": blockwise, "global_max": global_max}
    for fn in paths.values():                      # warm-up: code objects, the workspace, both max buffers
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(args.rounds):
        for name, fn in paths.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) * 1e3 / args.iters)   # us per step
    lines = []
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append(json.dumps({"path": name, "n": n, "dtype": "fp32", "optimizer": "adam", "iters": args.iters,
                                 "us_per_step": [round(t, 1) for t in ts], "median_us": round(med[name], 1),
                                 "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                                 "bytes_per_element": BYTES[name],
                                 "achieved_TB_per_s": round(BYTES[name] * n / med[name] / 1e6, 3)}))
    lines.append(json.dumps({"ratio_global_max_over_blockwise": round(med["global_max"] / med["blockwise"], 3),
                             "traffic_ratio": round(BYTES["global_max"] / BYTES["blockwise"], 3),
                             "device": torch.cuda.get_device_name(0)}))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
