"""One default-route gemm_4bit call per row of the few-token plan table (tests/golden/fewtoken_plan_v1.json), in table
order, and the SHA-256 of every output.

Run it under a kernel trace (rocprofv3 --kernel-trace -- python tools/fewtoken_plan_dump.py): the weights are
quantised and the device synchronised before the first call, so the trace's 4-bit GEMM / GEMV kernels after that point
are, in order, the table's rows (a k_skinny_reduce / k_splitk_reduce belongs to the row before it).  That trace is the
source of the table's recorded plans; the hashes compare two builds bit for bit.

usage: fewtoken_plan_dump.py [--table FILE] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitsandbytes-sycl_amd")]
import python_src_quants.functional as F  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=os.path.join(ROOT, "tests", "golden", "fewtoken_plan_v1.json"))
    ap.add_argument("--out", default="fewtoken_plan_sha256.json")
    args = ap.parse_args()
    with open(args.table) as f:
        table = json.load(f)["rows"]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    work = []
    for r in table:
        W = (torch.randn(r["N"], r["K"], device=dev, generator=g) * 0.02).to(torch.bfloat16)
        q, st = F.quantize_4bit(W, blocksize=r["blocksize"], quant_type="nf4", compress_statistics=bool(r["nested"]))
        if r["nested"]:
            assert st.state2.blocksize == r["blocksize2"], (st.state2.blocksize, r)
        X = torch.randn(r["rows"], r["K"], device=dev, dtype=torch.bfloat16, generator=g)
        work.append((X, q, st, torch.empty(r["rows"], r["N"], device=dev, dtype=torch.bfloat16)))
    torch.cuda.synchronize()
    for X, q, st, out in work:
        F.gemm_4bit(X, q, st, out=out)
    torch.cuda.synchronize()
    sums = [hashlib.sha256(out.cpu().view(torch.int16).numpy().tobytes()).hexdigest() for _, _, _, out in work]
    with open(args.out, "w") as f:
        json.dump([dict(N=r["N"], rows=r["rows"], K=r["K"], blocksize=r["blocksize"], nested=r["nested"], sha256=s)
                   for r, s in zip(table, sums)], f, indent=1)
    print(f"{len(sums)} rows -> {args.out}")


if __name__ == "__main__":
    main()
