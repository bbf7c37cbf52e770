"""Lab: what does reading a K-strided int8 operand in place cost, against copying it K-contiguous first?

For C = A @ B with A [m, k], B [k, n] int8 (batched or not), each of the three forms that hand functional.igemm a
transposed view -- NN (B K-strided), TT (A K-strided), TN (both) -- is timed against what the package offered before
igemm: functional.igemm_rowmajor(A, Bt) on operands made K-contiguous with .t().contiguous(), copy included.  The
batched baseline loops igemm_rowmajor over the batch after one batched copy.  The both-K-contiguous form (NT, no copy
needed) and the box's int8 MFMA rate from the library's probe kernel (csrc/probe.hip, as bench.py measures it) give
the scale; unbatched, NT is also forced onto the new kernel's K-contiguous instance (NT_on_strided_kernel), which
separates the cost of the transposition from that of the 128 x 128 geometry.  Outputs of the two sides are compared
for equality at the timed sizes first; a mismatch ends the run.  The third shape, 4096 x 4104 x 4096, stores B [k, n]
with a leading dimension that is no multiple of 16 B: in NN and TN the K-strided B takes the kernel's guarded bytewise
loads (the baseline's copy of B is aligned again).

Timing: device events around `inner` back-to-back calls, `reps` windows per side, the two sides alternating, after a
warm-up of both; medians reported.  Writes a JSON (default profiles/igemm_strided_lab.json).

  python tools/igemm_strided_lab.py [--out FILE] [--reps 7] [--quick]
"""
import argparse
import ctypes as ct
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bitsandbytes-sycl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import python_src_quants.functional as F  # noqa: E402


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / inner          # us per call


def ab(fns, inner, reps, warm_s=0.3):
    """Median us per call of each function in `fns`, windows alternating between them."""
    t_end = time.perf_counter() + warm_s
    while time.perf_counter() < t_end:
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(window(fn, inner))
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in ts.items()}


def int8_peak_tops(dev, reps=5):
    blocks, iters = 256, 40000
    sink = torch.empty(blocks * 512, device=dev)
    best = 0.0
    for waves, kind in ((4, 1), (8, 3)):
        F.pre_call(dev)
        t_end = time.perf_counter() + 0.3
        while time.perf_counter() < t_end:
            F.lib.cprobe_mfma(kind, blocks, iters, 7, F.get_ptr(sink))
            torch.cuda.synchronize()
        ts = [window(lambda: F.lib.cprobe_mfma(kind, blocks, iters, 7, F.get_ptr(sink)), 1) for _ in range(reps)]
        best = max(best, blocks * waves * 8 * iters * (16 * 16 * 64 * 2) / (statistics.median(ts) * 1e-6) / 1e12)
    return best


def rand_i8(dev, *shape):
    return torch.randint(-128, 128, shape, dtype=torch.int8, device=dev)


def forms(dev, nb, m, n, k):
    """name -> (new-form call, baseline call, check).  Storage: 'N' operand contiguous as the matmul reads it."""
    lead = (nb,) if nb else ()
    tr = (lambda t: t.transpose(-1, -2))
    A, At = rand_i8(dev, *lead, m, k), rand_i8(dev, *lead, k, m)       # At: A stored transposed ([k, m])
    B, Bt = rand_i8(dev, *lead, k, n), rand_i8(dev, *lead, n, k)       # Bt: B stored transposed ([n, k])
    out = torch.empty(*lead, m, n, dtype=torch.int32, device=dev)
    out2 = torch.empty_like(out)

    def rowmajor(a_kc, b_kc, o):            # what the parent offers: C = a_kc @ b_kc^T, both K-contiguous, 2-D
        if nb:
            for i in range(nb):
                F.igemm_rowmajor(a_kc[i], b_kc[i], out=o[i])
        else:
            F.igemm_rowmajor(a_kc, b_kc, out=o)

    table = {
        # B [k, n] contiguous: K-strided for the product
        "NN": (lambda: F.igemm(A, B, out=out), lambda: rowmajor(A, tr(B).contiguous(), out2)),
        # A handed over as the transpose of a contiguous [k, m]
        "TT": (lambda: F.igemm(tr(At), tr(Bt), out=out), lambda: rowmajor(tr(At).contiguous(), Bt, out2)),
        # both K-strided (grad_B = A^T @ G)
        "TN": (lambda: F.igemm(tr(At), B, out=out),
               lambda: rowmajor(tr(At).contiguous(), tr(B).contiguous(), out2)),
        # both K-contiguous: no copy on either side (scale only)
        "NT": (lambda: F.igemm(A, tr(Bt), out=out), lambda: rowmajor(A, Bt, out2)),
    }
    if not nb:
        # the same both-K-contiguous product forced onto k_igemm_strided<KC, KC>: cbatched_igemm with one batch always
        # runs the new kernel (cigemm sends this form to the existing 256 x 256 route).  Row-major out = A @ Bt^T is the
        # column-major product with the library's A = Bt (transposed), B = A.
        def nt_strided():
            F.pre_call(dev)
            F.lib.cbatched_igemm(None, ct.c_bool(True), ct.c_bool(False), ct.c_int32(n), ct.c_int32(m), ct.c_int32(k),
                                 F.get_ptr(Bt), F.get_ptr(A), F.get_ptr(out), ct.c_int32(k), ct.c_int32(k),
                                 ct.c_int32(n), ct.c_long(0), ct.c_long(0), ct.c_long(0), ct.c_int32(1))
        table["NT_on_strided_kernel"] = (nt_strided, table["NT"][1])
    return table, out, out2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "igemm_strided_lab.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("igemm_strided_lab needs a GPU")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = [(0, 256, 256, 256), (2, 128, 128, 128)] if args.quick else [(0, 4096, 4096, 4096), (16, 512, 512, 512),
                                                                                (0, 4096, 4104, 4096)]
    res = {"device": torch.cuda.get_device_name(0), "int8_mfma_peak_tops": round(int8_peak_tops(dev), 1),
           "method": "device events around `inner` back-to-back calls; median of `reps` windows, sides alternating",
           "reps": args.reps, "shapes": []}
    for nb, m, n, k in shapes:
        table, out, out2 = forms(dev, nb, m, n, k)
        ops = 2.0 * max(nb, 1) * m * n * k
        inner = 20 if ops >= 1e11 else 50
        entry = {"batch": nb, "m": m, "n": n, "k": k, "inner": inner, "forms": {}}
        for name, (new, base) in table.items():
            new()
            base()
            torch.cuda.synchronize()
            same = bool(torch.equal(out, out2))
            if not same:
                raise SystemExit(f"igemm_strided_lab: form {name} at batch {nb}, {m} x {n} x {k}: igemm and the "
                                 "copy + igemm_rowmajor baseline disagree; nothing timed")
            t = ab({"igemm": new, "copy_then_rowmajor": base}, inner, args.reps)
            entry["forms"][name] = {
                "equal_outputs": same, "igemm": t["igemm"], "copy_then_rowmajor": t["copy_then_rowmajor"],
                "ratio_igemm_over_baseline": round(t["igemm"]["median_us"] / t["copy_then_rowmajor"]["median_us"], 3),
                "igemm_tops": round(ops / (t["igemm"]["median_us"] * 1e-6) / 1e12, 1),
                "igemm_share_of_measured_peak": round(ops / (t["igemm"]["median_us"] * 1e-6) / 1e12 /
                                                      res["int8_mfma_peak_tops"], 3)}
            print(name, entry["forms"][name], flush=True)
        res["shapes"].append(entry)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
