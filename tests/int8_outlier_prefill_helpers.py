"""numpy restatement of the threshold > 0 LLM.int8 prefill forward without a host round trip
(csrc/int8_outlier_prefill.hip, F.int8_linear_outliers), built on oracle.ref and int8_outlier_helpers, with the tolerance
its GPU tests assert.

  S          = columns of A holding a value with |a| >= thr                                (fp32 compare)
  row_stats  = oracle colrow_absmax(A, thr)'s row half
  CA         = oracle double_quant(A, row_stats, ., thr)'s row half with the whole columns of S zeroed
  v32        = ((float(CA . B^T) * 6.200012e-05f) * row_stats) * colStats in fp32   (outlier_reference's, bit-defined)
  first16    = fp16(v32 + float32(bias))                             -- the bits of igemmlt_dequant(CA, B, ...)
  exact      = float64(first16) + (colStats / 127) * sum_{c in S} A[r, c] * B[j, c]           (float64)

Tolerance (derived, not measured): after the bit-defined first16 the side kernel does |S| additions of exact products,
the division colStats / 127, its product with the sum and the final addition, each within 2^-24 relative of a partial
result bounded by the sum of magnitudes; that first-order bound is doubled, and the one rounding to fp16 follows:

  tol = ulp16(exact) / 2 + (|S| + 3) * 2^-23 * (|first16| + (colStats / 127) * sum_{c in S} |A[r, c] * B[j, c]|)

`unfused_tol` and `unfused_exact` are outlier_reference's: what the unfused composition (the fallback of uncovered
shapes, and the default layer) is held to.
"""
import numpy as np

from int8_outlier_helpers import FP16_MAX, outlier_reference, ulp16
from oracle import ref

F32 = np.float32


def mask_bytes(k):
    """Bytes of the workspace's column bit mask: one bit per column, padded to 16 bytes."""
    return ((k + 31) // 32 * 4 + 15) // 16 * 16


def workspace_layout(k):
    """(bytes, int32 index of count, int32 index of idx[0]) of the workspace the C entries document: the count, 12
    unused bytes, the bit mask, idx[k]."""
    head = 16 + mask_bytes(k)
    return head + 4 * k, 0, head // 4


def prefill_reference(A, B, col_stats, bias, thr):
    """A fp16 [M, K], B int8 [N, K], col_stats fp32 [N], bias fp16 [N] or None, thr > 0.
    Returns a dict: S (ascending column indices), row_stats (fp32 [M]), CA (int8 [M, K]), first16 (fp16 [M, N]),
    exact, tol (float64 [M, N]), and outlier_reference's unfused_exact / unfused_tol."""
    A = np.asarray(A, dtype=np.float16)
    B = np.asarray(B, dtype=np.int8)
    cs = np.asarray(col_stats, dtype=F32)
    r = outlier_reference(A, B, cs, bias, thr)
    S, row_stats, v32 = r["S"], r["row_stats"], r["v32"]
    with np.errstate(invalid="ignore", divide="ignore"):
        CA, _ = ref.double_quant(A, row_stats, np.ones(A.shape[1], dtype=F32), thr)
    CA = CA.copy()
    CA[:, S] = 0
    first32 = v32 if bias is None else (v32 + np.asarray(bias, dtype=np.float16).astype(F32)[None, :]).astype(F32)
    first16 = first32.astype(np.float16)
    aS, bS = A[:, S].astype(np.float64), B[:, S].astype(np.float64)
    scale = cs.astype(np.float64) / 127.0
    side = (aS @ bS.T) * scale[None, :]
    side_abs = (np.abs(aS) @ np.abs(bS).T) * scale[None, :]
    exact = first16.astype(np.float64) + side
    assert float(np.abs(exact).max()) < FP16_MAX
    tol = 0.5 * ulp16(exact) + (len(S) + 3) * 2.0 ** -23 * (np.abs(first16.astype(np.float64)) + side_abs)
    return {"S": S, "row_stats": row_stats, "CA": CA, "first16": first16, "exact": exact, "tol": tol,
            "unfused_exact": r["exact"], "unfused_tol": r["unfused_tol"]}
