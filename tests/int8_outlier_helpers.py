"""numpy restatement of the threshold > 0 LLM.int8 decode forward (csrc/igemv8_outlier.hip), built on oracle.ref, with
the tolerance its GPU tests assert.

  S          = columns of A holding a value with |a| >= thr
  rowStat    = oracle colrow_absmax(A, thr)'s row half
  q          = oracle double_quant(A, rowStat, ., thr)'s row half with the whole columns of S zeroed
  v32        = ((float(q . B^T) * 6.200012e-05f) * rowStat) * colStats in fp32 -- bit-equal to the kernel's (exact int32
               sum, the same three fp32 products)
  exact      = float64(v32) + bias + (colStats / 127) * sum_{c in S} A[r, c] * B[j, c]           (float64)

Tolerance (derived, not measured): the kernel rounds to fp16 once, after at most |S| + 3 fp32 operations past v32
(|S| additions of exact products, colStats / 127, its product with the sum, two additions), each within 2^-24 relative
of a partial result that is bounded by the sum of magnitudes; twice that first-order bound, for any summation order:

  tol = ulp16(exact) / 2 + (|S| + 4) * 2^-23 * (|v32| + |bias| + (colStats / 127) * sum_{c in S} |A[r, c] * B[j, c]|)

The unfused composition (double_quant, whole-column zeroing, igemmlt_dequant, fp16 outlier matmul, fp16 add) rounds its
three intermediates to fp16 and the dequantised weight columns to fp16 (2^-11 relative) before the outlier product:

  unfused_tol = tol + ulp16(v32 + bias) / 2 + ulp16(side) / 2 + 2^-11 * (colStats / 127) * sum |A * B|
                    + ulp16(|exact| + the two terms before) / 2
"""
import numpy as np

from oracle import ref

F32 = np.float32
FP16_MAX = 65504.0


def ulp16(x):
    """The spacing of fp16 at |x| (float64 in, float64 out): 2^(e - 10) in the binade 2^e, 2^-24 below 2^-14."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def outlier_reference(A, B, col_stats, bias, thr):
    """A fp16 [M, K], B int8 [N, K], col_stats fp32 [N], bias fp16 [N] or None, thr > 0.
    Returns a dict: row_stats (fp32 [M]), S (ascending column indices), v32, exact, tol, unfused_tol ([M, N])."""
    A = np.asarray(A, dtype=np.float16)
    B = np.asarray(B, dtype=np.int8)
    cs = np.asarray(col_stats, dtype=F32)
    with np.errstate(invalid="ignore"):
        row_stats, _, _ = ref.colrow_absmax(A, thr)
        a32 = A.astype(F32)
        S = np.flatnonzero((np.abs(a32) >= F32(thr)).any(axis=0))
        q, _ = ref.double_quant(A, row_stats, np.ones(A.shape[1], dtype=F32), thr)
    q = q.copy()
    q[:, S] = 0                                             # the whole column leaves the int8 product
    acc = ref.igemmlt(q, B).astype(F32)
    v32 = (acc * ref.MM_DEQUANT_CONST).astype(F32)
    v32 = (v32 * row_stats[:, None]).astype(F32)
    v32 = (v32 * cs[None, :]).astype(F32)
    b64 = np.zeros(B.shape[0]) if bias is None else np.asarray(bias, dtype=np.float16).astype(np.float64)
    aS, bS = A[:, S].astype(np.float64), B[:, S].astype(np.float64)
    scale = cs.astype(np.float64) / 127.0
    side = (aS @ bS.T) * scale[None, :]
    side_abs = (np.abs(aS) @ np.abs(bS).T) * scale[None, :]
    first = v32.astype(np.float64) + b64[None, :]
    exact = first + side
    mags = np.abs(v32.astype(np.float64)) + np.abs(b64)[None, :] + side_abs
    tol = 0.5 * ulp16(exact) + (len(S) + 4) * 2.0 ** -23 * mags
    e12 = 0.5 * ulp16(first) + 0.5 * ulp16(side) + 2.0 ** -11 * side_abs
    unfused_tol = tol + e12 + 0.5 * ulp16(np.abs(exact) + e12)
    return {"row_stats": row_stats, "S": S, "v32": v32, "exact": exact, "tol": tol, "unfused_tol": unfused_tol}


def entry_only_reference(A, B, col_stats, bias, thr):
    """What the forward would be if only the entries |a| >= thr left the int8 product (double_quant's own zeroing)
    and only they entered the side product, rounded to fp16: the whole-column rule must not give these bits."""
    A = np.asarray(A, dtype=np.float16)
    cs = np.asarray(col_stats, dtype=F32)
    row_stats, _, _ = ref.colrow_absmax(A, thr)
    q, _ = ref.double_quant(A, row_stats, np.ones(A.shape[1], dtype=F32), thr)
    v = ref.igemmlt(q, B).astype(np.float64) * float(ref.MM_DEQUANT_CONST) * row_stats[:, None] * cs[None, :]
    a_out = np.where(np.abs(A.astype(F32)) >= F32(thr), A.astype(np.float64), 0.0)
    side = (a_out @ np.asarray(B, dtype=np.float64).T) * (cs.astype(np.float64) / 127.0)[None, :]
    b64 = 0.0 if bias is None else np.asarray(bias, dtype=np.float16).astype(np.float64)[None, :]
    return (v + b64 + side).astype(np.float16)
