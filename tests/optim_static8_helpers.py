"""numpy restatement of one optimizer step with 8-bit states quantised against one global maximum per state
tensor (csrc/optim.hip: k_static8_precondition, k_static8_finish, k_optimizer_8bit_static), in the style of
tests/optim_norm_helpers.py.

  precondition, 2 / 1 states  kPreconditionOptimizerStatic8bit{2,1}State  ref:sycl/sycl_code/kernel_quant.cpp:2030-2174, 2369-2474
  update, 2 / 1 states        kOptimizerStatic8bit{2,1}State              ref:sycl/sycl_code/kernel_quant.cpp:2180-2367, 2476-2645

Every fp32 operation is one numpy float32 operation, in the reference's association, with the departures of
DESIGN.md §2 (Q28-Q35): every element is updated, new_max is the exact maximum of the new state values (weight
decay included) and replaces what new_max held, the re-quantisation quotient is the IEEE division s / new_max
(oracle.optim._requant), momentum's state takes the scaled and weight-decayed gradient, Adam's decayed weight
is not multiplied by update_scale.  The update norm is the fp64 sum of the fp32 squares, taken in the fixed
order of the kernels (fixed_order_sum) and rounded once to fp32.

With one 2048-block, max = the previous step's absmax and max_unorm = 0, static_step equals
oracle.optim.update_8bit_blockwise bit for bit (tests/test_optim_static8_cpu.py), which pins this file to the
frozen oracle.
"""
import math

import numpy as np

from oracle import optim as oref
from oracle.ref import F32, FLT_MAX, as_f32, cast_out

CHUNK, SLOTS, THREADS, NPT = 4096, 1024, 256, 8    # the partition of csrc/optim.hip
NAMES = ("adam", "momentum", "rmsprop", "lion")
UNORM_NAMES = ("adam", "momentum")


def _wg_sum256(v):
    """wg_sum256 over the last axis (256 accumulators): per wave a butterfly over lane distances 32..1, then
    (w0 + w1) + (w2 + w3)."""
    v = v.reshape(v.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ d]
    w = v[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def fixed_order_sum(terms):
    """The fp64 sum of `terms` in the order of k_sumsq_partials / k_sumsq_finish: slot b takes chunks b,
    b + 1024, ...; thread t adds elements [8t, 8t + 8) and [2048 + 8t, 2048 + 8t + 8) of a chunk to one
    accumulator; wg_sum256 per slot; thread t of the finishing workgroup adds slots t, t + 256, t + 512, t + 768;
    wg_sum256.  Missing elements and slots add +0.0, which leaves the non-negative sums unchanged."""
    terms = np.asarray(terms, np.float64).reshape(-1)
    chunks = -(-terms.size // CHUNK)
    rounds = max(1, -(-chunks // SLOTS))
    per_round = min(max(chunks, 1), SLOTS)         # more than one round only when every slot is taken
    full = np.zeros(rounds * per_round * CHUNK, np.float64)
    full[:terms.size] = terms
    v = full.reshape(rounds, per_round, 2, THREADS, NPT)
    acc = np.zeros((per_round, THREADS), np.float64)
    for r in range(rounds):
        for h in range(2):
            for j in range(NPT):
                acc = acc + v[r, :, h, :, j]
    partial = np.zeros(SLOTS, np.float64)
    partial[:per_round] = _wg_sum256(acc)
    fin = np.zeros(THREADS, np.float64)
    for q in range(SLOTS // THREADS):
        fin = fin + partial[q * THREADS:(q + 1) * THREADS]
    return _wg_sum256(fin)


def update_scale(unorm, max_unorm, param_norm):
    """kernel_quant.cpp:2211-2217, 2499-2505: the static kernels add no eps to the bound."""
    if not max_unorm > 0.0:
        return F32(1.0)
    un = np.sqrt(F32(unorm)).astype(F32)
    bound = F32(F32(max_unorm) * F32(param_norm))
    return F32(bound / un) if un > bound else F32(1.0)


def static_step(name, g, p, c1, c2, code1, code2, max1, max2, beta1, beta2, eps, step, lr, weight_decay=0.0,
                gnorm_scale=1.0, dtype="fp32", max_unorm=0.0, param_norm=0.0, code_idx=None):
    """One step.  g, p: arrays in `dtype` storage (bf16 as uint16 bits); c1, c2: uint8 codes (c2 None for one
    state); max1, max2: the fp32 maxima the codes were stored against.  Returns (p_new in `dtype` storage, c1,
    c2, new_max1, new_max2, unorm, update_scale); new_max2 is None for one state, unorm None without max_unorm.
    With `code_idx` (an index array) only those elements are re-quantised and the returned c1, c2 hold them
    alone: the numpy search dominates the cost at millions of elements; everything else is always computed in
    full."""
    if name not in NAMES:
        raise ValueError(name)
    if max_unorm > 0.0 and name not in UNORM_NAMES:
        raise ValueError(f"max_unorm with {name}")
    opt = oref.NAME2OPT[name]
    k = oref.scalars(beta1, beta2, eps, step, lr, weight_decay)
    b1, b2, eps, lr, wd, gsc = F32(beta1), F32(beta2), F32(eps), F32(lr), F32(weight_decay), F32(gnorm_scale)
    one = F32(1.0)
    code1 = np.asarray(code1, F32)
    gv = as_f32(np.asarray(g).reshape(-1), dtype)
    pv = as_f32(np.asarray(p).reshape(-1), dtype)
    q1 = np.asarray(c1).reshape(-1).astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        gs = (gsc * gv).astype(F32)
        d1 = (code1[q1] * F32(max1)).astype(F32)
        s2 = None
        if opt == oref.ADAM:
            code2 = np.asarray(code2, F32)
            q2 = np.asarray(c2).reshape(-1).astype(np.int64)
            d2 = (code2[q2] * F32(max2)).astype(F32)
            s1 = (d1 * b1 + ((one - b1) * gs).astype(F32)).astype(F32)
            s2 = (d2 * b2 + (((one - b2) * gs).astype(F32) * gs).astype(F32)).astype(F32)
        else:
            if wd > 0 and opt in (oref.MOMENTUM, oref.RMSPROP):
                gs = (gs + (pv * wd).astype(F32)).astype(F32)
            if opt == oref.MOMENTUM:
                s1 = gs if step == 1 else (d1 * b1 + gs).astype(F32)
            elif opt == oref.LION:
                s1 = (d1 * b2 + ((one - b2) * gs).astype(F32)).astype(F32)
            else:
                s1 = (d1 * b1 + ((one - b1) * (gs * gs).astype(F32)).astype(F32)).astype(F32)
        # precondition: the exact maxima of what is quantised, and the update norm
        nm1 = F32(np.fmax.reduce(np.abs(s1), initial=-FLT_MAX))
        nm2 = F32(np.fmax.reduce(np.abs(s2), initial=-FLT_MAX)) if opt == oref.ADAM else None
        unorm = None
        if max_unorm > 0.0:
            if opt == oref.ADAM:
                # 1.0f / (1.0f - pow(beta, step)): pow(float, int) is double, the quotient is rounded once
                pc1 = F32(1.0 / (1.0 - math.pow(float(b1), float(step))))
                pc2 = F32(1.0 / (1.0 - math.pow(float(b2), float(step))))
                u = ((s1 * pc1).astype(F32) / (np.sqrt((s2 * pc2).astype(F32)).astype(F32) + eps).astype(F32)).astype(F32)
            else:
                u = s1
            unorm = F32(fixed_order_sum((u * u).astype(F32).astype(np.float64)))
        us = update_scale(unorm, max_unorm, param_norm)
        # update
        if opt == oref.ADAM:
            upd = (F32(us * k["step_size"]) * (s1 / (np.sqrt(s2).astype(F32) + k["c2eps"]).astype(F32)).astype(F32))
            pn = oref._t((pv + upd.astype(F32)).astype(F32), dtype)
            if wd > 0:
                pn = oref._t((pn * k["decay"]).astype(F32), dtype)
        elif opt == oref.MOMENTUM:
            pn = (pv + (F32(-lr * us) * s1).astype(F32)).astype(F32)
        elif opt == oref.LION:
            pd = oref._t((pv * k["decay"]).astype(F32), dtype) if wd > 0 else pv
            t = (d1 * b1 + ((one - b1) * gs).astype(F32)).astype(F32)
            pn = (pd - (lr * oref._sgn(t)).astype(F32)).astype(F32)
        else:
            pn = (pv - ((lr * gs).astype(F32) / (np.sqrt(s1).astype(F32) + eps).astype(F32)).astype(F32)).astype(F32)
        pick = (lambda a: a) if code_idx is None else (lambda a: a[code_idx])
        n1 = oref._requant(code1, pick(s1), np.full(pick(s1).size, nm1, F32), True)
        n2 = oref._requant(code2, pick(s2), np.full(pick(s2).size, nm2, F32), False) if opt == oref.ADAM else None
    return cast_out(pn, dtype), n1, n2, nm1, nm2, unorm, us
