"""numpy restatement of the reference's norm-clipped 32-bit optimizer step, for the tests of percentile
clipping, max_unorm and LAMB (the frozen oracle, oracle/optim.py, covers max_unorm = 0 only).

  gradient norm        kPercentileClipping                ref:sycl/sycl_code/kernel_quant.cpp:2653-2703
  update norm, Adam    kPreconditionOptimizer32bit2State  ref:sycl/sycl_code/kernel_quant.cpp:1577-1590
  update norm, 1 state kPreconditionOptimizer32bit1State  ref:sycl/sycl_code/kernel_quant.cpp:1834-1855
  update_scale         kOptimizer32bit2State / 1State     ref:sycl/sycl_code/kernel_quant.cpp:1635-1641, 1897-1903
  scaled updates                                          ref:sycl/sycl_code/kernel_quant.cpp:1725, 1982, 1990

Every fp32 operation of the reference is one numpy float32 operation, in the reference's order.  The sums
are where the build departs from the reference on purpose: the per-element terms are
the reference's, their sum is taken in fp64 and rounded once to fp32.  With max_unorm = 0 and
gnorm_scale = 1 update_32bit here equals oracle.optim.update_32bit bit for bit
(tests/test_optim_norms_cpu.py), which pins this file to the frozen oracle.
"""
import math
import types

import numpy as np

from oracle import optim as oref
from oracle.ref import F32, as_f32, cast_out

UNORM_NAMES = ("adam", "momentum", "rmsprop")


def optimizer_args(optim_bits=32, min_8bit_size=4096, percentile_clipping=100, block_wise=True, max_unorm=0.0,
                   skip_zeros=False):
    """The ``args`` object of the optimizer constructors (ref:optim/optimizer.py:410-425): the way to give
    max_unorm to the classes whose signatures, like the reference's, have no such keyword."""
    return types.SimpleNamespace(optim_bits=optim_bits, min_8bit_size=min_8bit_size,
                                 percentile_clipping=percentile_clipping, block_wise=block_wise, max_unorm=max_unorm,
                                 skip_zeros=skip_zeros)


def ulps(a, b) -> int:
    """Distance in fp32 units in the last place between two finite non-negative floats."""
    a, b = np.float32(a), np.float32(b)
    assert np.isfinite(a) and np.isfinite(b) and a >= 0 and b >= 0, (a, b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def gnorm_sq(g, dtype):
    """Squared L2 norm of a gradient in `dtype` storage: exact fp64 squares, fp64 sum, one rounding to fp32."""
    v = as_f32(np.asarray(g).reshape(-1), dtype).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return F32(np.sum(v * v))


def unorm_sq(name, g, s1, s2, beta1, beta2, eps, step, gnorm_scale=1.0, dtype="fp32"):
    """Squared L2 norm of the trial update (the precondition kernels): fp32 terms, fp64 sum, fp32 result.
    As in the reference the precondition applies neither weight decay nor skip_zeros."""
    b1, b2, eps, gsc, one = F32(beta1), F32(beta2), F32(eps), F32(gnorm_scale), F32(1.0)
    gv = as_f32(np.asarray(g).reshape(-1), dtype)
    s1 = np.asarray(s1, F32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        gt = oref._t((gsc * gv).astype(F32), dtype)
        if name == "adam":
            s2 = np.asarray(s2, F32).reshape(-1)
            # 1.0f / (1.0f - pow(beta, step)): pow(float, int) is double, the quotient is rounded once
            pc1 = F32(1.0 / (1.0 - math.pow(float(b1), float(step))))
            pc2 = F32(1.0 / (1.0 - math.pow(float(b2), float(step))))
            a = (s1 * b1 + ((one - b1) * gt).astype(F32)).astype(F32)
            b = (s2 * b2 + ((one - b2) * (gt * gt).astype(F32)).astype(F32)).astype(F32)
            a = (a * pc1).astype(F32)
            b = (b * pc2).astype(F32)
            u = (a / (np.sqrt(b).astype(F32) + eps).astype(F32)).astype(F32)
        elif name == "momentum":
            u = gt if step == 1 else (s1 * b1 + gt).astype(F32)
        elif name == "rmsprop":
            a = (s1 * b1 + (((one - b1) * gt).astype(F32) * gt).astype(F32)).astype(F32)
            u = (gt / (np.sqrt(a).astype(F32) + eps).astype(F32)).astype(F32)
        else:
            raise ValueError(name)
        return F32(np.sum((u * u).astype(F32).astype(np.float64)))


def update_scale(name, unorm, max_unorm, param_norm, eps):
    if not max_unorm > 0.0:
        return F32(1.0)
    un = np.sqrt(F32(unorm)).astype(F32)
    bound = F32(F32(max_unorm) * F32(param_norm))
    if name != "adam":
        bound = F32(bound + F32(eps))
    return F32(bound / un) if un > bound else F32(1.0)


def update_32bit(name, g, p, s1, s2, beta1, beta2, eps, step, lr, weight_decay=0.0, gnorm_scale=1.0,
                 skip_zeros=False, dtype="fp32", max_unorm=0.0, param_norm=0.0, unorm=0.0):
    """kOptimizer32bit{2,1}State for adam, momentum and rmsprop with update-norm clipping; `unorm` is the
    squared update norm the update reads.  Returns (p_new in `dtype` storage, s1, s2, update_scale)."""
    if name not in UNORM_NAMES:
        raise ValueError(name)
    opt = oref.NAME2OPT[name]
    k = oref.scalars(beta1, beta2, eps, step, lr, weight_decay)
    us = update_scale(name, unorm, max_unorm, param_norm, eps)
    b1, b2, eps, lr, wd, gsc = F32(beta1), F32(beta2), F32(eps), F32(lr), F32(weight_decay), F32(gnorm_scale)
    one = F32(1.0)
    gv = as_f32(g.reshape(-1), dtype)
    pv = as_f32(p.reshape(-1), dtype)
    s1 = np.asarray(s1, F32).reshape(-1).copy()
    s2 = None if s2 is None else np.asarray(s2, F32).reshape(-1).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        gt = oref._t((gsc * gv).astype(F32), dtype)
        if opt != oref.ADAM and wd > 0:
            gt = oref._t((gt + (pv * wd).astype(F32)).astype(F32), dtype)
        m = np.ones(gv.size, bool) if not skip_zeros else (gt != 0)
        if opt == oref.ADAM:
            n1 = (s1 * b1 + ((one - b1) * gt).astype(F32)).astype(F32)
            n2 = (s2 * b2 + ((one - b2) * (gt * gt).astype(F32)).astype(F32)).astype(F32)
            upd = (F32(us * k["step_size"]) * (n1 / (np.sqrt(n2).astype(F32) + k["c2eps"]).astype(F32)).astype(F32))
            pn = oref._t((pv + upd.astype(F32)).astype(F32), dtype)
            if wd > 0:
                pn = (pn * k["decay"]).astype(F32)
            s2 = np.where(m, n2, s2)
        elif opt == oref.MOMENTUM:
            n1 = gt if step == 1 else (s1 * b1 + gt).astype(F32)
            pn = (pv + (us * (-(lr * n1).astype(F32))).astype(F32)).astype(F32)
        else:
            n1 = (s1 * b1 + (((one - b1) * gt).astype(F32) * gt).astype(F32)).astype(F32)
            q = ((lr * gt).astype(F32) / (np.sqrt(n1).astype(F32) + eps).astype(F32)).astype(F32)
            pn = (pv - (us * q).astype(F32)).astype(F32)
        s1 = np.where(m, n1, s1)
        pn = np.where(m, pn, pv)
    return cast_out(pn, dtype), s1, s2, us
