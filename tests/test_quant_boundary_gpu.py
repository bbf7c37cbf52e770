"""GPU: every quantiser decision on its boundaries, bit for bit against the oracle.

The probes of tests/quant_boundary_helpers.py (map entries, fp32 midpoints, 4-bit threshold literals, each at -2..+2
ulp, before and after scaling by a block's absmax; tests/test_quant_boundary_cpu.py shows what they reach) through
every route that selects a code:

  R1  F.quantize_no_absmax                      k_quantize_map            quantize_dynamic8 (scalar search)
  R2  cquantize_blockwise_{fp32,fp16,bf16}      k_quantize_blockwise      quantize_dynamic8_n
  R3  the same entry points, nf4 / fp4          k_quantize_blockwise      quantize_nf4 / quantize_fp4
  R4  special blocks through R2 and R3          (zero, NaN, inf, subnormal, huge absmax, last element only)
  R5  F.optimizer_update_8bit_blockwise         k_optimizer_8bit_blockwise_{2,1}state   dynmap_stage,
                                                dynmap_quantize_n, requant8 and its sign fix
  R6  F.optimizer_update_8bit                   k_optimizer_8bit_static   the same re-quantiser, one global maximum
  R7  cquantize_blockwise_bytes_fp32            k_quantize_cpu_semantics  division, upper_bound, closer-right rule

One item per (route, map or 4-bit type, input type); scales, rotations and block sizes loop inside and every failing
variant is collected before the item fails.  A failure lists up to 8 offenders: route, map, rotation, scale, the
input's bits, the quotient the oracle formed, expected / got.
"""
import ctypes as ct

import numpy as np
import pytest
import torch

import optim_static8_helpers as sh
import quant_boundary_helpers as qb
from helpers import to_numpy, to_torch
from oracle import optim as oref
from oracle import ref

pytestmark = pytest.mark.gpu

F32 = np.float32
MAPS = qb.maps()
MAP_PARAMS = [pytest.param(n, marks=pytest.mark.skipif(n == "normal" and qb.SCIPY_MISSING is not None,
                                                       reason=str(qb.SCIPY_MISSING))) for n in qb.MAP_NAMES]
KINDS = ["fp32", "fp16", "bf16"]
BLOCKSIZES = (64, 512, 1024, 4096)                 # lane groups within a wave, one wave, and the LDS combine
SCALES16 = qb.SCALES16


def _F():
    import python_src_quants.functional as F
    return F


class Offenders:
    """collects every mismatch of an item; finish() fails with the first 8."""

    def __init__(self, route, what):
        self.route, self.what, self.lines, self.count = route, what, [], 0

    def codes(self, tag, scale, x, quot, exp, got):
        exp, got = np.asarray(exp).reshape(-1), np.asarray(got).reshape(-1)
        if exp.shape != got.shape:
            self.count += 1
            self.lines.append(f"{self.route} {self.what} {tag} A={scale!r}: {got.size} codes for {exp.size}")
            return
        bad = np.flatnonzero(exp != got)
        self.count += bad.size
        for i in bad[:max(0, 8 - len(self.lines))]:
            self.lines.append(f"{self.route} {self.what} {tag} A={float(scale)!r} element {i}: input "
                              f"{qb.hexbits(x[i])} ({x[i]!r}) quotient {qb.hexbits(quot[i])} ({quot[i]!r}) "
                              f"expected {exp[i]} got {got[i]}")

    def bits(self, tag, scale, label, exp, got):
        e = np.ascontiguousarray(exp).reshape(-1)
        g = np.ascontiguousarray(got).reshape(-1)
        ok = e.shape == g.shape and e.dtype == g.dtype
        bad = np.flatnonzero(e.view(np.uint8).reshape(e.size, -1) != g.view(np.uint8).reshape(g.size, -1)) if ok else [0]
        if len(bad):
            self.count += len(bad)
            if len(self.lines) < 8:
                i = int(bad[0]) // e.itemsize if ok else 0
                self.lines.append(f"{self.route} {self.what} {tag} A={float(scale)!r} {label}[{i}]: expected "
                                  f"{e[i]!r} got {g[i]!r}" if ok else f"{label}: shape or type differs")

    def finish(self):
        assert self.count == 0, f"{self.count} mismatches, the first {len(self.lines)}:\n" + "\n".join(self.lines)


# ----------------------------------------------------------------------------- R1
@pytest.mark.parametrize("name", MAP_PARAMS)
def test_r1_quantize_no_absmax(dev, name):
    F = _F()
    code = MAPS[name]
    tcode = torch.from_numpy(code).to(dev)
    x = qb.probes8(code)
    exp = ref.quantize_8bit_dynamic(code, x)
    assert np.array_equal(exp, qb.closed_form_dynamic8(code, x))
    off = Offenders("R1 quantize_no_absmax", name)
    assert x.size % 256 != 0
    runs = [("n=2566", slice(None))] + [(f"n=1 probe {i}", slice(i, i + 1)) for i in range(1280, 1295)]
    for tag, sl in runs:                           # (the n = 1 runs: the first three midpoints' five probes each)
        got = F.quantize_no_absmax(torch.from_numpy(x[sl].copy()).to(dev), tcode).cpu().numpy()
        off.codes(tag, F32(1), x[sl], x[sl], exp[sl], got)
    off.finish()


# ----------------------------------------------------------------------------- R2, R3, R4: the blockwise quantiser
def _quantize_blockwise(F, dev, x32, kind, qtype, bs, tcode, misaligned):
    """cquantize_blockwise_<kind>[_<qtype>] on x32 (values `kind` represents).  misaligned: the input is a view one
    element into its buffer, which selects the kernel's scalar load / store path (its pointer is not 16-B aligned)."""
    n = x32.size
    a = qb.to_storage(x32, kind)
    if misaligned:
        A = to_torch(np.concatenate([a[:1], a]), kind, dev)[1:]
        assert A.data_ptr() % 16 != 0
    else:
        A = to_torch(a, kind, dev)
        assert A.data_ptr() % 16 == 0
    nb = (n + bs - 1) // bs
    absmax = torch.full((nb,), -7.0, dtype=torch.float32, device=dev)
    out = torch.full((n if qtype == "8bit" else (n + 1) // 2,), 0xA5, dtype=torch.uint8, device=dev)
    fn = getattr(F.lib, f"cquantize_blockwise_{kind}" + ("" if qtype == "8bit" else f"_{qtype}"))
    fn(F.get_ptr(tcode if qtype == "8bit" else None), F.get_ptr(A), F.get_ptr(absmax), F.get_ptr(out), ct.c_int32(bs),
       ct.c_int(n))
    torch.cuda.synchronize()
    assert F.lib.cget_last_error() == 0
    return absmax.cpu().numpy(), out.cpu().numpy()


def _check_blockwise(off, F, dev, tag, scale, x, kind, qtype, bs, code, tcode, misaligned):
    with np.errstate(all="ignore"):
        ea, eq = ref.quantize_blockwise(x, bs, qtype, code=code)
        quot = (x * np.repeat((F32(1.0) / ea).astype(F32), bs)[:x.size]).astype(F32)
    absmax, q = _quantize_blockwise(F, dev, x, kind, qtype, bs, tcode, misaligned)
    tag = f"{tag} bs={bs} n={x.size} {'scalar path' if misaligned else 'vector path'}"
    off.bits(tag, scale, "absmax", ea, absmax)
    if qtype != "8bit":
        eq, q = ref.unpack_4bit(eq, x.size), ref.unpack_4bit(q, x.size)
    off.codes(tag, scale, x, quot, eq, q)


def _sweep_blockwise(dev, what, kind, qtype, code, targets, targets16):
    F = _F()
    tcode = torch.from_numpy(code).to(dev) if code is not None else None
    off = Offenders(f"{'R2' if qtype == '8bit' else 'R3'} cquantize_blockwise_{kind}", what)
    for a in (qb.SCALES if kind == "fp32" else (F32(1), F32(-1))):
        v = qb.scaled(targets, a) if kind == "fp32" else qb._inside(targets16, a)
        for bs in BLOCKSIZES:
            for rot in range(8):
                x = qb.layout(v, a, bs, rot)
                assert x.size % 8 == 0
                _check_blockwise(off, F, dev, f"rot={rot}", a, x, kind, qtype, bs, code, tcode, False)
                # n cut by 3 (odd) behind a one-element offset: scalar loads and stores, a ragged last block
                _check_blockwise(off, F, dev, f"rot={rot}", a, x[:-3], kind, qtype, bs, code, tcode, True)
    off.finish()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", MAP_PARAMS)
def test_r2_blockwise_8bit(dev, name, kind):
    code = MAPS[name]
    _sweep_blockwise(dev, name, kind, "8bit", code, qb.probes8(code),
                     None if kind == "fp32" else qb.probes8_16(code, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qtype", ["nf4", "fp4"])
def test_r3_blockwise_4bit(dev, qtype, kind):
    _sweep_blockwise(dev, qtype, kind, qtype, None, qb.probes4(qtype), None if kind == "fp32" else qb.probes4(qtype, kind))


def _special_blocks(kind, bs, targets):
    """name -> one block of `bs` elements (values `kind` represents)."""
    t = targets[np.isfinite(targets) & (np.abs(targets) <= 1)]
    fill = np.resize(t, bs).astype(F32)
    blocks = {"all zero": np.zeros(bs, F32), "all NaN": np.full(bs, np.nan, F32)}
    inf = fill.copy()
    inf[bs // 2] = np.inf
    blocks["holds +inf"] = inf
    last = np.zeros(bs, F32)
    last[-1] = fill[5] if fill[5] != 0 else F32(0.3)
    blocks["only the last element"] = last
    k = (np.arange(bs) % 97 + 1).astype(F32) * np.where(np.arange(bs) % 3 == 0, F32(-1), F32(1))
    if kind == "fp32":
        blocks["fp32 subnormals"] = (k * qb.TINY).astype(F32)
        blocks["subnormals under a normal absmax"] = np.concatenate([[F32(2.0 ** -120)], (k * qb.TINY).astype(F32)[1:]])
        big = F32(1.5 * 2.0 ** 126)                # 1 / absmax is subnormal
        blocks["absmax >= 2^126"] = np.concatenate([[big], (fill[1:] * big).astype(F32)])
    elif kind == "fp16":
        blocks["fp16 subnormals"] = (k * F32(2.0 ** -24)).astype(F32)
    else:
        sub = ref.bf16_bits_to_f32((np.arange(bs) % 97 + 1).astype(np.uint16))
        blocks["bf16 subnormals"] = (sub * np.sign(k)).astype(F32)
    return blocks


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("what", list(MAP_PARAMS) + ["nf4", "fp4"])
def test_r4_special_blocks(dev, what, kind):
    F = _F()
    qtype = what if what in ("nf4", "fp4") else "8bit"
    code = MAPS[what] if qtype == "8bit" else None
    tcode = torch.from_numpy(code).to(dev) if code is not None else None
    if kind == "fp32":
        targets = qb.probes8(code) if qtype == "8bit" else qb.probes4(qtype)
    else:
        targets = qb.probes8_16(code, kind) if qtype == "8bit" else qb.probes4(qtype, kind)
    off = Offenders(f"R4 cquantize_blockwise_{kind}", what)
    for bs in (64, 1024):
        blocks = _special_blocks(kind, bs, targets)
        plain = qb.layout(targets[np.isfinite(targets) & (np.abs(targets) <= 1)][:bs - 1], F32(1), bs, 0)[:bs]
        for name, blk in blocks.items():           # each special block between two ordinary ones, and on its own
            for x in (np.concatenate([plain, blk, plain]), blk):
                for mis in (False, True):
                    _check_blockwise(off, F, dev, name, F32(1), x if not mis else x[:-3], kind, qtype, bs, code,
                                     tcode, mis)
    off.finish()


# ----------------------------------------------------------------------------- R5: 8-bit blockwise optimizers
OPT_N = ((3 * 2048, 3 * 2047 - 8), (2 * 2048 + 777, 2 * 2047 + 776 - 8))    # (n, probes that fit beside the anchors)
CODE1, CODE2 = MAPS["dynamic"], MAPS["udynamic"]
# hyper-parameters that make the new state a chosen value exactly, from zero state: (beta1, beta2, eps, step, lr)
S1_ROUTES = {"adam": (0.0, 0.0, 1e-8, 1, 1e-3), "momentum": (0.9, 0.0, 0.0, 1, 1e-2), "lion": (0.9, 0.0, 0.0, 1, 1e-4)}
S2_ROUTES = {"adam": (0.0, 0.0, 1e-8, 1, 1e-3), "rmsprop": (0.0, 0.0, 1e-8, 1, 1e-2),
             "adagrad": (0.0, 0.0, 1e-10, 1, 1e-2)}


def _div(s, absmax):
    """the quotient the oracle forms (oracle.optim._requant, ref.quantize_cpu): the fp32 division."""
    with np.errstate(all="ignore"):
        return (np.asarray(s, F32) / np.asarray(absmax, F32)).astype(F32)


def _opt_chunks(values):
    """(n, chunk, rot): the probes cut into pieces that fit n = 3 * 2048 and n = 2 * 2048 + 777 in turn, the slot
    rotation advancing with each piece."""
    out, i, k = [], 0, 0
    while i < values.size:
        n, cap = OPT_N[k % 2]
        out.append((n, values[i:i + cap], k % 8))
        i, k = i + cap, k + 1
    return out


def _blockwise_step(off, F, dev, name, kind, hp, g32, code1, code2, tag, scale, s_of_g):
    b1, b2, eps, step, lr = hp
    n = g32.size
    nb = (n + 2047) // 2048
    two = name == "adam"
    g = qb.to_storage(g32, kind)
    p = ref.cast_out(np.linspace(-1, 1, n).astype(F32), kind)
    tg, tp = to_torch(g, kind, dev), to_torch(p, kind, dev)
    t1 = torch.zeros(n, dtype=torch.uint8, device=dev)
    t2 = torch.zeros(n, dtype=torch.uint8, device=dev) if two else None
    ta1 = torch.zeros(nb, device=dev)
    ta2 = torch.zeros(nb, device=dev) if two else None
    q1 = torch.from_numpy(code1).to(dev)
    q2 = torch.from_numpy(code2).to(dev) if two else None
    F.optimizer_update_8bit_blockwise(name, tg, tp, t1, t2, b1, b2, eps, step, lr, q1, q2, ta1, ta2)
    z = np.zeros(n, np.uint8)
    ep, e1, e2, ea1, ea2 = oref.update_8bit_blockwise(name, g, p, z, z, code1, code2, np.zeros(nb, F32),
                                                      np.zeros(nb, F32), b1, b2, eps, step, lr, 0.0, 1.0, False, kind)
    torch.cuda.synchronize()
    assert F.lib.cget_last_error() == 0
    tag = f"{tag} n={n}"
    blk = np.arange(n) // 2048
    s1, s2 = s_of_g(g32)
    off.bits(tag, scale, "absmax1", ea1, ta1.cpu().numpy())
    off.codes(tag + " state1", scale, g32, _div(s1, ea1[blk]), e1, t1.cpu().numpy())
    if two:
        off.bits(tag, scale, "absmax2", ea2, ta2.cpu().numpy())
        off.codes(tag + " state2", scale, g32, _div(s2, ea2[blk]), e2, t2.cpu().numpy())
    off.bits(tag, scale, "param", np.ascontiguousarray(ep), to_numpy(tp, kind))
    return ea1, ea2


def _s1_of(g):
    return g, (g * g).astype(F32)


def _s2_of(g):
    return (g * g).astype(F32), (g * g).astype(F32)


def _finite(v):
    return v[np.isfinite(v)]                       # (a NaN state makes a NaN parameter, whose payload is no contract)


def _sweep_s1(dev, name, kind, code1, what):
    F = _F()
    off = Offenders(f"R5 {name} state1 {kind}", what)
    targets = qb.probes8(code1)
    for a in (qb.SCALES if kind == "fp32" else SCALES16):
        v = _finite(qb.scaled_div(targets, a) if kind == "fp32" else qb.scaled_div16(targets, a, kind))
        for n, chunk, rot in _opt_chunks(v):
            g32 = qb.layout(chunk, a, 2048, rot)[:n]
            ea1, _ = _blockwise_step(off, F, dev, name, kind, S1_ROUTES[name], g32, code1, CODE2, f"rot={rot}", a, _s1_of)
            assert np.all(ea1 == abs(a)), (name, a, ea1)             # one anchor per block: the absmax is |A|
    off.finish()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(S1_ROUTES))
def test_r5_blockwise_optimizer_state1(dev, name, kind):
    """s1 = g exactly: adam with beta1 = 0, momentum at step 1, lion with beta2 = 0."""
    _sweep_s1(dev, name, kind, CODE1, "dynamic")


@pytest.mark.parametrize("what", [p for p in MAP_PARAMS if p.values[0] in ("linear", "normal", "ragged")])
def test_r5_momentum_on_other_maps(dev, what):
    """As qmap1: the signed linear map (its zero is doubled, or 2^-28 from its twin) and the normal map (241 zeros)
    -- which of the equal entries the search returns, and what the sign fix makes of it -- and the ragged map, the
    only one on which a midpoint staged by another formula than RN(RN(a + b) / 2) is another float."""
    _sweep_s1(dev, "momentum", "fp32", MAPS[what], what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(S2_ROUTES))
def test_r5_blockwise_optimizer_squared_state(dev, name, kind):
    """s = g * g exactly: adam state2 with beta2 = 0 (unsigned map), rmsprop with beta1 = 0 and adagrad (signed map)."""
    F = _F()
    code = CODE2 if name == "adam" else CODE1
    off = Offenders(f"R5 {name} squared state {kind}", "udynamic" if name == "adam" else "dynamic")
    targets = qb.probes8(code)
    for a in (qb.SCALES if kind == "fp32" else SCALES16):
        ganchor, A = qb.squared_anchor(a, kind)
        for n, chunk, rot in _opt_chunks(qb.squared(targets, A, kind)):
            g32 = qb.layout(chunk, ganchor, 2048, rot)[:n]
            ea1, ea2 = _blockwise_step(off, F, dev, name, kind, S2_ROUTES[name], g32, CODE1, CODE2, f"rot={rot}", A,
                                       _s1_of if name == "adam" else _s2_of)
            assert np.all((ea2 if name == "adam" else ea1) == A), (name, A)
    off.finish()


@pytest.mark.parametrize("name", ["adam", "momentum"])
def test_r5_stored_codes_are_a_fixed_point(dev, name):
    """No oracle: every code 0..255 under absmax A, a zero gradient, and an update that keeps the state (adam with
    beta1 = beta2 = 1; momentum with beta1 = 1 at step 2): decode, divide by the block's maximum and search again
    must give the code back, for every A."""
    F = _F()
    n = 2048 + 777
    codes = np.tile(np.arange(256, dtype=np.uint8), 12)[:n]
    q1, q2 = torch.from_numpy(CODE1).to(dev), torch.from_numpy(CODE2).to(dev)
    assert len(np.unique(CODE1)) == 256 and len(np.unique(CODE2)) == 256
    off = Offenders(f"R5 {name} fixed point", "dynamic / udynamic")
    for a in sorted({abs(float(s)) for s in qb.SCALES}):
        t1, t2 = torch.from_numpy(codes).to(dev), (torch.from_numpy(codes).to(dev) if name == "adam" else None)
        ta1 = torch.full((2,), a, device=dev)
        ta2 = torch.full((2,), a, device=dev) if name == "adam" else None
        g, p = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        F.optimizer_update_8bit_blockwise(name, g, p, t1, t2, 1.0, 1.0, 1e-8, 2, 1e-3, q1, q2 if name == "adam" else None,
                                          ta1, ta2)
        torch.cuda.synchronize()
        assert F.lib.cget_last_error() == 0
        for label, code, t, ta in (("state1", CODE1, t1, ta1), ("state2", CODE2, t2, ta2))[:2 if name == "adam" else 1]:
            s = (code[codes] * F32(a)).astype(F32)
            # block 0 holds code 255 (1.0) so its maximum is A; block 1 (777 elements) holds it too
            off.bits(label, F32(a), "absmax", np.full(2, a, F32), ta.cpu().numpy())
            off.codes(label, F32(a), s, qb.quotient_div(s, a), codes, t.cpu().numpy())
    off.finish()


# ----------------------------------------------------------------------------- R6: one global maximum
@pytest.mark.parametrize("name", ["adam", "momentum"])
def test_r6_static_optimizer(dev, name):
    F = _F()
    b1, b2, eps, step, lr = S1_ROUTES[name]
    two = name == "adam"
    off = Offenders(f"R6 optimizer_update_8bit {name}", "dynamic" + (" / udynamic" if two else ""))
    targets = qb.probes8(CODE1)
    q1, q2 = torch.from_numpy(CODE1).to(dev), (torch.from_numpy(CODE2).to(dev) if two else None)
    for a in qb.SCALES:
        g = np.concatenate([[a], _finite(qb.scaled_div(targets, a))]).astype(F32)
        n = g.size
        p = np.linspace(-1, 1, n).astype(F32)
        tp, tg = torch.from_numpy(p.copy()).to(dev), torch.from_numpy(g).to(dev)
        t1 = torch.zeros(n, dtype=torch.uint8, device=dev)
        t2 = torch.zeros(n, dtype=torch.uint8, device=dev) if two else None
        m = [torch.zeros(1, device=dev) if (two or i % 2 == 0) else None for i in range(4)]   # max1, max2, new1, new2
        F.optimizer_update_8bit(name, tg, tp, t1, t2, b1, b2, eps, step, lr, q1, q2, m[0], m[1], m[2], m[3])
        z = np.zeros(n, np.uint8)
        ep, e1, e2, nm1, nm2, _, _ = sh.static_step(name, g, p, z, z if two else None, CODE1, CODE2, F32(0), F32(0),
                                                    b1, b2, eps, step, lr)
        torch.cuda.synchronize()
        assert F.lib.cget_last_error() == 0 and nm1 == abs(a)
        off.bits("", a, "new_max1", np.array([nm1], F32), m[2].cpu().numpy())
        off.codes("state1", a, g, qb.quotient_div(g, nm1), e1, t1.cpu().numpy())
        if two:
            s2 = (g * g).astype(F32)
            off.bits("", a, "new_max2", np.array([nm2], F32), m[3].cpu().numpy())
            off.codes("state2", a, g, qb.quotient_div(s2, nm2), e2, t2.cpu().numpy())
        off.bits("", a, "param", ep, tp.cpu().numpy())
    off.finish()


# ----------------------------------------------------------------------------- R7: CPU semantics on the device
@pytest.mark.parametrize("name", MAP_PARAMS)
def test_r7_cpu_semantics_on_device(dev, name):
    """cquantize_blockwise_bytes_fp32 against ref.quantize_cpu, and against the host cquantize_blockwise_cpu_fp32 on
    the same input: two implementations of one rule (division, left neighbour, strictly closer right)."""
    F = _F()
    code = MAPS[name]
    tcode = torch.from_numpy(code).to(dev)
    off = Offenders("R7 cquantize_blockwise_bytes_fp32", name)
    targets = qb.probes8(code)
    for a in qb.SCALES:
        v = qb.scaled_div(targets, a)
        for bs in (64, 77):
            x = np.ascontiguousarray(qb.layout(v, a, bs, 0)[:-3])
            n, nb = x.size, (x.size + bs - 1) // bs
            ea, eq, _ = ref.quantize_cpu(code, x, bs)
            absmax = torch.full((nb,), -7.0, device=dev)
            out = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
            tx = torch.from_numpy(x).to(dev)
            F.lib.cquantize_blockwise_bytes_fp32(F.get_ptr(tcode), F.get_ptr(tx), F.get_ptr(absmax), F.get_ptr(out),
                                                 ct.c_longlong(bs), ct.c_longlong(n))
            torch.cuda.synchronize()
            assert F.lib.cget_last_error() == 0
            hcode, habs, hout = code.copy(), np.zeros(nb, F32), np.zeros(n, np.uint8)
            F.lib.cquantize_blockwise_cpu_fp32(*(ct.c_void_p(t.ctypes.data) for t in (hcode, x, habs, hout)),
                                               ct.c_longlong(bs), ct.c_longlong(n))
            quot = _div(x, np.repeat(ea, bs)[:n])
            tag = f"bs={bs} n={n}"
            off.bits(tag, a, "absmax", ea, absmax.cpu().numpy())
            off.codes(tag + " device vs oracle", a, x, quot, eq, out.cpu().numpy())
            off.bits(tag, a, "host absmax", ea, habs)
            off.codes(tag + " device vs host", a, x, quot, hout, out.cpu().numpy())
    assert torch.equal(tcode.cpu(), torch.from_numpy(code))         # the caller's map is not rewritten
    off.finish()
