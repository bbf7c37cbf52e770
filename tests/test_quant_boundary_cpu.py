"""The boundary probes of tests/quant_boundary_helpers.py stand on their own (no GPU): on the oracle alone they
reach every code and both sides of every decision boundary, before and after scaling; the two restatements of the
reference search agree on all of them; the optimizers' fp64 quotient shortcut equals the fp32 division on every pair
the probes form; and the 4-bit oracles change code exactly one ulp above each threshold.

The coverage figures are conditions the generators were adjusted to meet, not measurements of a kernel.  The shares
printed (run with -s) are quoted in DESIGN.md.
"""
import numpy as np
import pytest

import quant_boundary_helpers as qb
from oracle import ref

F32 = np.float32
MAPS = qb.maps()
MAP_PARAMS = [pytest.param(n, marks=pytest.mark.skipif(n == "normal" and qb.SCIPY_MISSING is not None,
                                                       reason=str(qb.SCIPY_MISSING))) for n in qb.MAP_NAMES]
NONPOW2 = [a for a in qb.SCALES if not qb.is_pow2(a)]


def test_maps_are_the_public_ones():
    assert set(MAPS) == set(qb.MAP_NAMES) - ({"normal"} if qb.SCIPY_MISSING else set())
    assert len(np.unique(MAPS["dynamic"])) == 256 and len(np.unique(MAPS["udynamic"])) == 256
    # the signed linear map: torch.linspace(-1, 1, 255) passes zero at 3.7e-9, so the zero inserted beside it makes a
    # pair 2^-28 apart (a true duplicate where linspace is symmetric); either way the narrowest gap of any map
    lin = MAPS["linear"]
    assert lin[127] == 0 and 0 <= lin[128] < F32(1e-8) and np.count_nonzero(MAPS["ulinear"] == 0) == 1
    if "normal" in MAPS:
        assert np.count_nonzero(MAPS["normal"] == 0) == 241
    # only the ragged map tells the reference's midpoint from another formula for it, on both kinds of neighbour pair
    # (code[2L], code[2L+1]) and (code[2L-1], code[2L]); all its entries are normal numbers
    for name, code in MAPS.items():
        d = qb.midpoint_variants_differ(code)
        assert (d.size == 0) == (name != "ragged"), (name, d)
    d = qb.midpoint_variants_differ(MAPS["ragged"])
    assert np.sum(d % 2 == 0) >= 4 and np.sum(d % 2 == 1) >= 4, d
    assert len(np.unique(MAPS["ragged"])) == 256 and np.abs(MAPS["ragged"]).min() > F32(2.0 ** -120)


@pytest.mark.parametrize("name", MAP_PARAMS)
def test_probes8_reach_every_code_and_both_sides_of_every_boundary(name):
    code = MAPS[name]
    x = qb.probes8(code)
    q = ref.quantize_8bit_dynamic(code, x)
    # every index the map's entries allow: of a run of equal entries the search can return only some, so the
    # reachable set is what a dense sweep of [-2, 2] and of each entry's neighbourhood gives
    dense = np.concatenate([np.linspace(-2, 2, 400001).astype(F32), x])
    reachable = np.unique(ref.quantize_8bit_dynamic(code, dense))
    assert np.array_equal(np.unique(q), reachable), (name, np.setdiff1d(reachable, np.unique(q)))
    assert reachable.size >= len(np.unique(code))
    distinct = code[:-1] != code[1:]
    mids = qb.midpoints(code)[distinct]
    below, above, exact = qb.side_distances(x, mids)
    assert exact.all() and np.all(below == 1) and np.all(above == 1), name
    # the two sides get different codes, and the exact probe shows the tie rule (strict comparisons: a tie stays)
    qm, ql, qh = (ref.quantize_8bit_dynamic(code, qb.step(mids, k)) for k in (0, -1, 1))
    assert np.all(ql != qh), (name, np.flatnonzero(ql == qh)[:8])
    assert np.all(code[ql] == code[:-1][distinct]) and np.all(code[qh] == code[1:][distinct]), name
    assert np.all((qm == ql) | (qm == qh)), name
    print(f"{name}: {reachable.size} reachable codes, {mids.size} boundaries, tie goes down at "
          f"{int(np.sum(qm == ql))}, up at {int(np.sum(qm == qh))}")


@pytest.mark.parametrize("how", ["scaled", "scaled_div"])
@pytest.mark.parametrize("name", MAP_PARAMS)
def test_scaled_probes_reach_both_sides_after_the_quotient(name, how):
    """Non-power-of-two scales: every boundary has a quotient within 2 ulp below and within 2 ulp above.  Power-of-two
    scales are exact: the quotient is the probe itself wherever the product neither overflows nor underflows."""
    code = MAPS[name]
    gen, quot = (qb.scaled, qb.quotient_mul) if how == "scaled" else (qb.scaled_div, qb.quotient_div)
    bounds = qb.boundaries(code)
    targets = qb.probes8(code)
    for a in qb.SCALES:
        v = gen(targets, a)
        assert not np.any(np.abs(v[~np.isnan(v)]) > abs(a)), (name, a)       # the block's absmax stays |A|
        q = quot(v, a)
        below, above, exact = qb.side_distances(q, bounds)
        if qb.is_pow2(a):
            big = np.abs(targets) >= F32(2.0 ** -100)                         # (subnormal products may round)
            kept = targets[big & (np.abs(targets) <= 1)]
            assert np.isin(qb.ordinal(kept), qb.ordinal(q)).all(), (name, a)
            assert exact.all() and np.all(below == 1) and np.all(above == 1), (name, a)
        else:
            assert np.all(below <= 2) and np.all(above <= 2), (name, how, a, int(below.max()), int(above.max()))
            print(f"{name} {how} A={float(a)!r}: {bounds.size} boundaries, {100.0 * np.mean(~exact):.1f} % without "
                  f"an exact hit, worst side distance {int(max(below.max(), above.max()))} ulp")


@pytest.mark.parametrize("name", ["dynamic", "udynamic"])
def test_squared_probes_step_past_every_boundary(name):
    """adam state2, rmsprop, adagrad: s = RN(g * g), quotient s / A.  Every boundary in [0, 1] has a quotient within
    4 ulp on each side (over the scales; with A = 1 alone within 3).  Per scale the step cannot be made finer than the
    arithmetic allows: one ulp of g moves g * g by 2g ulp(g) <= 2 sqrt(2) ulp(s), and an ulp of s is up to 2 ulp of
    s / A for an A that is no power of two, so consecutive quotients lie up to 5.7 ulp apart and the nearer one on a
    given side up to 6 away with the two roundings: 6 is asserted per scale, the worst met is printed (5, at A = 0.7).
    """
    code = MAPS[name]
    bounds = qb.boundaries(code)
    bounds = bounds[bounds >= 0]
    targets = qb.probes8(code)
    best_below = best_above = None
    for a in qb.SCALES:
        ganchor, A = qb.squared_anchor(a)
        g = qb.squared(targets, A)
        s = (g * g).astype(F32)
        assert np.all(s <= A) and (ganchor * ganchor).astype(F32) == A
        below, above, exact = qb.side_distances(qb.quotient_div(s, A), bounds)
        assert np.all(below <= 6) and np.all(above <= 6), (name, a, int(below.max()), int(above.max()))
        best_below = below if best_below is None else np.minimum(best_below, below)
        best_above = above if best_above is None else np.minimum(best_above, above)
        print(f"{name} squared A={float(A)!r}: {100.0 * np.mean(~exact):.1f} % of {bounds.size} boundaries without an "
              f"exact hit, worst side distance {int(max(below.max(), above.max()))} ulp")
    assert np.all(best_below <= 4) and np.all(best_above <= 4), (name, int(best_below.max()), int(best_above.max()))
    print(f"{name} squared: worst side distance of a boundary's nearest probe over the scales "
          f"{int(max(best_below.max(), best_above.max()))} ulp")


@pytest.mark.parametrize("name", MAP_PARAMS)
def test_the_two_restatements_of_the_search_agree(name):
    code = MAPS[name]
    targets = qb.probes8(code)
    assert np.array_equal(ref.quantize_8bit_dynamic(code, targets), qb.closed_form_dynamic8(code, targets)), name
    for kind in ("fp16", "bf16"):
        x = qb.probes8_16(code, kind)
        assert np.array_equal(ref.quantize_8bit_dynamic(code, x), qb.closed_form_dynamic8(code, x)), (name, kind)
    for a in qb.SCALES:
        for q in (qb.quotient_mul(qb.scaled(targets, a), a), qb.quotient_div(qb.scaled_div(targets, a), a)):
            assert np.array_equal(ref.quantize_8bit_dynamic(code, q), qb.closed_form_dynamic8(code, q)), (name, a)


def _shortcut(s, absmax):
    """requant8's quotient (csrc/optim.hip): (float)((double)s * (1.0 / (double)absmax))."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (s.astype(np.float64) * (np.float64(1.0) / np.float64(absmax))).astype(F32)


@pytest.mark.parametrize("name", [p for p in MAP_PARAMS if p.values[0] != "ulinear"])
def test_quotient_shortcut_equals_the_division_on_every_probe_pair(name):
    """A difference here is a finding about the kernel's proof sketch, not a test to relax."""
    code = MAPS[name]
    targets = qb.probes8(code)
    pairs = 0
    for kind, a in [("fp32", a) for a in qb.SCALES] + [(k, a) for k in ("fp16", "bf16") for a in qb.SCALES16]:
        if kind != "fp32" and name not in ("dynamic", "udynamic"):
            continue                               # 16-bit gradients and the squared routes run on the dynamic maps
        cases = [(qb.scaled_div(targets, a) if kind == "fp32" else qb.scaled_div16(targets, a, kind), F32(abs(a)))]
        if name in ("dynamic", "udynamic"):
            _, A = qb.squared_anchor(a, kind)
            g = qb.squared(targets, A, kind)
            cases.append(((g * g).astype(F32), A))
        for s, absmax in cases:
            want = qb.quotient_div(s, absmax)
            got = _shortcut(s, absmax)
            same = (want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))
            bad = np.flatnonzero(~same)
            assert bad.size == 0, [(name, float(a), qb.hexbits(s[i]), qb.hexbits(want[i]), qb.hexbits(got[i]))
                                   for i in bad[:8]]
            pairs += s.size
    print(f"{name}: {pairs} (s, absmax) pairs, 0 differences")


@pytest.mark.parametrize("qtype", ["nf4", "fp4"])
def test_4bit_oracles_change_code_one_ulp_above_each_threshold(qtype):
    th = qb.thresholds4(qtype)
    assert th.size == (15 if qtype == "nf4" else 14) and np.all(np.diff(th) > 0)
    quant = ref.quantize_nf4 if qtype == "nf4" else ref.quantize_fp4
    x = qb.probes4(qtype)
    below, above, exact = qb.side_distances(x, th)
    assert exact.all() and np.all(below == 1) and np.all(above == 1)
    q2, q1, q0, qp1, qp2 = (quant(qb.step(th, k)) for k in (-2, -1, 0, 1, 2))
    pos = th > 0
    # '>' on the value for NF4 and on the magnitude for FP4: the code changes between t and the next float away
    # from zero (FP4, negative side) or above (everywhere else), and nowhere else within 2 ulp
    if qtype == "nf4":
        assert np.all(q0 != qp1) and np.all(q2 == q0) and np.all(q1 == q0) and np.all(qp1 == qp2)
        assert np.array_equal(q0, np.arange(15)) and np.array_equal(qp1, np.arange(1, 16))
    else:
        assert np.all(q0[pos] != qp1[pos]) and np.all(q1[pos] == q0[pos]) and np.all(q2[pos] == q0[pos])
        assert np.all(q0[~pos] != q1[~pos]) and np.all(qp1[~pos] == q0[~pos]) and np.all(qp2[~pos] == q0[~pos])
        assert np.all(q1[~pos] == q2[~pos]) and np.all(qp1[pos] == qp2[pos])
    assert len(np.unique(quant(x))) == 16
    for kind in ("fp16", "bf16"):                  # the 16-bit probes bracket every threshold
        x16 = qb.probes4(qtype, kind)
        b16, a16, _ = qb.side_distances(x16, th)
        exact16 = np.isin(qb.ordinal(th), qb.ordinal(x16))
        assert np.all((b16 < 1 << 40) | exact16) and np.all(a16 < 1 << 40), (qtype, kind)
        lo = np.array([x16[~np.isnan(x16) & (x16 <= t)].max() for t in th])
        hi = np.array([x16[~np.isnan(x16) & (x16 > t)].min() for t in th])
        if qtype == "nf4":
            assert np.all(quant(lo) != quant(hi)), (qtype, kind)
        qb.to_storage(x16, kind)


def test_layout_keeps_one_anchor_per_block_and_rotates_the_slots():
    v = np.arange(1, 200, dtype=F32) / F32(256)
    for bs in (64, 512):
        slots = set()
        for rot in range(8):
            x = qb.layout(v, F32(-3), bs, rot)
            assert x.size % bs == 0 and np.all(np.sum(x.reshape(-1, bs) == -3, axis=1) == 1)
            assert np.array_equal(ref.block_absmax(x, bs), np.full(x.size // bs, 3, F32))
            slots.add(int(np.flatnonzero(x == v[0])[0]) % 8)
            assert int(np.flatnonzero(x == -3)[0]) == rot
        assert slots == set(range(8))
