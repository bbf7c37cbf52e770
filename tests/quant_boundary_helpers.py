"""Probe generators for the quantisers' decision boundaries, and an independent expectation (pure numpy, no GPU).

A quantiser goes wrong where it decides: at a map entry, at the fp32 midpoint of two entries, at a threshold literal,
and one ulp to either side of each -- before and after the scaling by the block's absmax.  Gaussian data does not go
there.  The generators below do, for every 8-bit map of the public API and both 4-bit types:

  probes8 / probes4     the boundary values themselves (map space, |x| <= 1 and the specials outside);
  scaled / scaled_div   inputs v whose quotient v * RN(1 / A) (blockwise quantiser) or v / A (optimizers, CPU path)
                        lands on and around each target, for the scales SCALES;
  squared               gradients g whose square, divided by the block's absmax, lands around each target;
  layout                blocks of [anchor, probes...] rotated over the 8 per-thread slots;
  closed_form_dynamic8  the reference search (kernel_quant.cpp:765-819) restated without a loop.

tests/test_quant_boundary_cpu.py shows on the oracle alone that the probes reach what they are meant to reach;
tests/test_quant_boundary_gpu.py runs them through every kernel route.
"""
import numpy as np

from oracle import ref
from oracle.maps import create_dynamic_map

F32 = np.float32
INF = F32(np.inf)
TINY = np.nextafter(F32(0), F32(1))                          # the smallest fp32 subnormal
MAP_NAMES = ("dynamic", "udynamic", "linear", "ulinear", "normal", "ragged")
# each also negated: the anchor of a block is +A or -A (absmax comes from fabs)
SCALES = tuple(s * a for a in (F32(1), F32(2.0 ** -9), F32(2.0 ** 6), F32(3), F32(0.7), np.nextafter(F32(2), F32(0)))
               for s in (F32(1), F32(-1)))
SCALES16 = tuple(F32(v) for v in (1, -1, 3, -3, 64, 2.0 ** -9))   # for 16-bit gradients: fp16 and bf16 hold them

try:
    import scipy.stats  # noqa: F401
    SCIPY_MISSING = None
except ImportError as e:                                      # create_normal_map needs scipy.stats.norm
    SCIPY_MISSING = f"create_normal_map needs scipy ({e}): the normal map is not probed"


def ragged_map():
    """A caller's own map (the API takes any sorted 256-entry tensor): neighbours lie 1.02x to 3.5x apart with full
    24-bit significands, all normal.  Every public map is so regular that b - a is exact for neighbours (b <= 2a), and
    then a + (b - a) / 2 and RN(RN(a + b) / 2) are the same float; here the difference rounds, and a midpoint formed
    any other way than the reference forms it lands on another float for some pairs (midpoint_variants_differ)."""
    rng = np.random.default_rng(5)

    def half(top):
        r = np.where(rng.random(127) < 0.5, rng.uniform(2.2, 3.5, 127), rng.uniform(1.02, 1.2, 127))
        return np.concatenate([[top], top / np.cumprod(r)])
    pos = half(1.0)
    return np.sort(np.concatenate([-half(0.97), pos]).astype(F32))


def midpoint_variants_differ(code):
    """indices i where a + RN(RN(b - a) / 2) is not RN(RN(a + b) / 2) for a = code[i], b = code[i + 1]."""
    a, b = np.asarray(code, F32)[:-1], np.asarray(code, F32)[1:]
    return np.flatnonzero((a + (F32(0.5) * (b - a).astype(F32)).astype(F32)).astype(F32) != midpoints(code))


def maps():
    """name -> 256-entry fp32 map: the two dynamic maps, the two linear maps (the signed one holds a doubled zero),
    the normal map (241 zeros; left out, with SCIPY_MISSING as the message, where scipy does not import) and
    ragged_map()."""
    import python_src_quants.functional as F                  # the map constructors only (torch on the CPU)
    out = {"dynamic": create_dynamic_map(True), "udynamic": create_dynamic_map(False),
           "linear": F.create_linear_map(signed=True).numpy(), "ulinear": F.create_linear_map(signed=False).numpy(),
           "ragged": ragged_map()}
    if SCIPY_MISSING is None:
        out["normal"] = F.create_normal_map().numpy()
    for name, code in out.items():
        code = out[name] = np.ascontiguousarray(code, F32)
        assert code.shape == (256,) and np.all(np.diff(code) >= 0), f"{name}: not sorted ascending"
        assert code[255] == 1, f"{name}: code[255] = {code[255]!r}"
    return out


# ----------------------------------------------------------------------------- fp32 and 16-bit neighbours
def ordinal(x):
    """fp32 -> int64, monotonic in the value (-0 and +0 both 0): differences count ulps."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)


def step(x, k):
    """x moved by k fp32 ulps (np.nextafter |k| times)."""
    x = np.asarray(x, F32).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, INF if k > 0 else -INF).astype(F32)
    return x


def around(x):
    """each value at -2, -1, 0, +1 and +2 ulp, flattened value-major."""
    x = np.asarray(x, F32).reshape(-1)
    return np.stack([step(x, k) for k in (-2, -1, 0, 1, 2)], axis=1).reshape(-1)


def specials():
    return np.array([0.0, -0.0, np.nan, np.inf, -np.inf, TINY, -TINY, np.nextafter(F32(1), F32(2)),
                     np.nextafter(F32(-1), F32(-2)), 2.0, -2.0], F32)


def _bf16_step(bits, up):
    """bf16 bit pattern of the next representable value above (up) or below."""
    b = np.asarray(bits, np.uint16).astype(np.int64)
    mag, neg = b & 0x7FFF, (b & 0x8000) != 0
    o = np.where(neg, -mag, mag) + (1 if up else -1)          # sign-magnitude -> ordered, one step, and back
    return np.where(o < 0, 0x8000 | -o, o).astype(np.uint16)


def neighbours16(t, kind):
    """fp32 values of the three `kind` ("fp16" / "bf16") numbers around each fp32 t: RN_kind(t) and the representable
    value on either side of it.  They bracket t whichever way RN went."""
    t = np.asarray(t, F32).reshape(-1)
    if kind == "fp16":
        with np.errstate(over="ignore"):
            h = t.astype(np.float16)
        lo, hi = np.nextafter(h, np.float16(-np.inf)), np.nextafter(h, np.float16(np.inf))
        out = np.stack([lo, h, hi], axis=1).astype(F32)
    else:
        b = ref.f32_to_bf16_bits(t)
        out = np.stack([ref.bf16_bits_to_f32(_bf16_step(b, False)), ref.bf16_bits_to_f32(b),
                        ref.bf16_bits_to_f32(_bf16_step(b, True))], axis=1)
    return out.reshape(-1)


def specials16(kind):
    """+-0, NaN, the smallest subnormals of `kind` and the values next to +-1, as fp32."""
    tiny = F32(2.0 ** -24) if kind == "fp16" else ref.bf16_bits_to_f32(np.array([1], np.uint16))[0]
    one = neighbours16(np.array([1.0, -1.0], F32), kind)
    return np.concatenate([np.array([0.0, -0.0, np.nan, tiny, -tiny], F32), one])


def to_storage(x, kind):
    """fp32 values that `kind` represents exactly -> the array a kernel takes (bf16 as uint16 bits)."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        a = ref.cast_out(x, kind)
    back = ref.as_f32(a, kind)
    assert np.array_equal(back.view(np.uint32)[~np.isnan(x)], x.view(np.uint32)[~np.isnan(x)]), f"not exact in {kind}"
    return a


# ----------------------------------------------------------------------------- boundaries and probes
def midpoints(code):
    """the 255 fp32 midpoints RN(RN(code[i] + code[i+1]) * 0.5), as the search forms them."""
    code = np.asarray(code, F32)
    return ((code[:-1] + code[1:]).astype(F32) * F32(0.5)).astype(F32)


def boundaries(code):
    """the midpoints between adjacent *distinct* entries: where the code of a sorted map changes."""
    code = np.asarray(code, F32)
    return midpoints(code)[code[:-1] != code[1:]]


def probes8(code):
    """2566 values: every entry and every midpoint at -2..+2 ulp, and the specials."""
    out = np.concatenate([around(code), around(midpoints(code)), specials()])
    assert out.size == 2566
    return out


def probes8_16(code, kind):
    """the representable neighbours of every entry and midpoint for 16-bit inputs (anchor 1), and the specials."""
    return np.concatenate([neighbours16(code, kind), neighbours16(midpoints(code), kind), specials16(kind)])


def thresholds4(qtype):
    """the fp32 literals the 4-bit decision compares with: 15 for NF4, the 7 FP4 magnitudes with both signs."""
    if qtype == "nf4":
        return ref.NF4_THRESHOLDS.copy()
    return np.concatenate([-ref.FP4_MAG_THRESHOLDS[::-1], ref.FP4_MAG_THRESHOLDS]).astype(F32)


def probes4(qtype, kind="fp32"):
    if kind == "fp32":
        return np.concatenate([around(thresholds4(qtype)), specials()])
    return np.concatenate([neighbours16(thresholds4(qtype), kind), specials16(kind)])


# ----------------------------------------------------------------------------- scaling
def is_pow2(a):
    m, _ = np.frexp(abs(float(a)))
    return m == 0.5


def _inside(v, a):
    """drop what would move the block's absmax off |A| (the probes above 1, the infinities); NaN stays: fmax skips it"""
    with np.errstate(invalid="ignore"):
        return v[~(np.abs(v) > abs(a))]


def quotient_mul(v, a):
    """the blockwise quantiser's arithmetic: v * RN(1 / |A|) (kernel_quant.cpp:1304, 1328)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(v, F32) * (F32(1.0) / F32(abs(a))).astype(F32)).astype(F32)


def quotient_div(v, a):
    """the optimizers' and the CPU path's arithmetic: v / |A|."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(v, F32) / F32(abs(a))).astype(F32)


def scaled(targets, a):
    """inputs v with v * RN(1 / |A|) on and around each target.  Power-of-two A: v = target * |A| is exact.  Other A:
    the fp32 nearest target / RN(1 / |A|) (formed in fp64) at -2..+2 ulp."""
    t = np.asarray(targets, F32).reshape(-1)
    aa = F32(abs(a))
    with np.errstate(invalid="ignore", over="ignore"):
        if is_pow2(aa):
            return _inside((t * aa).astype(F32), aa)
        r = (F32(1.0) / aa).astype(F32)
        return _inside(around((t.astype(np.float64) / np.float64(r)).astype(F32)), aa)


def scaled_div(targets, a):
    """the same for v / |A|: RN(target * |A|) at -2..+2 ulp."""
    t = np.asarray(targets, F32).reshape(-1)
    aa = F32(abs(a))
    with np.errstate(invalid="ignore", over="ignore"):
        v = (t * aa).astype(F32)
        return _inside(v if is_pow2(aa) else around(v), aa)


def squared_anchor(a, kind="fp32"):
    """(g_anchor, A) for the squared routes: the block's absmax is A = RN(g_anchor^2) with g_anchor = RN(sqrt(|a|)),
    rounded to `kind` for 16-bit gradients."""
    g = ref.round_to(np.sqrt(F32(abs(a))).astype(F32).reshape(1), kind)[0]
    return (-g if a < 0 else g), (g * g).astype(F32)


def squared(targets, A, kind="fp32"):
    """gradients g >= 0 among the 5 fp32 values (the 3 of a 16-bit `kind`) nearest sqrt(target * A), for targets in
    [0, 1]: s = RN(g * g) cannot hit every target, so it steps past it in the smallest steps there are."""
    t = np.asarray(targets, F32).reshape(-1)
    t = t[(t >= 0) & (t <= 1)]
    g0 = np.sqrt(t.astype(np.float64) * np.float64(A)).astype(F32)
    g = around(g0) if kind == "fp32" else neighbours16(g0, kind)
    g = g[g >= 0]
    return g[(g * g).astype(F32) <= A]


def scaled_div16(targets, a, kind):
    """scaled_div for 16-bit gradients: the representable neighbours of RN(target * |A|); |A| itself representable."""
    t = np.asarray(targets, F32).reshape(-1)
    aa = F32(abs(a))
    with np.errstate(invalid="ignore", over="ignore"):
        v = (t[np.isfinite(t)] * aa).astype(F32)
    return _inside(neighbours16(v, kind), aa)


def side_distances(q, bounds):
    """for each boundary the ulp distance to the nearest quotient strictly below, strictly above, and whether one hits
    it exactly: (below, above, exact); a side without a quotient gives a huge distance."""
    oq = np.unique(ordinal(q[~np.isnan(q)]))
    ob = ordinal(bounds)
    big = np.int64(1) << 40
    lo_i = np.searchsorted(oq, ob, side="left") - 1
    hi_i = np.searchsorted(oq, ob, side="right")
    below = np.where(lo_i >= 0, ob - oq[np.clip(lo_i, 0, oq.size - 1)], big)
    above = np.where(hi_i < oq.size, oq[np.clip(hi_i, 0, oq.size - 1)] - ob, big)
    return below, above, np.isin(ob, oq)


# ----------------------------------------------------------------------------- layout
def layout(values, anchor, blocksize, rot):
    """Blocks of [anchor, probes...], the last one filled up by repeating the probes from the start, the whole vector
    rotated right by `rot` elements.  Over rot = 0..7 every probe meets each of the 8 slots of a thread (both nibbles,
    all 4 byte positions) and the anchor the first and the last lane of a block's lane group; every block still holds
    one anchor, so its absmax is |anchor|."""
    values = np.asarray(values, F32).reshape(-1)
    per = blocksize - 1
    nb = max(1, -(-values.size // per))
    body = np.resize(values, nb * per).reshape(nb, per)
    x = np.concatenate([np.full((nb, 1), anchor, F32), body], axis=1).reshape(-1)
    return np.roll(x, rot)


# ----------------------------------------------------------------------------- the independent expectation
def closed_form_dynamic8(code, x):
    """dQuantize<0> (kernel_quant.cpp:765-819) without the loop: on a sorted map the binary search ends on the even
    pivot p = 2 * #{odd i <= 253 : x > code[i]}, bracketed by p - 1 and p + 1 (0 and 255 at the ends), and picks
    x > code[p] ? (x > mid(p, min(p+1, 255)) ? p+1 : p) : (x < mid(max(p-1, 0), p) ? p-1 : p)   -- strict, NaN -> p."""
    code = np.asarray(code, F32)
    x = np.asarray(x, F32)
    shp = x.shape
    x = x.reshape(-1)
    with np.errstate(invalid="ignore"):
        p = 2 * (x[:, None] > code[1:254:2][None, :]).sum(axis=1)
        up, dn = np.minimum(p + 1, 255), np.maximum(p - 1, 0)
        mid_up = ((code[up] + code[p]).astype(F32) * F32(0.5)).astype(F32)
        mid_dn = ((code[dn] + code[p]).astype(F32) * F32(0.5)).astype(F32)
        res = np.where(x > code[p], np.where(x > mid_up, up, p), np.where(x < mid_dn, dn, p))
    return res.astype(np.uint8).reshape(shp)


def hexbits(x):
    return f"0x{int(np.asarray(x, F32).reshape(-1)[:1].view(np.uint32)[0]):08x}"
