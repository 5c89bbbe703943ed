"""The quantiser's definition, the values designed against every copy of it in the library, and what those values reach.

The reference quantises with one line, quant(v, q) = sign(v) * ((|v| << 2) / qf[q]) (Quantisation.cpp:69-76), and scales
back with scale (Quantisation.cpp:86-95); the library holds nine implementations of the first and as many of the second,
each exact only inside a domain that a guard protects (DESIGN.md section 27 lists them).  This module holds, without a line
from the library's arithmetic:

  the definition     quant / scale in Python integers with C `int` wrap-around over tests/golden/quant_factor_table.json,
                     quant_np / scale_np the same in int64 numpy;
  boundary values    first(q, k) = ceil(k * qf / 4) is the least magnitude that quantises to k, first(q, k) - 1 the greatest
                     that quantises to k - 1 ("hit" / "miss"); k runs over K_VALUES and the largest k of a domain;
  float-adversarial  magnitudes in [2^20, 2^22) where the truncated float32 product with the rounded-up reciprocal differs
                     from the integer quotient (computed here in float32 numpy: what a widened guard would get wrong);
  requantise pairs   coded values c whose scale(c, q_s) just reaches or just misses a step of index q';
  dequantiser values 0, +-1, +-2, the fused forms' domain limits and the magnitude where |v| * qf + offset passes 2^31;
  sheets             planes of 30 x 4 slices at depth 2, slice s at index s: every index 0 .. 119 in one fine-grained call;
  designed pictures  Haar0 coefficient fields per slice record (tests/cbr_ref.py's coding order), picture =
                     oracle.dwt_inverse, thinned until the samples fit their range; a ladder quantisation matrix spreads one
                     picture's index over the subbands;
  reach              per copy and adjusted index, how many designed values of each (k, side, sign) a design delivers.

What IS restated from the library is control flow and constants, so that a value can be said to reach a copy: the table
path's limit P16_MAXQ, the code table's size VLC_LUT_N, the 16-bit store's escape, pack16_plan's head / body split, the
rule of make_tables for magic / shift / inv4 (from the standard's formula) and the two fillings of the fused dequantisers'
domain limit.  tests/test_quant_ref.py asserts on the CPU that the definition equals the oracle on every designed value."""
import json
import os
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import cbr_ref as cr
from vc2lib import KERNELS

HERE = os.path.dirname(os.path.abspath(__file__))
_TABLE = json.load(open(os.path.join(HERE, "golden", "quant_factor_table.json")))["quant_factor"]

P16_MAXQ = 126          # |quotient| the table path of k_hq_pack16 / k_hq_pack16w takes
VLC_LUT_N = 1024        # codes8 / load8_tab: code table entries
ST_SENTINEL = -32768    # the 16-bit store's escape mark
CODE_MAX = 65534        # the greatest magnitude the reference's 32-bit code words hold (VLC.h:27)
FLOAT_GUARD = 1 << 20   # load8_tab leaves the float product from this magnitude on
INT_GUARD = 1 << 29     # (|v| << 2) wraps from this magnitude on: quant_core's literal division


# ------------------------------------------------------------------------------------------
# the definition
# ------------------------------------------------------------------------------------------
def i32(x):
    """x as a C int (two's complement wrap)"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def cdiv(a, b):
    """C's integer division: truncation towards zero"""
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


QF = [i32(int(s, 16)) for s in _TABLE]          # static_cast<int>(lookup[q]): negative from 116 on
assert len(QF) == 120


def quant_factor(q):
    if q > 119:
        raise ValueError("quantization index exceeds maximum implemented value.")
    return QF[max(q, 0)]


def quant_offset(q):
    q = max(q, 0)
    if q == 0:
        return 1
    if q == 1:
        return 2
    return cdiv(i32(quant_factor(q) + 1), 2)


OFF = [quant_offset(q) for q in range(120)]


def quant(v, q):
    neg = v < 0
    a = i32(-v) if neg else v
    a = i32(a << 2)
    a = cdiv(a, quant_factor(q))
    return i32(-a) if neg else a


def scale(v, q):
    neg = v < 0
    a = i32(-v) if neg else v
    a = i32(a * quant_factor(q))
    if a > 0:
        a = i32(a + quant_offset(q))
    a = cdiv(i32(a + 2), 4)
    return i32(-a) if neg else a


def _wrap(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _tdiv(a, b):
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


def quant_np(v, q):
    """quant element by element: v and q broadcast (int64 inside, the result as int32)"""
    v = np.asarray(v, np.int64)
    qf = np.asarray(QF, np.int64)[np.maximum(np.asarray(q), 0)]
    neg = v < 0
    a = _wrap(_wrap(np.where(neg, -v, v)) << 2)
    a = _tdiv(a, qf)
    return _wrap(np.where(neg, -a, a)).astype(np.int32)


def scale_np(v, q):
    v = np.asarray(v, np.int64)
    q = np.maximum(np.asarray(q), 0)
    qf, off = np.asarray(QF, np.int64)[q], np.asarray(OFF, np.int64)[q]
    neg = v < 0
    a = _wrap(_wrap(np.where(neg, -v, v)) * qf)
    a = np.where(a > 0, _wrap(a + off), a)
    a = _tdiv(_wrap(a + 2), np.int64(4))
    return _wrap(np.where(neg, -a, a)).astype(np.int32)


def band_plane(shape, depth):
    """the subband of every coefficient of a plane in the reference's in-place order"""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    band = np.zeros(shape, np.int32)
    for level in range(1, depth + 1):            # level 1: the coarsest detail bands
        s = 1 << (depth + 1 - level)
        o = s // 2
        for kind, (oy, ox) in enumerate(((0, o), (o, 0), (o, o))):
            band[(yy % s == oy) & (xx % s == ox)] = 3 * (level - 1) + 1 + kind
    return band


def band_index_plane(shape, depth, ys, xs, qidx, qm):
    """the adjusted index max(q - qm[band], 0) of every coefficient of a plane"""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    q = np.asarray(qidx, np.int32)[yy * ys // h, xx * xs // w]
    return np.maximum(q - np.asarray(qm, np.int32)[band_plane(shape, depth)], 0)


# ------------------------------------------------------------------------------------------
# boundary values
# ------------------------------------------------------------------------------------------
K_VALUES = sorted({1, 2, 3, P16_MAXQ, P16_MAXQ + 1, P16_MAXQ + 2, 255, 256, VLC_LUT_N - 1, VLC_LUT_N, CODE_MAX, CODE_MAX + 1}
                  | {(1 << K) - 1 for K in range(1, 16)} | {1 << K for K in range(1, 16)})


def first(q, k):
    """the least magnitude that quantises to k at index q (positive factors: q <= 115)"""
    f = QF[q]
    assert f > 0 and k >= 1
    return -(-k * f // 4)


@dataclass(frozen=True)
class Designed:
    v: int        # the signed value
    q: int        # the (adjusted) index it is designed for
    k: int        # the quotient of the boundary
    side: str     # "hit": |quant(v, q)| = k; "miss": k - 1
    kmax: bool = False   # k is the largest of the domain it was drawn for

    @property
    def kind(self):
        return (self.k, self.side, "-" if self.v < 0 else "+")

    @property
    def want(self):
        sign = (-1 if self.v < 0 else 1) * (-1 if QF[self.q] < 0 else 1)      # (a wrapped factor turns the quotient's sign)
        return (self.k if self.side == "hit" else self.k - 1) * sign


def designed(q, vmax):
    """every designed value of index q whose magnitude lies within vmax, both sides of every boundary, both signs"""
    out = []
    if QF[q] < 0:
        # 116 .. 119: a / qf is 0 until (|v| << 2) reaches |qf| as a C int, then -1 (the sign of the factor)
        m = -(-abs(QF[q]) // 4)
        for mag, side in ((m, "hit"), (m - 1, "miss")):
            if mag <= vmax:
                out += [Designed(mag, q, 1, side), Designed(-mag, q, 1, side)]
        return out
    kmax = 4 * vmax // QF[q]
    for k in sorted(set(K_VALUES) | ({kmax} if kmax >= 1 else set())):
        m = first(q, k)
        if m > vmax:
            continue
        for mag, side in ((m, "hit"), (m - 1, "miss")):
            out += [Designed(mag, q, k, side, k == kmax), Designed(-mag, q, k, side, k == kmax)]
    return out


def domain_edges(q):
    """magnitudes at the edges of the copies' domains, whatever they quantise to: the 16-bit store's limit and escape, the
    float guard, the wrap of |v| << 2 (2^29: a = INT_MIN; 2^30: a = 0 again) and the ends of int"""
    mags = [32767, 32768, 65535, 65536, FLOAT_GUARD - 1, FLOAT_GUARD, FLOAT_GUARD + 1, (1 << 22) - 1, 1 << 22,
            INT_GUARD - 1, INT_GUARD, INT_GUARD + 1, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, (1 << 31) - 1]
    return [s * m for m in mags for s in (1, -1)] + [-(1 << 31)]


# ------------------------------------------------------------------------------------------
# the float form: |v| * inv4[q] truncated, inv4 = 4 / qf rounded up to float32
# ------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def inv4_table(rounding="up"):
    out = np.zeros(120, np.float32)
    for q in range(120):
        r = 4.0 / float(QF[q] & 0xFFFFFFFF)
        f = np.float32(r)
        if rounding == "up" and float(f) < r:
            f = np.nextafter(f, np.float32(np.inf))
        out[q] = f
    return out


def float_quotient(mag, inv):
    """trunc(float32(|v|) * inv) as the kernels form it: one float32 multiply, round to nearest, truncating conversion"""
    return (np.asarray(mag).astype(np.float32) * np.float32(inv)).astype(np.int64)


@lru_cache(maxsize=None)
def float_adversarial(q, count=4):
    """the lowest `count` magnitudes in [2^20, 2^22) whose float quotient differs from the integer one.  A factor that is
    a power of two has an exact reciprocal and an exact product: no such magnitude (the CPU test scans them all the same)."""
    f = QF[q]
    if f <= 0 or f & (f - 1) == 0:
        return ()
    inv, found = inv4_table()[q], []
    for lo in range(FLOAT_GUARD, 1 << 22, 1 << 18):
        m = np.arange(lo, lo + (1 << 18), dtype=np.int64)
        bad = m[float_quotient(m, inv) != 4 * m // f]
        found += bad[:count - len(found)].tolist()
        if len(found) >= count:
            break
    return tuple(found)


def lowest_float_failure():
    """(magnitude, index) of the lowest failure of the float form beyond its guard, over the indices 0 .. 115"""
    return min((float_adversarial(q)[0], q) for q in range(116) if float_adversarial(q))


# ------------------------------------------------------------------------------------------
# the integer form: __umulhi by magic[q], shift[q] (make_tables' rule: round-up reciprocal of an l-bit divisor)
# ------------------------------------------------------------------------------------------
def magic_shift(q):
    d = QF[q]
    if d <= 1:
        return 0, 0
    l = (d - 1).bit_length()                     # the least l with 2^l >= d
    return ((((1 << l) - d) << 32) // d + 1) & 0xFFFFFFFF, l - 1


def umulhi_quotient(a, magic, shift):
    """(t + ((a - t) >> 1)) >> shift with t = the high word of magic * a, in unsigned 32-bit arithmetic"""
    t = (magic * a) >> 32
    return ((t + (((a - t) & 0xFFFFFFFF) >> 1)) & 0xFFFFFFFF) >> shift


# ------------------------------------------------------------------------------------------
# models of the copies (the forms of DESIGN.md section 27), each with the knobs a wrong copy would turn
# ------------------------------------------------------------------------------------------
def model_magic(v, q, magic=None, shift=None):
    """copy 1 (quant_core): reciprocal multiply while qf > 1 and (|v| << 2) >= 0 as an int, else the literal division"""
    f = QF[q]
    mag = abs(v) & 0xFFFFFFFF
    a = i32(mag << 2)
    if not (f > 1 and a >= 0):
        return quant(v, q)
    m, s = magic_shift(q)
    k = umulhi_quotient(a, m if magic is None else magic, s if shift is None else shift)
    return -k if v < 0 else k


def model_float(v, q, inv=None, guard=FLOAT_GUARD, sign_from=1):
    """copy 2 (load8_tab): the float product below the guard, the literal division from it on"""
    mag = abs(v)
    if mag >= guard:
        return quant(v, q)
    k = int(float_quotient(mag, inv4_table()[q] if inv is None else inv))
    return -k if v < 0 and k >= sign_from else k


def model_table(v, q, inv=None, limit=P16_MAXQ + 1):
    """copy 3 (p16_group): the signed float product's low byte read as a signed byte; `slow` (escape, or float magnitude
    times reciprocal at or beyond the limit) hands the value to the exact division"""
    inv = inv4_table()[q] if inv is None else inv
    if abs(v) >= 32768 or np.float32(abs(v)) * np.float32(inv) >= np.float32(limit):
        return quant(v, q)
    t = int(np.float32(v) * np.float32(inv))     # truncation towards zero of the signed product
    b = t & 0xFF
    return b - 256 if b >= 128 else b


# ------------------------------------------------------------------------------------------
# requantise pairs: quant(scale(c, q_s), q')
# ------------------------------------------------------------------------------------------
def requant_values(qs, qd, cmax=CODE_MAX, per_side=6):
    """coded values c (positive) whose scale(c, qs) is a `hit` or a `miss` of some step k of index qd: (c, k, side), the
    lowest per_side of each side and the highest"""
    f, hits, misses = QF[qd], [], []
    for c in range(1, cmax + 1):
        s = scale(c, qs)
        if s >= 1 << 29:
            break
        if 4 * s >= f and (4 * s) % f < 4:
            hits.append((c, 4 * s // f, "hit"))
        elif 4 * (s + 1) >= f and (4 * (s + 1)) % f < 4:
            misses.append((c, 4 * (s + 1) // f, "miss"))
        if len(hits) > 4 * per_side and len(misses) > 4 * per_side and c > 4096:
            break
    return hits[:per_side] + hits[-1:] + misses[:per_side] + misses[-1:]


# ------------------------------------------------------------------------------------------
# dequantiser values
# ------------------------------------------------------------------------------------------
def fused_limits(q):
    """the two fillings of "domain limit per index" of the fused dequantisers: the register-blocked inverse kernels
    ((2^31 - 1 - offset - 2) / qf) and the streaming / pair kernels (min((2^25 - offset - 8) / qf, 2^23 - 1), factors below
    2^24); -1: the index has no fast domain"""
    f, o = QF[q], OFF[q]
    a = (0x7FFFFFFF - o - 2) // f if f > 0 else -1
    b = min(((1 << 25) - o - 8) // f, 0x7FFFFF) if 0 < f < 1 << 24 else -1
    return a, b


def dequant_values(q, vmax=(1 << 31) - 1):
    """signed inputs of scale at index q: 0, +-1, +-2, limit - 1 / limit / limit + 1 of both fused forms, and the three
    magnitudes around the least one whose |v| * qf + offset reaches 2^31"""
    mags = {0, 1, 2}
    for lim in fused_limits(q):
        if lim > 0:
            mags |= {lim - 1, lim, lim + 1}
    if QF[q] > 0:
        m = -(-((1 << 31) - OFF[q]) // QF[q])
        mags |= {max(m - 1, 0), m, m + 1}
    return sorted({s * m for m in mags if m <= vmax for s in (1, -1)})


# ------------------------------------------------------------------------------------------
# sheets: the fine-grained calls, every index in one plane
# ------------------------------------------------------------------------------------------
SHEET_YS, SHEET_XS, SHEET_DEPTH, SHEET_SH, SHEET_SW = 30, 4, 2, 8, 16     # 120 slices of 8 x 16 coefficients


def sheet_qidx():
    return np.arange(120, dtype=np.int32).reshape(SHEET_YS, SHEET_XS)


def sheet_values(q):
    """every signed value index q meets on the int32 entry points"""
    vals = [d.v for d in designed(q, INT_GUARD - 1)] + domain_edges(q)
    vals += [s * m for m in float_adversarial(q) for s in (1, -1)] if q < 116 else []
    return sorted(set(vals))


def _sheets_from(lists, seed, fill):
    """planes that hold lists[q] in slice q, 128 values a sheet, at seeded places among `fill` values"""
    rng = np.random.default_rng(seed)
    per = SHEET_SH * SHEET_SW
    n = max(-(-len(v) // per) for v in lists)
    out = []
    for k in range(n):
        rec = np.zeros((120, per), np.int64)
        for q in range(120):
            part = lists[q][k * per:(k + 1) * per]
            r = fill(rng, q, per)
            r[rng.permutation(per)[:len(part)]] = part
            rec[q] = r
        plane = rec.reshape(SHEET_YS, SHEET_XS, SHEET_SH, SHEET_SW).transpose(0, 2, 1, 3).reshape(SHEET_YS * SHEET_SH, SHEET_XS * SHEET_SW)
        out.append(np.ascontiguousarray(plane, np.int32))
    return out


@lru_cache(maxsize=None)
def quant_sheets():
    """(mixed sheets, slow sheets): the designed values among small ones -- a wavefront holds lanes of both branches of
    quant_core -- and sheets whose every value has (|v| << 2) < 0 as an int: every lane on the literal division"""
    mixed = _sheets_from([sheet_values(q) for q in range(120)], 2701, lambda rng, q, n: rng.integers(-3, 4, n))
    slow_vals = [[v for v in sheet_values(q) if i32(abs(v) << 2) < 0] for q in range(120)]
    slow = _sheets_from(slow_vals, 2702, lambda rng, q, n: rng.integers(INT_GUARD, 1 << 30, n) * rng.choice([-1, 1], n))
    return mixed, slow


@lru_cache(maxsize=None)
def dequant_sheets():
    return _sheets_from([dequant_values(q) for q in range(120)], 2703, lambda rng, q, n: rng.integers(-2, 3, n))


def sheet_want(plane, fn):
    """the definition over a sheet: fn = quant_np or scale_np (the matrix of the sheets is all zeros)"""
    q = np.repeat(np.repeat(sheet_qidx(), SHEET_SH, axis=0), SHEET_SW, axis=1)
    return fn(plane, q)


# ------------------------------------------------------------------------------------------
# designed pictures
# ------------------------------------------------------------------------------------------
@dataclass
class PictureGeom:
    name: str
    w: int
    h: int
    cf: str
    depth: int
    u: int
    a: int
    body_lo: int      # the first subband of the pack16 kernels' body (whole runs of sixteen); all bands are "head" below it
    store16: bool     # the default context keeps the 16-bit store
    bits: int = 16
    wavelet: str = "Haar0"

    def case(self, oracle, q, scalar):
        import proxy_ref as pr
        return pr.Case(oracle, self.w, self.h, self.cf, self.bits, self.wavelet, self.depth, self.u, self.a, q=q, scalar=scalar)

    def geometry(self, oracle):
        return cr.picture_geometry(oracle, self.w, self.h, self.cf, self.depth, self.u, self.a)

    @property
    def n_bands(self):
        return 3 * self.depth + 1

    def ladder(self):
        """the ladder matrix: entry b for subband b, so that a picture at index q meets q, q - 1 .. q - 3 * depth"""
        return np.arange(self.n_bands, dtype=np.int32)


# 32 x 16 luma slices at depth 3 on a picture too small for the 16-bit store (k_hq_pack, load8_tab on the int32 store); the
# smallest pictures that get the store and k_hq_pack16 / k_hq_pack16w (tests/test_gpu_pack16.py)
P32 = PictureGeom("P32", 256, 128, "422", 3, 2, 4, 4, False)
P16 = PictureGeom("P16", 2048, 256, "422", 4, 1, 2, 7, True)
P16W = PictureGeom("P16W", 2048, 512, "444", 5, 1, 1, 7, True)
GEOMS = {g.name: g for g in (P32, P16, P16W)}


def picture_indices(geom):
    """the indices q of a geometry's designed pictures under its ladder matrix.  The body subbands body_lo .. 3 * depth of a
    picture at q meet the adjusted indices q - 3 * depth .. q - body_lo, the subbands below them q - body_lo + 1 .. q; the
    pictures follow each other so closely that the body meets every index 0 .. 59 (the 16-bit body's non-zero quotients end
    there: 4 * 32767 < qf[60]) and, where the pack16 kernels code the leading subbands apart as heads, the heads every index
    0 .. 63 (4 * 65535 < qf[64]); on the int32 store all subbands run through one code and meet 0 .. 63 between them"""
    nb = geom.n_bands
    heads = range(1, geom.body_lo if geom.store16 else nb)       # LL holds averages of samples: |LL| <= 32768, no index beyond 59
    step = min(nb - geom.body_lo, geom.body_lo - 1) if geom.store16 else nb - geom.body_lo
    qs = [geom.body_lo - 1]
    while qs[-1] - geom.body_lo < 59 or not set(range(60, 64)) <= {q - b for q in qs for b in heads}:
        qs.append(qs[-1] + step)
    body = {q - b for q in qs for b in range(geom.body_lo, nb)}
    head = {max(q - b, 0) for q in qs for b in range(geom.body_lo)}
    assert set(range(60)) <= body and set(range(64)) <= (head if geom.store16 else head | body)
    return qs


def pack16_heads(g):
    """(head, body lanes) per component by pack16_plan's rule: the leading subbands that are not whole runs of sixteen"""
    out = []
    for c in range(3):
        start, head = 0, -1
        for size in g.band_sizes(c):
            if head < 0 and size % 16 == 0 and start % 16 == 0:
                head = start
            start += size
        head = g.comp_n[c] if head < 0 else head
        out.append((head, (g.comp_n[c] - head) // 16))
    return out


SAMPLE_BUDGET = 30000


@dataclass
class Design:
    geom: PictureGeom
    q: int
    qm: np.ndarray
    g: object                      # cbr_ref.Geometry
    recs: list                     # per component: (slices, coefficients) in coding order
    placed: list                   # (component, slice, position, Designed)
    dropped: int = 0               # designed values thinned out for the sample range
    raw: bytes = b""
    refused: bool = False          # holds k = 65535: both sides refuse the picture


def _band_starts(g, c):
    sizes = g.band_sizes(c)
    return np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(int), sizes


def design_records(oracle, geom, q, seed, vmax, with_refused=False):
    """slice records that carry the designed values of the adjusted indices max(q - b, 0), subband by subband.
    Per (slice, component) the values' weights -- |c| for LL, |c| / 2 for HL and LH, |c| / 4 for HH: what Haar0's inverse
    adds to a sample at most -- stay within SAMPLE_BUDGET, which keeps most slices inside the sample range before any
    thinning.  On a geometry with the 16-bit store three slices of four accept only quotients the table path takes
    (|k| <= 126, no escape), the fourth accepts everything; every 64th slice fills every body run with a quotient beyond
    the table where the values stay small: all lanes slow."""
    g = geom.geometry(oracle)
    qm = geom.ladder()
    rng = np.random.default_rng(seed)
    ns = g.n_slices
    recs = [rng.integers(-2, 3, size=(ns, g.comp_n[c])).astype(np.int64) * (rng.random((ns, g.comp_n[c])) < 0.3) for c in range(3)]
    placed = []
    for c in range(3):
        starts, sizes = _band_starts(g, c)
        load = np.zeros(ns, int)
        used = [set() for _ in range(ns)]
        cursor = int(rng.integers(0, ns))
        for b in range(geom.n_bands):
            aq = max(q - int(qm[b]), 0)
            vals = [d for d in designed(aq, vmax) if with_refused or d.k <= CODE_MAX or (d.k == CODE_MAX + 1 and d.side == "miss")]
            if with_refused:
                vals = [d for d in vals if d.k == CODE_MAX + 1 and d.side == "hit"]
            for d in vals:
                want_k = abs(d.want)
                mag = abs(d.v)
                for _ in range(ns):
                    s = cursor
                    cursor = (cursor + 1) % ns
                    if geom.store16 and s % 4 != 3 and (want_k > P16_MAXQ or mag > 32767):
                        continue
                    weight = mag if b == 0 else (mag + 3) // 4 if b % 3 == 0 else (mag + 1) // 2
                    if load[s] + weight > SAMPLE_BUDGET:
                        continue
                    free = [j for j in range(starts[b], starts[b] + sizes[b]) if j not in used[s]]
                    if not free:
                        continue
                    j = free[int(rng.integers(0, len(free)))]
                    used[s].add(j)
                    load[s] += weight
                    recs[c][s, j] = d.v
                    placed.append((c, s, j, d))
                    break
        # all-slow slices: a quotient of P16_MAXQ + 2 at the head of every body run whose value stays within 512
        head = pack16_heads(g)[c][0]
        for s in ([] if with_refused else range(63, ns, 64)):
            for b in range(geom.body_lo, geom.n_bands):
                aq = max(q - int(qm[b]), 0)
                m = first(aq, P16_MAXQ + 2)
                if m > 512:
                    continue
                for j in range(starts[b], starts[b] + sizes[b], 16):
                    if j >= head and j not in used[s]:
                        d = Designed(m if (j // 16) % 2 else -m, aq, P16_MAXQ + 2, "hit")
                        recs[c][s, j] = d.v
                        used[s].add(j)
                        placed.append((c, s, j, d))
    return g, qm, recs, placed


def _emit(planes, bits):
    half = 1 << (bits - 1)
    return b"".join(((p.astype(np.int64) + half).astype(np.uint16) << (16 - bits)).astype(">u2").tobytes() for p in planes)


def build_design(oracle, geom, q, seed=None, refused=False):
    """a designed picture: the records, thinned until oracle.dwt_inverse of their planes fits the sample range.  Haar0's
    two-tap filters keep a slice's coefficients inside the slice's own block of samples, so a slice whose samples leave the
    range is mended by itself: its largest designed coefficient goes, until none is left out of range."""
    vmax = 65535
    g, qm, recs, placed = design_records(oracle, geom, q, 2710 + q if seed is None else seed, vmax, with_refused=refused)
    half = 1 << (geom.bits - 1)
    K = KERNELS[geom.wavelet]
    shapes = [(geom.h, geom.w)] + [cr_chroma(geom)] * 2
    dropped = 0
    by_slice = {}
    for i, (c, s, j, d) in enumerate(placed):
        by_slice.setdefault((c, s), []).append(i)
    alive = np.ones(len(placed), bool)
    for _ in range(64):
        planes = cr.planes_from_records(g, [r.astype(np.int32) for r in recs])
        pics = [oracle.dwt_inverse(p, K, geom.depth) for p in planes]
        bad_any = False
        for c in range(3):
            sh, sw = g.slice_dims(c)
            pic = pics[c]
            over = (pic < -half) | (pic > half - 1)
            if not over.any():
                continue
            bad_any = True
            per = over.reshape(g.ys, sh, g.xs, sw).any(axis=(1, 3)).ravel()
            for s in np.flatnonzero(per):
                ids = [i for i in by_slice.get((c, int(s)), []) if alive[i]]
                if ids:
                    i = max(ids, key=lambda t: abs(placed[t][3].v))
                    alive[i] = False
                    recs[c][s, placed[i][2]] = 0
                    dropped += 1
                else:                                   # only filler left: halve it
                    recs[c][s] //= 2
        if not bad_any:
            break
    else:
        raise AssertionError("the design does not settle inside the sample range")
    placed = [p for i, p in enumerate(placed) if alive[i]]
    crop = [pic[:h, :w] for pic, (h, w) in zip(pics, shapes)]
    d = Design(geom, q, qm, g, [r.astype(np.int32) for r in recs], placed, dropped, _emit(crop, geom.bits), refused)
    return d


def cr_chroma(geom):
    return (geom.h // 2 if geom.cf == "420" else geom.h), (geom.w if geom.cf == "444" else geom.w // 2)


_design_cache = {}


def design(oracle, name, q, refused=False):
    key = (name, q, refused)
    if key not in _design_cache:
        _design_cache[key] = build_design(oracle, GEOMS[name], q, refused=refused)
    return _design_cache[key]


def design_planes(d):
    return cr.planes_from_records(d.g, d.recs)


def check_design(oracle, d):
    """the two conditions of a kept design: the samples fit, and the forward transform of the ingested picture gives the
    designed planes back exactly"""
    geom = d.geom
    shapes = [(geom.h, geom.w)] + [cr_chroma(geom)] * 2
    at = 0
    for plane, (h, w) in zip(design_planes(d), shapes):
        pic = oracle.dwt_inverse(plane, KERNELS[geom.wavelet], geom.depth)
        half = 1 << (geom.bits - 1)
        assert pic.min() >= -half and pic.max() <= half - 1, (geom.name, d.q, int(pic.min()), int(pic.max()))
        got = oracle.dwt_forward(oracle.ingest(d.raw[at:at + 2 * h * w], 2, geom.bits, (h, w)), KERNELS[geom.wavelet], geom.depth)
        assert np.array_equal(got, plane), (geom.name, d.q)
        at += 2 * h * w


# ------------------------------------------------------------------------------------------
# reach
# ------------------------------------------------------------------------------------------
def slice_paths(d):
    """per slice: does k_hq_pack16 (a slice per wavefront) leave the table path -- an escape in a body run, a float
    magnitude times reciprocal at or beyond P16_MAXQ + 1 in one, eight codes beyond 63 bits, a head quotient beyond the
    code words.  For k_hq_pack16w (a component per wavefront, P16W) the same per (slice, component)."""
    g = d.g
    heads = pack16_heads(g)
    inv = inv4_table()
    ns = g.n_slices
    slow = np.zeros((ns, 3), bool)
    for c in range(3):
        starts, sizes = _band_starts(g, c)
        head = heads[c][0]
        band_of = np.repeat(np.arange(len(sizes)), sizes)
        aq = np.maximum(d.q - d.qm[band_of], 0)
        rec = d.recs[c].astype(np.int64)
        body, baq = rec[:, head:], aq[head:]
        if body.shape[1]:
            mag = np.abs(body)
            prod = mag.astype(np.float32) * inv[baq][None, :]
            s1 = (mag >= 32768).any(axis=1) | (prod >= np.float32(P16_MAXQ + 1)).any(axis=1)
            k = np.abs(quant_np(body, baq[None, :])).astype(np.int64)
            bits = np.where(k == 0, 1, 2 * np.floor(np.log2(k + 1.0)).astype(np.int64) + 2)
            s2 = (bits.reshape(ns, -1, 8).sum(axis=2) > 63).any(axis=1)
            slow[:, c] |= s1 | s2
        if head:
            hk = np.abs(quant_np(rec[:, :head], aq[None, :head]).astype(np.int64))
            slow[:, c] |= (hk > CODE_MAX).any(axis=1)
    return slow


def reach(d, context):
    """{(copy, adjusted index, place, k, side, sign): count} of a design under a context:
       "pack16"   k_hq_pack16 / k_hq_pack16w on the 16-bit store: p16_group (body, table path), quant_core (head), and for a
                  slice (P16W: a component) that leaves the table path p16_general -- with place "mixed" where some run of the
                  slice stays within the table and "all-slow" where every body run of the component is beyond it
       "tab"      k_hq_pack's load8_tab on the int32 store: the float product for all (no design passes 2^20)"""
    g = d.g
    heads = pack16_heads(g)
    out = {}
    slow = slice_paths(d) if context == "pack16" else None
    if context == "pack16" and d.geom.name != "P16W":
        slow = np.repeat(slow.any(axis=1)[:, None], 3, axis=1)
    inv = inv4_table()
    all_slow = {}
    if context == "pack16":
        for c in range(3):
            head = heads[c][0]
            starts, sizes = _band_starts(g, c)
            band_of = np.repeat(np.arange(len(sizes)), sizes)
            aq = np.maximum(d.q - d.qm[band_of], 0)[head:]
            prod = np.abs(d.recs[c][:, head:]).astype(np.float32) * inv[aq][None, :]
            lanes = (prod >= np.float32(P16_MAXQ + 1)).reshape(g.n_slices, -1, 16).any(axis=2)
            all_slow[c] = lanes.all(axis=1)
    for c, s, j, dv in d.placed:
        place = "head" if j < heads[c][0] else "body"
        if context == "tab":
            copy = "load8_tab"
        elif slow[s, c]:
            copy, place = "p16_general", ("all-slow" if all_slow[c][s] else "mixed") if place == "body" else "head"
        else:
            copy = "p16_group" if place == "body" else "quant_core"
        key = (copy, dv.q, place) + dv.kind
        out[key] = out.get(key, 0) + 1
    return out


def reach_summary(r):
    """{(copy, place): (indices, k values, kinds, values)} of a reach table"""
    out = {}
    for (copy, aq, place, k, side, sign), n in r.items():
        e = out.setdefault((copy, place), [set(), set(), set(), 0])
        e[0].add(aq)
        e[1].add(k)
        e[2].add((k, side, sign))
        e[3] += n
    return out


# |coefficient| of a Haar0 transform of samples within 16 bits: LL is an average of samples (32768), HL and LH a difference of
# two averages (65535), HH a difference of two such differences (131070) -- far below the float guard
HAAR0_BOUND = 131070


def pack_kernel(g, store16):
    """which slice coder vc2_launch_pack gives a geometry (VBR, no prefix, short slices): pack16_plan's and pack16w_plan's
    rules on the head / body split -- every head coefficient and every body run of sixteen needs a lane of its component
    (32 / 16 / 16 lanes in k_hq_pack16, 64 each in k_hq_pack16w), at least 40 (120) body runs in all"""
    if not store16 or g.slice_coefs % 8:
        return "k_hq_pack"
    hb = pack16_heads(g)
    if all(h % 8 == 0 for h, _ in hb):
        if all(h <= w and n <= w for (h, n), w in zip(hb, (32, 16, 16))) and sum(n for _, n in hb) >= 40:
            return "k_hq_pack16"
        if all(h <= 64 and n <= 64 for h, n in hb) and sum(n for _, n in hb) >= 120:
            return "k_hq_pack16w"
    return "k_hq_pack"


# ------------------------------------------------------------------------------------------
# the LD quantisers: planes with given indices
# ------------------------------------------------------------------------------------------
# name -> (depth, ys, xs, luma plane, chroma plane, the fast kernels take it)
LD_GEOMS = {"fast": (3, 6, 5, (96, 160), (96, 80), True),         # slices of 16 x 32 luma, 16 x 16 chroma: n0 = 8 / 4
            "general": (2, 4, 6, (64, 96), (64, 48), False)}      # slices of 16 x 16 luma at depth 2: n0 = 16


def ld_fast(depth, ys, xs, lshape, cshape):
    """vc2_launch_ld_quantise's `fast`: components of up to 512 / 256 coefficients with LL blocks of up to 8 / 4"""
    n = [lshape[0] // ys * (lshape[1] // xs), cshape[0] // ys * (cshape[1] // xs)]
    n0 = [x >> (2 * depth) for x in n]
    return n[0] <= 512 and 0 < n[1] <= 256 and 3 * depth + 1 <= 32 and n0[0] <= 8 and n0[1] <= 4 and n[0] % 4 == 0


LEGALL_MATRIX = {2: [4, 2, 2, 0, 4, 4, 2], 3: [4, 2, 2, 0, 4, 4, 2, 5, 5, 3]}    # (asserted against the oracle on the CPU)


@lru_cache(maxsize=None)
def ld_planes(geom):
    """[( [Y, U, V], indices )] * 3: designed values of every slice's adjusted indices in every subband behind LL and in the LL
    sample at (0, 0) of the plane, every other LL sample 0.  Sheets 0 and 1: every other place designed, small values
    between (mixed wavefronts); sheet 2: every place beyond 2^29, where the dividend wraps (every lane slow)"""
    depth, ys, xs, lshape, cshape, _ = LD_GEOMS[geom]
    qm = LEGALL_MATRIX[depth]
    rng = np.random.default_rng(2730 + depth)
    qidx = ((7 * np.arange(ys * xs) + 3) % 68).astype(np.int32)
    qidx[-4:] = (116, 117, 118, 119)          # the wrapped factors, where the reciprocal's domain ends on the factor alone
    qidx = qidx.reshape(ys, xs)
    out = []
    for sheet in range(3):
        planes = []
        for c, shape in enumerate((lshape, cshape, cshape)):
            band = band_plane(shape, depth)
            sh, sw = shape[0] // ys, shape[1] // xs
            p = rng.integers(-3, 4, shape).astype(np.int64)
            for sy in range(ys):
                for sx in range(xs):
                    q = int(qidx[sy, sx])
                    blk = p[sy * sh:(sy + 1) * sh, sx * sw:(sx + 1) * sw]
                    bb = band[sy * sh:(sy + 1) * sh, sx * sw:(sx + 1) * sw]
                    for b in range(1, 3 * depth + 1):
                        aq = max(q - qm[b], 0)
                        pool = [d.v for d in designed(aq, INT_GUARD - 1)] + domain_edges(aq)
                        if sheet == 2:
                            pool = [v for v in pool if abs(v) >= INT_GUARD]
                        at = np.flatnonzero(bb.ravel() == b)
                        if sheet < 2:
                            at = at[(sheet + c) % 2::2]
                        off = (977 * sheet + 131 * (sy * xs + sx) + 17 * c) % len(pool)
                        blk[np.unravel_index(at, blk.shape)] = [pool[(off + i) % len(pool)] for i in range(at.size)]
            p[::1 << depth, ::1 << depth] = 0
            pool = [d.v for d in designed(max(int(qidx[0, 0]) - qm[0], 0), INT_GUARD - 1)]
            p[0, 0] = pool[(31 * sheet + 7 * c) % len(pool)]
            planes.append(np.ascontiguousarray(p, np.int32))
        out.append((planes, qidx))
    return out


# ------------------------------------------------------------------------------------------
# the transcoders: coded pictures whose values sit on the boundaries of the target's steps
# ------------------------------------------------------------------------------------------
REQUANT_TARGETS = (14, 21, 27, 40)            # every residue mod 4
REQUANT_SOURCES = (0, 3, 5, 6, 10, 7, 2, 30)   # (pairs whose steps have both a `hit` and a `miss`: not every pair has)
REQUANT_PAIRS = [(qs, t) for t in REQUANT_TARGETS for qs in REQUANT_SOURCES if qs < t]      # what the transcoders are driven with


@lru_cache(maxsize=None)
def _requant_cached(qs, qd):
    return tuple(requant_values(qs, qd))


def requant_inputs(oracle, t):
    """(case, the flat matrix, two payloads): 512 x 64 pictures in 256 slices, slice s coded at REQUANT_SOURCES[s % 8] -- at or
    above the target the slice is kept, below it every designed value c has scale(c, q_s) on a boundary of index t; luma and
    chroma, both signs, the second picture with the signs turned.  Built with oracle.hq_pack of the quantised planes"""
    import proxy_ref as pr
    case = pr.Case(oracle, 512, 64, "422", 10, "Haar0", 3, 1, 2, q=0, scalar=8)
    qm = np.zeros(3 * case.depth + 1, np.int32)
    ns = case.ys * case.xs
    qidx = np.array([REQUANT_SOURCES[s % len(REQUANT_SOURCES)] for s in range(ns)], np.int32).reshape(case.ys, case.xs)
    pays = []
    for pic in range(2):
        rng = np.random.default_rng(2740 + 10 * t + pic)
        planes = []
        for shape in ((case.ph, case.pw), (case.cph, case.cpw), (case.cph, case.cpw)):
            sh, sw = shape[0] // case.ys, shape[1] // case.xs
            p = rng.integers(-2, 3, shape).astype(np.int64)
            for s in range(ns):
                qs = int(qidx.ravel()[s])
                vals = _requant_cached(qs, t) if qs < t else _requant_cached(0, 4)
                sy, sx = divmod(s, case.xs)
                blk = p[sy * sh:(sy + 1) * sh, sx * sw:(sx + 1) * sw]
                at = rng.permutation(sh * sw)[:len(vals)]
                sign = np.where((np.arange(len(vals)) + s + pic) % 2 == 0, 1, -1)
                blk[np.unravel_index(at, blk.shape)] = np.array([c for c, _, _ in vals])[:at.size] * sign[:at.size]
            planes.append(np.ascontiguousarray(p, np.int32))
        pays.append(oracle.hq_pack(planes[0], planes[1], planes[2], case.depth, qidx, case.prefix, case.scalar).tobytes())
    return case, qm, pays


# ------------------------------------------------------------------------------------------
# the searches: slices whose budget the longer code just overflows
# ------------------------------------------------------------------------------------------
# The signed exp-Golomb code of a quotient k has 2 floor(log2(k + 1)) + 2 bits: it grows by two bits from 2^K - 2 to 2^K - 1.
# A search slice holds m values (m a multiple of four) in the first m places of each component's record, all on one side of
# the boundary k = 2^K - 1 at the slice's index T (flat matrix: the adjusted index is T everywhere):
#   "miss"  quotients 2^K - 2: 2K bits each, whole bytes in every component; the budget is exactly those bytes.  One quotient
#           one too high adds two bits, a byte more than the budget: the search would leave T
#   "hit"   quotients 2^K - 1, on exact multiples of the factor where the index has them: 2K + 2 bits each, whole bytes; the
#           budget is ONE BYTE LESS than those bytes, so T does not fit.  One quotient one too low (what a reciprocal rounded
#           down gives on an exact multiple) takes two bits off and T fits: the search would stop at T
SEARCH_GEOM = (128, 512, 128, 256, 3, 16, 32)      # tests/cbr_ref.py's BIG: 512 slices of 8 x 16 luma, 8 x 8 chroma


def search_slices():
    """[(T, K, side)] per slice: indices 1 .. 53 in turn, K the boundaries 2^K - 1 whose values stay within 16 bits"""
    out = []
    for s in range(SEARCH_GEOM[5] * SEARCH_GEOM[6]):
        T = 1 + s % 53
        ks = [K for K in range(2, 16) if first(T, (1 << K) - 1) <= 32767]
        out.append((T, ks[(s // 53 + s // 2) % len(ks)], "miss" if s % 2 == 0 else "hit"))
    return out


@lru_cache(maxsize=None)
def search_design():
    """(records per component, per-slice budgets in bytes with the four header bytes, the slices' (T, K, side))"""
    g = cr.Geometry(*SEARCH_GEOM)
    spec = search_slices()
    recs = [np.zeros((g.n_slices, g.comp_n[c]), np.int32) for c in range(3)]
    sb = np.zeros(g.n_slices, np.int32)
    for s, (T, K, side) in enumerate(spec):
        k = (1 << K) - 1
        v = first(T, k) - (side == "miss")
        bits = 2 * K + (2 if side == "hit" else 0)
        total = 0
        for c, m in enumerate((8, 4, 4)):
            recs[c][s, :m] = [v if (i + s + c) % 2 == 0 else -v for i in range(m)]
            assert (bits * m) % 8 == 0
            total += bits * m // 8
        sb[s] = 4 + total - (side == "hit")
    return recs, sb.reshape(g.ys, g.xs), spec


def search_planes():
    g = cr.Geometry(*SEARCH_GEOM)
    recs, sb, spec = search_design()
    return g, cr.planes_from_records(g, recs), np.zeros(g.n_bands, np.int32), sb, spec


# the LD search: slices of the fast and the general geometry whose luma holds four values on the `miss` side of 2^K - 1 at the
# slice's index T in one subband behind LL (LL stays 0: no prediction ties the slices together).  The budgets are found with
# the oracle: per slice the least number of bytes at which its index is at most T.
# Every eighth slice climbs to the wrapped factors instead (see below): its budget is four bytes, its index 116.
def ld_search_planes(geom):
    depth, ys, xs, lshape, cshape, _ = LD_GEOMS[geom]
    qm = LEGALL_MATRIX[depth]
    planes = [np.zeros(lshape, np.int32), np.zeros(cshape, np.int32), np.zeros(cshape, np.int32)]
    band = band_plane(lshape, depth)
    sh, sw = lshape[0] // ys, lshape[1] // xs
    spec = []
    for s in range(ys * xs):
        sy, sx = divmod(s, xs)
        blk = planes[0][sy * sh:(sy + 1) * sh, sx * sw:(sx + 1) * sw]
        bb = band[sy * sh:(sy + 1) * sh, sx * sw:(sx + 1) * sw]
        if s % 8 == 7:
            # climbs to 116: one value in a subband whose matrix entry m is 4 or 5, non-zero up to the adjusted index 115 - m
            # (trial 115) and zero from there on; small values in the coarsest HH subband (entry 0), which meet the wrapped
            # factors at the trials 119, 117 and 116 and must quantise to 0 there for the slice to fit its four bytes
            bm = max(range(1, 3 * depth + 1), key=lambda b: (qm[b], -b))
            y, x = np.argwhere(bb == bm)[0]
            blk[y, x] = first(115 - qm[bm], 1) * (1 if s % 16 == 7 else -1)
            for i, (y, x) in enumerate(np.argwhere(bb == 3)):
                blk[y, x] = 3 if i % 2 else -2
            spec.append((116, 0))
            continue
        T = 6 + (5 * s) % 50
        b = 1 + s % (3 * depth)
        aq = max(T - qm[b], 0)
        ks = [K for K in range(2, 12) if first(aq, (1 << K) - 1) < 1 << 20]
        K = ks[s % len(ks)]
        v = first(aq, (1 << K) - 1) - 1
        at = np.argwhere(bb == b)[:4]
        for i, (y, x) in enumerate(at):
            blk[y, x] = v if i % 2 == 0 else -v
        spec.append((T, K))
    return planes, spec


def ld_tight_budgets(oracle, geom, planes, spec):
    """per slice the least budget (bytes) at which the oracle's index is at most the slice's T, by bisection of all slices
    side by side (they do not interact: every LL sample is 0); (budgets, the oracle's indices there, its indices one byte lower)"""
    depth, ys, xs, _, _, _ = LD_GEOMS[geom]
    qm = np.array(LEGALL_MATRIX[depth], np.int32)
    want = np.array([t for t, _ in spec]).reshape(ys, xs)
    lo, hi = np.full((ys, xs), 3, np.int32), np.full((ys, xs), 400, np.int32)      # lo: too small, hi: enough
    lo[want == 116], hi[want == 116] = 3, 4                                        # (the climbing slices: four bytes)
    assert (oracle.ld_qindices(*planes, depth, qm, hi) <= want).all()
    while (hi - lo > 1).any():
        mid = ((lo + hi) // 2).astype(np.int32)
        ok = oracle.ld_qindices(*planes, depth, qm, mid) <= want
        hi, lo = np.where(ok, mid, hi).astype(np.int32), np.where(ok, lo, mid).astype(np.int32)
    return hi, oracle.ld_qindices(*planes, depth, qm, hi), oracle.ld_qindices(*planes, depth, qm, lo)

