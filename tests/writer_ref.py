"""The HQ slice writer defined on the CPU, designed coefficients for the edges of the writers' own bit strings, and
k_hq_pack's decisions restated (pure CPU: no GPU import).

  plain / slice_bytes / payload   the reference's writer in Python integers: SignedVLC codes, component_slice_bytes and the
                                  bounded write and flush (Slices.cpp:97-119, VLC.cpp:151-213).  Nothing here comes from the
                                  library or from the oracle; tests/test_writer_ref.py makes the oracle its second witness
  generators                      strings, phase, last, units, cbr, tiles, random: slice records in coding order whose codes
                                  stand on a lane's 64 bits, on the words of a slice image, on the places of the last
                                  non-zero coefficient, on whole length units, on V's room under HQ_CBR and on the byte
                                  alignment of the copy-out
  pack_form                       which form of k_hq_pack a geometry, prefix and scalar get (pack_lanes, vc2_pack_image_mode,
                                  one_round, big_lut; on quant_ref.pack_kernel)
  model                           k_hq_pack's decisions transcribed -- lanes of eight, scans, comp_len's float form, write8
                                  against write8_short, the limit, seg_off, the copy-out's head and tail -- with what an
                                  input reaches counted on the way
  batch_inputs / batch_picture    strings, last and random as Haar0 pictures for vc2hip_encode_batch_dev (the quantising loads,
                                  k_hq_pack16, k_hq_pack16w)
MUTANTS names one-line wrong copies of plain and of the model; tests/test_writer_ref.py shows that every one of them is caught
by a designed input and by no random one.  They stand in for wrong kernels, which are never committed."""
from collections import Counter, namedtuple
from functools import lru_cache

import numpy as np

import cbr_ref as cr
import quant_ref as qr

SEED = 29
LENGTHS = (1,) + tuple(range(4, 34, 2))      # a zero, then K = 1 .. 15 pairs: no code has 2 or 3 bits

# what both sides refuse: (the reference's words, the library's error code)
REFUSALS = {"scalar": ("Slice scalar is too small", -3),
            "toobig": ("Too many bytes", -4),
            "len": ("Slice component length exceeds 1 byte", -5)}


class Refused(Exception):
    def __init__(self, kind):
        super().__init__(REFUSALS[kind][0])
        self.kind = kind


# ---------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def code(v):
    """'1' for 0, (0 b)^K 1 s otherwise (VLC.cpp:21-52, 78-94)"""
    if v == 0:
        return "1"
    return "".join("0" + b for b in bin(abs(v) + 1)[3:]) + "1" + ("1" if v < 0 else "0")


def plain(values, scalar, room=None, mut=None):
    """(length byte, data bytes) of one component: the count runs through the last non-zero code, the length is whole
    units of `scalar` bytes, the codes go inside 8 * bytes bits -- what does not fit is the '1' of a zero, which the bounded
    write drops (a '0' there would be its length_error) -- and the flush pads with '0'.  room: V's bytes under HQ_CBR"""
    codes = [code(int(v)) for v in values]
    gross = count = 0
    for c in codes:
        gross += len(c)
        if len(c) > 1 or mut == "count through the last code":
            count = gross
    units = -(-(-(-count // 8)) // scalar)
    if units > 255:
        raise Refused("scalar")
    nbytes = need = units * scalar
    if room is not None:
        if room < nbytes:
            raise Refused("toobig")
        if room // scalar > 255:
            raise Refused("len")
        nbytes = room
    bits = "".join(codes)
    assert "0" not in bits[8 * nbytes:]
    data = bits[:8 * nbytes].ljust(8 * nbytes, "0")
    lb = (need if mut == "length byte from need" else nbytes) // scalar
    return lb, (int(data, 2).to_bytes(nbytes, "big") if nbytes else b"")


def slice_bytes(q, comps, prefix, scalar, budget=None, mut=None):
    """one slice: prefix bytes of zero, the index byte, then length byte and data of Y, U and V.  budget: the slice's bytes
    under HQ_CBR (the four header bytes counted, the prefix not), of which V takes what Y and U leave"""
    out = bytearray(prefix) + bytes([q & 0xFF])
    used = 0
    for c, values in enumerate(comps):
        room = None if budget is None or c < 2 else budget - 4 - used
        lb, data = plain(values, scalar, room, mut)
        used += len(data)
        out.append(lb)
        out += data
    return bytes(out)


def payload(inp, prefix, scalar, mut=None):
    """the picture's payload: its slices in raster order"""
    ns = inp.geo.ys * inp.geo.xs
    return b"".join(slice_bytes(int(inp.qidx[s]), [inp.recs[c][s] for c in range(3)], prefix, scalar,
                                None if inp.budgets is None else int(inp.budgets[s]), mut) for s in range(ns))


# ---------------------------------------------------------------------------------------------------------------------
# geometries
# ---------------------------------------------------------------------------------------------------------------------
Geo = namedtuple("Geo", "name luma chroma depth ys xs")      # luma, chroma: (rows, columns) of one slice


def geo_n(g):
    return g.luma[0] * g.luma[1], g.chroma[0] * g.chroma[1], g.chroma[0] * g.chroma[1]


GEOS = {g.name: g for g in (
    Geo("n4", (2, 2), (2, 2), 1, 5, 7),            # 4:4:4, 4 coefficients: half a group of eight
    Geo("n36", (6, 6), (6, 6), 1, 5, 7),           # 4:4:4, 36 coefficients: four groups and a half
    Geo("w16", (8, 16), (8, 8), 2, 3, 6),          # 128 + 2 x 64: four slices a wavefront at its limit
    Geo("w32", (16, 16), (8, 16), 2, 3, 5),        # 256 + 2 x 128: two slices a wavefront
    Geo("fast", (16, 32), (16, 16), 3, 3, 5),      # 512 + 2 x 256: a wavefront a slice, one round
    Geo("r520", (20, 26), (10, 26), 1, 3, 4),      # 520 + 2 x 260: a second round of 8 and of 4
    Geo("r1024", (32, 32), (16, 32), 3, 3, 4),     # 1024 + 2 x 512: two full rounds
    Geo("r2304", (48, 48), (24, 48), 2, 3, 4),     # 2304 + 2 x 1152: five rounds, three rounds
)}
SMALL = "w16"                                      # the geometry of the large scalars
HUGE = Geo("n16384", (128, 128), (128, 128), 2, 1, 2)    # 32 rounds a component: 255 units up to a scalar of 257 (`longest` only)


def order(sh, sw, depth):
    """flat positions of a slice's coefficients in coding order: LL, then HL, LH, HH of every level from the coarsest"""
    out = []
    for band in range(3 * depth + 1):
        if band == 0:
            s, oy, ox = 1 << depth, 0, 0
        else:
            level, kind = (band - 1) // 3 + 1, (band - 1) % 3
            s = 1 << (depth + 1 - level)
            oy, ox = (0 if kind == 0 else s // 2), (0 if kind == 1 else s // 2)
        out += [y * sw + x for y in range(oy, sh, s) for x in range(ox, sw, s)]
    assert sorted(out) == list(range(sh * sw))
    return out


def planes(geo, recs):
    """the three coefficient planes that hold the records (slices, coefficients in coding order)"""
    out = []
    for c, (sh, sw) in enumerate((geo.luma, geo.chroma, geo.chroma)):
        t = np.zeros((geo.ys * geo.xs, sh * sw), np.int32)
        t[:, order(sh, sw, geo.depth)] = recs[c]
        out.append(np.ascontiguousarray(t.reshape(geo.ys, geo.xs, sh, sw).transpose(0, 2, 1, 3).reshape(geo.ys * sh, geo.xs * sw)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# which form of k_hq_pack (vc2_launch_pack, run_pack)
# ---------------------------------------------------------------------------------------------------------------------
VLC_LUT_N = 1024
LDS_LIMIT = 144 * 1024
Form = namedtuple("Form", "kernel W S fast rounds big_lut mode waves gimg lookback tile_slices")


def img_words(prefix, scalar):
    # (+ scalar - 1: the remainder V's room may hold beyond 255 units under HQ_CBR -- the longest slice of the reference)
    return (prefix + 4 + 3 * 255 * scalar + scalar - 1 + 3) // 4 + 2


def pack_lds(prefix, scalar, spw, big_lut=False, waves=4, gimg=False):
    iw = 0 if gimg else img_words(prefix, scalar)
    return waves * spw * iw * 4 + VLC_LUT_N * 4 + 768 + waves * spw * 32 * 16 + (4096 if big_lut else 0)


def image_mode(prefix, scalar):
    """0: four slice images fit in LDS; 2, 1: wavefronts a workgroup; -1: the images in global memory"""
    for mode, waves in ((0, 4), (2, 2), (1, 1)):
        if pack_lds(prefix, scalar, 1, False, waves) <= LDS_LIMIT:
            return mode
    return -1


def pack_form(geo, prefix, scalar, single_pass=False, cbr=False, store16=False):
    """the form vc2hip_hq_pack runs a geometry in.  single_pass: a context with SINGLE_PASS_VBR"""
    g = cr.Geometry(geo.ys * geo.luma[0], geo.xs * geo.luma[1], geo.ys * geo.chroma[0], geo.xs * geo.chroma[1], geo.depth, geo.ys, geo.xs)
    kernel = qr.pack_kernel(g, store16)
    assert kernel == "k_hq_pack"
    n, bands = geo_n(geo), 3 * geo.depth + 1
    mode = image_mode(prefix, scalar)
    lookback = single_pass and mode == 0 and not cbr
    W = 64
    if not lookback:
        if n[0] <= 128 and n[1] <= 64 and bands <= 16 and pack_lds(prefix, scalar, 4) <= LDS_LIMIT:
            W = 16
        elif n[0] <= 256 and n[1] <= 128 and bands <= 32 and pack_lds(prefix, scalar, 2) <= LDS_LIMIT:
            W = 32
    one_round = n[0] <= 512 and n[1] <= 256
    big_lut = W == 64 and not one_round and n[0] <= 2048 and n[1] <= 2048 and bands <= 32 and pack_lds(prefix, scalar, 1, True) <= LDS_LIMIT
    fast = n[0] <= 8 * W and n[1] <= 4 * W
    rounds = tuple(1 if fast else -(-x // 512) for x in n)
    waves = 4 if mode <= 0 else mode
    tile_slices = 0 if (mode != 0 or cbr or lookback or W == 64) else 4 * (64 // W)
    return Form(kernel, W, 64 // W, fast, rounds, big_lut and mode == 0, mode, waves, mode < 0, lookback, tile_slices)


def mode_scalars(prefix=0):
    """the last scalar of every image mode and the first of the next: [(45, 46), ...] by the restated rule"""
    out, s = [], 1
    while len(out) < 3:
        if image_mode(prefix, s) != image_mode(prefix, s + 1):
            out.append((s, s + 1))
        s += 1
    return out


def lane_scalars(geo, prefix=0):
    """the last scalar at which a geometry keeps its lanes a slice and the first of the next width"""
    out, s = [], 1
    while image_mode(prefix, s) == 0:
        if pack_form(geo, prefix, s).W != pack_form(geo, prefix, s + 1).W:
            out.append((s, s + 1))
        s += 1
    return out


def inv_up(scalar):
    """the smallest float32 >= 1 / scalar (vc2_launch_pack)"""
    f = np.float32(1.0) / np.float32(scalar)
    if float(f) < 1.0 / scalar:
        f = np.nextafter(f, np.float32(np.inf))
    return np.float32(f)


# ---------------------------------------------------------------------------------------------------------------------
# designed inputs
# ---------------------------------------------------------------------------------------------------------------------
# recs: per component (slices, coefficients) in coding order; named: (slice, component, position) of the values an input is
# there for; budgets: bytes per slice under HQ_CBR; refused: a key of REFUSALS where both sides refuse the picture
Input = namedtuple("Input", "gen tag geo recs qidx named budgets refused", defaults=(None, None))


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) if not isinstance(k, str) else sum(map(ord, k)) for k in key])


_CAP = 32        # the longest code the seeded fillers may use (batch_inputs lowers it: the samples of a picture must fit)


def feasible(bits, k):
    """can k codes have `bits` bits in all"""
    if k < 0 or bits < k:
        return False
    # t codes of one bit and k - t of 4 .. _CAP bits: 4 (k - t) <= bits - t <= _CAP (k - t), t of the parity of bits
    lo, hi = max(0, -((bits - 4 * k) // 3)), min(k, (_CAP * k - bits) // (_CAP - 1))
    lo += (lo - bits) % 2
    return lo <= hi


def lengths_exact(bits, k, rng, last_nonzero=True):
    """k code lengths of `bits` bits in all, seeded; the last one of a non-zero value if asked"""
    if last_nonzero:
        opts = [L for L in LENGTHS[1:] if L <= _CAP and feasible(bits - L, k - 1)]
        assert opts, (bits, k)
        last = opts[int(rng.integers(0, len(opts)))]
        return lengths_exact(bits - last, k - 1, rng, False) + [last]
    out = []
    for left in range(k, 0, -1):
        opts = [L for L in LENGTHS if L <= _CAP and feasible(bits - L, left - 1)]
        assert opts, (bits, k)
        w = np.array([3.0 if L in (1, 8) else 1.0 for L in opts])
        L = opts[int(rng.choice(len(opts), p=w / w.sum()))]
        out.append(L)
        bits -= L
    assert bits == 0
    return out


def value_of(L, rng, extreme=None, sign=None):
    """a value whose code has L bits: seeded within its class, or the class's least (0) or largest (1) magnitude"""
    if L == 1:
        return 0
    K = (L - 2) // 2
    lo, hi = (1 << K) - 1, (1 << (K + 1)) - 2
    m = (lo, hi)[extreme] if extreme is not None else int(rng.integers(lo, hi + 1))
    s = sign if sign is not None else (1, -1)[int(rng.integers(0, 2))]
    return s * m


def values_exact(bits, k, rng, last_nonzero=True):
    return [value_of(L, rng) for L in lengths_exact(bits, k, rng, last_nonzero)]


def other_class(v):
    """the value moved by one code-length class (two bits longer; shorter from the top class)"""
    if v == 0:
        return 1
    L = len(code(v))
    m = (1 << ((L - 2) // 2 + 1)) - 1 if L < 32 else (1 << 14) - 1
    return -m if v < 0 else m


def _blank(geo, rng, density=0.25):
    """short neighbours: zeros, some +-1 and +-2"""
    ns = geo.ys * geo.xs
    return [(rng.integers(-2, 3, (ns, n)) * (rng.random((ns, n)) < density)).astype(np.int32) for n in geo_n(geo)]


def _qidx(geo, k=0):
    ns = geo.ys * geo.xs
    return ((37 * np.arange(ns) + 11 + k) % 120).astype(np.int32)


def _fit(recs, named, scalar):
    """keep every component within 255 units: what lies behind the last non-zero value that still fits becomes zero (a
    component of 2304 coefficients has 288 bytes of zeros alone), and the named places that went with it are dropped"""
    limit = 8 * 255 * scalar
    for r in recs:
        bits = np.where(r == 0, 1, 2 * np.floor(np.log2(np.abs(r.astype(np.int64)) + 1.0)).astype(np.int64) + 2)
        r[(np.cumsum(bits, axis=1) > limit) & (r != 0)] = 0
    return [(s, c, j) for s, c, j in named if recs[c][s, j] != 0]


def _group(n, g):
    """positions of lane g's group of eight in a component of n coefficients"""
    return range(8 * g, min(8 * g + 8, n))


def gen_strings(geo, prefix=0, scalar=1):
    """a lane's string of 62 .. 66 bits: (A) on every lane of the first round in turn and on lanes 0, 31 and 63 of later
    rounds, among short neighbours; (B) one such lane between lanes of 80 bits"""
    out = []
    ns, ncs = geo.ys * geo.xs, geo_n(geo)
    for bits in (62, 63, 64, 65, 66):
        for turn in range(4):
            rng = _rng("strings", geo.name, bits, turn)
            recs, named = _blank(geo, rng, 0.1), []
            for s in range(ns):
                for c, n in enumerate(ncs):
                    lanes = -(-n // 8)
                    want = [g for g in range(min(lanes, 64)) if g % 4 == (turn + s + c) % 4]
                    want += [r * 64 + (0, 31, 63, 17)[(turn + s) % 4] for r in range(1, -(-lanes // 64))]
                    for g in want:
                        at = _group(n, g)
                        if g >= lanes or not feasible(bits, len(at)):
                            continue
                        recs[c][s, list(at)] = values_exact(bits, len(at), rng, False)
                        named += [(s, c, j) for j in at if recs[c][s, j]][-1:]
            out.append(Input("strings", f"A{bits}.{turn}", geo, recs, _qidx(geo, turn), _fit(recs, named, scalar)))
        rng = _rng("strings", geo.name, bits, "B")
        recs, named = _blank(geo, rng, 0.1), []
        for s in range(ns):
            for c, n in enumerate(ncs):
                lanes = -(-n // 8)
                if lanes < 3:               # no neighbour in the component: every other slice is long instead
                    at = _group(n, 0)
                    recs[c][s, list(at)] = values_exact(bits if s % 2 == 0 else 18 * len(at), len(at), rng, False)
                    if s % 2 == 0:
                        named += [(s, c, j) for j in at if recs[c][s, j]][-1:]
                    continue
                g0 = (7 * s + 3 * c + bits) % lanes
                for g in range(max(g0 - 2, 0), min(g0 + 3, lanes)):
                    at = _group(n, g)
                    k = len(at)
                    b = bits if g == g0 else 10 * k
                    if not feasible(b, k):
                        continue
                    recs[c][s, list(at)] = values_exact(b, k, rng, False)
                    if g == g0:
                        named += [(s, c, j) for j in at if recs[c][s, j]][-1:]
        out.append(Input("strings", f"B{bits}", geo, recs, _qidx(geo), _fit(recs, named, scalar)))
    return out


def _data_start(comps, c, prefix, scalar):
    """bit position in the slice of component c's first data bit, from the definition's lengths of the components before"""
    at = prefix + 1
    for k in range(c):
        at += 1 + len(plain(comps[k], scalar)[1])
    return 8 * (at + 1)


def gen_phase(geo, prefix=0, scalar=1):
    """one code of every length 4 .. 32 (least and largest magnitude of its class, both signs) that ends at bit 30 .. 34 of a
    word of the slice image, in lane 0, an inner lane and the last lane of a component; zeros behind it"""
    ns, ncs = geo.ys * geo.xs, geo_n(geo)
    todo = [(L, ext, sign, end) for L in LENGTHS[1:] for ext in (0, 1) for sign in (1, -1) for end in (30, 31, 32, 33, 34)]
    out, at, pic = [], 0, 0
    while at < len(todo):
        rng = _rng("phase", geo.name, prefix, scalar, pic)
        recs, named = [np.zeros((ns, n), np.int32) for n in ncs], []
        for s in range(ns):
            for c, n in enumerate(ncs):
                if at >= len(todo):
                    break
                L, ext, sign, end = todo[at]
                lanes = -(-n // 8)
                g = (0, lanes // 2, lanes - 1)[(at + c) % 3]
                j = min(8 * g + 7, n - 1)
                if j == 0:
                    continue
                start = _data_start([recs[k][s] for k in range(3)], c, prefix, scalar)
                before = (end - L - start) % 32
                while before < j or not feasible(before, j):
                    before += 32
                if before > 32 * j or before + L > 8 * 255 * scalar:
                    continue
                recs[c][s, :j] = values_exact(before, j, rng, False)
                recs[c][s, j] = value_of(L, rng, ext, sign)
                named.append((s, c, j))
                at += 1
        if not named:
            break
        out.append(Input("phase", f"p{prefix}.{pic}", geo, recs, _qidx(geo, pic), _fit(recs, named, scalar)))
        pic += 1
    return out


def _last_places(n):
    lanes = -(-n // 8)
    groups = sorted({0, lanes // 2, lanes - 1, 15, 16, 31} & set(range(lanes)))
    return sorted({j for g in groups for j in _group(n, g)} | {0, n - 1})


LONE = (1, -3, 1023, 1024, -1024, 1025, -32767, 65534)      # lone values: 1024 is the first magnitude beyond the code table


def fit_k(bits, n):
    """the most codes (at most n) that can have `bits` bits in all with a non-zero value last, or 0"""
    for k in range(min(n, bits), 0, -1):
        if any(feasible(bits - L, k - 1) for L in LENGTHS[1:] if L <= _CAP and bits - L >= 0):
            return k
    return 0


def gen_last(geo, prefix=0, scalar=1):
    """the last non-zero coefficient at every place of the first, an inner and the last group of eight (also the groups
    15, 16 and 31: chroma's lanes 47, 48 and 63 of the one-round form), everything behind it zero and short values before
    it; a lone non-zero value; an all-zero component; counts of exactly 8k - 1, 8k and 8k + 1 bits"""
    ns, ncs = geo.ys * geo.xs, geo_n(geo)
    jobs = []
    for c, n in enumerate(ncs):
        jobs += [(c, "place", j) for j in _last_places(n)] + [(c, "lone", (j, v)) for j in (0, n - 1) for v in LONE] + [(c, "zero", 0)]
        top = min(32 * n, 8 * 255 * scalar) // 8
        jobs += [(c, "count", b) for k in sorted({1, 2, top}) for b in (8 * k - 1, 8 * k, 8 * k + 1)
                 if 4 <= b <= min(32 * n, 8 * 255 * scalar) and fit_k(b, n)]
    out, pic = [], 0
    while jobs:
        rng = _rng("last", geo.name, scalar, pic)
        recs, named = [np.zeros((ns, n), np.int32) for n in ncs], []
        left = list(jobs)
        for s in range(ns):
            for c in range(3):
                job = next((j for j in left if j[0] == c), None)
                if job is None:
                    continue
                left.remove(job)
                _, kind, x = job
                if kind == "place":
                    recs[c][s, :x] = rng.integers(-1, 2, x) * (rng.random(x) < 0.3)
                    recs[c][s, x] = value_of(int(rng.choice((4, 6, 8))), rng)
                    named.append((s, c, x))
                elif kind == "lone":
                    recs[c][s, x[0]] = x[1]
                    named.append((s, c, x[0]))
                elif kind == "count":
                    k = fit_k(x, ncs[c])
                    recs[c][s, :k] = values_exact(x, k, rng, True)
                    named.append((s, c, k - 1))
        jobs = left
        out.append(Input("last", f"l{pic}", geo, recs, _qidx(geo, pic), _fit(recs, named, scalar)))
        pic += 1
    return out


def _component_of_bytes(n, nbytes, rng):
    """values of a component whose count needs exactly nbytes bytes (seeded: its last code ends on the last bit of the last
    byte, on its first or inside it), or None where n coefficients cannot hold them"""
    for count in rng.permutation([8 * nbytes, 8 * nbytes - 7, 8 * nbytes - 3]).tolist():
        k = fit_k(count, n) if count >= 4 else 0
        if k:
            return values_exact(count, k, rng, True)
    return None


def gen_units(geo, prefix=0, scalar=1):
    """components of m * scalar - 1, m * scalar and m * scalar + 1 bytes for m = 1, 2, 254, 255, as far as n coefficients
    hold them; 255 * scalar + 1 bytes need 256 units and are refused, in a picture of their own"""
    ns, ncs = geo.ys * geo.xs, geo_n(geo)
    sizes = sorted({m * scalar + d for m in (1, 2, 254, 255) for d in (-1, 0, 1)} - {0})
    jobs = [(c, b) for c, n in enumerate(ncs) for b in sizes if 8 * b - 7 <= 32 * n and b <= 255 * scalar]
    out, pic = [], 0
    while jobs:
        rng = _rng("units", geo.name, scalar, pic)
        recs, named, left = _blank(geo, rng, 0.05), [], []
        _fit(recs, [], scalar)
        free = {(s, c) for s in range(ns) for c in range(3)}
        for c, b in jobs:
            s = next((s for s in range(ns) if (s, c) in free), None)
            vals = None if s is None else _component_of_bytes(ncs[c], b, rng)
            if s is None:
                left.append((c, b))
                continue
            if vals is None:
                continue
            free.discard((s, c))
            recs[c][s] = 0
            recs[c][s, :len(vals)] = vals
            named.append((s, c, len(vals) - 1))
        out.append(Input("units", f"u{pic}", geo, recs, _qidx(geo, pic), named))
        jobs, pic = left, pic + 1
    for c, n in enumerate(ncs):
        if c < 2 and 8 * (255 * scalar + 1) - 7 <= 32 * n:
            rng = _rng("units", geo.name, scalar, "refused", c)
            recs = _blank(geo, rng, 0.05)
            _fit(recs, [], scalar)
            vals = _component_of_bytes(n, 255 * scalar + 1, rng)
            s = ns // 2
            recs[c][s] = 0
            recs[c][s, :len(vals)] = vals
            out.append(Input("units", f"refused{c}", geo, recs, _qidx(geo), [(s, c, len(vals) - 1)], None, "scalar"))
    return out


def needs(inp, scalar):
    """(slices, 3) bytes of every component by the definition (VBR)"""
    ns = inp.geo.ys * inp.geo.xs
    return np.array([[len(plain(inp.recs[c][s], scalar)[1]) for c in range(3)] for s in range(ns)])


def gen_cbr(geo, prefix=0, scalar=1):
    """budgets around what a slice needs: V's room = need, need + 1, need + scalar - 1 (a remainder the length byte does not
    show), and a room of 255 units with and without a remainder; slices of every total mod 4 at every offset mod 4.  Refused,
    each in a call of its own: need - 1, and a room of 256 units"""
    ns = geo.ys * geo.xs
    rng = _rng("cbr", geo.name, scalar)
    recs = _blank(geo, rng, 0.3)
    for s in range(ns):
        for c, n in enumerate(geo_n(geo)):
            k = int(rng.integers(1, min(n, 8 * 150 * scalar) + 1))
            bits = int(rng.integers(4 * 1, min(12 * k, 8 * 200 * scalar) + 1))
            while not feasible(bits, k) or bits - 4 < k - 1:
                bits += 1
            recs[c][s] = 0
            recs[c][s, :k] = values_exact(bits, k, rng, True)
    base = Input("cbr", "base", geo, recs, _qidx(geo), [(s, 2, int(np.flatnonzero(recs[2][s])[-1])) for s in range(ns)])
    need = needs(base, scalar)
    tot = need.sum(axis=1) + 4
    out = []
    extras = {"need": np.zeros(ns, int), "plus1": np.ones(ns, int), "rem": np.full(ns, scalar - 1),
              "mix": (np.arange(ns) * 3 + np.arange(ns) // 4) % max(2 * scalar, 4),
              "full": 255 * scalar - need[:, 2], "fullrem": 255 * scalar + scalar - 1 - need[:, 2]}
    for tag, extra in extras.items():
        out.append(base._replace(tag=tag, budgets=(tot + extra).astype(np.int32)))
    s = ns // 3
    b = tot.copy()
    b[s] -= 1
    out.append(base._replace(tag="refused_toobig", budgets=b.astype(np.int32), refused="toobig"))
    b = tot.copy()
    b[s] += 256 * scalar - need[s, 2]
    out.append(base._replace(tag="refused_len", budgets=b.astype(np.int32), refused="len"))
    return out + [x for x in (longest(geo, scalar), longest(geo, scalar, dense=True)) if x]


def longest(geo, scalar, dense=False):
    """Y, U and V's room at 255 units, every other slice with a remainder of scalar - 1 bytes in V's room beyond them: the
    longest slice the reference writes, 4 + 3 * 255 * scalar + scalar - 1 bytes.  dense: V's codes end exactly on its 255
    units and 8 * scalar zeros follow, whose '1's the reference writes into the remainder (the bounded write keeps what
    fits): 0xFF there, not padding.  None where the coefficients cannot hold 255 units"""
    ns, n = geo.ys * geo.xs, geo_n(geo)
    if not all(8 * 255 * scalar <= 32 * x for x in n):
        return None
    if dense and not feasible(8 * 255 * scalar - 32, n[2] - 8 * scalar - 1):
        return None
    rng = _rng("cbr", geo.name, scalar, "longest", int(dense))
    recs = _blank(geo, rng, 0.05)
    _fit(recs, [], scalar)
    for s in range(ns):
        for c in range(2):
            vals = _component_of_bytes(n[c], 255 * scalar, rng)
            recs[c][s] = 0
            recs[c][s, :len(vals)] = vals
        if dense:
            recs[2][s] = 0
            recs[2][s, :n[2] - 8 * scalar] = values_exact(8 * 255 * scalar, n[2] - 8 * scalar, rng, True)
    named = [(s, c, int(np.flatnonzero(recs[c][s])[-1])) for s in range(ns) for c in range(3) if recs[c][s].any()]
    inp = Input("cbr", "longest_dense" if dense else "longest", geo, recs, _qidx(geo), named)
    nd = needs(inp, scalar)
    return inp._replace(budgets=(4 + nd[:, 0] + nd[:, 1] + 255 * scalar + (scalar - 1) * (np.arange(ns) % 2)).astype(np.int32))


def gen_tiles(geo, prefix=0, scalar=1):
    """slice counts that leave 1, 2 and 3 slices (and a whole tile less one) in the last tile; slices of very different
    lengths side by side in a wavefront; a picture of zeros"""
    f = pack_form(geo, prefix, scalar)
    tile = 4 * f.S
    out = []
    for extra in (1, 2, 3, tile - 1, 0):
        ns = 2 * tile + extra if tile <= 8 else tile + extra + (tile if extra == 0 else 0)
        g2 = geo._replace(ys=1, xs=ns)
        rng = _rng("tiles", geo.name, scalar, extra)
        recs = [np.zeros((ns, n), np.int32) for n in geo_n(geo)]
        named = []
        for s in range(ns):
            for c, n in enumerate(geo_n(geo)):
                k = int(rng.integers(1, n + 1))
                hi = min(32 * k, 8 * (3, 40, 120, 250)[(s + c) % 4] * scalar)
                bits = int(rng.integers(4, max(hi, 5)))
                while not feasible(bits, k) or bits - 4 < k - 1:
                    bits += 1
                if bits > min(32 * k, 8 * 255 * scalar):
                    continue
                recs[c][s, :k] = values_exact(bits, k, rng, True)
                named.append((s, c, k - 1))
        out.append(Input("tiles", f"t{ns}", g2, recs, _qidx(g2), named))
    out.append(Input("tiles", "zeros", geo, [np.zeros((geo.ys * geo.xs, n), np.int32) for n in geo_n(geo)], _qidx(geo), []))
    return out


def _settle(rec, scalar):
    """keep a random component off the two edges that `last` and `units` are there for: its count is no whole number of
    units' bits, and the zeros behind its last value end before the component's last bit (so no code, not even the '1' of a
    zero, ends exactly on the limit, and the zeros do not reach another unit).  Where needed the last coefficient becomes
    +-1 or -3, also in a component of zeros.  A component whose n zeros alone pass 250 units (2304 coefficients at scalar 1)
    cannot be settled: unsettled()"""
    n = rec.shape[1]
    for v in rec:
        for _ in range(3):
            nz = np.flatnonzero(v)
            if nz.size == 0:                      # (an all-zero component is `last`'s and `tiles`')
                v[n - 1] = 1
                continue
            last = int(nz[-1])
            c = sum(len(code(int(x))) for x in v[:last + 1])
            limit = 8 * scalar * -(-(-(-c // 8)) // scalar)
            if c != limit and c + (n - 1 - last) < limit:
                break
            grow = (n - 1 - last) - 1 if last < n - 1 else -len(code(int(v[-1])))
            if c + grow + 6 > 8 * 250 * scalar:
                break
            v[n - 1] = 1 if (c + grow + 4) % (8 * scalar) else -3
    return rec


def unsettled(geo, scalar):
    """no random input of this geometry can stay off those edges: a component's zeros alone pass 250 units"""
    return max(geo_n(geo)) + 6 > 8 * 250 * scalar


def gen_random(geo, prefix=0, scalar=1, pictures=3):
    """K geometric over 1 .. 9 (magnitudes inside the code table), stretches of zeros: the net under the designed ones, what
    quantised pictures look like"""
    out = []
    ns = geo.ys * geo.xs
    for pic in range(pictures):
        rng = _rng("random", geo.name, scalar, pic)
        recs = []
        for n in geo_n(geo):
            K = np.minimum(rng.geometric(0.6, (ns, n)), 9)
            lo = (1 << K) - 1
            mag = lo + (rng.random((ns, n)) * (lo + 1)).astype(np.int64)
            v = mag * rng.choice((-1, 1), (ns, n))
            run = np.cumsum(rng.random((ns, n)) < 0.12, axis=1) % 2 == 1       # alternating stretches of zeros
            # (half the values zero, more where n coefficients would not fit 200 units: 1 + 4.3 p bits a coefficient)
            v[run | (rng.random((ns, n)) >= min(0.5, max((1600 * scalar / n - 1) / 4.3, 0.02)))] = 0
            budget = 8 * 250 * scalar                                            # keep every component within 255 units
            bits = np.where(v == 0, 1, 2 * np.floor(np.log2(np.abs(v) + 1.0)).astype(np.int64) + 2)
            v[np.cumsum(bits, axis=1) > budget] = 0
            recs.append(_settle(v.astype(np.int32), scalar))
        out.append(Input("random", f"r{pic}", geo, recs, _qidx(geo, pic), []))
    return out


GENERATORS = {"strings": gen_strings, "phase": gen_phase, "last": gen_last, "units": gen_units, "cbr": gen_cbr,
              "tiles": gen_tiles, "random": gen_random}
LARGE_GENERATORS = ("strings", "last", "units", "random")


@lru_cache(maxsize=None)
def inputs(gen, gname, prefix=0, scalar=1):
    return tuple(GENERATORS[gen](GEOS[gname], prefix, scalar))


def with_budgets(inp, scalar, seed=0):
    """an accepted VBR input under HQ_CBR: what every slice needs plus a seeded remainder for V"""
    nd = needs(inp, scalar)
    rng = _rng("budgets", inp.gen, inp.tag, seed)
    extra = np.minimum(rng.integers(0, 2 * scalar + 3, nd.shape[0]), 255 * scalar + scalar - 1 - nd[:, 2])    # a length byte of 255 at most
    return inp._replace(budgets=(nd.sum(axis=1) + 4 + extra).astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# k_hq_pack's decisions
# ---------------------------------------------------------------------------------------------------------------------
# (what catches it, the mutant): the first twelve are caught by designed inputs only; the rest are coarse enough for `random` too
MUTANTS = (
    ("strings", "write8_short limit 65"),                    # !__any(c.sum > 65): a string of 65 bits in a register pair
    ("phase", "sign bit position at K = 15"),
    ("last", "table of 1025 codes"),                         # mag >= VLC_LUT_N + 1: 1024 read from the table's entry 0
    ("units", "refusal at 254 units"),                       # len > 254
    ("units", "no refusal at 256 units"),                    # len > 256
    ("cbr", "length byte from need"),                        # under HQ_CBR
    ("cbr", "V refused at room = need"),                     # vb <= need
    ("cbr", "no refusal at a room of 256 units"),            # vb / scalar > 256
    ("cbr", "a room of 255 units and a remainder refused"),  # vb > 255 * scalar
    ("cbr", "an image of three times 255 units"),            # the image as it was: see Found
    ("last", "count through the last code"),                 # last_end set by zeros too
    ("units", "code dropped when it ends at the limit"),     # pos + nb < limit
    ("tiles", "seg_off over s2 <= seg"),
    ("strings", "run not carried across rounds"),
    ("phase", "short string cut one bit early"),             # keep = limit - pos - 1
    ("last", "U's total from the wrong lane"),               # __shfl(incl, seg * W + W / 2) for W / 2 - 1
)
DESIGNED_ONLY = 12
PLAIN_MUTANTS = ("count through the last code", "length byte from need")


def _code_bits(v, mut):
    c = code(int(v))
    if mut == "sign bit position at K = 15" and len(c) == 32:
        c = c[:30] + c[31] + c[30]
    if mut == "table of 1025 codes" and abs(int(v)) == 1024:
        c = "1"                                        # entry 0's code of one bit, the sign OR-ed into it
    return c


def _or(img, total_bits, pos, bits):
    return img | (int(bits, 2) << (total_bits - pos - len(bits))) if bits else img


def model(inp, prefix, scalar, single_pass=False, mut=None, reach=None):
    """the payload as k_hq_pack's decisions make it -- plain's for the unmutated model -- or Refused.  reach: a Counter"""
    geo = inp.geo
    cbr = inp.budgets is not None
    f = pack_form(geo, prefix, scalar, single_pass, cbr)
    reach = Counter() if reach is None else reach
    ns, ncs = geo.ys * geo.xs, geo_n(geo)
    W, S = f.W, f.S
    iw = img_words(prefix, scalar)
    nbits = 32 * iw
    inv = inv_up(scalar)
    refused = set()

    def hit(key, cond):
        if cond:
            reach[key] += 1
    per_wave = S
    totals, images = [0] * ns, [b""] * ns

    def comp_len(count):
        nb = (count + 7) >> 3
        ln = int(np.float32(nb + scalar - 1) * inv)
        assert mut or ln == -(-nb // scalar)
        if ln > {"refusal at 254 units": 254, "no refusal at 256 units": 256}.get(mut, 255):
            refused.add("scalar")
            ln = 255
        if ln in (1, 2, 254, 255):
            reach["units", ln] += 1
        return ln * scalar

    def lanes_of(values, j0s):
        """per lane: (codes, sum, last_end)"""
        out = []
        n = len(values)
        for j0 in j0s:
            cs = [_code_bits(values[j], mut) for j in range(j0, min(j0 + 8, n))] if j0 < n else []
            sm = le = 0
            for k, c in enumerate(cs):
                sm += len(c)
                if values[j0 + k] != 0 or mut == "count through the last code":
                    le = sm
            out.append((cs, sm, le))
        return out

    def write8(img, pos, limit, cs):
        for c in cs:
            ok = pos + len(c) < limit if mut == "code dropped when it ends at the limit" else pos + len(c) <= limit
            if ok:
                img = _or(img, nbits, pos, c)
                hit("ends at the limit", pos + len(c) == limit and len(c) > 1)
            pos += len(c)
        return img

    def write8_short(img, pos, limit, cs, sm):
        bits = "".join(cs)
        if sm > 64:                                # (only a wrong copy comes here: the register pair loses the leading bits)
            bits = bits[-64:]
        if pos + sm > limit:
            keep = max(limit - pos - (1 if mut == "short string cut one bit early" else 0), 0)
            reach["short string cut"] += 1
            bits = bits[:keep]
        if bits:
            reach["short string over words", (pos % 32 + len(bits) + 31) // 32] += 1
        return _or(img, nbits, pos, bits)

    for w0 in range(0, ns, per_wave):
        wave = list(range(w0, min(w0 + per_wave, ns)))
        st = {s: dict(img=0, base=prefix + 1, bytes=[0, 0, 0], bad=False) for s in wave}

        def cbr_v(s, need):
            if not cbr:
                return need
            vb = int(inp.budgets[s]) - 4 - st[s]["bytes"][0] - st[s]["bytes"][1]
            if vb < need or (mut == "V refused at room = need" and vb == need):
                refused.add("toobig")
                st[s]["bad"] = True
                return need
            if mut == "a room of 255 units and a remainder refused" and vb > 255 * scalar:
                refused.add("len")
                st[s]["bad"] = True
                return need
            if vb // scalar > (256 if mut == "no refusal at a room of 256 units" else 255):
                refused.add("len")
                st[s]["bad"] = True
                return need
            reach["V room", "need" if vb == need else "remainder" if vb % scalar else "units"] += 1
            hit("V room of 255 units", vb // scalar == 255)
            return vb

        def put_len(s, base, nbytes, c):
            lb = nbytes // scalar
            if cbr and c == 2 and mut == "length byte from need":
                lb = st[s]["need_v"] // scalar
            st[s]["img"] = _or(st[s]["img"], nbits, 8 * base, format(lb & 0xFF, "08b"))

        if f.fast:
            # luma
            L = {s: lanes_of(inp.recs[0][s], range(0, 8 * W, 8)) for s in wave}
            short = not any(sm > (65 if mut == "write8_short limit 65" else 64) for s in wave for _, sm, _ in L[s])
            mx = max(sm for s in wave for _, sm, _ in L[s])
            reach["write8_short" if short else "write8", min(mx, 67)] += 1
            for s in wave:
                d = st[s]
                incl, count = 0, 0
                starts = []
                for cs, sm, le in L[s]:
                    starts.append(incl)
                    if le:
                        count = max(count, incl + le)
                    incl += sm
                d["bytes"][0] = comp_len(count)
                lim = 8 * (d["base"] + 1 + d["bytes"][0])
                for (cs, sm, le), at in zip(L[s], starts):
                    pos = 8 * (d["base"] + 1) + at
                    if short:
                        hit(("string of", sm), 62 <= sm <= 64)
                        d["img"] = write8_short(d["img"], pos, lim, cs, sm)
                    else:
                        hit(("string of (write8)", sm), 62 <= sm <= 66)
                        d["img"] = write8(d["img"], pos, lim, cs)
                put_len(s, d["base"], d["bytes"][0], 0)
                d["base"] += 1 + d["bytes"][0]
            # chroma: U on the lower half of the lanes, V on the upper
            half = W // 2
            L = {s: lanes_of(inp.recs[1][s], range(0, 8 * half, 8)) + lanes_of(inp.recs[2][s], range(0, 8 * half, 8)) for s in wave}
            short = not any(sm > (65 if mut == "write8_short limit 65" else 64) for s in wave for _, sm, _ in L[s])
            mx = max(sm for s in wave for _, sm, _ in L[s])
            reach["write8_short" if short else "write8", min(mx, 67)] += 1
            for s in wave:
                d = st[s]
                incl, starts = 0, []
                for cs, sm, le in L[s]:
                    starts.append(incl)
                    incl += sm
                total_u = starts[half] if mut != "U's total from the wrong lane" else starts[half] + L[s][half][1]
                cnt = [0, 0]
                for lane, ((cs, sm, le), at) in enumerate(zip(L[s], starts)):
                    h = lane >= half
                    rel = at - (total_u if h else 0)
                    if le:
                        cnt[h] = max(cnt[h], rel + le)
                d["bytes"][1] = comp_len(cnt[0])
                d["need_v"] = comp_len(cnt[1])
                d["bytes"][2] = cbr_v(s, d["need_v"])
                for lane, ((cs, sm, le), at) in enumerate(zip(L[s], starts)):
                    h = lane >= half
                    rel = at - (total_u if h else 0)
                    base_c = d["base"] + 1 + d["bytes"][1] if h else d["base"]
                    lim = 8 * (base_c + 1 + d["bytes"][1 + h])
                    pos = 8 * (base_c + 1) + rel
                    if short:
                        hit(("string of", sm), 62 <= sm <= 64)
                        d["img"] = write8_short(d["img"], pos, lim, cs, sm)
                    else:
                        hit(("string of (write8)", sm), 62 <= sm <= 66)
                        d["img"] = write8(d["img"], pos, lim, cs)
                put_len(s, d["base"], d["bytes"][1], 1)
                put_len(s, d["base"] + 1 + d["bytes"][1], d["bytes"][2], 2)
        else:
            for s in wave:
                d = st[s]
                for c in range(3):
                    vals, n = inp.recs[c][s], ncs[c]
                    run = count = 0
                    rounds = []
                    for r0 in range(0, n, 512):
                        L = lanes_of(vals, range(r0, r0 + 512, 8))
                        incl, starts = 0, []
                        for cs, sm, le in L:
                            starts.append(run + incl)
                            if le:
                                count = max(count, run + incl + le)
                            incl += sm
                        rounds.append((L, starts))
                        if mut != "run not carried across rounds":
                            run += incl
                    reach["rounds", len(rounds)] += 1
                    reach["last round of", min(n - 512 * (len(rounds) - 1), 512)] += 1
                    nb = comp_len(count)
                    if c == 2:
                        d["need_v"] = nb
                        nb = cbr_v(s, nb)
                    d["bytes"][c] = nb
                    lim = 8 * (d["base"] + 1 + nb)
                    for L, starts in rounds:
                        for (cs, sm, le), at in zip(L, starts):
                            d["img"] = write8(d["img"], 8 * (d["base"] + 1) + at, lim, cs)
                    put_len(s, d["base"], nb, c)
                    d["base"] += 1 + nb
        for s in wave:
            d = st[s]
            d["img"] = _or(d["img"], nbits, 8 * prefix, format(int(inp.qidx[s]) & 0xFF, "08b"))
            totals[s] = prefix + 4 + sum(d["bytes"])
            images[s] = d["img"].to_bytes(nbits // 8, "big")
            old = 4 * ((prefix + 4 + 3 * 255 * scalar + 3) // 4 + 2)
            if mut == "an image of three times 255 units" and totals[s] > old:      # what lay behind it was another image's
                images[s] = images[s][:old] + b"\xA5" * (totals[s] - old)
            assert totals[s] <= 4 * iw - 8
            hit("slice bytes beyond three times 255 units", totals[s] > prefix + 4 + 3 * 255 * scalar)
    if refused:
        raise Refused(sorted(refused)[0])
    # where every slice goes: the offsets of the form's copy-out
    out = bytearray(sum(totals))
    per_tile = f.waves * S
    base = 0
    for t0 in range(0, ns, per_tile):
        tile = list(range(t0, min(t0 + per_tile, ns)))
        reach["tile start mod 4", base % 4] += 1
        hit(("slices in the last tile", len(tile)), t0 + per_tile >= ns)
        for s in tile:
            w = (s - t0) // S
            seg = (s - t0) % S
            w_first = t0 + w * S
            off = sum(totals[t0:w_first])
            off += sum(totals[w_first + k] for k in range(S) if w_first + k < ns and (k <= seg if mut == "seg_off over s2 <= seg" and S > 1 else k < seg))
            at = base + off
            head = min((4 - at % 4) % 4, totals[s])
            tail = (totals[s] - head) % 4
            if f.lookback or cbr or f.tile_slices:
                reach["copy-out head", head] += 1
                reach["copy-out tail", tail] += 1
            if S > 1:
                hit("slices of a wavefront differ", len({totals[k] for k in range(w_first, min(w_first + S, ns))}) > 1 and seg == 0)
            out[at:at + totals[s]] = images[s][:totals[s]]
        base += sum(totals[s] for s in tile)
    return bytes(out[:sum(totals)])


def trace(inp, prefix, scalar, single_pass=False):
    r = Counter()
    try:
        model(inp, prefix, scalar, single_pass, reach=r)
    except Refused as e:
        r["refused", e.kind] += 1
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the quantising path: designed records as pictures (Haar0, a flat matrix and index 0: every quotient is its coefficient)
# ---------------------------------------------------------------------------------------------------------------------
BATCH_SCALAR = 4
BATCH_SLICES = 16           # the designed slices of a picture: its first ones, zeros behind them
# quant_ref's three pictures, and a 256 x 128 4:2:2 picture (int32 store, k_hq_pack with load8_tab) cut into slices of 16 x 8
# luma (four slices a wavefront, shared slots), 32 x 32 (MID: two rounds kept in registers) and 64 x 32 (MID with the
# bits8_tab measuring pass)
BATCH_GEOMS = dict(qr.GEOMS)
BATCH_GEOMS.update({g.name: g for g in (qr.PictureGeom("S16", 256, 128, "422", 2, 2, 4, 4, False),
                                        qr.PictureGeom("M1024", 256, 128, "422", 3, 4, 4, 4, False),
                                        qr.PictureGeom("M2048", 256, 128, "422", 3, 4, 8, 4, False))})


def batch_inputs(oracle, name, gens=("strings", "last", "random")):
    """[(tag, Input on the picture's whole slice grid)] for a geometry of quant_ref (P32, P16, P16W): the generators run on
    the picture's slice dimensions, on BATCH_SLICES slices; `strings` keeps one turn of variant A and variant B"""
    global _CAP
    pg = BATCH_GEOMS[name]
    g = pg.geometry(oracle)
    sub = Geo(name, g.slice_dims(0), g.slice_dims(1), pg.depth, 1, min(BATCH_SLICES, g.n_slices))
    out = []
    for gen in gens:
        _CAP = 14                     # seeded codes of at most 14 bits (|v| <= 126): the samples fit, and the 16-bit store's table path takes them
        try:
            made = gen_last16(sub, heads_of(oracle, name), BATCH_SCALAR) if gen == "last16" else GENERATORS[gen](sub, 0, BATCH_SCALAR)
        finally:
            _CAP = 32
        for inp in made:
            if inp.refused or (gen == "strings" and inp.tag[0] == "A" and not inp.tag.endswith(".0")):
                continue
            recs = [np.zeros((g.n_slices, n), np.int32) for n in geo_n(sub)]
            for c in range(3):
                recs[c][:sub.xs] = inp.recs[c]
            full = Geo(name, sub.luma, sub.chroma, pg.depth, g.ys, g.xs)
            out.append(Input(gen, inp.tag, full, recs, np.zeros(g.n_slices, np.int32), inp.named))
    return out


def batch_picture(oracle, name, inp):
    """(raw picture, quant_ref's Design) of an input: oracle.dwt_inverse of its planes.  A picture is kept only if its samples
    fit, and quant_ref.check_design asserts that oracle.dwt_forward of the ingested picture returns the field"""
    pg = BATCH_GEOMS[name]
    g = pg.geometry(oracle)
    shapes = [(pg.h, pg.w)] + [qr.cr_chroma(pg)] * 2
    pics = [oracle.dwt_inverse(p, qr.KERNELS[pg.wavelet], pg.depth) for p in cr.planes_from_records(g, inp.recs)]
    half = 1 << (pg.bits - 1)
    if min(int(p.min()) for p in pics) < -half or max(int(p.max()) for p in pics) > half - 1:
        return None, None                              # a seeded long code took the samples out of range: not kept
    raw = qr._emit([p[:h, :w] for p, (h, w) in zip(pics, shapes)], pg.bits)
    d = qr.Design(pg, 0, np.zeros(pg.n_bands, np.int32), g, inp.recs, [], 0, raw)
    qr.check_design(oracle, d)
    return raw, d


# ---------------------------------------------------------------------------------------------------------------------
# k_hq_pack16 / k_hq_pack16w's decisions (vc2hip_pack16.h), for the pictures of batch_inputs: a flat matrix and index 0, so
# that the float quotient of a body coefficient is the coefficient itself (inv4[0] is 1.0)
# ---------------------------------------------------------------------------------------------------------------------
P16_MAXQ = 126
MUTANTS16 = (
    ("strings", "string limit 65"),                                  # max(L0, L1) > 65: a string of 65 bits in a register pair
    ("last16", "quotient limit 129"),                                # maxf * fb >= 130: 129 read from the table's entry of -127
    ("last16", "head code dropped when it ends at the room"),        # hpos + hbits < room
    ("last16", "count from the head ballot first"),                  # m = h ? h : b
    ("last16", "body_last from the first string first"),             # last0 ? last0 : L0 + last1
)
EQUIVALENT16 = "string limit 64 for 63"      # max(L0, L1) > 64: no accepted input shows it


def heads_of(oracle, name):
    """[(head coefficients, body lanes of sixteen)] per component, by pack16_plan's rule (quant_ref.pack16_heads)"""
    return qr.pack16_heads(BATCH_GEOMS[name].geometry(oracle))


def gen_last16(geo, heads, scalar):
    """for the 16-bit store's coders: the last non-zero value in the head only (every head lane in turn), in the first string
    of a body lane only and in the second only (first, an inner and the last lane of the component: luma's lanes 0 and 31,
    chroma's 32, 47, 48, 63), a head whose codes end exactly on a whole unit, and +-129 in a body (the first quotient whose
    low byte is another quotient's)"""
    ns, ncs = geo.ys * geo.xs, geo_n(geo)
    jobs = []
    for c, (hn, bn) in enumerate(heads):
        jobs += [(c, "head", i) for i in range(hn)] + [(c, "headend", min(hn, 8 * scalar // 4))]
        for lane in sorted({0, bn // 2, bn - 1}):
            jobs += [(c, "s0", lane), (c, "s1", lane)]
        jobs += [(c, "q129", 0), (c, "q129", bn - 1)]
    out, pic = [], 0
    while jobs:
        rng = _rng("last16", geo.name, pic)
        recs, named, left = [np.zeros((ns, n), np.int32) for n in ncs], [], list(jobs)
        for s in range(ns):
            for c in range(3):
                job = next((j for j in left if j[0] == c), None)
                if job is None:
                    continue
                left.remove(job)
                _, kind, x = job
                hn = heads[c][0]
                if kind == "head":
                    recs[c][s, :x] = rng.integers(-2, 3, x)
                    recs[c][s, x] = (3, -5, 1, -2)[x % 4]
                    named.append((s, c, x))
                elif kind == "headend":                      # x codes of four bits: 8 * scalar bits when x = 2 * scalar
                    recs[c][s, :x] = rng.choice((1, -1, 2, -2), x)
                    named.append((s, c, x - 1))
                else:
                    at = hn + 16 * x + (int(rng.integers(0, 8)) if kind == "s0" else int(rng.integers(8, 16)) if kind == "s1" else 5)
                    recs[c][s, :at] = rng.integers(-1, 2, at) * (rng.random(at) < 0.2)
                    recs[c][s, at] = (129 if s % 2 else -129) if kind == "q129" else (6, -9)[x % 2]
                    named.append((s, c, at))
        jobs = left
        out.append(Input("last16", f"h{pic}", geo, recs, np.zeros(ns, np.int32), named))
        pic += 1
    return out


def model16(inp, heads, wide, prefix, scalar, mut=None, reach=None, slices=BATCH_SLICES):
    """the payload of a batch picture as k_hq_pack16's (wide: k_hq_pack16w's) decisions make it: table path or p16_general and
    why, the head's code and the two strings of every body lane against the component's room, count_of's ballots.  The first
    `slices` slices (the designed ones: the rest of a batch picture is zeros)"""
    reach = Counter() if reach is None else reach
    inv = inv_up(scalar)
    limit = {"string limit 65": 65, EQUIVALENT16: 64}.get(mut, 63)
    qmax = 129 if mut == "quotient limit 129" else P16_MAXQ
    out = bytearray()

    def tcode(v):                     # the table's entry of the quotient's low byte
        t = int(v) & 0xFF
        return code(t if t < 128 else t - 256)

    for s in range(min(slices, inp.geo.ys * inp.geo.xs)):
        why = []
        for c, (hn, bn) in enumerate(heads):
            v = inp.recs[c][s]
            body = np.abs(v[hn:].astype(np.int64)).reshape(bn, 16) if bn else np.zeros((0, 16), np.int64)
            L = [[sum(len(code(int(x))) for x in v[hn + 16 * k + 8 * h:hn + 16 * k + 8 * h + 8]) for h in (0, 1)] for k in range(bn)]
            w = set()
            if (body >= 32768).any():
                w.add("escape")
            if (body > qmax).any():
                w.add("quotient")
            if any(max(l) > limit for l in L):
                w.add("string")
            if (np.abs(v[:hn].astype(np.int64)) > 65534).any():
                w.add("head")
            why.append(w)
        if not wide and any(why):
            why = [set().union(*why)] * 3
        sl = bytearray(prefix) + bytes([int(inp.qidx[s]) & 0xFF])
        for c, (hn, bn) in enumerate(heads):
            v = [int(x) for x in inp.recs[c][s]]
            if why[c]:
                for r in why[c]:
                    reach["p16_general", r] += 1
                lb, data = plain(v, scalar)
                sl.append(lb)
                sl += data
                continue
            reach["table path"] += 1
            hb = [len(code(x)) for x in v[:hn]]
            hpos = [sum(hb[:i]) for i in range(hn)]
            lanes, at = [], sum(hb)
            for k in range(bn):
                g = [v[hn + 16 * k + 8 * h:hn + 16 * k + 8 * h + 8] for h in (0, 1)]
                st = ["".join(tcode(x) for x in grp) for grp in g]
                last = [max([sum(len(tcode(y)) for y in grp[:i + 1]) for i, x in enumerate(grp) if x] or [0]) for grp in g]
                if mut == "body_last from the first string first":
                    bl = last[0] if last[0] else (len(st[0]) + last[1] if last[1] else 0)
                else:
                    bl = len(st[0]) + last[1] if last[1] else last[0]
                lanes.append((at, st, bl))
                for h in (0, 1):
                    if 62 <= len(st[h]) <= 63:
                        reach["string of", len(st[h]), h] += 1
                at += len(st[0]) + len(st[1])
            nzb = [k for k, (_, _, bl) in enumerate(lanes) if bl]
            nzh = [i for i in range(hn) if v[i]]
            first, second = (nzh, nzb) if mut == "count from the head ballot first" else (nzb, nzh)
            m = first or second
            if not m:
                count = 0
            elif m is nzb:
                count = lanes[m[-1]][0] + lanes[m[-1]][2]
            else:
                count = hpos[m[-1]] + hb[m[-1]]
            reach["count_of", "body" if nzb else "head" if nzh else "none"] += 1
            if nzb:
                reach["last in string", 1 if lanes[nzb[-1]][2] > len(lanes[nzb[-1]][1][0]) else 0] += 1
            nbytes = int(np.float32(((count + 7) >> 3) + scalar - 1) * inv) * scalar
            room = 8 * nbytes
            bits = ["0"] * room

            def put(pos, text):
                bits[pos:pos + len(text)] = text

            for i in range(hn):
                ends = hpos[i] + hb[i]
                reach["head code ends at the room"] += ends == room and v[i] != 0
                if ends < room or (ends == room and mut != "head code dropped when it ends at the room"):
                    put(hpos[i], code(v[i]))
            for pos, st, _ in lanes:
                G = [x[-64:] for x in st]                     # (a register pair: only a wrong copy brings more than 64 bits here)
                keep = min(max(room - pos, 0), len(st[0]) + len(st[1]))
                k0 = min(keep, len(st[0]))
                put(pos, G[0][:k0])
                put(pos + len(st[0]), G[1][:keep - k0])
            sl.append(nbytes // scalar)
            if room:
                sl += int("".join(bits[:room]), 2).to_bytes(nbytes, "big")
        out += sl
    return bytes(out)
