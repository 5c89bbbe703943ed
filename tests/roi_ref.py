"""The CPU definition of vc2hip_set_index_offsets (include/vc2hip.h), on tests/cap_ref.py and
tests/capfill_ref.py: capfill_ref's matrix (cap_ref's ten rows plus 1520 x 136), the same three unlike pictures per row, the
caps of cap_ref.caps (from picture 0's lengths WITHOUT offsets).

With a map of int8 offsets o_s, slice s at base b is coded at e_s(b) = min(max(b + o_s, 0), 115).
  HQ_CONSTQ       the payload is ONE quantise_np + hq_pack of the whole picture with the map e_s(q_index)
  HQ_CAPPED       the base b_i is the smallest b in floor .. 115 at which that payload exists and is at most cap bytes -- found
                  by looking at every b, no monotonicity assumed -- or 115 if there is none
  HQ_CAPPED_FILL  capfill_ref's steps with q_i := b_i: a slice's length at e_s(b_i) and e_s(b_i - 1) comes from the oracle on a
                  one-slice picture (capfill_ref.slice_lengths' tiles), a promoted slice gets e_s(b_i - 1), every other
                  e_s(b_i); the payload is one quantise_np + hq_pack of the whole picture with that map
"Not codable" is an OracleError (a length byte beyond 255) or a quantised magnitude above 65534, whose code would pass 32 bits
(VLC.h:27; the oracle's slice coder does not look, so the check is made here on its quantiser's output, as quant_ref.CODE_MAX
and transcode_ref do): under a cap the base does not fit, in the final encode the library raises VC2HIP_ESCALAR or
VC2HIP_ECODE32 at vc2hip_sync."""
import numpy as np

import cap_ref as cr
import capfill_ref as cf
from vc2lib import OracleError

Q_TOP = cr.Q_TOP
MATRIX, IDS, NEW = cf.MATRIX, cf.IDS, cf.NEW
FAST, ESCAPES, WHOLE_PLANE = cf.FAST, cf.ESCAPES, cf.WHOLE_PLANE
NOT_CODABLE = cr.NOT_CODABLE
CODE_MAX = 65534        # the greatest magnitude the reference's 32-bit code words hold
PATTERNS = ("zero", "ramp", "roi", "extremes")
# HQ_CONSTQ runs at floor + CONSTQ_ABOVE, so that the negative offsets of `ramp` and `roi` (-6) stay at or above floor + 6.
# Rows 0, 1 and 2 are raised: at floor + 12 the oracle refused BOTH their noise pictures under `ramp` and `roi` (their noise
# codes from index 28, 37 and 11 on: a length byte beyond 255 below), and tests/test_roi_ref.py allows one refused picture per
# row and pattern.  Their index is the smallest at which index - 6 codes every picture.
CONSTQ_ABOVE = 12
CONSTQ_RAISED = {0: 34, 1: 43, 2: 17}


def eff(b, offs):
    """e_s(b) for every slice"""
    return np.clip(int(b) + np.asarray(offs, np.int64), 0, Q_TOP).astype(np.int32)


def central(n):
    """the central third of n slice rows or columns: [n // 3, max(n // 3 + 1, ceil(2 n / 3)))"""
    lo = n // 3
    return lo, max(lo + 1, (2 * n + 2) // 3)


def pattern(name, ys, xs):
    """the designed maps: ns int8 offsets in raster order"""
    ns = ys * xs
    s = np.arange(ns)
    v, h = s // xs, s % xs
    if name == "zero":
        o = np.zeros(ns, np.int64)
    elif name == "ramp":            # a distinct value per neighbour: raster order and the picture stride show
        o = s % 13 - 6
    elif name == "roi":
        (v0, v1), (h0, h1) = central(ys), central(xs)
        o = np.where((v >= v0) & (v < v1) & (h >= h0) & (h < h1), -6, 4)
    elif name == "extremes":        # both clamps act at every base
        o = np.where((v + h) % 2 == 0, -128, 127)
    elif name == "absolute":        # with q_index 0: the map itself, 0 .. 115
        o = (s * 7 + 3) % (Q_TOP + 1)
    else:
        raise KeyError(name)
    return o.astype(np.int8)


def constq_index(i):
    return CONSTQ_RAISED.get(i, MATRIX[i][9]["floor"] + CONSTQ_ABOVE)


def slice_len(pic, s, q):
    """len_s(q): slice s (raster order) coded alone at index q, as capfill_ref.slice_lengths codes it; None where refused"""
    cache = pic.__dict__.setdefault("_roi_slice_len", {})
    if (s, q) not in cache:
        c, o = pic.case, pic.oracle
        v, h = divmod(s, c.xs)
        qi = np.full((1, 1), q, np.int32)
        tiles = []
        for p in pic.planes:
            sh, sw = p.shape[0] // c.ys, p.shape[1] // c.xs
            tiles.append(np.ascontiguousarray(p[v * sh:(v + 1) * sh, h * sw:(h + 1) * sw], np.int32))
        try:
            y, u, w = (o.quantise_np(t, c.depth, qi, pic.qm) for t in tiles)
            if max(int(np.abs(x.astype(np.int64)).max()) for x in (y, u, w)) > CODE_MAX:
                raise OracleError(-11, "a code beyond 32 bits")
            cache[(s, q)] = len(o.hq_pack(y, u, w, c.depth, qi, c.prefix, c.scalar))
        except OracleError:
            cache[(s, q)] = None
    return cache[(s, q)]


class Mapped:
    """one cap_ref.Picture under one map of offsets"""

    def __init__(self, pic, offs):
        c = pic.case
        self.pic, self.case, self.ns = pic, c, c.ys * c.xs
        self.offs = np.asarray(offs, np.int8).reshape(-1)
        assert self.offs.size == self.ns
        self._pay, self._len = {}, {}

    def qmap(self, b):
        return eff(b, self.offs).reshape(self.case.ys, self.case.xs)

    def _code(self, qmap):
        c, o, p = self.case, self.pic.oracle, self.pic
        try:
            y, u, v = (o.quantise_np(pl, c.depth, qmap, p.qm) for pl in p.planes)
            if max(int(np.abs(x.astype(np.int64)).max()) for x in (y, u, v)) > CODE_MAX:
                return NOT_CODABLE
            return o.hq_pack(y, u, v, c.depth, qmap, c.prefix, c.scalar).tobytes()
        except OracleError:
            return NOT_CODABLE

    def coded(self, qmap):
        """the oracle's payload of the whole picture with the index map; NOT_CODABLE where its encoder refuses"""
        qmap = np.ascontiguousarray(qmap, np.int32).reshape(self.case.ys, self.case.xs)
        key = qmap.tobytes()
        if key not in self._pay:
            self._pay[key] = self._code(qmap)
        return self._pay[key]

    def payload(self, b):
        return self.coded(self.qmap(b))

    def length(self, b):
        """the payload's length at base b (the payloads of the search are not kept, their lengths are)"""
        qmap = np.ascontiguousarray(self.qmap(b))
        key = qmap.tobytes()
        if key not in self._len:
            pay = self._pay[key] if key in self._pay else self._code(qmap)
            self._len[key] = NOT_CODABLE if pay is NOT_CODABLE else len(pay)
        return self._len[key]

    def fits(self, b, cap):
        n = self.length(b)
        return n is not NOT_CODABLE and n <= cap

    def base(self, floor, cap):
        """the definition: every base is looked at"""
        fitting = [b for b in range(floor, Q_TOP + 1) if self.fits(b, cap)]
        return min(fitting) if fitting else Q_TOP


class Filled:
    """HQ_CAPPED_FILL of one Mapped picture under (floor, cap)"""

    def __init__(self, m, floor, cap):
        self.m, self.floor, self.cap, self.ns = m, floor, cap, m.ns
        self.b_i = m.base(floor, cap)
        self.filled = self.b_i != floor and m.fits(self.b_i, cap)
        self.order = cf.visit_order(self.ns)
        self.promoted = []
        self.spare = self.cost = self.eligible = None
        at_map = m.qmap(self.b_i).reshape(-1)
        self.qmap = at_map.copy()
        if self.filled:
            below_map = m.qmap(self.b_i - 1).reshape(-1)
            at = [slice_len(m.pic, s, int(at_map[s])) for s in range(self.ns)]
            below = [slice_len(m.pic, s, int(below_map[s])) for s in range(self.ns)]
            assert all(x is not None for x in at), "the picture codes at b_i, so every slice does"
            self.len_at, self.len_below = at, below
            self.spare = cap - sum(at)
            self.eligible = [x is not None for x in below]
            self.cost = [b - a if b is not None else 0 for a, b in zip(at, below)]
            run = 0
            for s in self.order:
                run += self.cost[s]
                if self.eligible[s] and run <= self.spare:
                    self.promoted.append(s)
            for s in self.promoted:
                self.qmap[s] = below_map[s]
        self.qmap = self.qmap.reshape(m.case.ys, m.case.xs)

    def payload(self):
        return self.m.coded(self.qmap)


_MAPPED = {}


def mapped(oracle, i, name, k):
    """Mapped(picture k of row i, pattern name), once per session"""
    if (i, name, k) not in _MAPPED:
        case, pics = cf.batch(oracle, i)
        _MAPPED[(i, name, k)] = Mapped(pics[k], pattern(name, case.ys, case.xs))
    return _MAPPED[(i, name, k)]


def fill(m, floor, cap):
    cache = m.__dict__.setdefault("_fills", {})
    if (floor, cap) not in cache:
        cache[(floor, cap)] = Filled(m, floor, cap)
    return cache[(floor, cap)]


def caps(oracle, i):
    case, pics = cf.batch(oracle, i)
    return cf.caps(case, pics[0])


def expected(oracle, i, name, k, mode, cname=None):
    """(index map, payload or NOT_CODABLE) of picture k of row i under pattern `name`: mode 0 at constq_index, 3 / 4 under
    the named cap of cap_ref.caps"""
    m = mapped(oracle, i, name, k)
    case = m.case
    if mode == 0:
        b = 0 if name == "absolute" else constq_index(i)
        return m.qmap(b), m.payload(b)
    cap = caps(oracle, i)[cname][0]
    if mode == cr.MODE:
        b = m.base(case.q, cap)
        return m.qmap(b), m.payload(b)
    f = fill(m, case.q, cap)
    return f.qmap, f.payload()


def refused(oracle, i, name, mode, cname=None):
    """the pictures of row i whose final encode the oracle refuses (the library raises its error at vc2hip_sync)"""
    return [k for k in range(3) if expected(oracle, i, name, k, mode, cname)[1] is NOT_CODABLE]
