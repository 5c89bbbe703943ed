"""The CPU definition of VC2HIP_HQ_CAPPED_FILL (include/vc2hip.h), on tests/cap_ref.py: the same matrix
plus one row, the same three unlike pictures per row, the same five caps.

Per picture: q_i is cap_ref's choice.  If q_i is the floor or the picture does not fit at q_i, every slice gets q_i.  Otherwise
every slice's length at q_i - 1 and at q_i comes from the oracle on a ONE-SLICE picture: slice (v, h) of a padded coefficient
plane is the tile plane[v * sh:(v + 1) * sh, h * sw:(h + 1) * sw] (the planes are in in-place order, so the tile holds exactly
the slice's coefficients of every subband), coded by quantise_np + hq_pack with a 1 x 1 index array; an OracleError there is
"not eligible".  The slices are visited in bit-reversed order and promoted to q_i - 1 while the running sum of their costs
stays within the spare bytes; the expected payload is ONE quantise_np + hq_pack of the whole picture with the mixed map."""
import numpy as np

import cap_ref as cr
from vc2lib import OracleError

MODE = 4          # VC2HIP_HQ_CAPPED_FILL
Q_TOP = cr.Q_TOP

# 17 x 95 = 1615 slices: above 1024 and no power of two (B = 11, 433 positions skipped); general form, LDS
NEW_ROW = (1520, 136, "422", 10, 2, "DD97", 3, 1, 2, dict(floor=6, scalar=1))
MATRIX = list(cr.MATRIX) + [NEW_ROW]
NEW = len(cr.MATRIX)
FAST, ESCAPES, WHOLE_PLANE = cr.FAST, cr.ESCAPES, cr.WHOLE_PLANE
IDS = ["-".join(str(x) for x in r[:9]) for r in MATRIX]
CAPS = ("floor", "mid", "mid-1", "empty", "none")

_NEW_BATCH = []


def batch(oracle, i):
    """(case, [Picture] * 3) of row i, computed once per session (rows of cap_ref.MATRIX: cap_ref's own)"""
    if i < NEW:
        return cr.batch(oracle, i)
    if not _NEW_BATCH:
        case = cr.matrix_case(oracle, NEW_ROW)
        _NEW_BATCH.append((case, [cr.Picture(oracle, case, raw) for raw in cr.pictures(case)]))
    return _NEW_BATCH[0]


caps = cr.caps


def visit_order(ns):
    """the slices in the order they are visited: rev_B(k) for k = 0 .. 2^B - 1, B = the bits of ns - 1, those >= ns skipped"""
    B = (ns - 1).bit_length()
    out = []
    for k in range(1 << B):
        s = int(format(k, "0%db" % B)[::-1], 2) if B else 0
        if s < ns:
            out.append(s)
    return out


def slice_lengths(pic, q):
    """len_s(q) of every slice in raster order, from one-slice pictures; None where the oracle refuses the slice"""
    cache = pic.__dict__.setdefault("_slice_lens", {})
    if q not in cache:
        c, o = pic.case, pic.oracle
        qi = np.full((1, 1), q, np.int32)
        out = []
        for v in range(c.ys):
            for h in range(c.xs):
                tiles = []
                for p in pic.planes:
                    sh, sw = p.shape[0] // c.ys, p.shape[1] // c.xs
                    tiles.append(np.ascontiguousarray(p[v * sh:(v + 1) * sh, h * sw:(h + 1) * sw], np.int32))
                try:
                    y, u, w = (o.quantise_np(t, c.depth, qi, pic.qm) for t in tiles)
                    out.append(len(o.hq_pack(y, u, w, c.depth, qi, c.prefix, c.scalar)))
                except OracleError:
                    out.append(None)
        cache[q] = out
    return cache[q]


def slice_indices(pay, ns, prefix, scalar):
    """the index byte of every slice header, by a walk over the length bytes"""
    pos, out = 0, []
    for _ in range(ns):
        pos += prefix
        out.append(pay[pos])
        pos += 1
        for _ in range(3):
            pos += 1 + pay[pos] * scalar
    assert pos == len(pay)
    return out


class Filled:
    """one picture under (floor, cap): q_i, the index map, and what the tests ask about the way there"""

    def __init__(self, pic, floor, cap):
        c = pic.case
        self.pic, self.floor, self.cap, self.ns = pic, floor, cap, c.ys * c.xs
        self.q_i = pic.chosen(floor, cap)
        self.filled = self.q_i != floor and pic.fits(self.q_i, cap)    # step 1
        self.order = visit_order(self.ns)
        self.promoted = []                                             # in visit order
        self.spare, self.cost, self.eligible = None, None, None
        if self.filled:
            at, below = slice_lengths(pic, self.q_i), slice_lengths(pic, self.q_i - 1)
            assert all(x is not None for x in at), "the picture codes at q_i, so every slice does"
            self.len_at, self.len_below = at, below
            self.spare = cap - sum(at)
            self.eligible = [b is not None for b in below]
            self.cost = [b - a if b is not None else 0 for a, b in zip(at, below)]
            run = 0
            for s in self.order:                                       # steps 3 and 4
                run += self.cost[s]
                if self.eligible[s] and run <= self.spare:
                    self.promoted.append(s)
        q = np.full(self.ns, self.q_i, np.int32)
        q[np.asarray(self.promoted, np.int64)] -= 1
        self.qmap = q.reshape(c.ys, c.xs)
        self._pay = None

    def payload(self):
        """step 5: the oracle's payload of the whole picture with the map"""
        if self._pay is None:
            if not self.promoted:
                self._pay = self.pic.payload(self.q_i)
            else:
                c, o, p = self.pic.case, self.pic.oracle, self.pic
                y, u, v = (o.quantise_np(pl, c.depth, self.qmap, p.qm) for pl in p.planes)
                self._pay = o.hq_pack(y, u, v, c.depth, self.qmap, c.prefix, c.scalar).tobytes()
        return self._pay


def fill(pic, floor, cap):
    """Filled(pic, floor, cap), computed once per session"""
    cache = pic.__dict__.setdefault("_fills", {})
    if (floor, cap) not in cache:
        cache[(floor, cap)] = Filled(pic, floor, cap)
    return cache[(floor, cap)]
