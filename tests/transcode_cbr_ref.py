"""The CPU definition of vc2hip_transcode_cbr_batch_dev (include/vc2hip.h), composed of the oracle's
own functions on top of tests/transcode_ref.py, and the budgets the HQ_CBR transcode tests share.

For one picture, from the bytes the call may look at, the way they are coded (the row's prefix and scalar) and the output's
(compressed_bytes, prefix, scalar), with B = oracle.slice_bytes(ys, xs, compressed_bytes, scalar):
  1. (y, u, v, q_s) = oracle.hq_unpack at the input's prefix and scalar (transcode_ref.Coded);
  2. need_s = the bytes of slice s's coefficient values as they are, per component trimmed behind the last non-zero value
     and rounded up to the output scalar (slice_need: component_slice_bytes, Slices.cpp:97-119).  A slice is KEPT iff each of
     its components is codable (length byte <= 255) and need_s <= B[s] - 4;
  3. a kept slice ends at q'_s = q_s, its values untouched;
  4. every other slice is SEARCHED: C = dequantise_np(c, q_s), q'_s = what oracle.cbr_qindices finds for it on C under B[s]
     and the output scalar, its values quantise_np(C, q'_s).  The search has no state across slices, so one whole-picture
     call with the kept slices' blocks set to zero gives every searched slice's index (and raises nothing for a kept one);
  5. oracle.hq_pack(y', u', v', q', prefix, scalar, cbr=B): B.sum() + slices * prefix bytes, always.
The composition refuses as its parts refuse: ESTREAM (the reader), EQINDEX (the dequantiser, a search trial), ESCALAR (a
search trial), ECBR_TOOBIG / ECBR_LEN (the CBR writer)."""
import numpy as np

import transcode_ref as tr
from vc2lib import OracleError

ECBR_TOOBIG, ECBR_LEN = -4, -5
ROWS_MIXED = ("A", "B", "C", "D", "E", "G", "H", "I")      # (row F: one slice per picture, its search is refused)
ROWS_CHANGED = ("A", "C", "G", "I")                        # the rows also coded at prefix + 1, scalar * 2


def _coded_order(sh, sw, depth):
    """(rows, columns) of a slice's coefficients inside its sh x sw block of the in-place plane, in coded order: subband by
    subband from the coarsest, LL, then HL, LH, HH of every level, each row by row"""
    ys, xs = [], []
    for band in range(3 * depth + 1):
        if band == 0:
            s, oy, ox = 1 << depth, 0, 0
        else:
            level, kind = (band - 1) // 3 + 1, (band - 1) % 3
            s = 1 << (depth + 1 - level)
            oy, ox = (0 if kind == 0 else s // 2), (0 if kind == 1 else s // 2)
        yy, xx = np.mgrid[oy:sh:s, ox:sw:s]
        ys.append(yy.ravel())
        xs.append(xx.ravel())
    return np.concatenate(ys), np.concatenate(xs)


def component_length_bytes(case, plane, scalar):
    """(ys, xs) int64: every slice's length byte for this component at `scalar` -- SignedVLC bits through the last non-zero
    value in coded order, in bytes, in units of the scalar; beyond 255 where the slice writer would refuse"""
    ph, pw = plane.shape
    sh, sw = ph // case.ys, pw // case.xs
    oy, ox = _coded_order(sh, sw, case.depth)
    blocks = plane.reshape(case.ys, sh, case.xs, sw).transpose(0, 2, 1, 3)[:, :, oy, ox].astype(np.int64)
    mag = np.abs(blocks)
    bits = np.where(mag == 0, 1, 2 * np.floor(np.log2(mag + 1)).astype(np.int64) + 2)
    gross = np.cumsum(bits, axis=2)
    count = np.where(mag != 0, gross, 0).max(axis=2)
    return ((count + 7) // 8 + scalar - 1) // scalar


def slice_need(case, planes, scalar):
    """(need_s, codable_s), both (ys, xs)"""
    lens = [component_length_bytes(case, p, scalar) for p in planes]
    return sum(lens) * scalar, np.logical_and.reduce([l <= 255 for l in lens])


def written_length_bytes(oracle, case, planes, q, scalar):
    """the three length bytes of every slice as oracle.hq_pack writes them (VBR, prefix 0): (3, ys, xs)"""
    pay = oracle.hq_pack(*planes, case.depth, q, 0, scalar).tobytes()
    out, p = np.zeros((case.ys * case.xs, 3), np.int64), 0
    for s in range(case.ys * case.xs):
        p += 1
        for c in range(3):
            out[s, c] = pay[p]
            p += 1 + pay[p] * scalar
    assert p == len(pay)
    return out.T.reshape(3, case.ys, case.xs)


def block_mask(case, per_slice, shape):
    return np.kron(per_slice, np.ones((shape[0] // case.ys, shape[1] // case.xs), bool)).astype(bool)


class Out:
    """what the definition makes of one picture under (s_out, prefix, scalar)"""

    def __init__(self, oracle, pic, s_out, prefix, scalar):
        case = pic.case
        self.budgets = oracle.slice_bytes(case.ys, case.xs, s_out, scalar)
        self.need, codable = slice_need(case, pic.planes, scalar)
        self.keep = codable & (self.need <= self.budgets - 4)
        # only the searched slices meet the dequantiser: a kept slice's block goes through it at index 0 and is then set to zero
        q_deq = np.where(self.keep, 0, pic.q).astype(np.int32)
        deq = [oracle.dequantise_np(c, case.depth, q_deq, pic.qm) for c in pic.planes]
        zeroed = [np.where(block_mask(case, self.keep, d.shape), 0, d).astype(np.int32) for d in deq]
        searched = oracle.cbr_qindices(*zeroed, case.depth, pic.qm, self.budgets, scalar)
        self.q = np.where(self.keep, pic.q, searched).astype(np.int32)
        self.planes = [np.where(block_mask(case, self.keep, c.shape), c, oracle.quantise_np(d, case.depth, self.q, pic.qm)).astype(np.int32)
                       for c, d in zip(pic.planes, deq)]
        self.payload = oracle.hq_pack(*self.planes, case.depth, self.q, prefix, scalar, cbr=self.budgets).tobytes()
        self.total = int(self.budgets.sum()) + case.ys * case.xs * prefix
        assert len(self.payload) == self.total


_OUTS = {}


def transcode_cbr(oracle, pic, s_out, prefix=None, scalar=None):
    """the definition's Out for a transcode_ref.Coded, or the OracleError it refuses with (returned, not raised); computed once"""
    prefix = pic.case.prefix if prefix is None else prefix
    scalar = pic.case.scalar if scalar is None else scalar
    key = (id(pic), s_out, prefix, scalar)
    if key not in _OUTS:
        try:
            _OUTS[key] = (pic, Out(oracle, pic, s_out, prefix, scalar))
        except OracleError as e:
            _OUTS[key] = (pic, e)
    return _OUTS[key][1]


class Unpacked:
    """what Out needs of a coded picture, without transcode_ref.Coded's dequantisation of every slice (which refuses an index
    the composition never dequantises: a kept slice's)"""

    def __init__(self, oracle, case, payload):
        import proxy_ref as pr
        from vc2lib import KERNELS
        self.case, self.payload = case, bytes(payload)
        self.qm = oracle.quant_matrix(KERNELS[case.kernel], case.depth)
        y, u, v, q = pr.quantised_planes(oracle, case, self.payload)
        self.planes, self.q = (y, u, v), q.astype(np.int32)
        self.in_domain = tr.in_domain(self.planes, self.q)


def reference(oracle, case, data, s_out, prefix, scalar):
    """what the composition makes of arbitrary slot bytes: ("refused", code, in the encoder's domain) or ("ok", bytes, q', in
    the encoder's domain).  The domain is that of the values the reader found (every |c| <= 65534, every index <= 115); a
    payload the reader itself refuses counts as inside it: its code is the call's."""
    try:
        pic = Unpacked(oracle, case, data)
    except OracleError as e:
        return ("refused", e.code, True)
    try:
        out = Out(oracle, pic, s_out, prefix, scalar)
    except OracleError as e:
        return ("refused", e.code, pic.in_domain)
    return ("ok", out.payload, out.q, pic.in_domain)


def changed(case):
    """the output's (prefix, scalar) of the rows that change both"""
    return case.prefix + 1, case.scalar * 2


def budget_mixed(case, pics, scalar):
    """slices * (the median over picture 2's slices of need_s + 4)"""
    need, _ = slice_need(case, pics[2].planes, scalar)
    return case.ys * case.xs * (int(np.median(need)) + 4)


def budget_roomy(oracle, case, pics, scalar):
    """the smallest multiple of the slice count at which every budget of the table holds every slice of all three pictures"""
    ns = case.ys * case.xs
    top = max(int(slice_need(case, p.planes, scalar)[0].max()) for p in pics) + 4
    s = ns * top
    while oracle.slice_bytes(case.ys, case.xs, s, scalar).min() < top:
        s += ns
    return s


def budget_tight(case, pics, scalar):
    return budget_mixed(case, pics, scalar) // 3


def budgets(oracle, name, scalar=None):
    """{"mixed", "roomy", "tight"} -> compressed_bytes for a row of transcode_ref.MATRIX at the output scalar (its own by default)"""
    case, pics = tr.batch(oracle, name)
    scalar = case.scalar if scalar is None else scalar
    return {"mixed": budget_mixed(case, pics, scalar), "roomy": budget_roomy(oracle, case, pics, scalar),
            "tight": budget_tight(case, pics, scalar)}
