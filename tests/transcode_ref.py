"""The CPU definition of vc2hip_transcode_batch_dev (include/vc2hip.h), composed of the oracle's own
functions, and the inputs the transcode tests share.

For one picture, from the bytes the call may look at and a target index t:
  1. (y, u, v, q_s) = oracle.hq_unpack: the quantised coefficients and every slice's own index (proxy_ref.quantised_planes);
  2. slice s ends at q'_s = max(q_s, t).  A slice with q'_s == q_s keeps its coefficient values; every other coefficient
     becomes quantise_np(dequantise_np(c, q_s), q'_s) with the default matrix.  A slice is a rectangular block of the
     in-place plane, so the kept-slice mask is np.kron(q_s >= t, ones(ph // ys, pw // xs));
  3. T(t) = oracle.hq_pack(y', u', v', depth, q', prefix, scalar): the VBR form.
The composition refuses as its parts refuse: hq_unpack where the reader runs off the end (ESTREAM), dequantise_np for an
index whose adjusted value passes 119 (EQINDEX), hq_pack for a length byte beyond 255 (ESCALAR).
Capped: q_i is the smallest t in floor .. 115 at which T(t) is not refused and len(T(t)) <= cap, found by looking at every t;
115 if there is none.

The input payloads come from oracle primitives only (recon_ref.transform_planes, quantise_np, cbr_qindices, hq_pack), so no
test here depends on the library's own encoder."""
import numpy as np

import cap_ref as cr
import proxy_ref as pr
import recon_ref as rr
from vc2lib import KERNELS, OracleError

Q_TOP = 115
NOT_CODABLE = None
ESTREAM, EQINDEX, ESCALAR, ECODE32 = -10, -2, -3, -11

# row: (w, h, cf, bits, word_bytes, wavelet, depth, u, a, how the input was coded)
MATRIX = {
    "A": (512, 64, "422", 10, 2, "DD97", 3, 1, 2, dict(q=8, scalar=2)),
    "B": (512, 64, "420", 8, 1, "DD137", 2, 2, 4, dict(q=0, scalar=4)),
    "C": (256, 64, "444", 10, 2, "Haar0", 4, 1, 1, dict(q=2, scalar=6, prefix=1)),
    "D": (1004, 60, "422", 10, 2, "DD97", 3, 1, 2, dict(q=4, scalar=3, prefix=2)),                  # padded to 1008 x 64
    "E": (1024, 64, "422", 10, 2, "LeGall", 3, 1, 2, dict(mode="HQ_CBR", s=60000, scalar=2)),       # indices differ per slice, padded slices
    "F": (512, 128, "444", 10, 2, "DD97", 3, 16, 64, dict(q=20, scalar=400)),                       # one slice per picture
    "G": (128, 32, "420", 8, 1, "Haar0", 1, 2, 2, dict(q=0, scalar=1)),                             # chroma components of 4 coefficients, luma of 16
    "H": (1024, 64, "422", 16, 2, "Daub97", 3, 1, 2, dict(q=30, scalar=8)),                         # values to ~10 000: long codes
    "I": (512, 64, "422", 10, 2, "LeGall", 3, 1, 2, dict(q=6, scalar=2, checker=(6, 40))),          # kept and requantised slices side by side
}
ROWS = tuple(MATRIX)


def matrix_case(oracle, name):
    w, h, cf, bits, wb, kernel, depth, u, a, kw = MATRIX[name]
    kw = {k: v for k, v in kw.items() if k != "checker"}
    return pr.Case(oracle, w, h, cf, bits, kernel, depth, u, a, word_bytes=wb, **kw)


def input_indices(oracle, name, case, planes, qm):
    """the indices the row's input is coded with"""
    kw = MATRIX[name][9]
    if case.mode == "HQ_CBR":
        sb = oracle.slice_bytes(case.ys, case.xs, case.s, case.scalar)
        return oracle.cbr_qindices(*planes, case.depth, qm, sb, case.scalar), sb
    if "checker" in kw:
        yy, xx = np.mgrid[0:case.ys, 0:case.xs]
        lo, hi = kw["checker"]
        return np.where((yy + xx) % 2 == 0, lo, hi).astype(np.int32), None
    return np.full((case.ys, case.xs), case.q, np.int32), None


def input_payload(oracle, name, case, raw):
    """one picture coded by the oracle's primitives as the row says; (payload bytes, indices)"""
    qm = oracle.quant_matrix(KERNELS[case.kernel], case.depth)
    planes = rr.transform_planes(oracle, case, raw)
    assert planes[1].shape == (case.cph, case.cpw), "the decoder derives other chroma planes than the encoder pads"
    qi, sb = input_indices(oracle, name, case, planes, qm)
    y, u, v = (oracle.quantise_np(p, case.depth, qi, qm) for p in planes)
    return oracle.hq_pack(y, u, v, case.depth, qi, case.prefix, case.scalar, cbr=sb).tobytes(), qi


def kept_mask(case, q_s, t, shape):
    return np.kron(q_s >= t, np.ones((shape[0] // case.ys, shape[1] // case.xs), bool)).astype(bool)


def in_domain(planes, q_s):
    """the encoder's domain: every coefficient codable in 32 bits, every index at most 115"""
    return bool((q_s <= Q_TOP).all() and all((np.abs(p.astype(np.int64)) <= 65534).all() for p in planes))


class Coded:
    """one coded picture: its unpacked planes, and T(t) by the definition.  Construction raises OracleError where the
    composition refuses whatever the target (the slice reader, the dequantiser)."""

    def __init__(self, oracle, case, payload):
        self.oracle, self.case, self.payload = oracle, case, bytes(payload)
        self.qm = oracle.quant_matrix(KERNELS[case.kernel], case.depth)
        y, u, v, q = pr.quantised_planes(oracle, case, self.payload)
        self.planes, self.q = (y, u, v), q.astype(np.int32)
        self.deq = [oracle.dequantise_np(p, case.depth, self.q, self.qm) for p in self.planes]
        self.in_domain = in_domain(self.planes, self.q)
        self._out = {}

    def requantised(self, t, blind=False):
        """(y', u', v', q'); blind: every slice through the arithmetic, the kept ones too"""
        q2 = np.maximum(self.q, t).astype(np.int32)
        out = []
        for c, d in zip(self.planes, self.deq):
            r = self.oracle.quantise_np(d, self.case.depth, q2, self.qm)
            out.append(r if blind else np.where(kept_mask(self.case, self.q, t, c.shape), c, r).astype(np.int32))
        return out[0], out[1], out[2], q2

    def transcode(self, t):
        """T(t) as bytes, or NOT_CODABLE where the slice writer refuses"""
        if t not in self._out:
            y, u, v, q2 = self.requantised(t)
            try:
                self._out[t] = self.oracle.hq_pack(y, u, v, self.case.depth, q2, self.case.prefix, self.case.scalar).tobytes()
            except OracleError:
                self._out[t] = NOT_CODABLE
        return self._out[t]

    def indices(self, t):
        return np.maximum(self.q, t).astype(np.int32)

    # ---- the capped form
    def table(self):
        if not hasattr(self, "_table"):
            self._table = []
            for t in range(Q_TOP + 1):
                pay = self.transcode(t)
                self._table.append(NOT_CODABLE if pay is NOT_CODABLE else len(pay))
        return self._table

    def fits(self, t, cap):
        L = self.table()[t]
        return L is not NOT_CODABLE and L <= cap

    def chosen(self, floor, cap):
        """the definition: every index is looked at"""
        fitting = [t for t in range(floor, Q_TOP + 1) if self.fits(t, cap)]
        return min(fitting) if fitting else Q_TOP

    def bisected(self, floor, cap):
        """what a search that trusts the monotonicity finds"""
        if self.fits(floor, cap):
            return floor
        lo, hi = floor, Q_TOP + 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if self.fits(mid, cap) else (mid, hi)
        return min(hi, Q_TOP)


def damaged_reference(oracle, case, data, t):
    """what the composition makes of arbitrary slot bytes at target t:
    ("refused", code) or ("ok", T(t), the output indices, whether the decoded picture lies in the encoder's domain)"""
    try:
        pic = Coded(oracle, case, data)
        y, u, v, q2 = pic.requantised(t)
        out = oracle.hq_pack(y, u, v, case.depth, q2, case.prefix, case.scalar).tobytes()
    except OracleError as e:
        return ("refused", e.code)
    return ("ok", out, q2, pic.in_domain)


def empty_bytes(case):
    return case.ys * case.xs * (case.prefix + 4)


_BATCHES = {}


def batch(oracle, name):
    """(case, [Coded] * 3) of a row: smooth, noise, half and half (cap_ref.pictures); computed once per session"""
    if name not in _BATCHES:
        case = matrix_case(oracle, name)
        _BATCHES[name] = (case, [Coded(oracle, case, input_payload(oracle, name, case, raw)[0]) for raw in cr.pictures(case)])
    return _BATCHES[name]


def floor_of(pics):
    """the smallest slice index of a batch's inputs: the floor the capped tests ask for"""
    return int(min(p.q.min() for p in pics))


def mid_target(pic0, floor):
    """an index between the floor and the empty picture at which picture 0's length drops"""
    L = pic0.table()
    empty = empty_bytes(pic0.case)
    drops = [t for t in range(floor + 1, Q_TOP + 1) if L[t] < L[t - 1] and L[t] > empty]
    assert drops, "picture 0 has no index above the floor at which its length drops"
    return drops[len(drops) // 2]


def caps(pic0, floor):
    """cap_ref.caps on picture 0's own table of transcoded lengths: name -> (cap, picture 0's expected index)"""
    L = pic0.table()
    assert L[floor] is not NOT_CODABLE
    empty = empty_bytes(pic0.case)
    mid = mid_target(pic0, floor)
    nxt = next(t for t in range(mid + 1, Q_TOP + 1) if L[t] < L[mid])
    first_empty = next((t for t in range(floor, Q_TOP + 1) if L[t] == empty), Q_TOP)
    return {"floor": (L[floor], floor), "mid": (L[mid], mid), "mid-1": (L[mid] - 1, nxt), "empty": (empty, first_empty),
            "none": (empty - 1, Q_TOP)}


def fixed_targets(pics):
    """the five targets of the fixed form: 0, the input's smallest index, that + 1, a mid index, 115"""
    floor = floor_of(pics)
    return sorted({0, floor, floor + 1, mid_target(pics[0], floor), Q_TOP})
