"""The CPU definition of VC2HIP_HQ_CAPPED (include/vc2hip.h), composed of what tests/recon_ref.py and
tests/proxy_ref.py have.

For one picture, L(q) for q in 0 .. 115 is the length of the oracle's HQ payload with the constant index q in every slice:
transform_planes -> oracle.quantise_np -> len(oracle.hq_pack(...)); an OracleError at q (a length byte beyond 255, a code
beyond 32 bits) means "q does not fit", whatever the cap.  The picture's index under (floor, cap) is the smallest q in
floor .. 115 with L(q) <= cap -- found by looking at every q, no monotonicity assumed -- or 115 if there is none, and the
expected payload is the oracle's at that index.  tests/test_cap_ref.py asserts on every row that L never grows with q, which
is what entitles the GPU path to bracket instead of looking everywhere."""
import numpy as np

import proxy_ref as pr
import recon_ref as rr
from vc2lib import KERNELS, OracleError

Q_TOP = 115
MODE = 3          # VC2HIP_HQ_CAPPED
NOT_CODABLE = None

# (w, h, cf, bits, word_bytes, wavelet, depth, u, a, dict(floor, scalar, prefix)); three pictures of unlike content per
# batch (pictures()), so that the indices differ inside one batch.  Each row's comment names the measuring kernel it takes
# on the default context (VC2HIP_FLAG_CAP_GENERAL and VC2HIP_FLAG_STORE32 send every row to the general one).  The fast
# form needs the 16-bit store, which the library keeps only where every transform level has at least one 128 x 32 tile
# in every component: 2048 x 256 at depth 4 and 1024 x 128 at depth 3 are the smallest 4:2:2 pictures that take it.
MATRIX = [
    (2048, 256, "422", 10, 2, "DD97", 4, 1, 2, dict(floor=16, scalar=2)),             # fast form: 32 x 16 slices, head 8 / 16
    (1024, 128, "422", 10, 2, "LeGall", 3, 2, 4, dict(floor=24, scalar=1)),           # fast form: 32 x 16 slices, no luma head; scalar 1: noise does not code near the floor
    (512, 64, "422", 10, 2, "DD97", 3, 1, 2, dict(floor=3, scalar=1)),                # general, LDS: 16 x 8 slices (too few runs for the fast form)
    (512, 64, "420", 8, 1, "DD137", 2, 2, 4, dict(floor=0, scalar=2)),                # general, LDS: 4:2:0, one-byte words
    (256, 64, "444", 10, 2, "Haar0", 4, 1, 1, dict(floor=2, scalar=6, prefix=1)),     # general, LDS: 4:4:4 (chroma as large as luma)
    (1004, 60, "422", 10, 2, "DD97", 3, 1, 2, dict(floor=4, scalar=3, prefix=2)),     # general, LDS: padded 1004 x 60 -> 1008 x 64
    (1024, 64, "422", 12, 2, "LeGall", 3, 1, 2, dict(floor=10, scalar=8, prefix=5)),  # general, LDS: prefix 5, scalar 8
    (1024, 128, "422", 16, 2, "LeGall", 3, 2, 4, dict(floor=16, scalar=8)),           # fast form + hand-back: 16-bit noise escapes the 16-bit store
    (512, 128, "444", 10, 2, "DD97", 3, 16, 64, dict(floor=20, scalar=400)),          # general, GLOBAL: one slice per picture, the whole-plane path
    (1024, 64, "422", 10, 2, "Daub97", 3, 1, 2, dict(floor=12, scalar=2)),            # general, LDS: Daub97 (int32 store)
]
FAST = (0, 1, 7)
ESCAPES = 7
WHOLE_PLANE = 8
IDS = ["-".join(str(x) for x in r[:9]) for r in MATRIX]


def matrix_case(oracle, row):
    w, h, cf, bits, wb, kernel, depth, u, a, kw = row
    return pr.Case(oracle, w, h, cf, bits, kernel, depth, u, a, word_bytes=wb, q=kw["floor"], scalar=kw["scalar"], prefix=kw.get("prefix", 0))


def _halves(case, left, right):
    """every row of every component: its left half from one picture, its right half from another"""
    out, at = [], 0
    for (h, w) in [(case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)]:
        nb = h * w * case.word_bytes
        a = np.frombuffer(left[at:at + nb], np.uint8).reshape(h, w * case.word_bytes).copy()
        b = np.frombuffer(right[at:at + nb], np.uint8).reshape(h, w * case.word_bytes)
        cut = (w // 2) * case.word_bytes
        a[:, cut:] = b[:, cut:]
        out.append(a.tobytes())
        at += nb
    return b"".join(out)


def pictures(case):
    """[smooth, noise, half smooth and half noise]"""
    from synth import noise_frame, synth
    seed = 70 + case.w + case.depth
    smooth = synth(case.w, case.h, case.cf, case.bits, seed, word_bytes=case.word_bytes)
    noise = noise_frame(case.w, case.h, case.cf, case.bits, seed + 1, word_bytes=case.word_bytes)
    other = noise_frame(case.w, case.h, case.cf, case.bits, seed + 2, word_bytes=case.word_bytes)
    return [smooth, noise, _halves(case, smooth, other)]


class Picture:
    """one picture's transform, its table L(0 .. 115) and its payloads, each computed once"""

    def __init__(self, oracle, case, raw):
        self.oracle, self.case, self.raw = oracle, case, raw
        self.planes = rr.transform_planes(oracle, case, raw)
        self.qm = oracle.quant_matrix(KERNELS[case.kernel], case.depth)
        self._pay = {}
        self.table = [self._len(q) for q in range(Q_TOP + 1)]

    def payload(self, q):
        """the oracle's HQ payload at the constant index q; NOT_CODABLE where its encoder refuses"""
        if q not in self._pay:
            c, qi = self.case, np.full((self.case.ys, self.case.xs), q, np.int32)
            try:
                y, u, v = (self.oracle.quantise_np(p, c.depth, qi, self.qm) for p in self.planes)
                self._pay[q] = self.oracle.hq_pack(y, u, v, c.depth, qi, c.prefix, c.scalar).tobytes()
            except OracleError:
                self._pay[q] = NOT_CODABLE
        return self._pay[q]

    def _len(self, q):
        pay = self.payload(q)
        if q != Q_TOP and q % 8:       # (the payloads stay for the indices a test is likely to ask for again)
            del self._pay[q]
        return NOT_CODABLE if pay is NOT_CODABLE else len(pay)

    def fits(self, q, cap):
        return self.table[q] is not NOT_CODABLE and self.table[q] <= cap

    def chosen(self, floor, cap):
        """the definition: every index is looked at"""
        fitting = [q for q in range(floor, Q_TOP + 1) if self.fits(q, cap)]
        return min(fitting) if fitting else Q_TOP

    def bisected(self, floor, cap):
        """what a search that trusts the monotonicity finds"""
        if self.fits(floor, cap):
            return floor
        lo, hi = floor, Q_TOP + 1      # lo does not fit; hi fits, or is past the top
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if self.fits(mid, cap) else (mid, hi)
        return min(hi, Q_TOP)


_BATCHES = {}


def batch(oracle, i):
    """(case, [Picture] * 3) of row i, computed once per session"""
    if i not in _BATCHES:
        case = matrix_case(oracle, MATRIX[i])
        _BATCHES[i] = (case, [Picture(oracle, case, raw) for raw in pictures(case)])
    return _BATCHES[i]


def chosen(case, picture, floor, cap):
    return picture.chosen(floor, cap)


def caps(case, pic0):
    """the five caps of DESIGN.md section 17, from picture 0's own lengths: name -> (cap, picture 0's expected index)"""
    floor, L = case.q, pic0.table
    assert L[floor] is not NOT_CODABLE, "the row's floor must code picture 0"
    empty = case.ys * case.xs * (case.prefix + 4)
    drops = [q for q in range(floor + 1, Q_TOP + 1) if L[q - 1] is not NOT_CODABLE and L[q] < L[q - 1] and L[q] > empty]
    assert drops, "picture 0 has no index between the floor and the empty picture at which its length drops"
    mid = drops[len(drops) // 2]
    nxt = next(q for q in range(mid + 1, Q_TOP + 1) if L[q] < L[mid])
    first_empty = next((q for q in range(floor, Q_TOP + 1) if L[q] == empty), Q_TOP)
    return {
        "floor": (L[floor], floor),
        "mid": (L[mid], mid),
        "mid-1": (L[mid] - 1, nxt),
        "empty": (empty, first_empty),
        "none": (empty - 1, Q_TOP),
    }
