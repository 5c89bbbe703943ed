"""The CPU definitions behind vc2hip_set_quant_matrix (include/vc2hip.h): every covered call composed
of the oracle's primitives with an explicit quantisation matrix qm, and the picture header with a matrix of its own.

  encode        recon_ref.transform_planes, then the indices (q everywhere / cbr_qindices / ld_qindices with qm), quantise_np /
                quantise_ld with qm, hq_pack / ld_pack
  capped        the smallest index from the floor up to 115 at which the HQ_ConstQ payload is written and fits, by looking at
                every index; 115 if there is none
  decode        the slice reader, dequantise_np / dequantise_ld with qm, the inverse transform (proxy_ref's reduced form for a
                drop count), clip and emit
  transcodes    transcode_ref.Coded and transcode_cbr_ref.Out with qm in place of the default matrix (Coded below restates
                the constructor's few lines; Out reads the matrix from the picture it is given)
  streams       picture data units and fragmented pictures whose transform parameters carry the matrix (frag_ref's cut and
                slice walk, its parameter bytes restated with the flag and the entries)
With the default matrix every composition is the existing default-matrix one (tests/test_qmatrix_ref.py)."""
from math import gcd

import numpy as np

import frag_ref
import proxy_ref as pr
import recon_ref as rr
import transcode_ref as tr
from vc2lib import KERNELS, OracleError

Q_TOP = 115
LD = 2   # vc2hip_coding_params.mode
MATRICES = ("flat", "default", "steep", "ragged", "edge")


# The rows of the GPU tests: A, E and C as transcode_ref.MATRIX has them; G at index 3 (transcode_ref codes it at 0, where
# max(q - m, 0) is 0 under every matrix and no matrix arithmetic runs); L, one LD picture; E2 and L2, rows E and L at budgets
# their searches can meet under `edge`, whose never-quantised bands put the budgets of E and L out of reach.
ROWS = {"A": ("A",), "E": ("E",), "C": ("C",),
        "G": (128, 32, "420", 8, "Haar0", 1, 2, 2, dict(q=3, scalar=1, word_bytes=1)),
        "L": (512, 64, "422", 10, "LeGall", 3, 1, 2, dict(mode="LD", s=12000)),
        "E2": (1024, 64, "422", 10, "LeGall", 3, 1, 2, dict(mode="HQ_CBR", s=200000, scalar=2)),
        "L2": (512, 64, "422", 10, "LeGall", 3, 1, 2, dict(mode="LD", s=120000))}
# the (row, matrix) pairs whose composition is MEANT to refuse, all three pictures with EQINDEX: the search climbs past 119 on
# the bands `edge` leaves at entry 0 without ever fitting the bands it never quantises (tests/test_qmatrix_ref.py pins the set)
REFUSES = {("E", "edge"): -2, ("L", "edge"): -2}


def case_of(oracle, name):
    row = ROWS[name]
    if len(row) == 1:
        return tr.matrix_case(oracle, row[0])
    w, h, cf, bits, kernel, depth, u, a, kw = row
    return pr.Case(oracle, w, h, cf, bits, kernel, depth, u, a, **kw)


def matrix(oracle, name, kernel, depth):
    """the named matrix for a wavelet and depth, 3 * depth + 1 entries (LL, then HL, LH, HH per level from the coarsest):
    flat     all zeros
    default  the wavelet's own, to be set explicitly
    steep    rising by 5 a band: with an index of 8 the coarse bands have m <= q, the fine ones m > q (the clamp at 0)
    ragged   non-monotone, LL larger than the finest band
    edge     119, 120 and 255 beside small entries"""
    n = 3 * depth + 1
    if name == "flat":
        return np.zeros(n, np.int32)
    if name == "default":
        return oracle.quant_matrix(KERNELS[kernel], depth).astype(np.int32)
    if name == "steep":
        return (5 * np.arange(n)).astype(np.int32)
    if name == "ragged":
        m = np.array(([9, 2, 7, 1, 6, 0, 5, 3, 8, 2, 4, 0, 7, 1, 6, 3, 5, 0, 8, 2, 4, 1] * 2)[:n], np.int32)
        m[-1] = 1
        return m
    if name == "edge":
        return np.array(([0, 255, 119, 120, 1, 2, 4, 119, 3, 255, 0, 120, 2, 1] * 2)[:n], np.int32)
    raise KeyError(name)


# ---- encode ------------------------------------------------------------------------------------------------------------
def indices(oracle, case, planes, qm):
    """(indices ys x xs, the per-slice budgets or None) as the mode finds them with qm"""
    if case.mode == "LD":
        sb = oracle.slice_bytes(case.ys, case.xs, case.s, 1)
        return oracle.ld_qindices(*planes, case.depth, qm, sb), sb
    if case.mode == "HQ_CBR":
        sb = oracle.slice_bytes(case.ys, case.xs, case.s, case.scalar)
        return oracle.cbr_qindices(*planes, case.depth, qm, sb, case.scalar), sb
    return np.full((case.ys, case.xs), case.q, np.int32), None


def pack(oracle, case, planes, q, sb, qm):
    """transform planes, indices -> payload bytes (HQ_ConstQ, HQ_CBR with budgets sb, LD)"""
    if case.mode == "LD":
        y, u, v = (oracle.quantise_ld(p, case.depth, q, qm) for p in planes)
        return oracle.ld_pack(y, u, v, case.depth, q, sb).tobytes()
    y, u, v = (oracle.quantise_np(p, case.depth, q, qm) for p in planes)
    return oracle.hq_pack(y, u, v, case.depth, q, case.prefix, case.scalar, cbr=sb).tobytes()


def encode(oracle, case, raw, qm):
    """one picture: (payload, indices ys x xs)"""
    planes = rr.transform_planes(oracle, case, raw)
    q, sb = indices(oracle, case, planes, qm)
    return pack(oracle, case, planes, q, sb, qm), q.astype(np.int32)


def encode_capped(oracle, case, raw, qm, floor, cap):
    """HQ_CAPPED: (payload, the picture's index) -- every index from the floor is looked at"""
    planes = rr.transform_planes(oracle, case, raw)
    assert case.mode == "HQ_ConstQ"
    last = None
    for t in range(floor, Q_TOP + 1):
        q = np.full((case.ys, case.xs), t, np.int32)
        try:
            last = pack(oracle, case, planes, q, None, qm)
        except OracleError:
            last = None
            continue
        if len(last) <= cap:
            return last, t
    assert last is not None, "the composition refuses the picture at 115"
    return last, Q_TOP


# ---- decode ------------------------------------------------------------------------------------------------------------
def dequantised_planes(oracle, case, payload, qm):
    y, u, v, q = pr.quantised_planes(oracle, case, payload)
    dq = oracle.dequantise_ld if case.mode == "LD" else oracle.dequantise_np
    return [dq(p, case.depth, q, qm) for p in (y, u, v)], q


def decode(oracle, case, payload, qm, k=0):
    """the decoder's bytes for one payload; k: the drop count of the reduced decoder"""
    shapes = [(case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)]
    out = []
    for plane, shape in zip(dequantised_planes(oracle, case, payload, qm)[0], shapes):
        if k:
            x = pr.reduced_component(oracle, plane, case.kernel, case.depth, k, shape)
        else:
            x = oracle.dwt_inverse(plane, KERNELS[case.kernel], case.depth, shape)
        out.append(oracle.clip_emit(x, case.word_bytes, case.bits).tobytes())
    return b"".join(out)


def recon(oracle, case, raw, payload, qm):
    """(the decoder's picture, [Y, U, V] squared errors) of an encode's payload"""
    pic = decode(oracle, case, payload, qm)
    return pic, rr.squared_errors(case, raw, pic)


def split_fields(case, frame):
    """an interleaved frame of case's format -> (first field, second field), top field first"""
    shapes = [(case.h, case.w * case.word_bytes)] + [(case.ch, case.cw * case.word_bytes)] * 2
    planes, at = [], 0
    buf = np.frombuffer(frame, np.uint8)
    for r, rw in shapes:
        planes.append(buf[at:at + r * rw].reshape(r, rw))
        at += r * rw
    return tuple(b"".join(p[first::2].tobytes() for p in planes) for first in (0, 1))


def merge_fields(case, first, second):
    """the inverse of split_fields: case is the FRAME's"""
    shapes = [(case.h, case.w * case.word_bytes)] + [(case.ch, case.cw * case.word_bytes)] * 2
    out, at = [], 0
    a, b = np.frombuffer(first, np.uint8), np.frombuffer(second, np.uint8)
    for r, rw in shapes:
        nb = (r // 2) * rw
        frame = np.empty((r, rw), np.uint8)
        frame[0::2], frame[1::2] = a[at:at + nb].reshape(r // 2, rw), b[at:at + nb].reshape(r // 2, rw)
        out.append(frame.tobytes())
        at += nb
    return b"".join(out)


# ---- the transcodes ------------------------------------------------------------------------------------------------------
class Coded(tr.Coded):
    """transcode_ref.Coded with qm in place of the default matrix (its constructor, restated)"""

    def __init__(self, oracle, case, payload, qm):
        self.oracle, self.case, self.payload = oracle, case, bytes(payload)
        self.qm = np.ascontiguousarray(qm, np.int32)
        y, u, v, q = pr.quantised_planes(oracle, case, self.payload)
        self.planes, self.q = (y, u, v), q.astype(np.int32)
        self.deq = [oracle.dequantise_np(p, case.depth, self.q, self.qm) for p in self.planes]
        self.in_domain = tr.in_domain(self.planes, self.q)
        self._out = {}


# ---- the picture header with a matrix ----------------------------------------------------------------------------------------
def _ab(cp):
    if cp.mode != LD:
        return cp.prefix, cp.scalar
    ns = cp.y_slices * cp.x_slices
    g = gcd(cp.compressed_bytes, ns)
    return cp.compressed_bytes // g, ns // g


def transform_parameters(cp, major, qm=None, asym=(0, 0)):
    """wavelet, depth, (major >= 3) the two asymmetric-transform flags, slice counts, prefix and scalar or LD's fraction, the
    custom_quant_matrix flag, its entries as unsigned exp-Golomb codes, zero bits to the byte boundary.  The entries go as they
    are (256 included: what the readers must refuse)"""
    w = frag_ref.Bits()
    w.uvlc(cp.kernel)
    w.uvlc(cp.depth)
    if major >= 3:
        w.bit(asym[0])
        if asym[0]:
            w.uvlc(cp.kernel + 1)
        w.bit(asym[1])
        if asym[1]:
            w.uvlc(1)
    w.uvlc(cp.x_slices)
    w.uvlc(cp.y_slices)
    a, b = _ab(cp)
    w.uvlc(a)
    w.uvlc(b)
    w.bit(0 if qm is None else 1)
    for m in ([] if qm is None else qm):
        w.uvlc(int(m))
    return w.bytes()


def picture_header(cp, major, number, qm=None, asym=(0, 0)):
    return (number & 0xFFFFFFFF).to_bytes(4, "big") + transform_parameters(cp, major, qm, asym)


class _Reader:
    def __init__(self, data, pos):
        self.d, self.pos = data, pos

    def bit(self):
        if self.pos >> 3 >= len(self.d):
            raise ValueError("past the end")
        b = self.d[self.pos >> 3] >> (7 - (self.pos & 7)) & 1
        self.pos += 1
        return b

    def uvlc(self):
        v = 1
        while not self.bit():
            v = (v << 1) | self.bit()
        return v - 1


def parse_picture_header(data, major, ld):
    """the model's reading: dict(number, kernel, depth, xs, ys, a, b, matrix or None, used bytes); ValueError for a truncated
    header, an asymmetric transform, an entry above 255"""
    if len(data) < 4:
        raise ValueError("past the end")
    r = _Reader(data, 32)
    kernel, depth = r.uvlc(), r.uvlc()
    if major >= 3:
        if r.bit() and r.uvlc() != kernel:
            raise ValueError("asymmetric")
        if r.bit() and r.uvlc() != 0:
            raise ValueError("asymmetric")
    xs, ys, a, b = r.uvlc(), r.uvlc(), r.uvlc(), r.uvlc()
    qm = None
    if r.bit():
        qm = [r.uvlc() for _ in range(3 * depth + 1)]
        if max(qm) > 255:
            raise ValueError("entry above 255")
    return dict(number=int.from_bytes(data[:4], "big"), kernel=kernel, depth=depth, xs=xs, ys=ys, a=a, b=b, matrix=qm,
                used=(r.pos + 7) // 8)


# ---- streams ---------------------------------------------------------------------------------------------------------------
def _chain(units, prev):
    out, offsets = bytearray(), []
    for code, body in units:
        nxt = 0 if code == 0x10 else 13 + len(body)
        offsets.append(len(out))
        out += b"BBCD" + bytes([code]) + nxt.to_bytes(4, "big") + prev.to_bytes(4, "big") + body
        prev = 13 + len(body)
    return bytes(out), offsets


def picture_stream(payloads, cp, major, qm=None, first_picture_number=0, prev_parse_offset=0, end_of_sequence=False):
    """what vc2hip_stream_write_dev writes: one picture data unit per payload, then the end of sequence if asked for"""
    code = 0xC8 if cp.mode == LD else 0xE8
    units = [(code, picture_header(cp, major, first_picture_number + k, qm) + pay) for k, pay in enumerate(payloads)]
    if end_of_sequence:
        units.append((0x10, b""))
    return _chain(units, prev_parse_offset)[0]


def fragment_stream(payloads, cp, fragment_length, qm=None, first_picture_number=0, prev_parse_offset=0, end_of_sequence=False,
                    ld_slice_bytes=None):
    """frag_ref.fragment_stream with the matrix in every picture's parameters fragment (major version 3)"""
    code = 0xCC if cp.mode == LD else 0xEC
    tp = transform_parameters(cp, 3, qm)
    units = []
    for k, pay in enumerate(payloads):
        number = ((first_picture_number + k) & 0xFFFFFFFF).to_bytes(4, "big")
        units.append((code, number + len(tp).to_bytes(2, "big") + bytes(2) + tp))
        if cp.mode == LD:
            sizes = [int(s) for s in ld_slice_bytes]
            assert sum(sizes) == len(pay)
        else:
            sizes = frag_ref.slice_sizes_hq(pay, cp.y_slices * cp.x_slices, cp.prefix, cp.scalar)
        starts = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        for first, count, size in frag_ref.cut(sizes, fragment_length):
            units.append((code, number + size.to_bytes(2, "big") + count.to_bytes(2, "big") + (first % cp.x_slices).to_bytes(2, "big") +
                          (first // cp.x_slices).to_bytes(2, "big") + pay[starts[first]:starts[first] + size]))
    if end_of_sequence:
        units.append((0x10, b""))
    return _chain(units, prev_parse_offset)[0]


def sequence_header_stub(major):
    """the shortest unit that tells the stream reader the major version: a sequence header whose first field is it (the reader
    reads no other field of a sequence header)"""
    w = frag_ref.Bits()
    w.uvlc(major)
    return w.bytes()
