"""The CPU definition of a reduced picture (vc2hip_decode_reduced_batch_dev), composed of the
oracle's own functions, and the helpers the reduced-picture tests share.

For a picture coded with wavelet K at depth d and a drop count k, 1 <= k <= d - 1, per component:
  1. slice decode and dequantise as the full decoder does: the padded coefficient plane P in the reference's in-place order;
  2. P[::2**k, ::2**k] is a depth d - k transform of a plane 2**k times smaller each way: the ordinary inverse transform
     of K at depth d - k over it, cropped to (h >> k) x (w >> k);
  3. x = (x + (1 << (n - 1))) >> n with n = k * LOWPASS_GAIN_BITS[K]: the forward transform shifts its input left once per
     level, so step 2's result carries the low-pass gain of the k levels that were not inverted;
  4. clip, offset, justify, big-endian words: the full decoder's emit.
Daub97 has no entry: its low-pass gain per level (about 3.03) is no power of two."""
import numpy as np

from vc2lib import CF, KERNELS, MODES, make_params

LOWPASS_GAIN_BITS = {"DD97": 1, "LeGall": 1, "DD137": 1, "Haar0": 0, "Haar1": 1, "Fidelity": 2}


def norm_bits(kernel, k):
    return k * LOWPASS_GAIN_BITS[kernel]


def normalise(x, n):
    x = np.asarray(x, np.int64)
    return (x if n == 0 else (x + (1 << (n - 1))) >> n).astype(np.int32)


def chroma_dims(h, w, cf):
    return (h // 2 if cf == "420" else h), (w if cf == "444" else w // 2)


class Case:
    """one coded picture geometry: the arguments of make_params plus what the decoder derives from them"""

    def __init__(self, oracle, w, h, cf, bits, kernel, depth, u, a, mode="HQ_ConstQ", q=0, s=0, scalar=1, prefix=0, word_bytes=2):
        self.w, self.h, self.cf, self.bits, self.kernel, self.depth, self.u, self.a = w, h, cf, bits, kernel, depth, u, a
        self.mode, self.q, self.s, self.scalar, self.prefix, self.word_bytes = mode, q, s, scalar, prefix, word_bytes
        ch, cw = chroma_dims(h, w, cf)
        self.ys = oracle.lib.vc2o_slice_size_is_valid(depth, h, ch, u)
        self.xs = oracle.lib.vc2o_slice_size_is_valid(depth, w, cw, a)
        assert self.ys and self.xs, "slice sizes do not fit the picture"
        # the decoder's planes: padded luma, chroma derived from it (DecodeStream.cpp:483-498)
        self.ph, self.pw = oracle.padded_size(h, depth), oracle.padded_size(w, depth)
        self.cph, self.cpw = chroma_dims(self.ph, self.pw, cf)
        self.ch, self.cw = ch, cw

    def params(self, **over):
        kw = dict(mode=self.mode, q=self.q, s=self.s, scalar=self.scalar, prefix=self.prefix, word_bytes=self.word_bytes)
        kw.update(over)
        return make_params(self.w, self.h, self.cf, self.bits, self.kernel, self.depth, self.u, self.a, **kw)

    def fmt_cp(self, hip_lib):
        import vc2hip_py
        fmt = vc2hip_py.picture_format(self.w, self.h, self.cf, self.bits, self.word_bytes)
        cp = vc2hip_py.coding_params(hip_lib, fmt, self.kernel, self.depth, self.u, self.a, mode=self.mode, q=self.q, s=self.s,
                                     prefix=self.prefix, scalar=self.scalar)
        assert (cp.y_slices, cp.x_slices) == (self.ys, self.xs)
        return fmt, cp

    def raw_bytes(self, k=0):
        return ((self.w >> k) * (self.h >> k) + 2 * (self.cw >> k) * (self.ch >> k)) * self.word_bytes

    def drops(self):
        """the drop counts the call accepts for this picture"""
        return [k for k in range(1, self.depth) if not (self.w | self.h | self.cw | self.ch) & ((1 << k) - 1)]


_LIB = []


def _hip_lib():
    """libvc2hip.so for its host-only helpers (slice counts, the picture header's bytes): no GPU is touched"""
    if not _LIB:
        import vc2hip_py
        _LIB.append(vc2hip_py.load_library())
    return _LIB[0]


def _major(stream):
    """major_version: the first exp-Golomb field of the sequence header that opens the stream"""
    pos, v = 8 * 13, 1
    while True:
        b = stream[pos >> 3] >> (7 - (pos & 7)) & 1
        pos += 1
        if b:
            return v - 1
        v = (v << 1) | (stream[pos >> 3] >> (7 - (pos & 7)) & 1)
        pos += 1


def oracle_payloads(oracle, case, raw, n=1):
    """the slice payloads of n pictures as the oracle's encoder writes them: what follows the picture header in every
    picture data unit of its stream (the header's bytes are checked against vc2hip_picture_header's, not skipped blindly)"""
    import vc2hip_py
    stream = oracle.encode_stream(case.params(), raw, n)
    _, cp = case.fmt_cp(_hip_lib())
    major, pos, out = _major(stream), 0, []
    while pos < len(stream):
        assert stream[pos:pos + 4] == b"BBCD"
        code, nxt = stream[pos + 4], int.from_bytes(stream[pos + 5:pos + 9], "big")
        size = nxt if nxt else 13
        if code in (0xE8, 0xC8):
            body = stream[pos + 13:pos + size]
            hdr = vc2hip_py.picture_header(_hip_lib(), cp, major, len(out))
            assert body.startswith(hdr), "picture header differs from vc2hip_picture_header"
            out.append(body[len(hdr):])
        pos += size
    assert len(out) == n
    return out


def quantised_planes(oracle, case, payload):
    """(y, u, v, qidx): the quantised coefficient planes of a payload, in-place order, and the slices' quantiser indices"""
    data = np.frombuffer(payload, np.uint8)
    if case.mode == "LD":
        sb = oracle.slice_bytes(case.ys, case.xs, case.s, 1)
        y, u, v, q, _ = oracle.ld_unpack(data, (case.ph, case.pw), (case.cph, case.cpw), case.depth, sb)
    else:
        y, u, v, q, _ = oracle.hq_unpack(data, (case.ph, case.pw), (case.cph, case.cpw), case.depth, case.ys, case.xs,
                                         case.prefix, case.scalar)
    return y, u, v, q


def pack_planes(oracle, case, y, u, v, qidx):
    """quantised planes -> payload, with the given indices (HQ: variable slice sizes; LD: the picture's slice sizes)"""
    if case.mode == "LD":
        return oracle.ld_pack(y, u, v, case.depth, qidx, oracle.slice_bytes(case.ys, case.xs, case.s, 1)).tobytes()
    assert case.mode == "HQ_ConstQ"
    return oracle.hq_pack(y, u, v, case.depth, qidx, case.prefix, case.scalar).tobytes()


def dequantised_planes(oracle, case, payload):
    y, u, v, q = quantised_planes(oracle, case, payload)
    qm = oracle.quant_matrix(KERNELS[case.kernel], case.depth)
    dq = oracle.dequantise_ld if case.mode == "LD" else oracle.dequantise_np
    return [dq(p, case.depth, q, qm) for p in (y, u, v)]


def reduced_component(oracle, plane, kernel, depth, k, shape):
    """steps 2 and 3 for one dequantised plane; shape: the component's unpadded (h, w)"""
    sub = np.ascontiguousarray(plane[::1 << k, ::1 << k])
    x = oracle.dwt_inverse(sub, KERNELS[kernel], depth - k, (shape[0] >> k, shape[1] >> k))
    return normalise(x, norm_bits(kernel, k))


def reduced_picture(oracle, case, payload, k):
    """the bytes vc2hip_decode_reduced_batch_dev writes for one picture"""
    assert 1 <= k <= case.depth - 1 and case.kernel in LOWPASS_GAIN_BITS
    shapes = [(case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)]
    out = []
    for plane, shape in zip(dequantised_planes(oracle, case, payload), shapes):
        assert shape[0] % (1 << k) == 0 and shape[1] % (1 << k) == 0
        out.append(oracle.clip_emit(reduced_component(oracle, plane, case.kernel, case.depth, k, shape), case.word_bytes, case.bits).tobytes())
    return b"".join(out)


def full_picture(oracle, case, payload):
    """the full decoder's bytes by the same composition (k = 0): ties the helpers above to oracle.decode_stream"""
    shapes = [(case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)]
    out = []
    for plane, shape in zip(dequantised_planes(oracle, case, payload), shapes):
        x = oracle.dwt_inverse(plane, KERNELS[case.kernel], case.depth, shape)
        out.append(oracle.clip_emit(x, case.word_bytes, case.bits).tobytes())
    return b"".join(out)


__all__ = ["Case", "CF", "MODES", "LOWPASS_GAIN_BITS", "norm_bits", "normalise", "oracle_payloads", "quantised_planes", "pack_planes",
           "dequantised_planes", "reduced_component", "reduced_picture", "full_picture", "chroma_dims"]
