"""The model of vc2hip_set_packed_format's contract (include/vc2hip.h), in numpy: where the samples of a batch of pictures
lie in v210 and in semi-planar buffers, and which bits are samples.

fmt is anything with the fields of vc2hip_picture_format, pf anything with those of vc2hip_packed_format (packing 1 = v210,
2 = semi-planar; little_endian, lsb_justified, pitch[2], plane_offset[2], picture_stride).  The ctypes structures of vc2hip_py
fit both.

    v210         groups of 6 pixels in four little-endian 32-bit words of three 10-bit fields at bits 0, 10, 20:
                 w0 = Cb0 | Y0 << 10 | Cr0 << 20, w1 = Y1 | Cb1 << 10 | Y2 << 20, w2 = Cr1 | Y3 << 10 | Cb2 << 20,
                 w3 = Y4 | Cr2 << 10 | Y5 << 20.  Read: bits 30 - 31 and the fields of a row's last group beyond the width are
                 ignored.  Written: they are zero, every group of a row is written whole, nothing else is touched.
    semi-planar  a Y plane as under a sample layout, and one plane of U, V word pairs.  Read: the bits of a word outside
                 the sample are ignored.  Written: they are zero; nothing outside the rows of the two planes is touched.

to_packed writes exactly what a decoder must write (with `fill` in every byte it must leave alone) and, given a generator,
puts random bits into every ignored position of an encoder's input.
"""
from types import SimpleNamespace

import numpy as np

import layout_ref

NONE, V210, SEMIPLANAR = 0, 1, 2
MAX_PITCH = layout_ref.MAX_PITCH
MAX_PLANE = layout_ref.MAX_PLANE


def v210_row_bytes(width):
    return (width + 5) // 6 * 16


def geometry(fmt, pf):
    """pf resolved for pictures of fmt: rows[k], row[k] (bytes), pitch[k], at[k] of plane 0 (the v210 rows / Y) and plane 1
    (UV, semi-planar only), extent, stride; None for what the calls refuse (no packed format included)"""
    if pf is None or pf.packing == NONE or pf.packing not in (V210, SEMIPLANAR):
        return None
    if pf.little_endian not in (0, 1) or pf.lsb_justified not in (0, 1):
        return None
    pitch_in, off_in, stride_in = list(pf.pitch), list(pf.plane_offset), int(pf.picture_stride)
    if any(x % 16 for x in pitch_in + off_in + [stride_in]):
        return None
    (h, w), (ch, cw), _ = layout_ref.planes(fmt)
    wb = fmt.word_bytes
    if pf.packing == V210:
        if pf.little_endian or pf.lsb_justified or pitch_in[1] or any(off_in):
            return None
        if fmt.chroma_format != 1 or fmt.bit_depth != 10 or fmt.chroma_bit_depth not in (0, 10) or wb != 2 or w % 2:
            return None
        rows, row = [h], [v210_row_bytes(w)]
    else:
        if wb not in (1, 2):
            return None
        rows, row = [h, ch], [w * wb, 2 * cw * wb]
    pitch, at, extent = [], [], 0
    for k in range(len(rows)):
        p = pitch_in[k] or row[k]
        if p < row[k] or p >= MAX_PITCH or rows[k] * p >= MAX_PLANE:
            return None
        pitch.append(p)
        at.append(off_in[k] if any(off_in) else (0 if k == 0 else at[0] + rows[0] * pitch[0]))
        extent = max(extent, at[k] + (rows[k] - 1) * p + row[k])
    stride = stride_in or extent
    if stride < extent:
        return None
    return SimpleNamespace(packing=pf.packing, le=int(pf.little_endian), lsb=int(pf.lsb_justified), rows=rows, row=row, pitch=pitch,
                           at=at, extent=extent, stride=stride)


def picture_bytes(fmt, pf):
    """the model of vc2hip_packed_picture_bytes (0: refused)"""
    g = geometry(fmt, pf)
    return g.extent if g else 0


def buffer_bytes(fmt, n, pf):
    """bytes of a buffer of n pictures: n picture strides (the last picture's tail is part of what must stay untouched)"""
    return n * geometry(fmt, pf).stride


def _put_rows(buf, o, pitch, b):
    for r in range(b.shape[0]):
        buf[o + r * pitch:o + r * pitch + b.shape[1]] = b[r]


def _get_rows(buf, o, pitch, rows, nbytes):
    return buf[o + np.arange(rows)[:, None] * pitch + np.arange(nbytes)[None, :]]


def _v210_words(y, u, v, garbage):
    """(rows, w), (rows, w / 2) x 2 sample arrays -> (rows, groups * 4) uint32 words"""
    rows, w = y.shape
    g = (w + 5) // 6

    def pad(s, per):
        out = np.zeros((rows, g * per), np.uint64)
        if garbage is not None:   # the fields beyond the row's width: ignored
            out[:] = garbage.integers(0, 1024, size=out.shape, dtype=np.uint64)
        out[:, :s.shape[1]] = s
        return out.reshape(rows, g, per)

    y, u, v = pad(y, 6), pad(u, 3), pad(v, 3)
    s10, s20 = np.uint64(10), np.uint64(20)
    words = np.stack([u[..., 0] | y[..., 0] << s10 | v[..., 0] << s20,
                      y[..., 1] | u[..., 1] << s10 | y[..., 2] << s20,
                      v[..., 1] | y[..., 3] << s10 | u[..., 2] << s20,
                      y[..., 4] | v[..., 2] << s10 | y[..., 5] << s20], axis=-1)
    if garbage is not None:       # bits 30 - 31: ignored
        words |= garbage.integers(0, 4, size=words.shape, dtype=np.uint64) << np.uint64(30)
    return words.reshape(rows, g * 4).astype("<u4")


def _sample_words(s, d, wb, lsb, garbage):
    shift = 0 if lsb else 8 * wb - d
    w = s << np.uint64(shift)
    if garbage is not None:
        keep = np.uint64(((1 << d) - 1) << shift)
        junk = garbage.integers(0, 1 << (8 * wb), size=s.shape, dtype=np.uint64)
        w |= junk & ~keep & np.uint64((1 << (8 * wb)) - 1)
    return w


def to_packed(file_bytes, fmt, n, pf, fill=0, garbage=None):
    """n file-format pictures under pf: a uint8 array of buffer_bytes(), `fill` in every byte a decoder must not write.
    Every ignored bit is zero (what the decoder writes) -- or, with garbage = a numpy Generator, random."""
    g = geometry(fmt, pf)
    assert g is not None, "a packed format the calls refuse"
    wb = fmt.word_bytes
    depths = layout_ref._depths(fmt)
    buf = np.full(n * g.stride, fill, np.uint8)
    for i, (y, u, v) in enumerate(layout_ref.file_samples(file_bytes, fmt, n)):
        base = i * g.stride
        if g.packing == V210:
            words = _v210_words(y, u, v, garbage)
            _put_rows(buf, base + g.at[0], g.pitch[0], words.view(np.uint8).reshape(words.shape[0], -1))
            continue
        yw = _sample_words(y, depths[0], wb, g.lsb, garbage)
        _put_rows(buf, base + g.at[0], g.pitch[0], layout_ref._bytes_from_words(yw, wb, g.le).reshape(y.shape[0], -1))
        uv = np.stack([_sample_words(u, depths[1], wb, g.lsb, garbage), _sample_words(v, depths[2], wb, g.lsb, garbage)], axis=-1)
        _put_rows(buf, base + g.at[1], g.pitch[1], layout_ref._bytes_from_words(uv, wb, g.le).reshape(u.shape[0], -1))
    return buf


def from_packed(buf, fmt, n, pf):
    """the inverse: the file-format bytes of n pictures read from a buffer under pf (ignored bits and fields dropped)"""
    g = geometry(fmt, pf)
    assert g is not None, "a packed format the calls refuse"
    wb = fmt.word_bytes
    depths = layout_ref._depths(fmt)
    buf = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    (h, w), (ch, cw), _ = layout_ref.planes(fmt)
    out = []
    for i in range(n):
        base = i * g.stride
        if g.packing == V210:
            b = np.ascontiguousarray(_get_rows(buf, base + g.at[0], g.pitch[0], h, g.row[0]))
            wd = b.view("<u4").astype(np.uint64).reshape(h, -1, 4)
            f = lambda k, s: (wd[..., k] >> np.uint64(s)) & np.uint64(1023)   # noqa: E731
            y = np.stack([f(0, 10), f(1, 0), f(1, 20), f(2, 10), f(3, 0), f(3, 20)], axis=-1).reshape(h, -1)[:, :w]
            u = np.stack([f(0, 0), f(1, 10), f(2, 20)], axis=-1).reshape(h, -1)[:, :cw]
            v = np.stack([f(0, 20), f(2, 0), f(3, 10)], axis=-1).reshape(h, -1)[:, :cw]
            comps = [y, u, v]
        else:
            yb = _get_rows(buf, base + g.at[0], g.pitch[0], h, g.row[0]).reshape(h, w, wb)
            uvb = _get_rows(buf, base + g.at[1], g.pitch[1], ch, g.row[1]).reshape(ch, cw, 2, wb)
            words = [layout_ref._words_from_bytes(yb, wb, g.le), layout_ref._words_from_bytes(uvb[:, :, 0], wb, g.le),
                     layout_ref._words_from_bytes(uvb[:, :, 1], wb, g.le)]
            comps = [(x >> np.uint64(0 if g.lsb else 8 * wb - d)) & np.uint64((1 << d) - 1) for x, d in zip(words, depths)]
        for s, d in zip(comps, depths):
            out.append(layout_ref._bytes_from_words(s << np.uint64(8 * wb - d), wb, 0).tobytes())
    return b"".join(out)


def v210(fmt, pitched=False, picture_gap=256):
    """the tests' v210 formats: tight, or rows pitched to 128 bytes with picture_gap bytes between pictures"""
    if not pitched:
        return SimpleNamespace(packing=V210, little_endian=0, lsb_justified=0, pitch=(0, 0), plane_offset=(0, 0), picture_stride=0)
    p = (v210_row_bytes(fmt.width) + 127) // 128 * 128
    return SimpleNamespace(packing=V210, little_endian=0, lsb_justified=0, pitch=(p, 0), plane_offset=(0, 0),
                           picture_stride=(fmt.height * p + picture_gap + 15) // 16 * 16)


def semiplanar(fmt, little_endian=0, lsb_justified=0, pitched=False, pad=64, plane_gap=4096, picture_gap=256):
    """the tests' semi-planar formats: tight, or pitch = row bytes + pad (rounded up to 16), plane_gap bytes between the
    planes and picture_gap between pictures"""
    if not pitched:
        return SimpleNamespace(packing=SEMIPLANAR, little_endian=little_endian, lsb_justified=lsb_justified, pitch=(0, 0),
                               plane_offset=(0, 0), picture_stride=0)
    (h, w), (ch, cw), _ = layout_ref.planes(fmt)
    wb = fmt.word_bytes
    py, pc = (w * wb + pad + 15) // 16 * 16, (2 * cw * wb + pad + 15) // 16 * 16
    at = h * py + plane_gap
    return SimpleNamespace(packing=SEMIPLANAR, little_endian=little_endian, lsb_justified=lsb_justified, pitch=(py, pc),
                           plane_offset=(0, at), picture_stride=(at + ch * pc + picture_gap + 15) // 16 * 16)
