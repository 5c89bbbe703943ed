"""The model of vc2hip_set_sample_layout's contract (include/vc2hip.h), in numpy: where the samples of a batch of pictures
lie under a layout, and which bits of a word are the sample.

fmt is anything with the fields of vc2hip_picture_format (width, height, chroma_format 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0,
bit_depth, word_bytes, chroma_bit_depth); layout anything with those of vc2hip_sample_layout, or None for the file
format.  The ctypes structures of vc2hip_py fit both.

    Read     a sample is the `depth` bits of its word at the layout's position; every other bit is ignored.
    Written  every bit of a word outside the sample is zero; no byte outside the rows of the planes is touched.

to_layout writes exactly what the decoder must write (with `fill` in every byte it must leave alone), and, given a
generator, puts random bits into every ignored position of an encoder's input.
"""
from types import SimpleNamespace

import numpy as np

MAX_PITCH = 1 << 23     # the header's limits of a plane under a layout: the kernels' 32-bit row offsets
MAX_PLANE = 1 << 31


def file_layout():
    return SimpleNamespace(little_endian=0, lsb_justified=0, pitch=(0, 0, 0), plane_offset=(0, 0, 0), picture_stride=0)


def planes(fmt):
    """[(rows, cols)] of Y, U, V"""
    w, h = fmt.width, fmt.height
    cw = w if fmt.chroma_format == 0 else w // 2
    ch = h // 2 if fmt.chroma_format == 2 else h
    return [(h, w), (ch, cw), (ch, cw)]


def geometry(fmt, layout):
    """the layout resolved for pictures of fmt: pitch[3], at[3] (plane offsets), extent (a picture's base to the end of its
    furthest plane row), stride (one picture's base to the next); None for a layout the calls refuse"""
    lay = layout if layout is not None else file_layout()
    wb = fmt.word_bytes
    pitch_in, off_in, stride_in = list(lay.pitch), list(lay.plane_offset), int(lay.picture_stride)
    if lay.little_endian not in (0, 1) or lay.lsb_justified not in (0, 1):
        return None
    if any(x % 16 for x in pitch_in + off_in + [stride_in]):
        return None
    custom = bool(lay.little_endian or lay.lsb_justified or stride_in or any(pitch_in) or any(off_in))
    pitch, at, extent = [], [], 0
    for k, (rows, cols) in enumerate(planes(fmt)):
        row = cols * wb
        p = pitch_in[k] or row
        if p < row:
            return None
        if custom and (p >= MAX_PITCH or rows * p >= MAX_PLANE):
            return None
        pitch.append(p)
        if any(off_in):
            at.append(off_in[k])
        else:
            at.append(0 if k == 0 else at[k - 1] + planes(fmt)[k - 1][0] * pitch[k - 1])
        extent = max(extent, at[k] + (rows - 1) * p + row)
    stride = stride_in or extent
    if stride < extent:
        return None
    return SimpleNamespace(pitch=pitch, at=at, extent=extent, stride=stride, le=int(lay.little_endian), lsb=int(lay.lsb_justified))


def picture_bytes(fmt, layout):
    """the model of vc2hip_layout_picture_bytes (0: refused)"""
    g = geometry(fmt, layout)
    return g.extent if g else 0


def buffer_bytes(fmt, n, layout):
    """bytes of a buffer of n pictures: n picture strides (the last picture's tail is part of what must stay untouched)"""
    g = geometry(fmt, layout)
    return n * g.stride


def _depths(fmt):
    c = fmt.chroma_bit_depth or fmt.bit_depth
    return [fmt.bit_depth, c, c]


def _words_from_bytes(b, wb, le):
    """(..., wb) uint8 -> (...) uint64 words"""
    b = b.astype(np.uint64)
    w = np.zeros(b.shape[:-1], np.uint64)
    for k in range(wb):
        w |= b[..., k] << np.uint64(8 * (k if le else wb - 1 - k))
    return w


def _bytes_from_words(w, wb, le):
    return np.stack([(w >> np.uint64(8 * (k if le else wb - 1 - k))) & np.uint64(0xFF) for k in range(wb)], axis=-1).astype(np.uint8)


def file_samples(file_bytes, fmt, n):
    """sample values of n file-format pictures: [picture][component] -> (rows, cols) uint64 (the bits below the depth dropped)"""
    wb = fmt.word_bytes
    raw = np.frombuffer(file_bytes, np.uint8)
    out, at = [], 0
    for _ in range(n):
        pic = []
        for (rows, cols), d in zip(planes(fmt), _depths(fmt)):
            b = raw[at:at + rows * cols * wb].reshape(rows, cols, wb)
            at += rows * cols * wb
            pic.append(_words_from_bytes(b, wb, 0) >> np.uint64(8 * wb - d))
        out.append(pic)
    assert at == raw.size, "file_bytes does not hold n pictures of fmt"
    return out


def to_layout(file_bytes, fmt, n, layout, fill=0, garbage=None):
    """n file-format pictures placed under `layout`: a uint8 array of buffer_bytes(), `fill` in every byte outside the rows of
    the planes.  Every bit of a word outside the sample is zero (what the decoder writes) -- or, with garbage = a numpy
    Generator, random (an encoder input whose ignored bits must not matter)."""
    g = geometry(fmt, layout)
    assert g is not None, "a layout the calls refuse"
    wb = fmt.word_bytes
    buf = np.full(n * g.stride, fill, np.uint8)
    for i, pic in enumerate(file_samples(file_bytes, fmt, n)):
        for k, (s, d) in enumerate(zip(pic, _depths(fmt))):
            shift = 0 if g.lsb else 8 * wb - d
            w = s << np.uint64(shift)
            if garbage is not None:
                keep = np.uint64(((1 << d) - 1) << shift)
                junk = garbage.integers(0, 1 << (8 * wb), size=s.shape, dtype=np.uint64)
                w |= junk & ~keep & np.uint64((1 << (8 * wb)) - 1)
            b = _bytes_from_words(w, wb, g.le).reshape(s.shape[0], -1)
            for r in range(s.shape[0]):
                o = i * g.stride + g.at[k] + r * g.pitch[k]
                buf[o:o + b.shape[1]] = b[r]
    return buf


def from_layout(buf, fmt, n, layout):
    """the inverse: the file-format bytes of n pictures read from a buffer under `layout` (ignored bits dropped)"""
    g = geometry(fmt, layout)
    assert g is not None, "a layout the calls refuse"
    wb = fmt.word_bytes
    buf = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    out = []
    for i in range(n):
        for k, ((rows, cols), d) in enumerate(zip(planes(fmt), _depths(fmt))):
            o = i * g.stride + g.at[k]
            idx = o + np.arange(rows)[:, None] * g.pitch[k] + np.arange(cols * wb)[None, :]
            w = _words_from_bytes(buf[idx].reshape(rows, cols, wb), wb, g.le)
            shift = 0 if g.lsb else 8 * wb - d
            s = (w >> np.uint64(shift)) & np.uint64((1 << d) - 1)
            out.append(_bytes_from_words(s << np.uint64(8 * wb - d), wb, 0).tobytes())
    return b"".join(out)


def pitched(fmt, little_endian=0, lsb_justified=0, pad=64, plane_gap=4096, picture_gap=256):
    """the tests' "pitched" layout: pitch = row bytes + pad (rounded up to 16), plane_gap bytes between planes, picture_gap
    between pictures"""
    wb = fmt.word_bytes
    pitch, off, at = [], [], 0
    for rows, cols in planes(fmt):
        p = (cols * wb + pad + 15) // 16 * 16
        pitch.append(p)
        off.append(at)
        at += rows * p + plane_gap
    at -= plane_gap
    stride = (at + picture_gap + 15) // 16 * 16
    off[0] = 0
    return SimpleNamespace(little_endian=little_endian, lsb_justified=lsb_justified, pitch=tuple(pitch), plane_offset=tuple(off),
                           picture_stride=stride)
