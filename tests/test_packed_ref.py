"""CPU-side checks of the packed-format interface (vc2hip_set_packed_format, vc2hip_packed_picture_bytes): the numpy model of
the contract (tests/packed_ref.py) round-trips against tests/layout_ref.py's reading of the file format, the v210 word
layout is pinned by hand-written groups, and the library's host arithmetic agrees with the model over the admitted and the
refused cases.  No GPU compute here."""
import itertools
import os
import re

import numpy as np
import pytest

import layout_ref
import packed_ref
from synth import words_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vc2-reference_amd", "libvc2hip.so")
HEADER = os.path.join(ROOT, "include", "vc2hip.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import vc2hip_py
    return vc2hip_py.load_library()


def _fmt(w, h, cf, wb, bits, chroma_bits=0):
    import vc2hip_py
    return vc2hip_py.picture_format(w, h, cf, bits, wb, chroma_bits)


def _pf(x):
    import vc2hip_py
    return vc2hip_py.packed_format(x.packing, x.little_endian, x.lsb_justified, x.pitch, x.plane_offset, x.picture_stride)


def _raw(fmt, n, seed):
    cf = {0: "444", 1: "422", 2: "420"}[fmt.chroma_format]
    return b"".join(words_frame(fmt.width, fmt.height, cf, fmt.bit_depth, seed + i, fmt.word_bytes, "noise") for i in range(n))


# widths with width % 6 = 0, 2, 4; one beyond a 48-pixel unit plus a tail
V210_SHAPES = [(48, 6), (50, 4), (52, 4), (110, 3), (1280, 2)]


@pytest.mark.parametrize("w,h", V210_SHAPES)
def test_v210_model_round_trips(w, h):
    fmt = _fmt(w, h, "422", 2, 10)
    n = 3
    raw = _raw(fmt, n, w)
    rng = np.random.default_rng(w)
    for pitched in (False, True):
        pf = packed_ref.v210(fmt, pitched)
        g = packed_ref.geometry(fmt, pf)
        assert g.row[0] == (w + 5) // 6 * 16 and g.pitch[0] % (128 if pitched else 16) == 0
        clean = packed_ref.to_packed(raw, fmt, n, pf, fill=0xA5)
        assert clean.size == packed_ref.buffer_bytes(fmt, n, pf)
        assert packed_ref.from_packed(clean, fmt, n, pf) == raw
        dirty = packed_ref.to_packed(raw, fmt, n, pf, fill=0xA5, garbage=rng)
        assert packed_ref.from_packed(dirty, fmt, n, pf) == raw, "ignored bits or fields changed a sample"
        assert (dirty != clean).any()
        # every group of a row is written whole; nothing else
        marked = packed_ref.to_packed(bytes(len(raw)), fmt, n, pf, fill=0xFF)
        assert int((marked == 0xFF).sum()) == n * (g.stride - h * g.row[0])
        # the samples are layout_ref's reading of the file format
        want = layout_ref.file_samples(raw, fmt, n)
        words = clean[:g.row[0]].view("<u4")
        assert int(words[0]) == int(want[0][1][0, 0]) | int(want[0][0][0, 0]) << 10 | int(want[0][2][0, 0]) << 20
        assert not (clean.reshape(n, -1)[:, :g.row[0]].copy().view("<u4") >> 30).any(), "bits 30 - 31 are written as zero"


def test_v210_word_layout_by_hand():
    """three groups with literal words: 14 pixels wide, so the third group holds two pixels and four empty fields"""
    fmt = _fmt(14, 1, "422", 2, 10)
    y = [0x001, 0x002, 0x004, 0x008, 0x010, 0x020, 0x040, 0x080, 0x100, 0x200, 0x3FF, 0x155, 0x2AA, 0x0F0]
    u = [0x111, 0x222, 0x333, 0x044, 0x055, 0x066, 0x3C3]
    v = [0x0AA, 0x0BB, 0x0CC, 0x1DD, 0x1EE, 0x1FF, 0x03C]
    raw = b"".join((np.array(p, np.uint16) << 6).astype(">u2").tobytes() for p in (y, u, v))
    pf = packed_ref.v210(fmt)
    got = packed_ref.to_packed(raw, fmt, 1, pf).view("<u4").tolist()
    want = [
        # group 0: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
        0x111 | 0x001 << 10 | 0x0AA << 20, 0x002 | 0x222 << 10 | 0x004 << 20, 0x0BB | 0x008 << 10 | 0x333 << 20, 0x010 | 0x0CC << 10 | 0x020 << 20,
        # group 1
        0x044 | 0x040 << 10 | 0x1DD << 20, 0x080 | 0x055 << 10 | 0x100 << 20, 0x1EE | 0x200 << 10 | 0x066 << 20, 0x3FF | 0x1FF << 10 | 0x155 << 20,
        # group 2: pixels 12 and 13, the rest zero
        0x3C3 | 0x2AA << 10 | 0x03C << 20, 0x0F0, 0, 0,
    ]
    assert want[0] == 0x0AA00511 and want[3] == 0x02033010 and want[9] == 0x000000F0   # (the arithmetic above, spelt out once)
    assert got == want
    assert packed_ref.from_packed(np.array(want, "<u4").view(np.uint8), fmt, 1, pf) == raw
    noisy = np.array(want, "<u4") | np.uint32(0xC0000000)
    noisy[9] |= 0x3FF << 10 | 0x3FF << 20
    noisy[10:] = 0xFFFFFFFF
    assert packed_ref.from_packed(noisy.view(np.uint8), fmt, 1, pf) == raw, "bits 30 - 31 and the fields beyond the width are ignored"


SP_SHAPES = [(40, 12, "422"), (33, 10, "444"), (48, 16, "420"), (392, 4, "420")]


@pytest.mark.parametrize("wb,bits", [(1, 8), (2, 10), (2, 16)])
def test_semiplanar_model_round_trips(wb, bits):
    rng = np.random.default_rng(bits)
    for (w, h, cf), (le, lsb), pitched in itertools.product(SP_SHAPES, itertools.product((0, 1), (0, 1)), (False, True)):
        fmt = _fmt(w, h, cf, wb, bits)
        n = 3
        raw = _raw(fmt, n, 7 * wb + w)
        pf = packed_ref.semiplanar(fmt, le, lsb, pitched)
        what = f"{w}x{h} {cf} {wb}-byte le{le} lsb{lsb} {'pitched' if pitched else 'tight'}"
        g = packed_ref.geometry(fmt, pf)
        clean = packed_ref.to_packed(raw, fmt, n, pf, fill=0xA5)
        assert clean.size == packed_ref.buffer_bytes(fmt, n, pf), what
        assert packed_ref.from_packed(clean, fmt, n, pf) == raw, what
        dirty = packed_ref.to_packed(raw, fmt, n, pf, fill=0xA5, garbage=rng)
        assert packed_ref.from_packed(dirty, fmt, n, pf) == raw, f"{what}: ignored bits changed a sample"
        assert (dirty != clean).any() == (bits < 8 * wb), what
        marked = packed_ref.to_packed(bytes(len(raw)), fmt, n, pf, fill=0xFF)
        assert int((marked == 0xFF).sum()) == n * (g.stride - len(raw) // n), what
        # the Y plane is layout_ref's plane 0 under the same word form; U and V alternate in the second plane
        lay = layout_ref.file_layout()
        lay.little_endian, lay.lsb_justified, lay.pitch = le, lsb, (g.pitch[0] if pitched else 0, 0, 0)
        planar = layout_ref.to_layout(raw[:len(raw) // n], fmt, 1, lay)
        gl = layout_ref.geometry(fmt, lay)
        assert np.array_equal(clean[:h * g.pitch[0]][:g.row[0]], planar[:g.row[0]]), what
        cw = layout_ref.planes(fmt)[1][1]
        uv = clean[g.at[1]:g.at[1] + g.row[1]].reshape(cw, 2, wb)
        assert np.array_equal(uv[:, 0].ravel(), planar[gl.at[1]:gl.at[1] + cw * wb]), f"{what}: U first"
        assert np.array_equal(uv[:, 1].ravel(), planar[gl.at[2]:gl.at[2] + cw * wb]), f"{what}: V second"


def test_p010_is_little_endian_msb_justified():
    fmt = _fmt(8, 2, "420", 2, 10)
    raw = _raw(fmt, 1, 1)
    s = layout_ref.file_samples(raw, fmt, 1)[0]
    buf = packed_ref.to_packed(raw, fmt, 1, packed_ref.semiplanar(fmt, 1, 0)).view("<u2")
    assert buf[0] == int(s[0][0, 0]) << 6 and buf[16] == int(s[1][0, 0]) << 6 and buf[17] == int(s[2][0, 0]) << 6


def _cases():
    """(name, fmt arguments, packed format, admitted)"""
    from types import SimpleNamespace as NS
    v = lambda **kw: NS(**{**dict(packing=1, little_endian=0, lsb_justified=0, pitch=(0, 0), plane_offset=(0, 0), picture_stride=0), **kw})   # noqa: E731
    s = lambda **kw: v(**{**dict(packing=2), **kw})   # noqa: E731
    f422 = (1280, 6, "422", 2, 10)
    row = 1280 // 6 * 16 + 16
    out = [
        ("v210 tight 1280", f422, v(), True),
        ("v210 128-byte pitch", f422, v(pitch=(3456, 0)), True),
        ("v210 pitch and stride", f422, v(pitch=(3456, 0), picture_stride=3456 * 6 + 256), True),
        ("v210 width 50", (50, 4, "422", 2, 10), v(), True),
        ("v210 chroma depth 10", (48, 4, "422", 2, 10, 10), v(), True),
        ("semi-planar NV12", (392, 8, "420", 1, 8), s(), True),
        ("semi-planar P010", (64, 8, "420", 2, 10), s(little_endian=1), True),
        ("semi-planar NV24 placed", (33, 4, "444", 1, 8), s(pitch=(48, 80), plane_offset=(0, 4096)), True),
        ("semi-planar chroma depth 8 of 10", (64, 8, "422", 2, 10, 8), s(little_endian=1, lsb_justified=1), True),
        ("no packing", f422, v(packing=0), False),
        ("unknown packing", f422, v(packing=3), False),
        ("negative packing", f422, v(packing=-1), False),
        ("flag 2", (64, 8, "420", 2, 10), s(little_endian=2), False),
        ("flag -1", (64, 8, "420", 2, 10), s(lsb_justified=-1), False),
        ("v210 little_endian set", f422, v(little_endian=1), False),
        ("v210 lsb_justified set", f422, v(lsb_justified=1), False),
        ("v210 second pitch", f422, v(pitch=(3456, 3456)), False),
        ("v210 plane offset", f422, v(plane_offset=(16, 0)), False),
        ("v210 second plane offset", f422, v(plane_offset=(0, 4096)), False),
        ("pitch not a multiple of 16", f422, v(pitch=(3456 + 8, 0)), False),
        ("offset not a multiple of 16", (64, 8, "420", 2, 10), s(plane_offset=(0, 4100)), False),
        ("stride not a multiple of 16", f422, v(picture_stride=3424 * 6 + 8), False),
        ("pitch below the row", f422, v(pitch=(row - 16, 0)), False),
        ("UV pitch below the row", (64, 8, "422", 2, 10), s(pitch=(128, 112)), False),
        ("stride below the picture", f422, v(picture_stride=row * 6 - 16), False),
        ("pitch 2^23", f422, v(pitch=(1 << 23, 0)), False),
        ("rows * pitch 2^31", (1280, 1024, "422", 2, 10), v(pitch=(1 << 21, 0)), False),
        ("v210 4:2:0", (1280, 6, "420", 2, 10), v(), False),
        ("v210 4:4:4", (1280, 6, "444", 2, 10), v(), False),
        ("v210 12 bits", (1280, 6, "422", 2, 12), v(), False),
        ("v210 chroma depth 8", (1280, 6, "422", 2, 10, 8), v(), False),
        ("v210 one-byte words", (1280, 6, "422", 1, 8), v(), False),
        ("v210 four-byte words", (1280, 6, "422", 4, 10), v(), False),
        ("v210 odd width", (1281, 6, "422", 2, 10), v(), False),
        ("semi-planar three-byte words", (64, 8, "420", 3, 12), s(), False),
        ("semi-planar four-byte words", (64, 8, "420", 4, 12), s(), False),
    ]
    return out


@pytest.mark.parametrize("name,fa,pf,ok", _cases(), ids=[c[0] for c in _cases()])
def test_library_arithmetic_agrees_with_the_model(lib, name, fa, pf, ok):
    """vc2hip_packed_picture_bytes of the built library against the model, over admitted and refused cases"""
    import vc2hip_py
    fmt = _fmt(*fa[:3], fa[3], fa[4], *(fa[5:]))
    want = packed_ref.picture_bytes(fmt, pf)
    assert (want > 0) == ok, f"{name}: the model"
    assert vc2hip_py.packed_picture_bytes(lib, fmt, _pf(pf)) == want, name


def test_library_arithmetic_values(lib):
    import vc2hip_py
    fmt = _fmt(1280, 720, "422", 2, 10)
    assert vc2hip_py.v210_pitch(1280) == 3456 and vc2hip_py.v210_pitch(1280, 16) == 214 * 16 and vc2hip_py.v210_pitch(3840) == 10240
    assert vc2hip_py.packed_picture_bytes(lib, fmt, vc2hip_py.packed_format("v210")) == 720 * 214 * 16
    assert vc2hip_py.packed_picture_bytes(lib, fmt, vc2hip_py.packed_format("v210", pitch=(3456, 0))) == 719 * 3456 + 214 * 16
    p010 = _fmt(1920, 1080, "420", 2, 10)
    assert vc2hip_py.packed_picture_bytes(lib, p010, vc2hip_py.packed_format("semiplanar", True)) == 1920 * 1080 * 3
    assert vc2hip_py.packed_picture_bytes(lib, fmt, None) == 0


def test_header_library_and_binding_carry_the_calls(lib):
    import vc2hip_py
    text = open(HEADER).read()
    for name in ("vc2hip_set_packed_format", "vc2hip_packed_picture_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in vc2hip_py.EXPORTS
        assert hasattr(lib, name)
    for word in ("VC2HIP_PACKING_NONE = 0", "VC2HIP_PACKING_V210 = 1", "VC2HIP_PACKING_SEMIPLANAR = 2", "NV21", "UYVY"):
        assert word in text, word
    # the struct of the binding is the header's: an int, two ints, two pairs of size_t, a size_t
    import ctypes as C
    assert C.sizeof(vc2hip_py.PackedFormat) == 16 + 5 * C.sizeof(C.c_size_t)
