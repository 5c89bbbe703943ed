"""CPU-side checks of the sample-layout interface (vc2hip_set_sample_layout, vc2hip_layout_picture_bytes): the numpy model of
the contract (tests/layout_ref.py) round-trips, the library's host arithmetic agrees with it, and the header, the library
and the binding all carry the new calls.  No GPU compute here."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import layout_ref
from synth import words_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vc2-reference_amd", "libvc2hip.so")
HEADER = os.path.join(ROOT, "include", "vc2hip.h")

# (width, height, chroma format, bit depth per word size): odd widths, so that tight rows are no multiple of 16 bytes
SHAPES = [(40, 12, "422"), (33, 10, "444"), (48, 16, "420")]
BITS = {1: 8, 2: 10, 3: 12, 4: 20}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    import vc2hip_py
    return vc2hip_py.load_library()


def _fmt(w, h, cf, wb, bits=None, chroma_bits=0):
    import vc2hip_py
    return vc2hip_py.picture_format(w, h, cf, bits or BITS[wb], wb, chroma_bits)


def _layouts(fmt):
    """the four byte order x justification combinations, tight and pitched"""
    import vc2hip_py
    for le, lsb in itertools.product((0, 1), (0, 1)):
        yield f"le{le} lsb{lsb} tight", vc2hip_py.sample_layout(le, lsb)
        p = layout_ref.pitched(fmt, le, lsb)
        yield f"le{le} lsb{lsb} pitched", vc2hip_py.sample_layout(le, lsb, p.pitch, p.plane_offset, p.picture_stride)


@pytest.mark.parametrize("wb", (1, 2, 3, 4))
def test_model_round_trips(wb):
    rng = np.random.default_rng(wb)
    for w, h, cf in SHAPES:
        fmt = _fmt(w, h, cf, wb)
        n = 3
        raw = b"".join(words_frame(w, h, cf, fmt.bit_depth, 10 * wb + i, wb, "noise") for i in range(n))
        for name, lay in _layouts(fmt):
            what = f"{w}x{h} {cf} {wb}-byte {name}"
            clean = layout_ref.to_layout(raw, fmt, n, lay, fill=0xA5)
            assert clean.size == layout_ref.buffer_bytes(fmt, n, lay), what
            assert layout_ref.from_layout(clean, fmt, n, lay) == raw, what
            dirty = layout_ref.to_layout(raw, fmt, n, lay, fill=0xA5, garbage=rng)
            assert layout_ref.from_layout(dirty, fmt, n, lay) == raw, f"{what}: ignored bits changed a sample"
            assert (dirty != clean).any() == (fmt.bit_depth < 8 * wb), f"{what}: garbage goes into the ignored bits, and only there"
            # the bytes outside the rows keep the fill: as many of them as the geometry says
            g = layout_ref.geometry(fmt, lay)
            rows_bytes = sum(r * c * wb for r, c in layout_ref.planes(fmt))
            marked = layout_ref.to_layout(bytes(len(raw)), fmt, n, lay, fill=0xFF)
            assert int((marked == 0xFF).sum()) == n * (g.stride - rows_bytes), what


def test_file_format_is_the_identity():
    fmt = _fmt(40, 12, "422", 2)
    raw = words_frame(40, 12, "422", 10, 3, 2, "noise") * 2
    assert layout_ref.to_layout(raw, fmt, 2, None).tobytes() == raw
    assert layout_ref.from_layout(raw, fmt, 2, None) == raw


def test_chroma_depth_of_its_own():
    fmt = _fmt(32, 8, "422", 2, bits=10, chroma_bits=8)
    import vc2hip_py
    lay = vc2hip_py.sample_layout(1, 1)
    y = words_frame(32, 8, "422", 10, 1, 2, "noise")
    c = words_frame(32, 8, "422", 8, 2, 2, "noise")
    raw = y[:32 * 8 * 2] + c[32 * 8 * 2:]
    buf = layout_ref.to_layout(raw, fmt, 1, lay, garbage=np.random.default_rng(0))
    assert layout_ref.from_layout(buf, fmt, 1, lay) == raw
    words = buf.view("<u2")
    assert (words[32 * 8:] & 0xFF).tolist() == (np.frombuffer(raw, ">u2")[32 * 8:] >> 8).tolist()


@pytest.mark.parametrize("wb", (1, 2, 3, 4))
def test_library_extent_equals_the_model(lib, wb):
    import vc2hip_py
    for w, h, cf in SHAPES:
        fmt = _fmt(w, h, cf, wb)
        file_bytes = lib.vc2hip_raw_picture_bytes(C.byref(fmt))
        assert vc2hip_py.layout_picture_bytes(lib, fmt, None) == file_bytes
        assert vc2hip_py.layout_picture_bytes(lib, fmt, vc2hip_py.sample_layout()) == file_bytes
        assert layout_ref.picture_bytes(fmt, None) == file_bytes
        for name, lay in _layouts(fmt):
            got = vc2hip_py.layout_picture_bytes(lib, fmt, lay)
            assert got == layout_ref.picture_bytes(fmt, lay) != 0, f"{w}x{h} {cf} {wb}-byte {name}"


def _refused(fmt):
    """(why, layout) for every layout the calls refuse for pictures of fmt"""
    import vc2hip_py
    row = fmt.width * fmt.word_bytes
    ok = layout_ref.pitched(fmt)
    yield "flag 2", vc2hip_py.sample_layout(2, 0)
    yield "flag -1", vc2hip_py.sample_layout(0, -1)
    yield "pitch not a multiple of 16", vc2hip_py.sample_layout(pitch=(ok.pitch[0] + 8, 0, 0))
    yield "plane offset not a multiple of 16", vc2hip_py.sample_layout(pitch=ok.pitch, plane_offset=(0, ok.plane_offset[1] + 4, ok.plane_offset[2]))
    yield "picture stride not a multiple of 16", vc2hip_py.sample_layout(pitch=ok.pitch, plane_offset=ok.plane_offset,
                                                                      picture_stride=ok.picture_stride + 2)
    yield "pitch below the row", vc2hip_py.sample_layout(pitch=((row - 1) // 16 * 16, 0, 0))
    yield "chroma pitch below the row", vc2hip_py.sample_layout(pitch=(0, 0, 16))
    yield "picture stride below the extent", vc2hip_py.sample_layout(pitch=ok.pitch, plane_offset=ok.plane_offset,
                                                                  picture_stride=(layout_ref.picture_bytes(fmt, ok) - 1) // 16 * 16)
    yield "pitch of 2^23 bytes", vc2hip_py.sample_layout(pitch=(1 << 23, 0, 0))
    yield "plane of 2^31 bytes", vc2hip_py.sample_layout(pitch=((1 << 31) // fmt.height // 16 * 16 + 16, 0, 0))


def test_refused_layouts_have_no_extent(lib):
    import vc2hip_py
    fmt = _fmt(1024, 256, "422", 2)
    seen = 0
    for why, lay in _refused(fmt):
        assert layout_ref.picture_bytes(fmt, lay) == 0, f"the model accepts: {why}"
        assert vc2hip_py.layout_picture_bytes(lib, fmt, lay) == 0, f"the library accepts: {why}"
        seen += 1
    assert seen == 10
    # the limits are exclusive: one step below them is accepted
    assert vc2hip_py.layout_picture_bytes(lib, fmt, vc2hip_py.sample_layout(pitch=((1 << 31) // 256 - 16, 0, 0))) != 0


def _declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return hdr, set(re.findall(r"\b(vc2hip_[a-z0-9_]+)\s*\(", hdr))


def test_header_library_and_binding_carry_the_layout_calls(lib):
    import vc2hip_py
    hdr, names = _declared()
    for name in ("vc2hip_set_sample_layout", "vc2hip_layout_picture_bytes"):
        assert name in names, f"{name} is not declared in include/vc2hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in vc2hip_py.EXPORTS, f"{name} is not bound"
    m = re.search(r"typedef struct \{([^}]*)\} vc2hip_sample_layout;", hdr)
    assert m, "vc2hip_sample_layout is not declared"
    fields = re.findall(r"\b(int|size_t)\s+(\w+)(\[3\])?;", m.group(1))
    assert fields == [("int", "little_endian", ""), ("int", "lsb_justified", ""), ("size_t", "pitch", "[3]"),
                      ("size_t", "plane_offset", "[3]"), ("size_t", "picture_stride", "")]
    assert [f[0] for f in vc2hip_py.SampleLayout._fields_] == [f[1] for f in fields]
    assert C.sizeof(vc2hip_py.SampleLayout) == 8 + 7 * C.sizeof(C.c_size_t)
    assert callable(vc2hip_py.torch_planes) and callable(vc2hip_py.Vc2Hip.set_sample_layout)


def test_torch_planes_reads_the_layout_from_the_views():
    torch = pytest.importorskip("torch")
    import vc2hip_py
    n, h, w, cw = 3, 8, 32, 16
    pitch = 48                                                   # elements: 96 bytes
    per = (h * pitch) * 3 + 64
    big = torch.zeros(n * per + 8, dtype=torch.int16)
    start = (-big.data_ptr() % 16) // 2                          # a 16-byte aligned base
    def view(at, cols):
        return big.as_strided((n, h, cols), (per, pitch, 1), start + at)
    y, u, v = view(0, w), view(h * pitch + 32, cw), view(2 * h * pitch + 64, cw)
    base, lay = vc2hip_py.torch_planes(y, u, v)
    assert base == y.data_ptr() and lay.little_endian == 1 and lay.lsb_justified == 1
    assert list(lay.pitch) == [96, 96, 96] and list(lay.plane_offset) == [0, (h * pitch + 32) * 2, (2 * h * pitch + 64) * 2]
    assert lay.picture_stride == per * 2
    fmt = vc2hip_py.picture_format(w, h, "422", 10)
    assert layout_ref.geometry(fmt, lay) is not None
    with pytest.raises(ValueError):
        vc2hip_py.torch_planes(big.as_strided((n, h, w // 2), (per, pitch, 2), start), u, v)      # words stepped over
    with pytest.raises(ValueError):
        vc2hip_py.torch_planes(y, u, big.as_strided((n, h, cw), (per + 8, pitch, 1), start + 64))  # another picture stride
    with pytest.raises(ValueError):
        vc2hip_py.torch_planes(y.float(), u.float(), v.float())
