"""CPU tests of vc2hip_picture_header, the one writer of the picture header and transform parameters (the host tools and the
device stream writer both use it): against the oracle's HQ header writer and against the LD picture units of oracle streams."""
import ctypes as C

import numpy as np
import pytest

from synth import synth
from vc2lib import KERNELS, make_params


@pytest.fixture(scope="module")
def lib():
    import vc2hip_py
    return vc2hip_py.load_library()


def _oracle_hq_header(oracle, picture_number, kernel, depth, xs, ys, prefix, scalar, major):
    f = oracle.lib.vc2o_write_hq_picture_header
    f.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                  C.POINTER(C.c_size_t)]
    out = (C.c_uint8 * 64)()
    n = C.c_size_t()
    assert f(picture_number, kernel, depth, xs, ys, prefix, scalar, major, out, 64, C.byref(n)) == 0
    return bytes(out[:n.value])


def _cp(kernel, depth, ys, xs, mode="HQ_ConstQ", compressed=0, prefix=0, scalar=1):
    import vc2hip_py
    return vc2hip_py.CodingParams(kernel, depth, ys, xs, vc2hip_py.MODES[mode], 0, compressed, prefix, scalar)


def _uvlc(data, bitpos):
    """interleaved exp-Golomb at bit `bitpos` of data: (value, next bit position)"""
    def bit():
        nonlocal bitpos
        b = data[bitpos >> 3] >> (7 - (bitpos & 7)) & 1
        bitpos += 1
        return b
    v = 1
    while not bit():
        v = (v << 1) | bit()
    return v - 1, bitpos


@pytest.mark.parametrize("major", [2, 3])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_hq_header_matches_the_oracle(lib, oracle, kernel, major):
    import vc2hip_py
    k = KERNELS[kernel]
    for depth in range(1, 6):
        for ys, xs in ((1, 1), (8, 15), (68, 120), (135, 240), (1000, 3)):
            for prefix, scalar in ((0, 1), (1, 3), (7, 255), (300, 1000)):
                for pn in (0, 1, 2 ** 32 - 1):
                    want = _oracle_hq_header(oracle, pn, k, depth, xs, ys, prefix, scalar, major)
                    for mode in ("HQ_ConstQ", "HQ_CBR"):
                        cp = _cp(k, depth, ys, xs, mode, 123456, prefix, scalar)
                        assert vc2hip_py.picture_header(lib, cp, major, pn) == want, (depth, ys, xs, prefix, scalar, pn, mode)


@pytest.mark.parametrize("w,h,cf,kernel,depth,u,a,s,interlaced", [
    (128, 64, "420", "LeGall", 3, 2, 2, 3000, False),
    (96, 48, "444", "DD97", 2, 2, 3, 5001, False),
    (64, 64, "422", "Haar1", 1, 4, 4, 777, True),
])
def test_ld_header_matches_oracle_stream(lib, oracle, w, h, cf, kernel, depth, u, a, s, interlaced):
    import vc2hip_py
    p = make_params(w, h, cf, 8, kernel, depth, u, a, mode="LD", s=s, word_bytes=1, interlaced=interlaced)
    stream = oracle.encode_stream(p, synth(w, h, cf, 8, 3, word_bytes=1), 1)
    seq = int.from_bytes(stream[5:9], "big")
    major, _ = _uvlc(stream, 8 * 13)
    ph = h // 2 if interlaced else h
    fmt = vc2hip_py.picture_format(w, ph, cf, 8, 1)
    cp = vc2hip_py.coding_params(lib, fmt, kernel, depth, u, a, mode="LD", s=s // 2 if interlaced else s)
    at = seq
    for pn in range(2 if interlaced else 1):
        assert stream[at + 4] == 0xC8
        unit = int.from_bytes(stream[at + 5:at + 9], "big")
        hdr = vc2hip_py.picture_header(lib, cp, major, pn)
        assert stream[at + 13:at + 13 + len(hdr)] == hdr
        assert unit - 13 - len(hdr) == _ld_payload_bytes(lib, cp)
        at += unit


def _ld_payload_bytes(lib, cp):
    sb = np.zeros(cp.y_slices * cp.x_slices, np.int32)
    assert lib.vc2hip_slice_bytes(cp.y_slices, cp.x_slices, cp.compressed_bytes, 1, sb) == 0
    return int(sb.sum())


def test_ld_fraction_in_lowest_terms(lib):
    import vc2hip_py
    cp = _cp(1, 3, 4, 6, "LD", compressed=24 * 100)  # 2400 / 24 = 100 / 1
    hdr = vc2hip_py.picture_header(lib, cp, 2, 0)
    pos = 32
    fields = []
    for _ in range(6):
        v, pos = _uvlc(hdr, pos)
        fields.append(v)
    assert fields == [1, 3, 6, 4, 100, 1]


def test_bad_arguments_and_short_buffer(lib):
    import vc2hip_py
    for cp in (_cp(7, 3, 4, 6), _cp(1, 3, 0, 6), _cp(1, 3, 4, 6, scalar=0), _cp(1, 3, 4, 6, "LD", compressed=0)):
        with pytest.raises(vc2hip_py.Vc2HipError):
            vc2hip_py.picture_header(lib, cp, 2, 0)
    cp = _cp(0, 4, 68, 120, prefix=1, scalar=3)
    full = vc2hip_py.picture_header(lib, cp, 3, 9)
    out = np.zeros(64, np.uint8)
    n = C.c_size_t()
    rc = lib.vc2hip_picture_header(C.byref(cp), 3, 9, out, len(full) - 1, C.byref(n))
    assert rc == -9 and n.value == len(full)   # VC2HIP_ECAP, with the bytes it needs
