"""CPU checks of the definition of VC2HIP_HQ_CAPPED (tests/cap_ref.py) and of the mode's host-only ABI.  No GPU compute here.
(The refusals of vc2hip_encode_batch_dev -- q_index 116, compressed_bytes 0 -- need a context, hence a device: they are in
tests/test_gpu_cap.py.)"""
import ctypes as C
import os
import re

import pytest

import cap_ref as cr
import proxy_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = range(len(cr.MATRIX))


@pytest.mark.parametrize("i", ROWS, ids=cr.IDS)
def test_lengths_never_grow_with_the_index(oracle, i):
    """on 0 .. 115: a codable index is followed by codable ones, and by lengths no larger; index 115 codes every picture of
    the matrix, and codes nothing but slice headers"""
    case, pics = cr.batch(oracle, i)
    for k, p in enumerate(pics):
        L = p.table
        assert len(L) == cr.Q_TOP + 1
        first = next(q for q in range(len(L)) if L[q] is not cr.NOT_CODABLE)
        assert all(x is not cr.NOT_CODABLE for x in L[first:]), (k, "a refused index above a coded one")
        assert all(L[q] <= L[q - 1] for q in range(first + 1, len(L))), (k, L)
        assert L[cr.Q_TOP] >= case.ys * case.xs * (case.prefix + 4)
    assert pics[0].table[case.q] is not cr.NOT_CODABLE   # the floor codes the smooth picture: the caps stand on its table


@pytest.mark.parametrize("i", ROWS, ids=cr.IDS)
def test_caps_and_choices(oracle, i):
    """the five caps give picture 0 the index DESIGN.md section 17 names for each; the exhaustive choice is the bisection's on every
    picture and cap; the mid cap separates the pictures of the batch"""
    case, pics = cr.batch(oracle, i)
    caps = cr.caps(case, pics[0])
    for name, (cap, want0) in caps.items():
        got = [cr.chosen(case, p, case.q, cap) for p in pics]
        assert got[0] == want0, (name, cap, got, want0)
        assert got == [p.bisected(case.q, cap) for p in pics], (name, cap)
        for p, q in zip(pics, got):
            assert p.fits(q, cap) or q == cr.Q_TOP
            assert q == case.q or not p.fits(q - 1, cap)
        print(cr.IDS[i], name, cap, got)
    assert len(set(cr.chosen(case, p, case.q, caps["mid"][0]) for p in pics)) >= 2
    assert all(cr.chosen(case, p, case.q, caps["none"][0]) == cr.Q_TOP and p.table[cr.Q_TOP] > caps["none"][0] for p in pics)
    assert cr.chosen(case, pics[0], case.q, caps["floor"][0]) == case.q


def test_the_escape_row_escapes_and_the_scalar_one_row_refuses(oracle):
    """what the matrix's comments promise: row ESCAPES has coefficients beyond 16 bits in every picture (the hand-back
    path of the fast form); row 1 (scalar 1) has a floor at which the oracle codes the smooth picture and refuses the noise"""
    _, pics = cr.batch(oracle, cr.ESCAPES)
    big = [max(int(abs(pl).max()) for pl in p.planes) for p in pics]
    assert min(big) > 32767, big
    case, pics = cr.batch(oracle, 1)
    assert pics[1].table[case.q] is cr.NOT_CODABLE and pics[0].table[case.q] is not cr.NOT_CODABLE


def test_mode_3_in_the_header_the_library_and_the_binding():
    import vc2hip_py
    text = open(os.path.join(ROOT, "include", "vc2hip.h")).read()
    assert re.search(r"VC2HIP_HQ_CAPPED\s*=\s*3\b", text) and re.search(r"#define\s+VC2HIP_FLAG_CAP_GENERAL\s+0x2000u", text)
    assert re.search(r"#define\s+VC2HIP_CAP_Q_TOP\s+115\b", text)
    assert vc2hip_py.MODES["HQ_Capped"] == cr.MODE == 3 and vc2hip_py.FLAGS["CAP_GENERAL"] == 0x2000


@pytest.mark.parametrize("prefix,scalar", [(0, 1), (3, 4)])
def test_calls_that_do_not_encode_read_the_mode_as_constq(prefix, scalar):
    """vc2hip_max_payload_bytes and vc2hip_picture_header (host arithmetic, no device): mode 3 = mode 0"""
    import vc2hip_py
    lib = pr._hip_lib()
    fmt = vc2hip_py.picture_format(1024, 64, "422", 10)
    const = vc2hip_py.coding_params(lib, fmt, "DD97", 4, 1, 2, mode="HQ_ConstQ", q=9, prefix=prefix, scalar=scalar)
    capped = vc2hip_py.coding_params(lib, fmt, "DD97", 4, 1, 2, mode="HQ_Capped", q=9, s=12345, prefix=prefix, scalar=scalar)
    assert capped.mode == 3 and capped.compressed_bytes == 12345
    lib.vc2hip_max_payload_bytes.restype = C.c_size_t
    assert lib.vc2hip_max_payload_bytes(C.byref(fmt), C.byref(capped)) == lib.vc2hip_max_payload_bytes(C.byref(fmt), C.byref(const)) \
        == const.y_slices * const.x_slices * (prefix + 4 + 3 * 255 * scalar)
    for major in (2, 3):
        assert vc2hip_py.picture_header(lib, capped, major, 7) == vc2hip_py.picture_header(lib, const, major, 7)
