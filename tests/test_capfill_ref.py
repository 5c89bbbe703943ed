"""CPU checks of the definition of VC2HIP_HQ_CAPPED_FILL (tests/capfill_ref.py) and of the mode's host-only ABI.  No GPU
compute here.  (The refusals need a context, hence a device: they are in tests/test_gpu_capfill.py.)"""
import ctypes as C
import os
import re

import pytest

import cap_ref as cr
import capfill_ref as cf
import proxy_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = range(len(cf.MATRIX))


def _fills(oracle, i):
    """[(cap name, picture number, Filled)] of row i: every cap, every picture"""
    case, pics = cf.batch(oracle, i)
    caps = cf.caps(case, pics[0])
    return case, [(name, k, cf.fill(p, case.q, caps[name][0])) for name in cf.CAPS for k, p in enumerate(pics)]


def test_the_new_row_and_the_visit_order():
    assert cf.visit_order(1) == [0] and cf.visit_order(2) == [0, 1] and cf.visit_order(4) == [0, 2, 1, 3]
    assert cf.visit_order(5) == [0, 4, 2, 1, 3] and cf.visit_order(8) == [0, 4, 2, 6, 1, 5, 3, 7]
    for ns in (1, 2, 3, 256, 504, 1024, 1615):
        assert sorted(cf.visit_order(ns)) == list(range(ns))
    assert (1 << (1615 - 1).bit_length()) - 1615 == 433


@pytest.mark.parametrize("i", ROWS, ids=cf.IDS)
def test_the_definition_on_every_cap(oracle, i):
    case, fills = _fills(oracle, i)
    ns, empty = case.ys * case.xs, case.prefix + 4
    if i == cf.NEW:
        assert (case.ys, case.xs) == (17, 95)
    for name, k, f in fills:
        tag, p, L = (cf.IDS[i], name, k), f.pic, f.pic.table
        want_cap = cr.Picture.chosen(p, case.q, f.cap)
        assert f.q_i == want_cap
        if not f.filled:  # the floor, or nothing fits: cap_ref's picture
            assert f.q_i == case.q or not p.fits(f.q_i, f.cap), tag
            assert (f.qmap == f.q_i).all() and f.payload() == p.payload(f.q_i), tag
            continue
        at, below = f.len_at, f.len_below
        # a slice's length never grows with the index, and an empty slice is its header
        assert all(b is None or b >= a >= empty for a, b in zip(at, below)), tag
        # the tiles' lengths are the picture's: their sum is the ConstQ payload's length, at q_i and (where it codes) below
        assert sum(at) == L[f.q_i], tag
        assert (L[f.q_i - 1] is cr.NOT_CODABLE) == (None in below), tag
        if None not in below:
            assert sum(below) == L[f.q_i - 1] > f.cap, tag
        assert f.spare == f.cap - L[f.q_i] >= 0, tag
        # the promoted slices: a prefix of the visit order among the eligible ones, as long as the cap allows
        eligible = [s for s in f.order if f.eligible[s]]
        assert f.promoted == eligible[:len(f.promoted)], tag
        spent = sum(f.cost[s] for s in f.promoted)
        pay = f.payload()
        assert len(pay) == L[f.q_i] + spent and L[f.q_i] <= len(pay) <= f.cap, tag
        if len(f.promoted) < len(eligible):
            assert L[f.q_i] + spent + f.cost[eligible[len(f.promoted)]] > f.cap, tag
        else:
            assert None in below, (tag, "every slice promoted: the picture fits at q_i - 1")
        # the payload carries the map
        assert cf.slice_indices(pay, ns, case.prefix, case.scalar) == list(f.qmap.reshape(-1)), tag
        assert sorted(f.promoted) == [s for s in range(ns) if f.qmap.reshape(-1)[s] == f.q_i - 1], tag
        print(cf.IDS[i], name, k, "q_i", f.q_i, "spare", f.spare, "ineligible", below.count(None), "promoted", len(f.promoted), "of", ns,
              "bytes", len(pay), "cap", f.cap)


def test_the_matrix_holds_the_hard_cases(oracle):
    """once over the matrix: ineligible slices, spare 0 with promotions, 0 and ns - 1 promoted, and in every row a picture with a
    mixed map (one slice per picture, row WHOLE_PLANE: a filled picture, whose one slice is either promoted or not)"""
    seen = set()
    for i in ROWS:
        case, fills = _fills(oracle, i)
        ns = case.ys * case.xs
        filled = [f for _, _, f in fills if f.filled]
        assert filled, cf.IDS[i]
        if ns > 1:
            assert any(0 < len(f.promoted) < ns for f in filled), cf.IDS[i]
        for f in filled:
            if None in f.len_below:
                seen.add("ineligible")
            if f.spare == 0 and f.promoted:
                seen.add("spare 0")
            if not f.promoted:
                seen.add("none promoted")
            if ns > 1 and len(f.promoted) == ns - 1:
                seen.add("all but one")
    assert seen == {"ineligible", "spare 0", "none promoted", "all but one"}, seen


def test_what_the_prototype_found(oracle):
    """the figures of DESIGN.md section 28: (row, cap, picture) -> what the definition gives there"""
    def at(i, name, k):
        case, pics = cf.batch(oracle, i)
        return case, cf.fill(pics[k], case.q, cf.caps(case, pics[0])[name][0])

    case, f = at(0, "floor", 2)      # the half-noise picture: not codable as a whole at 27, filled all the same
    assert f.q_i == 28 and f.pic.table[27] is cr.NOT_CODABLE and f.len_below.count(None) == 55
    assert (len(f.promoted), len(f.payload()), f.cap) == (683, 591084, 591106)
    case, f = at(0, "empty", 0)
    assert f.filled and f.spare == 0 and len(f.promoted) == 32 and all(f.cost[s] == 0 for s in f.promoted)
    assert len(at(0, "mid-1", 0)[1].promoted) == 1023
    assert at(2, "mid", 0)[1].filled and len(at(2, "mid", 0)[1].promoted) == 0
    assert len(at(3, "mid", 0)[1].promoted) == 1
    assert [(f.spare, len(f.promoted)) for f in (at(cf.NEW, "floor", 1)[1], at(cf.NEW, "floor", 2)[1])] == [(18162, 1284), (10733, 850)]
    f = at(cf.NEW, "empty", 1)[1]
    assert (f.spare, len(f.promoted)) == (0, 234)


def test_mode_4_in_the_header_and_the_binding():
    import vc2hip_py
    text = open(os.path.join(ROOT, "include", "vc2hip.h")).read()
    assert re.search(r"VC2HIP_HQ_CAPPED_FILL\s*=\s*4\b", text)
    assert vc2hip_py.MODES["HQ_CappedFill"] == cf.MODE == 4 and vc2hip_py.MODES["HQ_Capped"] == 3


@pytest.mark.parametrize("prefix,scalar", [(0, 1), (3, 4)])
def test_calls_that_do_not_encode_read_the_mode_as_constq(prefix, scalar):
    """vc2hip_max_payload_bytes and vc2hip_picture_header (host arithmetic, no device): mode 4 = mode 0"""
    import vc2hip_py
    lib = pr._hip_lib()
    fmt = vc2hip_py.picture_format(1024, 64, "422", 10)
    const = vc2hip_py.coding_params(lib, fmt, "DD97", 4, 1, 2, mode="HQ_ConstQ", q=9, prefix=prefix, scalar=scalar)
    fill = vc2hip_py.coding_params(lib, fmt, "DD97", 4, 1, 2, mode="HQ_ConstQ", q=9, s=12345, prefix=prefix, scalar=scalar)
    fill.mode = cf.MODE
    lib.vc2hip_max_payload_bytes.restype = C.c_size_t
    assert lib.vc2hip_max_payload_bytes(C.byref(fmt), C.byref(fill)) == lib.vc2hip_max_payload_bytes(C.byref(fmt), C.byref(const)) \
        == const.y_slices * const.x_slices * (prefix + 4 + 3 * 255 * scalar)
    for major in (2, 3):
        assert vc2hip_py.picture_header(lib, fill, major, 7) == vc2hip_py.picture_header(lib, const, major, 7)
