"""CPU checks of the definition of vc2hip_set_index_offsets (tests/roi_ref.py) and of the setter's place in the ABI.  No GPU
compute here.  (The refusals need a context, hence a device: they are in tests/test_gpu_roi.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

import cap_ref as cr
import capfill_ref as cf
import roi_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "vc2-reference_amd", "libvc2hip.so")
ROWS = range(len(rf.MATRIX))
CAPS = ("mid", "mid-1", "none")


def test_the_setter_is_exported_and_bound():
    import vc2hip_py
    lib = C.CDLL(LIB)
    assert hasattr(lib, "vc2hip_set_index_offsets"), "vc2hip_set_index_offsets is not exported"
    assert "vc2hip_set_index_offsets" in vc2hip_py.EXPORTS and hasattr(vc2hip_py.Vc2Hip, "set_index_offsets")
    text = open(os.path.join(ROOT, "include", "vc2hip.h")).read()
    assert "int vc2hip_set_index_offsets(vc2hip_ctx *ctx, const int8_t *d_offsets, size_t picture_stride);" in text


def test_the_patterns():
    assert rf.central(1) == (0, 1) and rf.central(8) == (2, 6) and rf.central(16) == (5, 11) and rf.central(95) == (31, 64)
    for ys, xs in ((1, 1), (8, 16), (17, 95)):
        ns = ys * xs
        for name in rf.PATTERNS + ("absolute",):
            o = rf.pattern(name, ys, xs)
            assert o.dtype == np.int8 and o.shape == (ns,)
        assert not rf.pattern("zero", ys, xs).any()
        ramp = rf.pattern("ramp", ys, xs).astype(int)
        assert list(ramp[:14]) == [(s % 13) - 6 for s in range(min(ns, 14))] and ramp.min() >= -6 and ramp.max() <= 6
        roi = rf.pattern("roi", ys, xs).reshape(ys, xs)
        assert set(roi.reshape(-1).tolist()) <= {-6, 4} and roi[ys // 2, xs // 2] == -6 and (ns == 1 or roi[0, 0] == 4)
        ext = rf.pattern("extremes", ys, xs).reshape(ys, xs)
        assert ext[0, 0] == -128 and (xs == 1 or ext[0, 1] == 127)
        a = rf.pattern("absolute", ys, xs)
        assert a.min() >= 0 and a.max() <= rf.Q_TOP and (ns < 116 or set(a.tolist()) == set(range(116)))
    assert list(rf.eff(10, np.array([-128, -11, -10, 0, 105, 106, 127], np.int8))) == [0, 0, 0, 10, 115, 115, 115]


@pytest.mark.parametrize("i", ROWS, ids=rf.IDS)
def test_the_definition_on_every_pattern(oracle, i):
    case, pics = cf.batch(oracle, i)
    caps = cf.caps(case, pics[0])
    ns, floor = case.ys * case.xs, case.q
    for name in rf.PATTERNS:
        for k in range(3):
            tag = (rf.IDS[i], name, k)
            m = rf.mapped(oracle, i, name, k)
            L = [m.length(b) for b in range(floor, rf.Q_TOP + 1)]
            # the length never grows with the base, and a base that codes is followed by bases that code
            for x, y in zip(L, L[1:]):
                assert x is rf.NOT_CODABLE or (y is not rf.NOT_CODABLE and y <= x), tag
            if name == "zero":
                assert L == pics[k].table[floor:], tag
            for cname in CAPS:
                cap = caps[cname][0]
                b = m.base(floor, cap)
                pay = m.payload(b)
                if name == "zero":
                    assert b == pics[k].chosen(floor, cap) and pay == pics[k].payload(b), (tag, cname)
                if any(m.fits(x, cap) for x in range(floor, rf.Q_TOP + 1)):
                    assert len(pay) <= cap and (b == floor or not m.fits(b - 1, cap)), (tag, cname)
                else:
                    assert b == rf.Q_TOP, (tag, cname)
                if pay is not rf.NOT_CODABLE:       # the payload carries the map
                    assert cf.slice_indices(pay, ns, case.prefix, case.scalar) == list(m.qmap(b).reshape(-1)), (tag, cname)
                f = rf.fill(m, floor, cap)
                assert f.b_i == b, (tag, cname)
                if name == "zero":
                    g = cf.fill(pics[k], floor, cap)
                    assert (f.qmap == g.qmap).all() and f.payload() == g.payload() and f.promoted == g.promoted, (tag, cname)
                if f.filled:
                    fp = f.payload()
                    assert m.length(b) <= len(fp) <= cap, (tag, cname)
                    assert len(fp) == m.length(b) + sum(f.cost[s] for s in f.promoted), (tag, cname)
                    assert cf.slice_indices(fp, ns, case.prefix, case.scalar) == list(f.qmap.reshape(-1)), (tag, cname)
                    below = m.qmap(b - 1).reshape(-1)
                    assert all(f.cost[s] == 0 for s in range(ns) if below[s] == m.qmap(b).reshape(-1)[s]), (tag, cname)
                else:
                    assert (f.qmap == m.qmap(b)).all(), (tag, cname)
            if name == "extremes" and ns > 1:
                q = m.qmap(floor).reshape(-1)
                assert q.min() == 0 and q.max() == rf.Q_TOP and (m.qmap(rf.Q_TOP) == m.qmap(floor)).all(), tag


def test_which_pictures_the_oracle_refuses_under_constq(oracle):
    """at most one picture per row and pattern outside `extremes` and `absolute` (roi_ref.CONSTQ_RAISED: rows 0, 1 and 2 run
    above floor + 12 for it); the refused ones of `extremes` are what tests/test_gpu_roi.py leaves out of its batches"""
    found = {}
    for i in ROWS:
        for name in ("ramp", "roi", "extremes", "absolute"):
            r = rf.refused(oracle, i, name, 0)
            if name in ("ramp", "roi"):
                assert len(r) <= 1, (rf.IDS[i], name, r)
            if r:
                found[(i, name)] = r
        floor = rf.MATRIX[i][9]["floor"]
        assert rf.constq_index(i) - 6 >= floor + 6 and rf.constq_index(i) + 6 <= rf.Q_TOP
    # the figures of DESIGN.md section 30: index 0 in half the slices is beyond the noise pictures wherever a length byte can
    # pass 255 (rows 0 and 1: beyond the smooth picture too); row 7's 16-bit pictures quantise beyond 65534 there
    assert found == {(0, "extremes"): [0, 1, 2], (0, "absolute"): [0, 1, 2], (1, "extremes"): [0, 1, 2], (1, "absolute"): [0, 1, 2],
                     (2, "extremes"): [1, 2], (2, "absolute"): [1, 2], (7, "extremes"): [0, 1, 2], (7, "absolute"): [0, 1, 2],
                     (8, "extremes"): [1, 2], (8, "absolute"): [1, 2],
                     (10, "extremes"): [1, 2], (10, "absolute"): [1, 2]}, found
    assert 1 in rf.refused(oracle, 1, "extremes", 0)    # the picture test_gpu_roi.py::test_a_refused_picture codes alone


def test_what_the_definition_found(oracle):
    """the figures of DESIGN.md section 30: (row, pattern, picture) under the cap mid-1 -> base, promoted slices, bytes, cap"""
    def at(i, name, k):
        case, pics = cf.batch(oracle, i)
        f = rf.fill(rf.mapped(oracle, i, name, k), case.q, cf.caps(case, pics[0])["mid-1"][0])
        return f.b_i, len(f.promoted), len(f.payload()), f.cap

    assert at(0, "ramp", 0) == (38, 260, 9602, 9611) and at(0, "roi", 1) == (56, 869, 9592, 9611)
    assert at(1, "ramp", 0) == (39, 159, 3606, 3606)                      # the cap met to the byte
    assert at(2, "ramp", 1) == (48, 4, 6393, 6393) and at(2, "roi", 0) == (28, 181, 6392, 6393)
    assert at(8, "ramp", 0) == (36, 0, 25204, 27603)                      # one slice per picture: filled, nothing promoted
    assert at(rf.NEW, "ramp", 0) == (33, 1482, 23443, 23451) and at(rf.NEW, "roi", 2) == (45, 1588, 23451, 23451)
    # `extremes` does not move with the base: under every cap the base is 115 and the picture, where it codes, is the ConstQ one
    case, pics = cf.batch(oracle, 3)
    m = rf.mapped(oracle, 3, "extremes", 0)
    assert m.base(case.q, cf.caps(case, pics[0])["mid"][0]) == rf.Q_TOP and m.length(rf.Q_TOP) == m.length(case.q) == 21386
