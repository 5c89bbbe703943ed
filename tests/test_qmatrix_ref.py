"""CPU checks of tests/qmatrix_ref.py and of the two host functions behind it (vc2hip_picture_header_qm,
vc2hip_parse_picture_header: host arithmetic, like the calls of tests/test_abi.py -- no GPU is touched)."""
import ctypes as C

import numpy as np
import pytest

import cap_ref as cr
import proxy_ref as pr
import qmatrix_ref as qr
import transcode_cbr_ref as tcr
import transcode_ref as tr
from vc2lib import KERNELS

EINVAL, ESYNTAX = -1, -12

HEADERS = [("DD97", 3, "422", 512, 64, 1, 2, dict(q=8, scalar=2)),
           ("Haar0", 4, "444", 256, 64, 1, 1, dict(q=2, scalar=6, prefix=1)),
           ("Haar0", 1, "420", 128, 32, 2, 2, dict(q=0)),
           ("LeGall", 3, "422", 512, 64, 1, 2, dict(mode="LD", s=12000))]


@pytest.fixture(scope="module")
def lib():
    import vc2hip_py
    return vc2hip_py.load_library()


def _case(oracle, row):
    kernel, depth, cf, w, h, u, a, kw = row
    return pr.Case(oracle, w, h, cf, 10 if cf != "420" else 8, kernel, depth, u, a, word_bytes=2 if cf != "420" else 1, **kw)


def test_bound_symbols():
    import vc2hip_py
    for name in ("vc2hip_set_quant_matrix", "vc2hip_get_quant_matrix", "vc2hip_picture_header_qm", "vc2hip_parse_picture_header"):
        assert name in vc2hip_py.EXPORTS


@pytest.mark.parametrize("major", [2, 3])
def test_clear_flag_is_the_oracles_header(oracle, lib, major):
    """the model without a matrix against the header of the oracle's own stream (vc2o_write_hq_picture_header's bytes, which
    proxy_ref.oracle_payloads finds in front of every payload) and against vc2hip_picture_header"""
    import vc2hip_py
    from synth import synth
    for row in HEADERS[:3]:
        case = _case(oracle, row)
        _, cp = case.fmt_cp(lib)
        raw = synth(case.w, case.h, case.cf, case.bits, 3, word_bytes=case.word_bytes)
        stream = oracle.encode_stream(case.params(), raw, 1)
        if pr._major(stream) != major:
            continue
        unit = stream[int.from_bytes(stream[5:9], "big"):]
        assert unit[4] == 0xE8
        want = qr.picture_header(cp, major, 0)
        assert unit[13:13 + len(want)] == want
    for row in HEADERS:
        case = _case(oracle, row)
        _, cp = case.fmt_cp(lib)
        for number in (0, 7, 0xFFFFFFFE):
            assert qr.picture_header(cp, major, number) == vc2hip_py.picture_header(lib, cp, major, number)


@pytest.mark.parametrize("major", [2, 3])
def test_header_functions_agree_with_the_model_and_round_trip(oracle, lib, major):
    import vc2hip_py
    for row in HEADERS:
        case = _case(oracle, row)
        _, cp = case.fmt_cp(lib)
        ld = case.mode == "LD"
        for name in qr.MATRICES:
            qm = qr.matrix(oracle, name, case.kernel, case.depth)
            got = vc2hip_py.picture_header(lib, cp, major, 5, matrix=qm)
            assert got == qr.picture_header(cp, major, 5, qm), (row, name)
            back, m, used = vc2hip_py.parse_picture_header(lib, got + b"\x5a" * 9, major, ld)
            model = qr.parse_picture_header(got + b"\x5a" * 9, major, ld)
            assert used == len(got) == model["used"] and m == qm.tolist() == model["matrix"]
            assert (back.kernel, back.depth, back.y_slices, back.x_slices) == (cp.kernel, cp.depth, cp.y_slices, cp.x_slices)
            if ld:
                assert back.mode == 2 and back.compressed_bytes == cp.compressed_bytes
            else:
                assert (back.prefix, back.scalar) == (cp.prefix, cp.scalar)
        plain = vc2hip_py.picture_header(lib, cp, major, 5)
        back, m, used = vc2hip_py.parse_picture_header(lib, plain, major, ld)
        assert m is None and used == len(plain) and back.depth == cp.depth


def test_header_refusals(oracle, lib):
    import vc2hip_py
    case = _case(oracle, HEADERS[0])
    _, cp = case.fmt_cp(lib)
    qm = qr.matrix(oracle, "ragged", case.kernel, case.depth)
    good = qr.picture_header(cp, 3, 1, qm)

    def refused(data, major=3):
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            vc2hip_py.parse_picture_header(lib, data, major)
        return e.value.code

    for cut in range(len(good)):                                   # every truncation
        assert refused(good[:cut]) == ESYNTAX, cut
        with pytest.raises(ValueError):
            qr.parse_picture_header(good[:cut], 3, False)
    big = qm.copy()
    big[4] = 256
    assert refused(qr.picture_header(cp, 3, 1, big)) == ESYNTAX
    assert refused(qr.picture_header(cp, 3, 1, qm, asym=(1, 0))) == ESYNTAX
    assert refused(qr.picture_header(cp, 3, 1, qm, asym=(0, 1))) == ESYNTAX
    for bad in (big, np.append(qm, 0), qm[:-3], np.where(np.arange(qm.size) == 2, -1, qm)):   # the writer: EINVAL
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            vc2hip_py.picture_header(lib, cp, 3, 1, matrix=bad)
        assert e.value.code == EINVAL


@pytest.mark.parametrize("name", ["A", "E", "G"])
def test_default_matrix_compositions_are_the_existing_ones(oracle, name):
    """encode, decode and the two transcodes with the default matrix passed explicitly against proxy_ref, transcode_ref and
    transcode_cbr_ref, which take it from the oracle themselves"""
    case = tr.matrix_case(oracle, name)
    qm = qr.matrix(oracle, "default", case.kernel, case.depth)
    raw = cr.pictures(case)[1]
    pay, q = qr.encode(oracle, case, raw, qm)
    assert pay == pr.oracle_payloads(oracle, case, raw, 1)[0]
    assert qr.decode(oracle, case, pay, qm) == pr.full_picture(oracle, case, pay)
    if case.depth > 1:
        assert qr.decode(oracle, case, pay, qm, 1) == pr.reduced_picture(oracle, case, pay, 1)
    mine, theirs = qr.Coded(oracle, case, pay, qm), tr.Coded(oracle, case, pay)
    for t in (0, int(q.min()) + 3, 40):
        assert mine.transcode(t) == theirs.transcode(t)
    s_out = tcr.budget_mixed(case, [theirs] * 3, case.scalar)
    assert tcr.Out(oracle, mine, s_out, case.prefix, case.scalar).payload == tcr.Out(oracle, theirs, s_out, case.prefix, case.scalar).payload


def test_the_compositions_refuse_exactly_where_they_are_meant_to(oracle):
    """every row of the GPU tests under every matrix, all three pictures: the composition codes the picture, but for the pairs
    of qr.REFUSES, which refuse every picture with the stated code.  Under `edge` the HQ_CBR and LD searches are compared
    positively on rows E2 and L2, whose budgets they meet with indices above 0; row G's matrices change its bytes"""
    refused, lengths = {}, {}
    for name in qr.ROWS:
        case = qr.case_of(oracle, name)
        for mname in qr.MATRICES:
            qm = qr.matrix(oracle, mname, case.kernel, case.depth)
            codes = set()
            for raw in cr.pictures(case):
                try:
                    pay, q = qr.encode(oracle, case, raw, qm)
                    codes.add(None)
                    lengths.setdefault((name, mname), []).append((len(pay), int(q.max())))
                except qr.OracleError as e:
                    codes.add(e.code)
            if codes != {None}:
                assert len(codes) == 1, (name, mname, "some pictures refuse and some do not", codes)
                refused[(name, mname)] = codes.pop()
    assert refused == qr.REFUSES
    for name in ("E2", "L2"):
        assert max(q for _, q in lengths[(name, "edge")]) > 0, (name, "the search under `edge` never leaves index 0")
    assert len({tuple(lengths[("G", m)]) for m in qr.MATRICES}) > 1, "row G's bytes do not depend on the matrix"


def test_capped_default_matrix_is_cap_refs_choice(oracle):
    case = tr.matrix_case(oracle, "A")
    qm = qr.matrix(oracle, "default", case.kernel, case.depth)
    raw = cr.pictures(case)[1]
    full, _ = qr.encode(oracle, case, raw, qm)
    pay, t = qr.encode_capped(oracle, case, raw, qm, case.q, len(full) // 2)
    assert t > case.q and len(pay) <= len(full) // 2
    lower, _ = qr.encode(oracle, pr.Case(oracle, case.w, case.h, case.cf, case.bits, case.kernel, case.depth, case.u, case.a,
                                         q=t - 1, scalar=case.scalar, word_bytes=case.word_bytes), raw, qm)
    assert len(lower) > len(full) // 2
    assert qr.encode_capped(oracle, case, raw, qm, case.q, len(full))[1] == case.q


def test_ld_default_matrix_is_the_oracles_stream(oracle):
    case = pr.Case(oracle, 512, 64, "422", 10, "LeGall", 3, 1, 2, mode="LD", s=12000)
    from synth import synth
    raw = synth(case.w, case.h, case.cf, case.bits, 11)
    qm = qr.matrix(oracle, "default", case.kernel, case.depth)
    pay, _ = qr.encode(oracle, case, raw, qm)
    assert pay == pr.oracle_payloads(oracle, case, raw, 1)[0]
    assert qr.decode(oracle, case, pay, qm) == pr.full_picture(oracle, case, pay)
