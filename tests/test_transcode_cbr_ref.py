"""tests/transcode_cbr_ref.py on the CPU: the facts the GPU tests of vc2hip_transcode_cbr_batch_dev rely on (DESIGN.md
section 24).  need_s is pinned against the length bytes the oracle's slice writer writes; the keep rule makes the call stable
across generations (a second transcode keeps every slice and returns the same bytes, an HQ_CBR input comes back from its own
budget byte for byte, no searched slice ends finer than it came); and the budgets the GPU tests use exercise both kinds of
slice, so that no GPU comparison passes on inputs that exercise nothing."""
import numpy as np
import pytest

import proxy_ref as pr
import transcode_cbr_ref as tc
import transcode_ref as tr
from vc2lib import OracleError

BUDGETS = ("mixed", "roomy", "tight")


@pytest.fixture(scope="module")
def rows(oracle):
    return {name: tr.batch(oracle, name) for name in tr.ROWS}


def output_case(oracle, case, s_out, prefix, scalar):
    """the row's geometry coded as the call's output is"""
    return pr.Case(oracle, case.w, case.h, case.cf, case.bits, case.kernel, case.depth, case.u, case.a, mode="HQ_CBR", s=s_out,
                   scalar=scalar, prefix=prefix, word_bytes=case.word_bytes)


def test_binding_and_header_declare_the_call():
    import os
    import vc2hip_py
    assert "vc2hip_transcode_cbr_batch_dev" in vc2hip_py.EXPORTS
    assert hasattr(vc2hip_py.Vc2Hip, "transcode_cbr_batch_dev")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vc2hip.h")).read()
    assert "int vc2hip_transcode_cbr_batch_dev(" in header


@pytest.mark.parametrize("name", tr.ROWS)
def test_need_is_what_the_slice_writer_writes(oracle, rows, name):
    """the length bytes of oracle.hq_pack (VBR, prefix 0, the output scalar) on every row, at the row's scalar and twice it"""
    case, pics = rows[name]
    for scalar in (case.scalar, 2 * case.scalar):
        for k, p in enumerate(pics):
            want = tc.written_length_bytes(oracle, case, p.planes, p.q, scalar)
            got = np.stack([tc.component_length_bytes(case, c, scalar) for c in p.planes])
            assert (got == want).all(), (name, k, scalar)
            need, codable = tc.slice_need(case, p.planes, scalar)
            assert codable.all() and (need == want.sum(axis=0) * scalar).all(), (name, k, scalar)


def test_need_marks_what_the_slice_writer_refuses(oracle, rows):
    """row H's values at scalar 1: a component beyond 255 bytes is not codable, and the oracle's writer refuses the picture"""
    case, pics = rows["H"]
    lens = [tc.component_length_bytes(case, c, 1) for c in pics[1].planes]
    assert max(int(l.max()) for l in lens) > 255
    assert not tc.slice_need(case, pics[1].planes, 1)[1].all()
    with pytest.raises(OracleError) as e:
        oracle.hq_pack(*pics[1].planes, case.depth, pics[1].q, 0, 1)
    assert e.value.code == tr.ESCALAR


def _outs(oracle, pics, s_out, prefix=None, scalar=None):
    return [tc.transcode_cbr(oracle, p, s_out, prefix, scalar) for p in pics]


@pytest.mark.parametrize("name", tc.ROWS_MIXED)
def test_mixed_budget_has_both_kinds_of_slice(oracle, rows, name):
    case, pics = rows[name]
    ns = case.ys * case.xs
    outs = _outs(oracle, pics, tc.budgets(oracle, name)["mixed"])
    assert not any(isinstance(o, OracleError) for o in outs), (name, outs)
    kept = int(outs[2].keep.sum())
    print(f"{name} mixed: picture 2 keeps {kept} of {ns}")
    assert 4 * kept >= ns and 4 * (ns - kept) >= ns, (name, kept, ns)


@pytest.mark.parametrize("name", tr.ROWS)
def test_roomy_budget_keeps_every_slice(oracle, rows, name):
    case, pics = rows[name]
    s_out = tc.budgets(oracle, name)["roomy"]
    for k, p in enumerate(pics):
        need, codable = tc.slice_need(case, p.planes, case.scalar)
        keep = codable & (need <= oracle.slice_bytes(case.ys, case.xs, s_out, case.scalar) - 4)
        assert keep.all(), (name, k)
    # the rule keeps every slice on every row; what the CBR writer makes of a kept slice is another matter: where a small
    # slice's V component has to fill a budget sized for the largest, its length byte passes 255 (row I by design, and the
    # smooth pictures of row F, whose one slice is sized for the noise picture's)
    outs = _outs(oracle, pics, s_out)
    refused = [k for k, o in enumerate(outs) if isinstance(o, OracleError)]
    assert all(outs[k].code == tc.ECBR_LEN for k in refused), (name, outs)
    assert refused == {"I": [0, 1, 2], "F": [0, 2]}.get(name, []), (name, refused)
    for k, (p, o) in enumerate(zip(pics, outs)):
        if k not in refused:
            assert o.keep.all() and (o.q == p.q).all() and all((a == b).all() for a, b in zip(o.planes, p.planes)), (name, k)


@pytest.mark.parametrize("name", [n for n in tr.ROWS if n != "I"])
def test_tight_budget_keeps_no_slice(oracle, rows, name):
    case, pics = rows[name]
    outs = _outs(oracle, pics, tc.budgets(oracle, name)["tight"])
    for k, o in enumerate(outs):
        assert not isinstance(o, OracleError), (name, k, o)
        assert not o.keep.any(), (name, k, int(o.keep.sum()))


@pytest.mark.parametrize("name", tc.ROWS_CHANGED)
def test_changed_prefix_and_scalar_still_have_both_kinds(oracle, rows, name):
    case, pics = rows[name]
    ns = case.ys * case.xs
    prefix, scalar = tc.changed(case)
    outs = _outs(oracle, pics, tc.budgets(oracle, name, scalar)["mixed"], prefix, scalar)
    assert not any(isinstance(o, OracleError) for o in outs), (name, outs)
    kept = int(outs[2].keep.sum())
    print(f"{name} prefix + 1, scalar x 2, mixed: picture 2 keeps {kept} of {ns}")
    assert 0 < kept < ns, (name, kept, ns)


def test_designed_refusals(oracle, rows):
    case, pics = rows["I"]
    o = tc.transcode_cbr(oracle, pics[0], tc.budgets(oracle, "I")["roomy"])
    assert isinstance(o, OracleError) and o.code == tc.ECBR_LEN, o
    case, pics = rows["F"]
    o = tc.transcode_cbr(oracle, pics[1], tc.budgets(oracle, "F")["mixed"])
    assert isinstance(o, OracleError) and o.code == tr.ESCALAR, o


@pytest.mark.parametrize("name", tr.ROWS)
def test_stable_across_generations(oracle, rows, name):
    """at three budgets a row: the output transcoded again to the same cp_out gives the same bytes, every slice kept the second
    time; and no searched slice ended at a finer index than it came with"""
    case, pics = rows[name]
    compared = 0
    for label, s_out in tc.budgets(oracle, name).items():
        for k, p in enumerate(pics):
            o = tc.transcode_cbr(oracle, p, s_out)
            if isinstance(o, OracleError):
                assert name in ("F", "I"), (name, label, k, o)      # (the designed refusals, and row F's one-slice search)
                continue
            assert (o.q >= p.q).all(), (name, label, k, "a searched slice ended finer than it came")
            assert (o.q[o.keep] == p.q[o.keep]).all()
            case2 = output_case(oracle, case, s_out, case.prefix, case.scalar)
            again = tc.Out(oracle, tr.Coded(oracle, case2, o.payload), s_out, case.prefix, case.scalar)
            assert again.keep.all(), (name, label, k, int(again.keep.sum()))
            assert again.payload == o.payload and (again.q == o.q).all(), (name, label, k)
            compared += 1
    assert compared >= (3 if name == "F" else 6), (name, compared)


def test_stable_across_generations_with_changed_prefix_and_scalar(oracle, rows):
    for name in tc.ROWS_CHANGED:
        case, pics = rows[name]
        prefix, scalar = tc.changed(case)
        s_out = tc.budgets(oracle, name, scalar)["mixed"]
        for k, p in enumerate(pics):
            o = tc.transcode_cbr(oracle, p, s_out, prefix, scalar)
            assert (o.q >= p.q).all(), (name, k)
            again = tc.Out(oracle, tr.Coded(oracle, output_case(oracle, case, s_out, prefix, scalar), o.payload), s_out, prefix, scalar)
            assert again.keep.all() and again.payload == o.payload, (name, k)


def test_hq_cbr_input_comes_back_from_its_own_budget(oracle, rows):
    case, pics = rows["E"]
    assert case.mode == "HQ_CBR"
    for k, p in enumerate(pics):
        o = tc.transcode_cbr(oracle, p, case.s)
        assert o.keep.all() and o.keep.size == 512, (k, int(o.keep.sum()))
        assert o.payload == p.payload, k


def test_zeroed_blocks_never_refuse_a_kept_slice(oracle, rows):
    """what entitles the definition to one whole-picture search: a kept slice's zeroed block raises nothing and its answer is
    never used -- the searched slices' indices are those of a search over the searched slices alone"""
    case, pics = rows["A"]
    p = pics[2]
    o = tc.transcode_cbr(oracle, p, tc.budgets(oracle, "A")["mixed"])
    whole = oracle.cbr_qindices(*p.deq, case.depth, p.qm, o.budgets, case.scalar)
    assert (whole[~o.keep] == o.q[~o.keep]).all()
