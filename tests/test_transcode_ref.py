"""tests/transcode_ref.py on the CPU: the facts the GPU path of vc2hip_transcode_batch_dev relies on,
for every row of the matrix and each of its three pictures -- the table of lengths never grows with the target (so a
bracketing search finds the definition's index), the kept-slice rule agrees with blind requantisation up to index 115, no
coefficient grows, the composition never refuses a payload an encoder wrote, and the two ends of the table are the input
itself and the empty picture."""
import numpy as np
import pytest

import transcode_ref as tr


@pytest.fixture(scope="module")
def rows(oracle):
    return {name: tr.batch(oracle, name) for name in tr.ROWS}


def test_binding_and_header_declare_the_call():
    import vc2hip_py
    assert "vc2hip_transcode_batch_dev" in vc2hip_py.EXPORTS
    tp = vc2hip_py.transcode_params(24)
    assert (tp.q_index, tp.cap_bytes) == (24, 0)
    assert vc2hip_py.transcode_params(3, 1000).cap_bytes == 1000
    assert hasattr(vc2hip_py.Vc2Hip, "transcode_batch_dev")


@pytest.mark.parametrize("name", tr.ROWS)
def test_inputs_are_what_the_rows_say(rows, name):
    case, pics = rows[name]
    kw = tr.MATRIX[name][9]
    for p in pics:
        assert p.in_domain
        if case.mode == "HQ_CBR":
            budget = int(p.oracle.slice_bytes(case.ys, case.xs, case.s, case.scalar).sum()) + case.ys * case.xs * case.prefix
            assert len(p.payload) == budget <= case.s and len(set(p.q.ravel().tolist())) > 1
        elif "checker" in kw:
            assert sorted(set(p.q.ravel().tolist())) == sorted(kw["checker"])
            assert p.q[0, 0] != p.q[0, 1] and p.q[0, 0] != p.q[1, 0]
        else:
            assert (p.q == case.q).all()
    if name == "E":
        qs = np.concatenate([p.q.ravel() for p in pics])
        assert qs.min() <= 18 and qs.max() >= 40, (qs.min(), qs.max())
    if name == "F":
        assert case.ys * case.xs == 1
    if name == "G":
        assert (case.cph // case.ys) * (case.cpw // case.xs) == 4 and (case.ph // case.ys) * (case.pw // case.xs) == 16
    if name == "H":
        assert max(int(np.abs(c).max()) for p in pics for c in p.planes) >= 5000


@pytest.mark.parametrize("name", tr.ROWS)
def test_tables_are_monotonic_and_codable(rows, name):
    case, pics = rows[name]
    for k, p in enumerate(pics):
        L = p.table()
        assert all(x is not tr.NOT_CODABLE for x in L), (name, k, "the composition refused a payload an encoder wrote")
        assert all(L[t] <= L[t - 1] for t in range(1, tr.Q_TOP + 1)), (name, k)
        assert len(set(L)) - 1 >= 14, (name, k, "fewer than 14 distinct drops")
        assert L[tr.Q_TOP] == tr.empty_bytes(case), (name, k)
        assert p.transcode(tr.Q_TOP) == _empty_picture(case, p), (name, k)


def _empty_picture(case, p):
    out = bytearray()
    for q in np.maximum(p.q, tr.Q_TOP).ravel():
        out += bytes(case.prefix) + bytes([int(q), 0, 0, 0])
    return bytes(out)


@pytest.mark.parametrize("name", tr.ROWS)
def test_low_targets_give_the_input(rows, name):
    case, pics = rows[name]
    for k, p in enumerate(pics):
        lo = int(p.q.min())
        for t in sorted({0, lo // 2, lo}):
            got = p.transcode(t)
            if case.mode == "HQ_CBR":
                assert len(got) < len(p.payload), (name, k, t)     # the input without its padding
                assert got == p.transcode(0)
                assert (tr.Coded(p.oracle, case, got).q == p.q).all()
                assert all((a == b).all() for a, b in zip(tr.Coded(p.oracle, case, got).planes, p.planes))
            else:
                assert got == p.payload, (name, k, t)


@pytest.mark.parametrize("name", tr.ROWS)
def test_kept_rule_is_blind_requantisation_and_nothing_grows(rows, name):
    case, pics = rows[name]
    for k, p in enumerate(pics):
        for t in range(tr.Q_TOP + 1):
            y, u, v, q2 = p.requantised(t)
            yb, ub, vb, _ = p.requantised(t, blind=True)
            for a, b, c in zip((y, u, v), (yb, ub, vb), p.planes):
                assert (a == b).all(), (name, k, t, "kept slices differ from quantise(dequantise(c, q), q)")
                assert (np.abs(a) <= np.abs(c)).all(), (name, k, t, "a coefficient grew")
            assert (q2 >= p.q).all() and (q2 >= t).all()


@pytest.mark.parametrize("name", tr.ROWS)
def test_caps_exhaustive_choice_is_bisection(rows, name):
    case, pics = rows[name]
    floor = tr.floor_of(pics)
    caps = tr.caps(pics[0], floor)
    for cname, (cap, want0) in caps.items():
        chosen = [p.chosen(floor, cap) for p in pics]
        assert chosen == [p.bisected(floor, cap) for p in pics], (name, cname)
        assert chosen[0] == want0, (name, cname, chosen, want0)
        if cname == "mid":
            assert len(set(chosen)) >= 2, (name, chosen)
        if cname == "none":
            assert chosen == [tr.Q_TOP] * 3 and all(len(p.transcode(tr.Q_TOP)) > cap for p in pics)
    for p in pics:      # a floor above the smallest index, caps from every eighth entry of the picture's own table
        L = p.table()
        for fl in (floor + 3, 60):
            for cap in sorted({L[t] for t in range(fl, tr.Q_TOP + 1, 8)} | {L[fl] + 1, 1}):
                assert p.chosen(fl, cap) == p.bisected(fl, cap), (name, fl, cap)


@pytest.mark.parametrize("name,refused_want", [("A", {"random": 1, "length": 70, "short": 6}), ("B2", {"random": 2, "length": 57, "short": 6})])
def test_damaged_inputs_keep_the_gpu_comparison_from_being_empty(oracle, name, refused_want):
    """tests/damage.py inputs A and B2 at target = the input's index + 6: what the composition refuses it refuses with
    ESTREAM or EQINDEX, and enough of every class lies in the encoder's domain for the byte comparison to carry weight"""
    import damage as dm
    base, _ = dm.load(oracle, name)
    case = base.case
    t = case.q + 6
    share = {"boundary": 1.0, "long": 1.0, "runff": 1.0, "random": 2 / 3, "run00": 0.5}
    for cls in dm.input_classes(name):
        refs = [tr.damaged_reference(oracle, case, dm.visible(base, m), t) for m in dm.input_mutations(base, name, cls)]
        refused = [r for r in refs if r[0] == "refused"]
        inside = [r for r in refs if r[0] == "ok" and r[3]]
        print(f"{name} {cls}: {len(refs)} mutations, {len(inside)} in domain, {len(refused)} refused")
        assert all(r[1] in (tr.ESTREAM, tr.EQINDEX) for r in refused), (name, cls, sorted({r[1] for r in refused}))
        if cls in share:
            assert len(inside) >= share[cls] * len(refs) - 1e-9, (name, cls, len(inside), len(refs))
        if cls in refused_want:
            assert len(refused) == refused_want[cls], (name, cls, len(refused))
    clean = tr.damaged_reference(oracle, case, base.payload, t)
    assert clean[0] == "ok" and clean[3] and len(clean[1]) < len(base.payload)


def test_fixed_targets_cover_a_drop(rows):
    for name in tr.ROWS:
        case, pics = rows[name]
        ts = tr.fixed_targets(pics)
        assert 0 in ts and tr.Q_TOP in ts and 4 <= len(ts) <= 5, (name, ts)
        mid = tr.mid_target(pics[0], tr.floor_of(pics))
        assert len(pics[0].transcode(mid)) < len(pics[0].transcode(mid - 1))
