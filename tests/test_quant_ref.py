"""CPU tests of tests/quant_ref.py: the Python definition of quant / scale equals the oracle on every designed value; the
claims the library's quantiser copies rest on hold (the float form is exact below 2^20 and first fails at 1 761 441, index
23; the reciprocal-multiply form is exact on every boundary dividend); every designed picture transforms back to its design
inside its sample range; the designs reach every copy at every index its domain holds (hand-written minimums); and wrong
copies of the models are caught by a designed value each, where the seeded uniform nets of tests/test_gpu_parity.py alone
see nothing."""
import numpy as np
import pytest

import cbr_ref as cr
import quant_ref as qr

QM0 = np.zeros(7, np.int32)


# ---- the definition against the second witness
def test_table_and_offsets_are_the_oracle_s(oracle):
    for q in range(120):
        assert qr.QF[q] == oracle.quant_factor(q)
        assert qr.scale(1, q) == oracle.scale(1, q) and qr.scale(-1, q) == oracle.scale(-1, q)   # (carries the offset)
    assert [q for q in range(120) if qr.QF[q] < 0] == [116, 117, 118, 119]
    with pytest.raises(ValueError, match="quantization index exceeds maximum implemented value."):
        qr.quant_factor(120)
    with pytest.raises(Exception, match="quantization index exceeds maximum implemented value."):
        oracle.quant_factor(120)


def test_wrapped_dividends_are_defined_by_the_oracle(oracle):
    """|v| >= 2^29: (|v| << 2) wraps as a C int.  The oracle computes it in unsigned arithmetic and divides as int: every such
    value has ONE result, which the definition must give -- asserted before any of them is designed into a sheet"""
    edges = [v for v in qr.domain_edges(0) if abs(v) >= qr.INT_GUARD]
    assert len(edges) >= 13 and -(1 << 31) in edges and (1 << 31) - 1 in edges
    for q in (0, 1, 23, 59, 60, 115, 116, 117, 118, 119):
        for v in edges:
            assert qr.quant(v, q) == oracle.quant(v, q), (v, q)
            assert qr.scale(v, q) == oracle.scale(v, q), (v, q)


def test_definition_equals_oracle_on_every_designed_value(oracle):
    n = 0
    for q in range(120):
        for v in qr.sheet_values(q):
            assert qr.quant(v, q) == oracle.quant(v, q), (v, q)
            n += 1
        for v in qr.dequant_values(q):
            assert qr.scale(v, q) == oracle.scale(v, q), (v, q)
        for d in qr.designed(q, qr.INT_GUARD - 1):
            assert qr.quant(d.v, q) == d.want, d
    assert n > 15000


def test_sheets_hold_every_value_and_equal_the_oracle_s_planes(oracle):
    mixed, slow = qr.quant_sheets()
    qi = qr.sheet_qidx()
    seen = [set() for _ in range(120)]
    for p in mixed + slow:
        want = qr.sheet_want(p, qr.quant_np)
        assert np.array_equal(oracle.quantise_np(p, qr.SHEET_DEPTH, qi, QM0), want)
        rec = p.reshape(qr.SHEET_YS, qr.SHEET_SH, qr.SHEET_XS, qr.SHEET_SW).transpose(0, 2, 1, 3).reshape(120, -1)
        for q in range(120):
            seen[q] |= set(rec[q].tolist())
    for q in range(120):
        assert set(qr.sheet_values(q)) <= seen[q], q
    for p in slow:       # every lane of every wavefront on the literal division
        a = (np.abs(p.astype(np.int64)) << 2) & 0xFFFFFFFF
        assert (a >= 1 << 31).all()
    for p in qr.dequant_sheets():
        want = qr.sheet_want(p, qr.scale_np)
        assert np.array_equal(oracle.dequantise_np(p, qr.SHEET_DEPTH, qi, QM0), want)


def test_dequantiser_values_sit_on_the_fused_limits():
    for q in (0, 1, 23, 59, 100, 115):
        a, b = qr.fused_limits(q)
        vals = set(qr.dequant_values(q))
        for lim in (a, b):
            if lim > 0:
                assert {lim - 1, lim, lim + 1, -lim} <= vals
                # the limit is the last magnitude whose |v| * qf + offset + 2 stays inside the form's range
        assert a == -1 or (a * qr.QF[q] + qr.OFF[q] + 2 <= 0x7FFFFFFF < (a + 1) * qr.QF[q] + qr.OFF[q] + 2)
        m = -(-((1 << 31) - qr.OFF[q]) // qr.QF[q])
        assert (m - 1) * qr.QF[q] + qr.OFF[q] < 1 << 31 <= m * qr.QF[q] + qr.OFF[q] and {m - 1, m, m + 1} <= vals
    assert qr.fused_limits(116) == (-1, -1)


# ---- the float claim
def test_float_form_is_exact_below_two_to_the_twenty_exhaustively():
    """for every index 0 .. 115 and every |v| < 2^20 the float32 product with the rounded-up reciprocal truncates to the
    integer quotient (what load8_tab, the cap's measure and the register searches rely on)"""
    mag = np.arange(qr.FLOAT_GUARD, dtype=np.int64)
    inv = qr.inv4_table()
    for q in range(116):
        bad = np.flatnonzero(qr.float_quotient(mag, inv[q]) != 4 * mag // qr.QF[q])
        assert bad.size == 0, (q, bad[:4])


def test_float_form_on_signed_sixteen_bit_operands():
    """p16_group's form: the SIGNED value times the reciprocal, truncated towards zero -- every 16-bit operand the table
    path admits (|v| <= 32767), every index 0 .. 119 (the wrapped factors' reciprocals are 4 / (unsigned) qf: quotient 0)"""
    v = np.arange(-32767, 32768, dtype=np.int64)
    inv = qr.inv4_table()
    for q in range(120):
        got = (v.astype(np.float32) * inv[q]).astype(np.int64)
        assert np.array_equal(got, qr.quant_np(v, q)), q


def test_lowest_failure_of_the_float_form_beyond_its_guard():
    assert qr.lowest_float_failure() == (1761441, 23)
    assert 1761441 in qr.float_adversarial(23) and 1761441 / qr.FLOAT_GUARD > 1.67
    for q in range(116):
        f = qr.QF[q]
        for m in qr.float_adversarial(q):
            assert qr.FLOAT_GUARD <= m < 1 << 22 and int(qr.float_quotient(m, qr.inv4_table()[q])) != 4 * m // f
            assert qr.model_float(m, q) == qr.quant(m, q) != qr.model_float(m, q, guard=1 << 22)


@pytest.mark.slow
def test_factors_that_are_powers_of_two_have_no_float_failure():
    mag = np.arange(qr.FLOAT_GUARD, 1 << 22, dtype=np.int64)
    for q in range(0, 116, 4):
        assert qr.float_adversarial(q) == () and qr.QF[q] & (qr.QF[q] - 1) == 0
        assert np.array_equal(qr.float_quotient(mag, qr.inv4_table()[q]), 4 * mag // qr.QF[q])


# ---- the magic claim
def test_reciprocal_multiply_is_exact_on_boundary_dividends():
    """magic / shift rebuilt by make_tables' rule (the round-up reciprocal of an l-bit divisor, Granlund & Montgomery):
    (t + ((a - t) >> 1)) >> shift == a / qf at every designed dividend a = 4 |v| < 2^31 and on a seeded sample of dividends
    k * qf - 1, k * qf, k * qf + 1 up to 2^31"""
    rng = np.random.default_rng(2720)
    n = 0
    for q in range(116):
        f = qr.QF[q]
        m, s = qr.magic_shift(q)
        assert 0 < m < 1 << 32 and (1 << s) < f <= (2 << s)
        for d in qr.designed(q, qr.INT_GUARD - 1):
            a = 4 * abs(d.v)
            assert qr.umulhi_quotient(a, m, s) == a // f == abs(d.want), (d, a)
            n += 1
        kmax = ((1 << 31) - 2) // f
        for k in set(rng.integers(1, kmax + 1, 1400).tolist()) | {1, kmax}:
            for a in (k * f - 1, k * f, k * f + 1):
                if a < 1 << 31:
                    assert qr.umulhi_quotient(a, m, s) == a // f, (q, a)
                    n += 1
    assert n > 300000


# ---- designed pictures and their reach
def _union(oracle, name, context):
    tot = {}
    for q in qr.picture_indices(qr.GEOMS[name]):
        for k, n in qr.reach(qr.design(oracle, name, q), context).items():
            tot[k] = tot.get(k, 0) + n
    return tot


@pytest.mark.slow
@pytest.mark.parametrize("name", list(qr.GEOMS))
def test_designed_pictures_transform_back_and_fit(oracle, name):
    for q in qr.picture_indices(qr.GEOMS[name]):
        d = qr.design(oracle, name, q)
        qr.check_design(oracle, d)
        assert len(d.placed) >= 40 and d.dropped <= len(d.placed) // 10, (name, q, len(d.placed), d.dropped)
        # no picture of 16-bit samples passes Haar0's bound, so none brings 2^20 to a coder; the designs stay within 65535
        assert max(int(np.abs(r).max()) for r in d.recs) <= 65535 < qr.HAAR0_BOUND < qr.FLOAT_GUARD


def test_no_haar0_coefficient_of_sixteen_bit_samples_passes_the_bound(oracle):
    """why no designed picture brings 2^20 to a coder: Haar0's low band is an average, HL / LH a difference of averages, HH a
    difference of differences -- a checkerboard of the extreme samples attains the bound"""
    from vc2lib import KERNELS
    rng = np.random.default_rng(2721)
    worst = 0
    for kind in range(4):
        p = rng.choice([-32768, 32767], size=(64, 128)) if kind < 3 else (np.indices((64, 128)).sum(axis=0) % 2 * 65535 - 32768)
        worst = max(worst, int(np.abs(oracle.dwt_forward(p.astype(np.int32), KERNELS["Haar0"], 4)).max()))
    assert worst == qr.HAAR0_BOUND


def test_the_refused_design_holds_the_first_uncodable_quotient(oracle):
    d = qr.design(oracle, "P32", 3, refused=True)
    qr.check_design(oracle, d)
    wants = {abs(dv.want) for _, _, _, dv in d.placed}
    assert wants == {qr.CODE_MAX + 1} and len(d.placed) >= 4
    ok = qr.design(oracle, "P32", 3)
    assert qr.CODE_MAX in {abs(dv.want) for _, _, _, dv in ok.placed} and max(abs(dv.want) for _, _, _, dv in ok.placed) == qr.CODE_MAX


# hand-written minimums: (geometry, context, copy, place) -> (indices that must all be met, the least number of distinct
# (k, side, sign) kinds over all indices, the least number of values)
REACH_MIN = {
    ("P32", "tab", "load8_tab", None): (range(64), 120, 15000),
    ("P16", "tab", "load8_tab", "body"): (range(60), 120, 10000),
    ("P16", "tab", "load8_tab", "head"): (range(64), 120, 10000),
    ("P16", "pack16", "p16_group", "body"): (range(60), 50, 5000),
    ("P16", "pack16", "quant_core", "head"): (range(64), 90, 5000),
    ("P16", "pack16", "p16_general", "mixed"): (range(60), 120, 5000),
    ("P16", "pack16", "p16_general", "head"): (range(40), 100, 3000),
    ("P16W", "pack16", "p16_group", "body"): (range(60), 50, 5000),
    ("P16W", "pack16", "quant_core", "head"): (range(64), 90, 3000),
    ("P16W", "pack16", "p16_general", "mixed"): (range(60), 120, 5000),
}


@pytest.mark.slow
@pytest.mark.parametrize("key", list(REACH_MIN), ids=lambda k: "-".join(str(x) for x in k))
def test_reach_minimums(oracle, key):
    name, context, copy, place = key
    indices, kinds, values = REACH_MIN[key]
    tot = _union(oracle, name, context)
    rows = {k: n for k, n in tot.items() if k[0] == copy and (place is None or k[2] == place)}
    got_idx = {k[1] for k in rows}
    assert set(indices) <= got_idx, (key, sorted(set(indices) - got_idx))
    assert len({k[3:] for k in rows}) >= kinds and sum(rows.values()) >= values, (key, len({k[3:] for k in rows}), sum(rows.values()))
    per = {}
    for k in rows:
        per.setdefault(k[1], set()).add(k[3:])
    if copy != "p16_general":          # every index from both sides of a boundary and with both signs
        for aq in indices:
            assert {s for _, s, _ in per[aq]} == {"hit", "miss"} and {s for _, _, s in per[aq]} == {"+", "-"}, (key, aq)
    # the table path's own edge: quotients 126 (taken) on it, 127 and 128 beside it in slices that leave it
    if copy == "p16_group":
        ks = {k[3] for k in rows if k[4] == "hit"}
        assert qr.P16_MAXQ in ks and max(ks) == qr.P16_MAXQ
    if copy == "p16_general" and place == "mixed":
        assert {qr.P16_MAXQ + 1, qr.P16_MAXQ + 2} <= {k[3] for k in rows if k[4] == "hit"}


@pytest.mark.slow
def test_all_slow_slices_exist_where_small_values_pass_the_table(oracle):
    """a slice whose every body run holds a quotient beyond the table: only where first(q, 128) stays within 512 (indices
    0 .. 8, qf <= 16): thirty such values fit one slice's samples; beyond that the reach table says "mixed" only"""
    tot = _union(oracle, "P16", "pack16")
    idx = {k[1] for k in tot if k[0] == "p16_general" and k[2] == "all-slow"}
    assert idx and idx <= set(range(9)), idx


def test_unreachable_values_are_pinned_on_the_int32_entry_points():
    """what no designed picture delivers: |v| >= 2^20 (Haar0's bound), so the float guard's three values, the float-adversarial
    magnitudes and everything from 2^29 on reach copy 1 through the sheets (and copy 7 through requantised values) only"""
    for q in (1, 23, 59):
        vals = set(qr.sheet_values(q))
        assert {qr.FLOAT_GUARD - 1, qr.FLOAT_GUARD, qr.FLOAT_GUARD + 1, qr.INT_GUARD - 1, qr.INT_GUARD, -(1 << 31)} <= vals
        assert set(qr.float_adversarial(q)) <= vals
    assert 32768 > max(abs(d.v) for d in qr.designed(0, 32767))      # no 16-bit body coefficient is 2^20: the store's type


# ---- requantise pairs
def test_requantise_pairs_sit_on_both_sides(oracle):
    for qs, qd in qr.REQUANT_PAIRS:
        vals = qr.requant_values(qs, qd)
        assert {s for _, _, s in vals} == {"hit", "miss"}, (qs, qd)
        for c, k, side in vals:
            for sign in (1, -1):
                s = oracle.scale(sign * c, qs)
                assert s == qr.scale(sign * c, qs)
                got = oracle.quant(s, qd)
                assert got == qr.quant(s, qd) == sign * (k if side == "hit" else k - 1), (qs, qd, c, side)
                if side == "hit":
                    assert abs(oracle.quant(s - sign, qd)) == k - 1
                else:
                    assert abs(oracle.quant(s + sign, qd)) == k


# ---- wrong copies of the models
def _nets():
    """the uniform nets of tests/test_gpu_parity.py (test_quantise_dequantise_match_oracle, test_quantiser_full_index_range)"""
    rng = np.random.default_rng(14)
    a = rng.integers(-20000, 20000, size=64 * 40)
    qa = rng.integers(0, 60, size=a.size)
    rng = np.random.default_rng(16)
    b = rng.integers(-(1 << 28), 1 << 28, size=116 * 32)
    qb = np.repeat(np.arange(116), 32)
    return list(zip(a.tolist(), qa.tolist())) + list(zip(b.tolist(), qb.tolist()))


def _signless(v, q, at):
    k = qr.model_float(v, q)
    return abs(k) if q == at and abs(k) == 1 else k


INV_NEAREST = qr.inv4_table("nearest")
# name -> (the wrong model, the designed value (v, q) that catches it)
MUTANTS = {
    "inv4 to nearest": (lambda v, q: qr.model_float(v, q, inv=INV_NEAREST[q]), (431, 27)),                      # k = 1 hit
    "magic minus 1 at index 41": (lambda v, q: qr.model_magic(v, q, magic=qr.magic_shift(q)[0] - (q == 41)), (4871, 41)),          # k = 4 hit
    "shift plus 1 at index 115": (lambda v, q: qr.model_magic(v, q, shift=qr.magic_shift(q)[1] + (q == 115)), (qr.first(115, 1), 115)),
    "float guard at 2^21": (lambda v, q: qr.model_float(v, q, guard=1 << 21), (1761441, 23)),                   # adversarial
    "table guard at 129": (lambda v, q: qr.model_table(v, q, limit=129) if abs(v) < 32768 else qr.quant(v, q), (128, 0)),   # k = 128 hit
    "sign dropped at k = 1, index 59": (lambda v, q: _signless(v, q, 59), (-qr.first(59, 1), 59)),
}


def test_model_mutants_are_caught_by_designed_values_only():
    net = _nets()
    des = [(d.v, d.q) for q in range(116) for d in qr.designed(q, qr.INT_GUARD - 1)]
    des += [(s * m, q) for q in range(116) for m in qr.float_adversarial(q) for s in (1, -1)]
    des_set = set(des)
    for v, q in net + des:        # the models themselves are right everywhere first
        want = qr.quant(v, q)
        assert qr.model_magic(v, q) == want and qr.model_float(v, q) == want
        if abs(v) < 32768:
            assert qr.model_table(v, q) == want
    caught = 0
    for name, (wrong, witness) in MUTANTS.items():
        by_net = [(v, q) for v, q in net if wrong(v, q) != qr.quant(v, q)]
        by_design = [(v, q) for v, q in des if wrong(v, q) != qr.quant(v, q)]
        assert not by_net, (name, "the uniform nets see it", by_net[:3])
        assert by_design, name
        if witness is not None:
            assert witness in des_set and witness in by_design, (name, witness, by_design[:3])
        caught += 1
    assert caught >= 6
    # "magic minus 1" shows on the `hit` side only: the quotient falls one short where 4 |v| is a multiple of the factor
    wrong = MUTANTS["magic minus 1 at index 41"][0]
    assert {d.side for d in qr.designed(41, qr.INT_GUARD - 1) if wrong(d.v, 41) != d.want} == {"hit"}


def test_table_guard_at_128_is_an_equivalent_mutant():
    """P16_MAXQ + 2 in the table path's `slow` test admits |quotient| 127: the signed byte and its table entry still hold
    +-127 (a code of 16 bits: a pair still fits 32), so no value shows it -- named equivalent, not counted as caught.  One
    more (129) admits 128, which the byte reads as -128: caught by k = 128."""
    v = np.arange(-32767, 32768)
    for q in range(64):
        for x in v[np.abs(qr.quant_np(v, q)) == 127][:4].tolist() + v[np.abs(qr.quant_np(v, q)) == 127][-4:].tolist():
            assert qr.model_table(x, q, limit=128) == qr.quant(x, q)
    assert qr.model_table(128, 0, limit=129) == -128 != qr.quant(128, 0)


# ---- which kernel a geometry gets, the LD planes and the transcoders' inputs
def test_geometries_get_the_kernels_their_rows_name(oracle):
    assert qr.pack_kernel(qr.P32.geometry(oracle), cr.store16(qr.P32.geometry(oracle))) == "k_hq_pack"
    assert qr.pack_kernel(qr.P16.geometry(oracle), cr.store16(qr.P16.geometry(oracle))) == "k_hq_pack16"
    assert qr.pack_kernel(qr.P16W.geometry(oracle), cr.store16(qr.P16W.geometry(oracle))) == "k_hq_pack16w"
    assert qr.pack_kernel(qr.P16.geometry(oracle), False) == "k_hq_pack"          # STORE32: load8_tab at a geometry with heads
    for name, g in qr.GEOMS.items():
        geo = g.geometry(oracle)
        assert cr.store16(geo) == g.store16 and geo.comp_n[0] <= 512 + 512 * (name == "P16W")
        assert [h for h, _ in qr.pack16_heads(geo)][0] == sum(geo.band_sizes(0)[:g.body_lo]), name
    assert qr.pack16_heads(qr.P16.geometry(oracle)) == [(32, 30), (16, 15), (16, 15)]
    assert qr.pack16_heads(qr.P16W.geometry(oracle)) == [(16, 63)] * 3
    for depth, ys, xs, lshape, cshape, fast in qr.LD_GEOMS.values():
        assert qr.ld_fast(depth, ys, xs, lshape, cshape) == fast


def test_ld_planes_hold_designed_values_in_every_band(oracle):
    from vc2lib import KERNELS
    for name, (depth, ys, xs, lshape, cshape, _) in qr.LD_GEOMS.items():
        qm = oracle.quant_matrix(KERNELS["LeGall"], depth)
        assert qm.tolist() == qr.LEGALL_MATRIX[depth]
        sheets = qr.ld_planes(name)
        assert len(sheets) == 3
        for sheet, (planes, qidx) in enumerate(sheets):
            assert qidx.min() == 0 or qidx.min() < 4
            assert qidx.max() > 63
            for p in planes:
                band = qr.band_plane(p.shape, depth)
                ll = p[::1 << depth, ::1 << depth]
                assert ll[0, 0] != 0 and np.count_nonzero(ll) == 1
                big = np.abs(p.astype(np.int64)) >= qr.INT_GUARD
                for b in range(1, 3 * depth + 1):
                    assert (np.abs(p[band == b].astype(np.int64)) > 3).mean() >= (0.45 if sheet < 2 else 1.0), (name, sheet, b)
                assert big[band > 0].all() == (sheet == 2)
                aq = qr.band_index_plane(p.shape, depth, ys, xs, qidx, qm)
                want = oracle.quantise_ld(p, depth, qidx, qm)
                assert np.array_equal(want[band > 0], qr.quant_np(p, aq)[band > 0])


@pytest.mark.parametrize("t", qr.REQUANT_TARGETS)
def test_transcoder_inputs_sit_on_both_sides_of_the_target_s_steps(oracle, t):
    import proxy_ref as pr
    case, qm, pays = qr.requant_inputs(oracle, t)
    assert pays[0] != pays[1]
    sides = {}
    for pay in pays:
        y, u, v, q = pr.quantised_planes(oracle, case, pay)
        assert set(q.ravel().tolist()) == set(qr.REQUANT_SOURCES)
        for plane in (y, u, v):
            sh, sw = plane.shape[0] // case.ys, plane.shape[1] // case.xs
            for s in range(case.ys * case.xs):
                qs = int(q.ravel()[s])
                if qs >= t:
                    continue
                sy, sx = divmod(s, case.xs)
                for c in plane[sy * sh:(sy + 1) * sh, sx * sw:(sx + 1) * sw].ravel().tolist():
                    if abs(c) < 3:
                        continue
                    sc = qr.scale(c, qs)
                    k = abs(qr.quant(sc, t))
                    step = 1 if c > 0 else -1
                    if k >= 1 and abs(qr.quant(sc - step, t)) == k - 1:
                        sides[(qs, "hit", step)] = sides.get((qs, "hit", step), 0) + 1
                    elif abs(qr.quant(sc + step, t)) == k + 1:
                        sides[(qs, "miss", step)] = sides.get((qs, "miss", step), 0) + 1
    for qs in qr.REQUANT_SOURCES:
        if qs < t:
            for side in ("hit", "miss"):
                for step in (1, -1):
                    assert sides.get((qs, side, step), 0) >= 8, (t, qs, side, step, sides.get((qs, side, step), 0))


# ---- the searches: slices whose budget the longer code just overflows
def test_search_sheets_are_tight(oracle):
    """every slice of the HQ_CBR sheets is tight in DESIGN section 18's sense (0 < T < 127 and the bytes at T - 1 do not fit),
    and tight on the boundary itself: a `miss` slice fills its budget with whole bytes at its designed index T, so that one
    quotient of 2^K - 1 instead of 2^K - 2 (two bits more) is a byte too many; a `hit` slice needs one byte more than its
    budget at T, so that one quotient of 2^K - 2 instead of 2^K - 1 lets it fit there"""
    g, planes, qm, sb, spec = qr.search_planes()
    assert cr.kernel_for(g, qm, False)[0] == "reg32"
    m = cr.analyse(oracle, g, planes, qm, 1, sb)
    c = cr.conditions(m)
    assert c["class:none"] == g.n_slices and not m.marked.any()          # the register kernel keeps every slice
    assert min(c[f"tight:{x}:head"] for x in "YUV") == g.n_slices
    want = oracle.cbr_qindices(*planes, g.depth, qm, sb, 1).ravel()
    seen = {"miss": set(), "hit": set()}
    for s, (T, K, side) in enumerate(spec):
        k = (1 << K) - 1
        for c_ in range(3):
            quot = np.abs(qr.quant_np(qr.search_design()[0][c_][s], T))
            assert set(quot[quot > 0].tolist()) == {k if side == "hit" else k - 1}, (s, T, K, side)
        if side == "miss":
            assert m.T[s] == T and m.need(T, s) == m.avail[s] and want[s] >= T, (s, T, K)
        else:
            assert m.T[s] > T and m.need(T, s) == m.avail[s] + 1 and want[s] > T, (s, T, K)
        seen[side].add((T, K))
    for side in seen:
        assert {t for t, _ in seen[side]} == set(range(1, 54)) and {k for _, k in seen[side]} >= set(range(2, 15)), side
    # exact multiples of the factor among the `hit` values: where a reciprocal rounded down falls one short
    exact = {T for T, K, side in spec if side == "hit" and 4 * qr.first(T, (1 << K) - 1) == ((1 << K) - 1) * qr.QF[T]}
    assert {4, 8, 12, 17, 20, 21, 25, 30} <= exact, sorted(exact)


@pytest.mark.parametrize("geom", list(qr.LD_GEOMS))
def test_ld_search_planes_are_tight(oracle, geom):
    planes, spec = qr.ld_search_planes(geom)
    budgets, at, below = qr.ld_tight_budgets(oracle, geom, planes, spec)
    want = np.array([t for t, _ in spec]).reshape(at.shape)
    climbs = want == 116
    assert climbs.sum() >= 3 and (at[climbs] == 116).all()          # the walk ends on the first wrapped factor
    assert (at <= want).all() and (at[~climbs] >= want[~climbs] - 1).all() and (at == want).mean() > 0.9
    assert (below[~climbs] > want[~climbs]).all()                    # one byte less and the slice leaves its index
    assert len({k for _, k in spec}) >= 8 and all((p[::1 << qr.LD_GEOMS[geom][0], ::1 << qr.LD_GEOMS[geom][0]] == 0).all() for p in planes)
