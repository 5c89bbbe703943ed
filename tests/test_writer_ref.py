"""CPU tests of tests/writer_ref.py: the definition of the HQ slice writer against the oracle on every designed input, the
named-value property, what the designs reach in k_hq_pack's restated decisions, the float forms of the length rule, and the
wrong copies of the model that the designed inputs catch.  No GPU."""
from collections import Counter

import numpy as np
import pytest

import cbr_ref as cr
import writer_ref as wr
from vc2lib import OracleError

SMALL_SCALARS = ((0, 1), (1, 2), (2, 3), (3, 7))
QUICK = ("n4", "n36", "w16")                              # the larger geometries take seconds in Python: marked slow
CASES = [pytest.param(g, p, s, marks=() if g in QUICK else pytest.mark.slow) for g in wr.GEOS for p, s in SMALL_SCALARS]


def _oracle(oracle, inp, prefix, scalar):
    geo = inp.geo
    qi = np.ascontiguousarray(inp.qidx.reshape(geo.ys, geo.xs))
    cb = None if inp.budgets is None else inp.budgets.reshape(qi.shape)
    return oracle.hq_pack(*wr.planes(geo, inp.recs), geo.depth, qi, prefix, scalar, cbr=cb).tobytes()


def _agree(oracle, inp, prefix, scalar, reach=None):
    """definition = oracle = model (through the slots and in one pass), refusals by the reference's words"""
    tag = (inp.geo.name, inp.gen, inp.tag, prefix, scalar)
    forms = (False,) if inp.budgets is not None else (False, True)
    if inp.refused:
        with pytest.raises(OracleError, match=wr.REFUSALS[inp.refused][0]):
            _oracle(oracle, inp, prefix, scalar)
        with pytest.raises(wr.Refused) as e:
            wr.payload(inp, prefix, scalar)
        assert e.value.kind == inp.refused, tag
        for sp in forms:
            with pytest.raises(wr.Refused) as e:
                wr.model(inp, prefix, scalar, sp)
            assert e.value.kind == inp.refused, tag
        return
    want = wr.payload(inp, prefix, scalar)
    assert _oracle(oracle, inp, prefix, scalar) == want, tag
    for sp in forms:
        assert wr.model(inp, prefix, scalar, sp, reach=reach) == want, (tag, sp)


@pytest.mark.parametrize("gname,prefix,scalar", CASES)
def test_definition_oracle_and_model_agree(oracle, gname, prefix, scalar):
    """on every input of every generator, VBR and under HQ_CBR -- what tests/test_gpu_writer.py runs"""
    for gen in wr.GENERATORS:
        ins = wr.inputs(gen, gname, prefix, scalar)
        assert ins and (gen == "random" or all(i.named or i.tag == "zeros" for i in ins)), gen
        for inp in ins:
            _agree(oracle, inp, prefix, scalar)
            if gen in ("last", "units", "tiles", "random") and not inp.refused:
                _agree(oracle, wr.with_budgets(inp, scalar), prefix, scalar)


@pytest.mark.slow
def test_large_scalars_and_longest_slices_agree(oracle):
    scalars = [s for pair in wr.lane_scalars(wr.GEOS[wr.SMALL]) + wr.mode_scalars() for s in pair]
    for scalar in scalars:
        for gen in wr.LARGE_GENERATORS:
            for inp in wr.inputs(gen, wr.SMALL, 1, scalar):
                _agree(oracle, inp, 1, scalar)
                if gen in ("last", "random") and not inp.refused:
                    _agree(oracle, wr.with_budgets(inp, scalar), 1, scalar)
    r = Counter()
    for inp in wr.inputs("cbr", "r2304", 0, 16):
        _agree(oracle, inp, 0, 16, r)
    assert r["slice bytes beyond three times 255 units"] == 12         # every second slice of `longest` and `longest_dense`
    gimg = wr.mode_scalars()[2][1]
    r = Counter()
    _agree(oracle, wr.longest(wr.HUGE, gimg), 0, gimg, r)
    _agree(oracle, wr.longest(wr.HUGE, gimg, dense=True), 0, gimg, r)
    assert r["slice bytes beyond three times 255 units"] == 2 and r["rounds", 32] == 12


def test_coding_order_and_planes():
    """the definition's own coding order is the one the suite's other references use"""
    for geo in wr.GEOS.values():
        for sh, sw in (geo.luma, geo.chroma):
            assert wr.order(sh, sw, geo.depth) == list(cr.coding_order(sh, sw, geo.depth)[0])
        inp = wr.inputs("random", geo.name)[0]
        g = cr.Geometry(geo.ys * geo.luma[0], geo.xs * geo.luma[1], geo.ys * geo.chroma[0], geo.xs * geo.chroma[1], geo.depth, geo.ys, geo.xs)
        for a, b in zip(wr.planes(geo, inp.recs), cr.planes_from_records(g, inp.recs)):
            assert np.array_equal(a, b)


def test_codes():
    assert [wr.code(v) for v in (0, 1, -1, 2, -3, 6)] == ["1", "0010", "0011", "0110", "000011", "010110"]
    assert {len(wr.code(v)) for v in range(-70000, 70000, 7)} <= set(wr.LENGTHS) | {34}
    assert len(wr.code(65534)) == 32 and len(wr.code(65535)) == 34 and len(wr.code(32766)) == 30 and len(wr.code(32767)) == 32
    for L in wr.LENGTHS[1:]:
        rng = np.random.default_rng(L)
        assert all(len(wr.code(wr.value_of(L, rng, e, s))) == L for e in (0, 1, None) for s in (1, -1))


# the form every geometry runs in at prefix 0, scalar 1: (lanes a slice, one round, rounds of Y / U / V, big_lut, slices a shared slot)
FORMS = {"n4": (16, True, (1, 1, 1), False, 16), "n36": (16, True, (1, 1, 1), False, 16), "w16": (16, True, (1, 1, 1), False, 16),
         "w32": (32, True, (1, 1, 1), False, 8), "fast": (64, True, (1, 1, 1), False, 0), "r520": (64, False, (2, 1, 1), True, 0),
         "r1024": (64, False, (2, 1, 1), True, 0), "r2304": (64, False, (5, 3, 3), False, 0)}


@pytest.mark.parametrize("gname", list(wr.GEOS))
def test_pack_form(gname):
    geo = wr.GEOS[gname]
    for prefix, scalar in SMALL_SCALARS:
        f = wr.pack_form(geo, prefix, scalar)
        assert (f.W, f.fast, f.rounds, f.big_lut, f.tile_slices) == FORMS[gname] and f.mode == 0 and f.kernel == "k_hq_pack", (gname, scalar, f)
        one = wr.pack_form(geo, prefix, scalar, single_pass=True)
        assert one.W == 64 and one.lookback and one.tile_slices == 0 and one.fast == (gname not in ("r520", "r1024", "r2304"))
        c = wr.pack_form(geo, prefix, scalar, cbr=True)
        assert c.W == f.W and c.tile_slices == 0 and not c.lookback


def test_scalars_where_the_form_changes():
    """by the restated rule: four slices a wavefront up to 10, two up to 22; four slice images in LDS up to 45, two up to 92, one up
    to 185, in global memory from 186 on.  The one-pass form ends with image mode 0"""
    small = wr.GEOS[wr.SMALL]
    assert wr.lane_scalars(small) == [(10, 11), (22, 23)] and wr.lane_scalars(wr.GEOS["w32"]) == [(22, 23)]
    assert wr.mode_scalars() == [(45, 46), (92, 93), (185, 186)]
    assert [wr.pack_form(small, 0, s).W for s in (10, 11, 22, 23)] == [16, 32, 32, 64]
    assert [(wr.pack_form(small, 0, s).waves, wr.pack_form(small, 0, s).gimg) for s in (45, 46, 92, 93, 185, 186)] == \
        [(4, False), (2, False), (2, False), (1, False), (1, False), (4, True)]
    assert wr.pack_form(small, 0, 45, single_pass=True).lookback and not wr.pack_form(small, 0, 46, single_pass=True).lookback


@pytest.mark.parametrize("gname", [pytest.param(g, marks=() if g in ("n4", "n36") else pytest.mark.slow) for g in wr.GEOS])
def test_a_named_value_of_another_length_changes_its_slice(gname):
    """every named value moved by one code-length class changes the definition's bytes of its own slice"""
    for prefix, scalar in ((0, 1), (2, 3)):
        for gen in wr.GENERATORS:
            for inp in wr.inputs(gen, gname, prefix, scalar):
                if inp.refused:
                    continue
                before_of = {}
                for s, c, j in inp.named:
                    comps = [inp.recs[k][s].copy() for k in range(3)]
                    budget = None if inp.budgets is None else int(inp.budgets[s])
                    if s not in before_of:
                        before_of[s] = wr.slice_bytes(int(inp.qidx[s]), comps, prefix, scalar, budget)
                    before = before_of[s]
                    comps[c][j] = wr.other_class(int(comps[c][j]))
                    try:
                        after = wr.slice_bytes(int(inp.qidx[s]), comps, prefix, scalar, budget)
                    except wr.Refused as e:
                        after = e.kind
                    assert after != before, (gname, gen, inp.tag, s, c, j)


def _reach(gen, gname, scalars=SMALL_SCALARS):
    r = Counter()
    for prefix, scalar in scalars:
        for inp in wr.inputs(gen, gname, prefix, scalar):
            for k, v in wr.trace(inp, prefix, scalar).items():
                r[k] += v
            if inp.budgets is None and not inp.refused:
                for k, v in wr.trace(inp, prefix, scalar, True).items():
                    r[("one pass",) + (k if isinstance(k, tuple) else (k,))] += v
    return r


@pytest.mark.slow
def test_reach_strings():
    """the least counts the design gives, by hand.  Through the slots at the four scalars, variant A: w16 has 18 slices in 5
    wavefronts, a luma and a chroma round each, 4 turns, 4 scalars: 160 wavefront rounds whose longest string has exactly
    62 (63, 64) bits and take write8_short, 160 of 65 (66) that take write8; a slice has 4 + 2 + 2 designed lanes: 2304
    strings of each length.  fast: 15 wavefronts, 480 rounds; 16 + 8 + 8 lanes: 7680 strings.  Variant B adds a string of every
    length between lanes of 80 bits per component: 216 (180) through write8"""
    for gname, rounds, strings, b in (("w16", 160, 2304, 216), ("fast", 480, 7680, 180)):
        r = _reach("strings", gname)
        for bits in (62, 63, 64):
            assert r["write8_short", bits] == rounds and r["string of", bits] == strings and r["string of (write8)", bits] == b, (gname, bits)
            assert r["one pass", "write8_short", bits] >= rounds, (gname, bits)
        for bits in (65, 66):
            assert r["write8", bits] == rounds and r["string of (write8)", bits] == strings + b, (gname, bits)
        assert all(r["short string over words", k] >= 5000 for k in (1, 2, 3)), gname
    r = _reach("strings", "n4")                   # half a group: four codes of 62 .. 66 bits
    assert all(r["string of", b] >= 100 for b in (62, 63, 64)) and all(r["string of (write8)", b] >= 100 for b in (65, 66))


@pytest.mark.slow
def test_reach_phase_last_units():
    """phase: 300 designed codes a (prefix, scalar), every one in a string that ends in the word it starts in, in the next or
    in the one after, through write8_short; the codes of 30 and 32 bits behind fillers also through write8"""
    for gname in ("w16", "fast"):
        r = _reach("phase", gname)
        assert r["short string over words", 1] >= 1000 and r["short string over words", 2] >= 1000 and r["short string over words", 3] >= 100
        assert all(r["write8", b] >= 5 for b in (65, 66, 67)), (gname, r)
    r = _reach("last", "fast")
    assert r["units", 1] >= 150 and r["units", 2] >= 50 and r["units", 255] >= 20 and r["ends at the limit"] >= 10
    for gname, least in (("w16", (30, 50, 5, 8, 3)), ("fast", (20, 25, 15, 25, 7)), ("r520", (20, 25, 15, 25, 7))):
        r = _reach("units", gname)
        assert all(r["units", m] >= x for m, x in zip((1, 2, 254, 255), least)) and r["refused", "scalar"] == least[4], (gname, r)
        assert r["ends at the limit"] >= 10
    r = _reach("units", "n4")                  # 4 coefficients hold 16 bytes: one and two units only, and never 256
    assert r["units", 1] >= 10 and r["units", 254] == 0 and r["refused", "scalar"] == 0


@pytest.mark.slow
def test_reach_cbr_and_tiles():
    for gname in ("w16", "fast", "r520"):
        r = _reach("cbr", gname)
        assert r["V room", "need"] >= 150 and r["V room", "remainder"] >= 140 and r["V room", "units"] >= 110 and r["V room of 255 units"] >= 130
        assert r["refused", "toobig"] == 4 and r["refused", "len"] == 4
        assert all(r["copy-out head", k] >= 60 and r["copy-out tail", k] >= 60 for k in range(4)), (gname, r)
    for gname, last in (("w16", (1, 2, 3, 15, 16)), ("w32", (1, 2, 3, 7, 8)), ("fast", (1, 2, 3, 4)), ("r520", (1, 2, 3, 4))):
        r = _reach("tiles", gname)
        assert all(r["slices in the last tile", k] >= 4 for k in last), (gname, r)
        assert all(r["one pass", "tile start mod 4", k] >= 4 for k in range(4)), (gname, r)
        assert all(r["one pass", "copy-out head", k] >= 40 and r["one pass", "copy-out tail", k] >= 40 for k in range(4))
        if gname in ("w16", "w32"):          # shared slots: seg_off between slices of different lengths
            assert r["slices of a wavefront differ"] >= 100 and all(r["copy-out head", k] >= 80 for k in range(4)), (gname, r)
    r = _reach("tiles", "r520")
    assert r["rounds", 2] >= 200 and r["last round of", 8] >= 200 and r["last round of", 260] >= 400
    r = _reach("tiles", "r2304", ((1, 2),))
    assert r["rounds", 5] >= 30 and r["rounds", 3] >= 60


@pytest.mark.parametrize("scalar", [1, 2, 3, 7, 10, 11, 16, 22, 23, 45, 46, 92, 93, 185, 186])
def test_float_forms_of_the_length_rule(scalar):
    """comp_len's (int)((bytes + scalar - 1) * inv_up) is the integer quotient for every byte count up to 256 units and a
    unit more, and the length byte's (int)(bytes * inv_up) is floor(bytes / scalar) for every V room up to the refusal:
    float32, as the kernels compute them"""
    inv = wr.inv_up(scalar)
    assert inv.dtype == np.float32 and float(inv) >= 1.0 / scalar > float(np.nextafter(inv, np.float32(0)))
    b = np.arange(0, 257 * scalar + 2, dtype=np.int64)
    assert np.array_equal(((b + scalar - 1).astype(np.float32) * inv).astype(np.int32), (b + scalar - 1) // scalar)
    assert np.array_equal((b.astype(np.float32) * inv).astype(np.int32), b // scalar)


MUTANT_GEOS = {"strings": ("fast", "r520"), "phase": ("fast",), "last": ("w16", "fast"), "units": ("fast",), "cbr": ("fast", "r2304"),
               "tiles": ("w16",)}


def _verdict(inp, prefix, scalar, mut):
    """does a wrong copy show on this input"""
    def run(f):
        try:
            return f()
        except wr.Refused as e:
            return e.kind
    want = run(lambda: wr.payload(inp, prefix, scalar))
    forms = (False,) if inp.budgets is not None else (False, True)
    return any(run(lambda: wr.model(inp, prefix, scalar, sp, mut=mut)) != want for sp in forms)


@pytest.mark.slow
@pytest.mark.parametrize("gen,mut", wr.MUTANTS, ids=[m for _, m in wr.MUTANTS])
def test_wrong_copies_are_caught(gen, mut):
    """every wrong copy of the model shows on a designed input of the generator named for it; the first DESIGNED_ONLY of them on
    no random input of any geometry (VBR at every scalar; under HQ_CBR with a remainder of one byte, which at scalar 1 is a unit).
    `random` is kept off the count's two edges by writer_ref._settle.  The four that `random` does catch cannot be kept from
    it: `seg_off over s2 <= seg` moves every slice behind the first of a wavefront by its own length, which is never 0"""
    scalars = ((0, 16),) if "an image of" in mut else SMALL_SCALARS
    geos = ("r2304",) if "an image of" in mut else MUTANT_GEOS[gen]
    assert any(_verdict(inp, p, s, mut) for g in geos for p, s in scalars for inp in wr.inputs(gen, g, p, s)), mut
    if (gen, mut) in wr.MUTANTS[:wr.DESIGNED_ONLY]:
        edge = mut in ("count through the last code", "code dropped when it ends at the limit")
        for g in wr.GEOS:
            for p, s in SMALL_SCALARS:
                if edge and wr.unsettled(wr.GEOS[g], s):      # (r2304 at scalar 1: 2304 zeros alone pass 250 units, every input there sits on the edge)
                    assert (g, s) == ("r2304", 1)
                    continue
                for inp in wr.inputs("random", g, p, s):
                    assert not _verdict(inp, p, s, mut), (mut, g, s, inp.tag)
                    if s > 1:
                        nd = wr.needs(inp, s).sum(axis=1) + 5
                        assert not _verdict(inp._replace(budgets=nd.astype(np.int32)), p, s, mut), (mut, g, s, inp.tag, "cbr")


def test_the_definitions_own_wrong_copies():
    for mut in wr.PLAIN_MUTANTS:
        gen = dict((m, g) for g, m in wr.MUTANTS)[mut]
        assert any(wr.payload(inp, 0, 3, mut) != wr.payload(inp, 0, 3) for inp in wr.inputs(gen, "w16", 0, 3) if not inp.refused), mut


@pytest.mark.slow
@pytest.mark.parametrize("name,kept", [("S16", 15), ("M1024", 17), ("M2048", 17), ("P32", 16), ("P16", 16), ("P16W", 17)])
def test_batch_pictures_are_their_fields_and_the_composition_is_the_definition(oracle, name, kept):
    """the designs as Haar0 pictures for vc2hip_encode_batch_dev: every kept picture transforms back to its field (asserted in
    batch_picture), and the oracle's composition at a flat matrix and index 0 writes the definition's payload of the field.
    Dropped: the `last` pictures that hold the lone values of 30 and 32 bits, whose samples leave 16 bits"""
    import qmatrix_ref as qmr
    case = wr.BATCH_GEOMS[name].case(oracle, 0, wr.BATCH_SCALAR)
    n = 0
    for inp in wr.batch_inputs(oracle, name):
        raw, d = wr.batch_picture(oracle, name, inp)
        if raw is None:
            assert inp.gen == "last", (name, inp.gen, inp.tag)
            continue
        n += 1
        assert qmr.encode(oracle, case, raw, d.qm)[0] == wr.payload(inp, 0, wr.BATCH_SCALAR), (name, inp.gen, inp.tag)
        if inp.gen == "strings":          # the strings sit in whole groups of eight of the 16-bit store's lanes of sixteen
            sums = Counter()
            for s, c, j in inp.named:
                grp = inp.recs[c][s, j // 8 * 8:j // 8 * 8 + 8]
                sums[sum(len(wr.code(int(v))) for v in grp), (j // 8) % 2] += 1
            bits = int(inp.tag[1:3])
            assert sums[bits, 0] >= 16 and sums[bits, 1] >= 16, (name, inp.tag, sums)      # first and second string of a lane
    assert n == kept


_BATCH16 = {}


def _batch16(oracle, name):
    """the kept batch inputs of a 16-bit store geometry with their definition's payloads, once"""
    if name not in _BATCH16:
        ins = [i for i in wr.batch_inputs(oracle, name, ("strings", "last", "random", "last16")) if wr.batch_picture(oracle, name, i)[0] is not None]
        _BATCH16[name] = [(i, wr.payload(i, 0, wr.BATCH_SCALAR)) for i in ins]
    return _BATCH16[name]


@pytest.mark.slow
@pytest.mark.parametrize("name", ["P16", "P16W"])
def test_pack16_model_reach_and_wrong_copies(oracle, name):
    """writer_ref.model16 -- k_hq_pack16's and k_hq_pack16w's decisions -- writes the definition's bytes of the designed slices
    of every batch picture; what the pictures reach, the least counts by hand; its wrong copies"""
    import qmatrix_ref as qmr
    heads, wide = wr.heads_of(oracle, name), name == "P16W"
    assert heads == ([(32, 30), (16, 15), (16, 15)] if name == "P16" else [(16, 63)] * 3)
    case = wr.BATCH_GEOMS[name].case(oracle, 0, wr.BATCH_SCALAR)
    r = Counter()
    for inp, want in _batch16(oracle, name):
        got = wr.model16(inp, heads, wide, 0, wr.BATCH_SCALAR, reach=r)
        assert len(got) > 16 * 4 and want.startswith(got), (name, inp.gen, inp.tag)
        if inp.gen == "last16":
            raw, d = wr.batch_picture(oracle, name, inp)
            assert qmr.encode(oracle, case, raw, d.qm)[0] == want, (name, inp.tag)
    # strings: 16 slices x (4 + 2 + 2 lanes on P16) x two pictures (A, B) of each length put a string of 62 and of 63 bits on
    # the table path in the first and in the second half of a lane 200 times or more; 64, 65 and 66 send their slices
    # (P16W: components) to p16_general by `max(L0, L1) > 63`: six pictures, 380 times or more
    assert all(r["string of", b, h] >= 200 for b in (62, 63) for h in (0, 1)), r
    assert r["p16_general", "string"] >= 380 and r["p16_general", "quotient"] >= 100       # (quotient: last16's +-129, `last`'s 1023 ..)
    # count_of: the body's ballot decides, the head's where the body is all zeros (last16's head lanes), and neither
    assert r["count_of", "body"] >= 200 and r["count_of", "head"] >= 90 and r["count_of", "none"] >= 40
    assert r["last in string", 0] >= 60 and r["last in string", 1] >= 150 and r["head code ends at the room"] >= 4
    caught = {m: {inp.gen for inp, want in _batch16(oracle, name) if not want.startswith(wr.model16(inp, heads, wide, 0, wr.BATCH_SCALAR, mut=m))}
              for m in [m for _, m in wr.MUTANTS16] + [wr.EQUIVALENT16]}
    for gen, m in wr.MUTANTS16:
        assert gen in caught[m], (name, m, caught[m])
    for _, m in wr.MUTANTS16[:3]:                      # the first three by designed inputs only
        assert "random" not in caught[m], (name, m)
    # `max(L0, L1) > 64` for `> 63` changes nothing that is written: a string of 64 bits fits the register pair exactly, and
    # p16_put's one weak place for n = 64 (keep = 0: a shift by 64) needs a string of 64 bits wholly beyond its component's
    # room -- but a string that long holds a non-zero value, and the room runs through the last one.  Equivalent, not caught
    assert caught[wr.EQUIVALENT16] == set(), (name, caught[wr.EQUIVALENT16])
