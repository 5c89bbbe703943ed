"""The slice index on the CPU (no GPU): tests/index_ref.py's plan against the plan table written out here by hand, its
transcription of the kernels against the plain walk on every designed chain, what every chain reaches by name, the oracle's
verdict on the designed payloads, and a list of one-line wrong copies of the transcription that the chains must catch.

emulate() runs on every designed input of every row (the whole file takes well under a minute): the largest is
(633, 42) `groups`, 6.2 MB in 190 chunks of 32767 entries."""
import numpy as np
import pytest

import damage as dm
import index_ref as ir

# (prefix, scalar): kind, CH, G, E, EU, merged walks, deduped composition, threads, PER, EPT -- written out from
# vc2_launch_slice_index and k_index_tables_nx by hand, not by calling plan()
TABLE = {
    (0, 1): ("tables", 8192, 1, 769, 769, True, True, 512, 16, 8),
    (255, 1): ("tables", 8192, 1, 1024, 1024, True, True, 512, 16, 8),
    (256, 1): ("tables", 16384, 1, 1025, 1025, True, True, 1024, 16, 4),
    (0, 2): ("tables", 16384, 2, 1534, 767, True, True, 512, 16, 8),
    (1, 2): ("tables", 16384, 1, 1535, 1535, True, True, 1024, 16, 4),
    (0, 4): ("tables", 16384, 4, 3064, 766, True, True, 512, 8, 8),
    (0, 7): ("tables", 16384, 1, 5359, 5359, False, True, 1024, 16, 4),
    (0, 8): ("tables", 16384, 4, 6124, 1531, True, True, 512, 8, 8),
    (537, 10): ("tables", 16384, 1, 8191, 8191, False, True, 1024, 16, 4),
    (538, 10): ("tables", 32768, 2, 8192, 4096, True, True, 1024, 16, 4),
    (0, 11): ("tables", 32768, 1, 8419, 8419, False, False, 1024, 32, 4),
    (0, 20): ("tables", 32768, 4, 15304, 3826, True, True, 512, 16, 8),
    (0, 24): ("tables", 32768, 4, 18364, 4591, False, True, 512, 16, 8),
    (0, 42): ("tables", 32768, 2, 32134, 16067, False, False, 1024, 16, 4),
    (633, 42): ("tables", 32768, 1, 32767, 32767, False, False, 1024, 32, 4),
    (634, 42): ("serial", 32768, 2, 32768, 16384, False, False, 1024, 16, 4),
    (0, 43): ("serial", 32768, 1, 32899, 32899, False, False, 1024, 32, 4),
}


def test_rows_are_the_table():
    assert ir.ROWS == list(TABLE)


@pytest.mark.parametrize("row", ir.ROWS, ids=str)
def test_plan_matches_the_table(row):
    pl = ir.plan(*row, 1 << 20)
    got = (pl.kind, pl.CH, pl.G, pl.E, pl.EU, pl.merge, pl.dedupe, pl.threads, pl.PER, pl.EPT)
    assert got == TABLE[row]
    assert pl.cause == ("long" if pl.kind == "serial" else "")
    assert dm.index_chunk(*row) == TABLE[row][1]     # (damage.py takes its chunk size from plan)
    if pl.kind == "tables":
        # the bounds the kernels' comments state: positions and exits in 16 bits, a chunk's slices in 16 bits, every
        # merged entry held by some thread, the carved LDS inside a gfx950 workgroup's 160 KiB
        assert pl.CH + pl.E - pl.G <= 0xFFFF and pl.E - pl.G <= 0x7FFF and pl.CH // (pl.prefix + 4) <= 0xFFFF
        assert not pl.merge or (pl.EU <= pl.threads * pl.EPT and 2 * pl.E <= pl.CH)
        assert pl.lds_tables <= ir.LDS_BYTES and pl.lds_group <= ir.LDS_BYTES, (pl.lds_tables, pl.lds_group)
        assert (pl.lds_group == 0) == (not pl.dedupe)


def test_plan_lds_and_levels():
    """the carved LDS of two rows by hand, and the plan's dependence on the slot stride: the third chain level from 129
    groups on, the serial walk from 16385 chunks on"""
    a = ir.plan(0, 1, 1 << 20)
    assert (a.lds_tables, a.lds_group) == (8992 + 16384 + 4614 + 100 + 16, 3080 + 6152 + 1538 + 16)
    b = ir.plan(633, 42, 1 << 20)
    assert (b.lds_tables, b.lds_group) == (65552 + 65536, 0)
    c = ir.plan(0, 1, 2047 * 8192)
    assert (c.kind, c.n_chunks, c.n_groups, c.n_supers) == ("tables", 2048, 128, 0)
    d = ir.plan(0, 1, 2047 * 8192 + 1)
    assert (d.kind, d.n_chunks, d.n_groups, d.n_supers) == ("tables", 2049, 129, 9)
    e = ir.plan(0, 1, 16383 * 8192)
    assert (e.kind, e.n_chunks, e.n_groups, e.n_supers) == ("tables", 16384, 1024, 64)
    f = ir.plan(0, 1, 16383 * 8192 + 1)
    assert (f.kind, f.cause, f.n_chunks) == ("serial", "too_many", 16385)
    assert ir.plan(0, 43, 16383 * 32768 + 1).cause == "long"


# ---------------------------------------------------------------------------------------------------------------------
# the designed inputs
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def designed(row, name):
    """[(input, payload, plan at vc2hip_hq_unpack's stride, slice starts, end)] of one generator on one row; shared"""
    if (row, name) not in _CACHE:
        out = []
        for inp in ir.inputs(*row, name):
            pay = ir.payload_of(inp)
            starts, end = ir.walk(pay, len(pay), inp.ns, inp.prefix, inp.scalar)
            assert end == len(pay) <= ir.MAX_PAYLOAD, (row, name, inp.tag, end, len(pay))
            # the plain walk is damage.hq_walk; index_ref.walk, which emulate() also is on the serial rows, must be the same
            assert [int(x) for x in starts] == [sl.start for sl in dm.hq_walk(pay, inp.ns, inp.prefix, inp.scalar)], (row, name, inp.tag)
            out.append((inp, pay, ir.plan(*row, ir.slot_stride(len(pay))), starts, end))
        _CACHE[(row, name)] = out
    return _CACHE[(row, name)]


CASES = [(row, name) for row in ir.ROWS for name in ir.GENERATORS]


@pytest.mark.parametrize("row,name", CASES, ids=lambda x: str(x))
def test_emulate_is_the_plain_walk(row, name):
    """the transcription gives the plain walk's offsets, and at every chunk the chain takes the table word (exit, slices)
    that the walk says the chunk has"""
    for inp, pay, pl, starts, end in designed(row, name):
        offs, taken = ir.emulate(pay, len(pay), pl, inp.ns)
        assert np.array_equal(offs, starts), f"{row} {name} {inp.tag}: first difference at slice {int(np.argmax(offs != starts))}"
        if pl.kind == "tables":
            assert taken == ir.chunk_functions(starts, end, pl), f"{row} {name} {inp.tag}"


@pytest.mark.parametrize("row,name", CASES, ids=lambda x: str(x))
def test_inputs_reach_what_they_are_named_for(row, name):
    for inp, pay, pl, starts, end in designed(row, name):
        tr = ir.trace(pay, len(pay), pl, inp.ns)
        what = f"{row} {name} [{inp.tag}]: {tr}"
        P, sizes = pl.prefix + 4, np.diff(np.concatenate([starts, [end]]))
        if name == "min":
            assert tr["chunks"] >= 2 and tr["max_count"] >= pl.CH // P, what      # a chunk full of minimal slices
        elif name == "max":
            assert (sizes == pl.E).all() and tr["chunks"] >= 5, what
        elif name == "mixed":
            assert set(np.unique(inp.lens)) == set(ir.MIXED) and tr["chunks"] >= 16, what
        elif name in ("land", "groups"):
            mult = ir.IDX_GROUP if name == "groups" else 1
            two = name == "groups" and row == (633, 42)     # (four landings would be 17 MB there: gen_groups)
            assert set(inp.info) == ({"end_b", "max_bG"} if two else set(ir.LANDINGS)) and ("two landings" in inp.tag) == two, what
            for kind, (b, t) in inp.info.items():
                d = {"end_b": 0, "end_bG": pl.G, "max_bG": -pl.G, "min_bG": -pl.G}[kind]
                i = int(np.searchsorted(starts, t))
                assert b % (pl.CH * mult) == 0 and starts[i] == t, f"{kind} missed: {what}"
                assert t == b + d or f"{kind} nearest {t - b - d:+d}" in inp.tag, f"{kind} missed and the tag does not say so: {what}"
                if kind == "max_bG":
                    assert sizes[i] == pl.E, f"{kind} missed: {what}"
                if kind == "min_bG":
                    assert sizes[i] == P, f"{kind} missed: {what}"
            exact = "nearest" not in inp.tag
            if exact:
                assert tr["exit0"] and tr["exit_max"] and tr["max_nx_chain"] == pl.CH + pl.E - pl.G, what
                if not two:
                    assert pl.G in tr["exits"], what
            if name == "groups":
                assert tr["groups"] >= 3, what
        elif name == "end":
            b, d = inp.info["boundary"], inp.info["delta"]
            assert b % pl.CH == 0 and tr["length"] == b + d + inp.info["tail"] * P, what
            assert d == 0 and "nearest" not in inp.tag, what     # gcd(prefix + 4, scalar) forbids no boundary on these rows
            assert tr["end_on_boundary"] == (inp.info["tail"] == 0), what
            if inp.info["tail"]:   # the last slice starts on the boundary and is the last chunk's only one
                assert starts[-1] == b and tr["exit0"] and sizes[-1] == P, what
        elif name == "short":
            assert tr["length"] < pl.E and (tr["chunks"] == 1 or pl.kind == "serial"), what
        if pl.kind == "tables" and tr["chunks"] > 1:
            assert (tr["landings"] > 0) == pl.merge, what                        # which walk filled the tables
            assert (tr["distinct_exits"] > 0) == pl.dedupe, what                 # which composition followed them


def test_every_row_reaches_both_edges_of_a_table():
    """exit 0 and exit E - G (nx = CH + E - G: 65534 of 65535 at E = 32767) on every row, by some input"""
    for row in ir.ROWS:
        seen0 = seenmax = False
        for name in ("land", "groups"):
            for inp, pay, pl, starts, end in designed(row, name):
                tr = ir.trace(pay, len(pay), pl, inp.ns)
                seen0, seenmax = seen0 or tr["exit0"], seenmax or (tr["exit_max"] and tr["max_nx_chain"] == pl.CH + pl.E - pl.G)
        assert seen0 and seenmax, row
    pl = ir.plan(633, 42, 0)
    assert pl.CH + pl.E - pl.G == 65534


def test_unreachable_landings_say_so():
    """prefix 4, scalar 8: every slice start is a multiple of 8 and the tables are kept per G = 4 bytes, so b - G and b + G
    are no slice starts: the generator takes the nearest reachable start and the tag names it"""
    (inp,) = ir.inputs(4, 8, "land")
    assert all(f"{k} nearest" in inp.tag for k in ("end_bG", "max_bG", "min_bG")) and "end_b nearest" not in inp.tag, inp.tag
    pay = ir.payload_of(inp)
    pl = ir.plan(4, 8, ir.slot_stride(len(pay)))
    starts, end = ir.walk(pay, len(pay), inp.ns, 4, 8)
    assert end == len(pay) and np.array_equal(ir.emulate(pay, len(pay), pl, inp.ns)[0], starts)


@pytest.mark.parametrize("row,name", CASES, ids=lambda x: str(x))
def test_oracle_accepts_every_designed_payload(oracle, row, name):
    """a condition, not a measurement: the generators make valid streams, whole and within the coefficient bound that
    build_chain's data bytes give (no escape on any decoder form)"""
    for inp, pay, pl, starts, end in designed(row, name):
        ls, cs, ys, xs = ir.shapes(inp.ns)
        y, u, v, q, used = oracle.hq_unpack(np.frombuffer(pay, np.uint8), ls, cs, 1, ys, xs, inp.prefix, inp.scalar)
        assert used == len(pay), (row, name, inp.tag)
        assert max(int(np.abs(p).max()) for p in (y, u, v)) <= ir.COEF_BOUND, (row, name, inp.tag)
        assert 0 <= q.min() and q.max() <= 31
        if name != "min":
            assert any(p.any() for p in (y, u, v)), (row, name, inp.tag)


# ---------------------------------------------------------------------------------------------------------------------
# the batches of tests/test_gpu_index.py that need a plan of their own
# ---------------------------------------------------------------------------------------------------------------------
def test_third_level_and_too_many_inputs():
    (inp,) = ir.inputs(0, 1, "max", ns=4096)
    pay = ir.payload_of(inp)
    starts, end = ir.walk(pay, len(pay), inp.ns, 0, 1)
    pl = ir.plan(0, 1, ir.THIRD_LEVEL_STRIDE)
    assert pl.kind == "tables" and pl.n_groups > 128 and pl.n_supers == 9
    offs, taken = ir.emulate(pay, len(pay), pl, inp.ns)
    assert np.array_equal(offs, starts) and taken == ir.chunk_functions(starts, end, pl)
    tr = ir.trace(pay, len(pay), pl, inp.ns)
    assert tr["supers"] == 2 and tr["groups"] > 16, tr           # over a super-group boundary (2 MiB)
    full = ir.plan(0, 1, ir.FULL_CHAIN_STRIDE)
    assert (full.kind, full.n_groups, full.n_supers) == ("tables", ir.IDX_MAX_GROUPS, ir.IDX_MAX_GROUPS // ir.IDX_GROUP)
    assert np.array_equal(ir.emulate(pay, len(pay), full, inp.ns)[0], starts)
    two = ir.plan(0, 1, ir.slot_stride(len(pay)))
    assert two.n_supers == 0 and np.array_equal(ir.emulate(pay, len(pay), two, inp.ns)[0], starts)   # two levels, same chain
    many = ir.plan(0, 1, ir.TOO_MANY_STRIDE)
    assert (many.kind, many.cause) == ("serial", "too_many")
    assert np.array_equal(ir.emulate(pay, len(pay), many, inp.ns)[0], starts)


# ---------------------------------------------------------------------------------------------------------------------
# wrong copies of emulate(): each must be caught by the inputs named for it
# ---------------------------------------------------------------------------------------------------------------------
CATCHERS = {
    "nx15": [((0, 20), "land"), ((633, 42), "max")],
    "exit14": [((0, 24), "land"), ((633, 42), "land")],
    "cnt4095": [((0, 2), "min"), ((0, 11), "min")],
    "lim_gt": [((0, 1), "mixed"), ((0, 7), "mixed")],
    "drop_last_entry": [((0, 1), "land"), ((0, 7), "land"), ((633, 42), "land")],
    "ept": [((0, 20), "land"), ((538, 10), "land")],
    "group15": [((0, 1), "groups"), ((0, 11), "groups")],
    "super_skip_last": ["third level"],
    "gsh_exits": [((0, 2), "land"), ((0, 20), "land")],
}


def _wrong(pay, pl, ns, starts, end, mut):
    """does the wrong copy show? (a wrong exit can also index past a table, where the kernel would read foreign memory, and a
    wrong nx[] can lead a walk in a circle, where it would never end)"""
    try:
        offs, taken = ir.emulate(pay, len(pay), pl, ns, mut=mut)
    except (IndexError, ir.Stuck):
        return True
    return not np.array_equal(offs, starts) or taken != ir.chunk_functions(starts, end, pl)


@pytest.mark.parametrize("mut", list(ir.MUTANTS))
def test_wrong_copies_are_caught(mut):
    """`lim_gt` changes no offset: the walk past the payload's end only spoils the last chunk's table word, which nothing
    reads.  It is caught by the comparison of the words the chain takes (the last one included), not by the offsets."""
    assert set(CATCHERS) == set(ir.MUTANTS)
    for where in CATCHERS[mut]:
        if where == "third level":
            (inp,) = ir.inputs(0, 1, "max", ns=4096)
            pay = ir.payload_of(inp)
            starts, end = ir.walk(pay, len(pay), inp.ns, 0, 1)
            todo = [(inp, pay, ir.plan(0, 1, ir.THIRD_LEVEL_STRIDE), starts, end)]
        else:
            todo = designed(*where)
        caught = [inp.tag for inp, pay, pl, starts, end in todo if _wrong(pay, pl, inp.ns, starts, end, mut)]
        assert caught, f"{ir.MUTANTS[mut]}: not caught by {where}"
