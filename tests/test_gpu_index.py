"""The slice index on every plan, against the CPU oracle, on designed length chains (tests/index_ref.py).

vc2_launch_slice_index picks what it launches from (prefix, scalar, payload stride) alone: chunk size, start granularity,
merged or plain entry walks, deduped or plain group composition, two or three chain levels, or the serial walk.  Every row
of index_ref.ROWS is one such plan; every generator designs a chain that stands on an edge of it (what each reaches is
asserted without a GPU in tests/test_index_ref.py).

  - single chains: every row x generator through vc2hip_hq_unpack, compared with the oracle's hq_unpack exactly -- the
    three coefficient planes, the quantiser indices and the bytes consumed.  The picture is the smallest of that many
    slices: depth 1, luma 4 x 4 and chroma 2 x 2 coefficients per slice.
  - batches through vc2hip_decode_batch_dev, every picture against proxy_ref.full_picture, slots filled with 0xA5 behind
    their lengths, the output between two guards: chains of different kinds side by side, over 1, 2 and 3 lanes; a slot
    stride that takes the third chain level, and the largest one the chain kernel holds groups for; the next stride beyond
    it (the serial walk); a chain shaped like an HQ_CBR picture, every slice on its budget, with and without the claim.
  - which kernels ran, by name from the profile, once per plan kind on a fresh context."""
import numpy as np
import pytest

import index_ref as ir
import proxy_ref as pr

pytestmark = pytest.mark.gpu

GUARD = 4096
GENERAL = {"slice_index_tables", "slice_index_chain", "slice_index_emit"}


@pytest.fixture(scope="module")
def ctxs():
    """contexts by (flags, lanes), made on first use and shared by the cases of this file"""
    from vc2hip_py import FLAGS, Vc2Hip
    made = {}

    def get(flags=(), lanes=1):
        key = (tuple(flags), lanes)
        if key not in made:
            made[key] = Vc2Hip(flags=sum(FLAGS[f] for f in flags))
            if lanes > 1:
                made[key].set_streams(lanes)
        return made[key]

    yield get
    for hip in made.values():
        hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# single chains through vc2hip_hq_unpack
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}


def chains(oracle, row, name):
    """[(input, payload bytes as an array, the oracle's (y, u, v, indices, consumed))] of one generator on one row; shared"""
    if (row, name) not in _REF:
        out = []
        for inp in ir.inputs(*row, name):
            data = np.frombuffer(ir.payload_of(inp), np.uint8)
            assert data.size <= ir.MAX_PAYLOAD
            ls, cs, ys, xs = ir.shapes(inp.ns)
            ref = oracle.hq_unpack(data, ls, cs, 1, ys, xs, inp.prefix, inp.scalar)
            assert ref[4] == data.size and max(int(np.abs(p).max()) for p in ref[:3]) <= ir.COEF_BOUND, (row, name, inp.tag)
            out.append((inp, data, ref))
        _REF[(row, name)] = out
    return _REF[(row, name)]


def check_unpack(hip, oracle, row, name, variant="default"):
    for inp, data, ref in chains(oracle, row, name):
        ls, cs, ys, xs = ir.shapes(inp.ns)
        got = hip.hq_unpack(data, ls, cs, 1, ys, xs, inp.prefix, inp.scalar)
        what = f"{row} {name} [{inp.tag}] [{variant}] {inp.ns} slices, {data.size} bytes"
        assert got[4] == ref[4], f"{what}: consumed {got[4]}, the oracle {ref[4]}"
        assert np.array_equal(got[3], ref[3]), f"{what}: {int((got[3] != ref[3]).sum())} quantiser indices differ"
        for c in range(3):
            bad = np.argwhere(got[c] != ref[c])
            assert not bad.size, f"{what}: component {c}: {len(bad)} coefficients differ, the first at {bad[0].tolist()}"


CASES = [(row, name) for row in ir.ROWS for name in ir.GENERATORS]


@pytest.mark.parametrize("row,name", CASES, ids=lambda x: str(x))
def test_chain_through_hq_unpack(ctxs, oracle, row, name):
    check_unpack(ctxs(), oracle, row, name)


# one row per chunk size: 8, 16 and 32 KiB
FLAG_ROWS = [(0, 1), (0, 4), (0, 20)]


@pytest.mark.parametrize("flag", ["STORE32", "PLANES8_NEVER"])
@pytest.mark.parametrize("row", FLAG_ROWS, ids=str)
def test_chain_through_hq_unpack_on_other_contexts(ctxs, oracle, row, flag):
    """the flags change the kernels that consume the offsets, not the index"""
    for name in ("mixed", "land"):
        check_unpack(ctxs((flag,)), oracle, row, name, flag)


# ---------------------------------------------------------------------------------------------------------------------
# batches through vc2hip_decode_batch_dev
# ---------------------------------------------------------------------------------------------------------------------
def case_of(oracle, ns, prefix, scalar, **kw):
    """the smallest picture of ns slices: 4:2:0, 8 bits in 1-byte words, LeGall at depth 1, slices of 4 x 4 luma samples"""
    ys, xs = ir.GEOMS[ns]
    c = pr.Case(oracle, 4 * xs, 4 * ys, "420", 8, "LeGall", 1, 2, 2, scalar=scalar, prefix=prefix, word_bytes=1, **kw)
    assert (c.ys, c.xs) == (ys, xs)
    return c


_PICS = {}


def picture(oracle, case, key, payload):
    if key not in _PICS:
        _PICS[key] = pr.full_picture(oracle, case, payload)
    return _PICS[key]


def decode_batch(hip, case, payloads, stride=None):
    """one vc2hip_decode_batch_dev call over the payloads, each in a slot that is 0xA5 behind its length
    -> (the pictures' bytes, guards intact)"""
    import torch
    fmt, cp = case.fmt_cp(hip.lib)
    n = len(payloads)
    stride = stride or (max(len(p) for p in payloads) + 64 + 255) // 256 * 256
    assert stride % 256 == 0 and all(len(p) <= stride for p in payloads)
    d_pay = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device="cuda:0")
    for i, p in enumerate(payloads):
        d_pay[i * stride:i * stride + len(p)] = torch.from_numpy(np.frombuffer(p, np.uint8).copy()).to("cuda:0")
    d_len = torch.tensor([len(p) for p in payloads], dtype=torch.int64, device="cuda:0")
    total = n * case.raw_bytes()
    buf = torch.full((GUARD + total + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()   # (torch fills on its stream, the library works on its own)
    hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, fmt, cp, buf.data_ptr() + GUARD)
    hip.sync()
    host = buf.cpu().numpy()
    guards = bool((host[:GUARD] == 0x5A).all() and (host[GUARD + total:] == 0x5A).all())
    return host[GUARD:GUARD + total].tobytes(), guards


def check_batch(hip, oracle, case, items, what, stride=None):
    """items: [(key, payload)]; every picture of the call against the oracle's"""
    got, guards = decode_batch(hip, case, [p for _, p in items], stride)
    step = case.raw_bytes()
    bad = [key for i, (key, p) in enumerate(items) if got[i * step:(i + 1) * step] != picture(oracle, case, key, p)]
    assert not bad, f"{what}: {len(bad)} of {len(items)} pictures differ from the oracle's: {bad}"
    assert guards, f"{what}: bytes outside the output were written"


def profiled(hip, fn):
    hip.profile_reset()
    hip.profile_enable(True)
    fn()
    hip.profile_enable(False)
    return {k for k, v in hip.profile().items() if v[0] > 0}


# `short` needs 1024 * 4 bytes < E; both `end` payloads need a row where 1024 slices can end on a boundary and 1023 too
SIDE_ROW, SIDE_NS = (0, 7), 1024


def side_by_side(row=SIDE_ROW, ns=SIDE_NS):
    """chains of different kinds for one call: `short`, `groups`, both `end` payloads, `land`, `mixed`, `max`"""
    items = []
    for name in ("short", "groups", "end", "land", "mixed", "max"):
        for inp in ir.inputs(*row, name, ns=ns):
            assert "nearest" not in inp.tag, (row, name, inp.tag)
            items.append((row + (name, inp.tag, ns), ir.payload_of(inp)))
    assert len({len(p) for _, p in items}) == len(items)
    return items


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_batch_of_different_chains(ctxs, oracle, lanes):
    """payloads of 5 KB to 5 MB in one call: the chunks of most slots lie behind their pictures' ends; over 2 and 3 lanes
    the call is split between the lanes' own index workspaces"""
    items = side_by_side()
    assert len(items) == 7 and min(len(p) for _, p in items) < ir.plan(*SIDE_ROW, 0).E < 100 * 16384 < max(len(p) for _, p in items)
    case = case_of(oracle, SIDE_NS, *SIDE_ROW)
    check_batch(ctxs((), lanes), oracle, case, items, f"{SIDE_ROW} side by side, {lanes} lanes")


@pytest.mark.parametrize("flag", ["default", "STORE32", "PLANES8_NEVER"])
@pytest.mark.parametrize("row", FLAG_ROWS, ids=str)
def test_batch_per_chunk_size(ctxs, oracle, row, flag):
    """one row per chunk size through the batch decoder, on the default context and the two other stores"""
    ns = 1024 if row[1] == 1 else 256
    items = [(row + (name, inp.tag, ns), ir.payload_of(inp)) for name in ("mixed", "land", "end") for inp in ir.inputs(*row, name, ns=ns)]
    assert not any("nearest" in key[3] for key, _ in items) and len({len(p) for _, p in items}) == len(items)
    check_batch(ctxs(() if flag == "default" else (flag,)), oracle, case_of(oracle, ns, *row), items, f"{row} [{flag}]")


@pytest.mark.parametrize("stride", [ir.THIRD_LEVEL_STRIDE, ir.FULL_CHAIN_STRIDE], ids=["129 groups", "1024 groups"])
def test_batch_third_chain_level(oracle, stride):
    """scalar 1, slots of 2048 chunks of 8 KiB: 129 groups, so the groups are composed into super-groups and the chain
    runs in three levels.  4096 maximal slices are 3.1 MB: over a super-group boundary (2 MiB).  Beside it a `mixed` and
    a `land` chain that end inside the first super-group.  The same in slots of 16383 chunks: 16384 chunks with the one
    the launcher adds, 1024 groups and 64 super-groups -- the last elements of k_index_chain's two arrays."""
    from vc2hip_py import Vc2Hip
    pl = ir.plan(0, 1, stride)
    assert pl.kind == "tables" and (pl.n_groups, pl.n_supers) == ((129, 9) if stride == ir.THIRD_LEVEL_STRIDE else (1024, 64))
    items = [((0, 1, name, inp.tag, 4096), ir.payload_of(inp)) for name in ("max", "mixed", "land") for inp in ir.inputs(0, 1, name, ns=4096)]
    assert len(items[0][1]) > 256 * 8192
    hip = Vc2Hip()
    try:
        seen = profiled(hip, lambda: check_batch(hip, oracle, case_of(oracle, 4096, 0, 1), items, f"third chain level, {pl.n_groups} groups", stride))
    finally:
        hip.close()
    assert GENERAL <= seen and "slice_index_serial" not in seen, sorted(seen)


def test_batch_too_many_chunks_takes_the_serial_walk(oracle):
    """scalar 1, slots of 16383 chunks of 8 KiB and 256 bytes (128 MiB): the launcher counts ceil(stride / CH) + 1 = 16385
    chunks, the first count beyond the 1024 groups k_index_chain holds, so it takes the serial walk although E is small
    (test_batch_third_chain_level's second stride is 256 bytes less: the last one on the tables).  Two small pictures."""
    from vc2hip_py import Vc2Hip
    assert ir.plan(0, 1, ir.TOO_MANY_STRIDE).cause == "too_many" and ir.plan(0, 1, ir.TOO_MANY_STRIDE - 256).kind == "tables"
    items = [((0, 1, name, inp.tag, 1024), ir.payload_of(inp)) for name in ("land", "mixed") for inp in ir.inputs(0, 1, name, ns=1024)]
    hip = Vc2Hip()
    try:
        seen = profiled(hip, lambda: check_batch(hip, oracle, case_of(oracle, 1024, 0, 1), items, "too many chunks", ir.TOO_MANY_STRIDE))
    finally:
        hip.close()
    assert "slice_index_serial" in seen and not (GENERAL & seen), sorted(seen)


def cbr_shaped(oracle, case, seed=ir.SEED):
    """a chain on the budgets of an HQ_CBR picture: slice i is prefix + budget[i] bytes long"""
    budgets = oracle.slice_bytes(case.ys, case.xs, case.s, case.scalar).ravel().astype(np.int64)
    assert ((budgets - 4) % case.scalar == 0).all() and budgets.min() >= 4 and budgets.max() <= 4 + 765 * case.scalar
    lens = ir._split((budgets - 4) // case.scalar, np.random.default_rng(seed))
    pay = ir.build_chain(budgets.size, case.prefix, case.scalar, lens, seed)
    assert len(pay) == int(budgets.sum()) + budgets.size * case.prefix
    return pay


@pytest.mark.parametrize("flags", [(), ("NO_CBR_INDEX",)], ids=["claim", "NO_CBR_INDEX"])
def test_batch_cbr_shaped_chain(oracle, flags):
    """1024 slices on the budgets of 307237 bytes (300 or 301 each, 37 chunks of 8 KiB): the decoder takes the offsets from
    the budgets and checks them against the length bytes (slice_index_cbr); with NO_CBR_INDEX the general index runs.  A
    second payload on the same budgets with other length bytes in the same call."""
    from vc2hip_py import FLAGS, Vc2Hip
    case = case_of(oracle, 1024, 0, 1, mode="HQ_CBR", s=307237)
    items = [(("cbr", seed), cbr_shaped(oracle, case, seed)) for seed in (ir.SEED, ir.SEED + 1)]
    hip = Vc2Hip(flags=sum(FLAGS[f] for f in flags))
    try:
        seen = profiled(hip, lambda: check_batch(hip, oracle, case, items, f"HQ_CBR-shaped {flags}"))
    finally:
        hip.close()
    if flags:
        assert GENERAL <= seen and "slice_index_cbr" not in seen, sorted(seen)
    else:
        assert "slice_index_cbr" in seen and "slice_index_serial" not in seen, sorted(seen)


# ---------------------------------------------------------------------------------------------------------------------
# which path ran
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [(0, 1), (0, 11), (633, 42), (634, 42), (0, 43)], ids=str)
def test_index_kernels_by_plan(oracle, row):
    """from the profile of one vc2hip_hq_unpack call on a fresh context: the chunk tables, the chain and the emit kernel
    where plan() says `tables` (E = 32767 included), the serial walk alone where it says `serial` (from E = 32768 on)"""
    from vc2hip_py import Vc2Hip
    (inp, data, ref), = chains(oracle, row, "land")
    pl = ir.plan(*row, ir.slot_stride(data.size))
    hip = Vc2Hip()
    try:
        seen = profiled(hip, lambda: check_unpack(hip, oracle, row, "land", "fresh"))
    finally:
        hip.close()
    if pl.kind == "tables":
        assert GENERAL <= seen and "slice_index_serial" not in seen, f"{row}: {sorted(seen)}"
    else:
        assert "slice_index_serial" in seen and not (GENERAL & seen), f"{row}: {sorted(seen)}"
