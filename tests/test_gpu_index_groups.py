"""The slice index's anchors and followers, against the CPU oracle, on chains designed for their edges.

Of every group of 16 chunks only the first (the anchor) gets a table for every entry offset; the other fifteen are walked
by k_index_follow from the few offsets at which chains leave the anchor, deduplicated again at every chunk boundary.  The
chains here stand on what that adds to the plans tests/test_gpu_index.py pins; what each reaches is asserted on the CPU with
a plain walk before anything runs on the GPU:

  - edges: a payload of a little over two groups whose true chain enters a follower chunk at offset 0 and at E - G (behind a
    maximal slice that starts G before the boundary), enters an anchor at E - G and at 0, and puts maximal slices over the
    boundaries anchor -> first follower, last follower -> anchor.  (The longest slice of a plan is E <= CH / 2 bytes, so no
    slice can lie over more than one chunk boundary: asserted.)
  - ends: payloads that end inside a follower chunk, inside the anchor of the second group, and exactly on a group boundary;
    a length beyond the slot stride raises the stream error and leaves the neighbours alone.
  - apart: payloads of one repeated byte.  Every position then reads the same three length bytes, every walk advances by the
    same L bytes, and walks that start at different residues mod L never meet: 331 chains (more than the follower has
    threads: its passes) and 149 chains survive every group.
  - one row per start granularity (scalar 1, 2, 8) and per chunk size (8, 16, 32 KiB; the 32 KiB chunks keep a table per chunk).
  - a slot stride that takes the third chain level, and batches of different chains side by side over 1 and 2 lanes."""
import numpy as np
import pytest

import index_ref as ir
import test_gpu_index as gi

pytestmark = pytest.mark.gpu
ctxs = gi.ctxs                               # the shared contexts by (flags, lanes): that file's fixture

ROWS = [(0, 1), (0, 2), (0, 8), (0, 20)]     # 8 KiB G 1, 16 KiB G 2, 16 KiB G 4, 32 KiB G 4
END_ROWS = [(0, 1), (0, 2), (0, 8)]          # rows where a whole picture's slices can end exactly on a group boundary
APART_ROWS = [(255, 1), (1, 2)]              # odd prefix + 4: G 1, so every byte of a period is a start of its own chain
APART_BYTE = 0x18


# ---------------------------------------------------------------------------------------------------------------------
# designs (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def entries_of(payload, length, ns, pl):
    """plain walk -> (slice starts, end, per live chunk the offset at which the true chain enters it)"""
    starts, end = ir.walk(payload, length, ns, pl.prefix, pl.scalar)
    fn = ir.chunk_functions(starts, end, pl)
    return starts, end, [0] + [x for x, _ in fn[:-1]]


def edges(row):
    """-> (ns, payload) of the `edges` chain of a row"""
    pl = ir.plan(*row, 0)
    P, s, G, CH, E = pl.prefix + 4, pl.scalar, pl.G, pl.CH, pl.E
    ns = 1024 if E <= 8191 else 256
    units, pos = [], 0
    for kmin, d, extra in ((2, 0, None), (4, -G, 765), (15, -G, 765), (16, -G, 765), (17, -G, 765), (20, 0, None), (32, 0, None)):
        k, t, f, note = ir._target(pl, pos, kmin, d)
        assert k == kmin and not note, (row, kmin, d, k, note)
        units += f
        pos = t
        if extra is not None:
            units.append(extra)
            pos += P + s * extra
    while pos <= 32 * CH + E:
        units.append(765)
        pos += P + s * 765
    assert len(units) <= ns, (row, len(units))
    units += [0] * (ns - len(units))
    pay = ir.build_chain(ns, pl.prefix, s, ir._split(units, np.random.default_rng(ir.SEED)), ir.SEED)
    starts, end, ent = entries_of(pay, len(pay), ns, pl)
    assert end == len(pay) and len(ent) == 2 * ir.IDX_GROUP + 1, (row, len(ent))
    follower = lambda c: c % ir.IDX_GROUP != 0
    assert ent[2] == 0 and follower(2) and ent[20] == 0 and follower(20), (row, ent)
    assert ent[4] == E - G and follower(4) and ent[15] == E - G and follower(15) and ent[17] == E - G and follower(17), (row, ent)
    assert ent[16] == E - G and ent[32] == 0, (row, ent)
    sizes = np.diff(np.concatenate([starts, [end]]))
    assert sizes.max() == E and 2 * E <= CH + (CH if E > 8191 else 0)     # the longest slice lies over one boundary at most
    for b in (4, 15, 16, 17):                                            # a maximal slice over each of these boundaries
        i = np.searchsorted(starts, b * CH - G)
        assert starts[i] == b * CH - G and sizes[i] == E, (row, b)
    return ns, pay


def ending_at(row, D, ns):
    """ns slices that are exactly D bytes long together"""
    pl = ir.plan(*row, 0)
    u = ir._fit(D, ns, pl.prefix + 4, pl.scalar)
    assert u is not None, (row, D, ns)
    pay = ir.build_chain(ns, pl.prefix, pl.scalar, ir._split(ir._spread(u, ns), np.random.default_rng(ir.SEED + D % 9973)), ir.SEED)
    assert len(pay) == D
    return pay


def ends(row, ns):
    """[(tag, payload)]: ends inside a follower chunk, inside the second group's anchor, exactly on a group boundary"""
    pl = ir.plan(*row, 0)
    CH, GR = pl.CH, ir.IDX_GROUP
    out = [("follower", ending_at(row, (GR + 2) * CH + 512, ns)), ("anchor", ending_at(row, GR * CH + 512, ns)),
           ("boundary", ending_at(row, GR * CH, ns))]
    for tag, pay in out:
        starts, end, ent = entries_of(pay, len(pay), ns, pl)
        last = (end - 1) // CH                                           # the chunk of the payload's last byte
        assert end == len(pay) and last == {"follower": GR + 2, "anchor": GR, "boundary": GR - 1}[tag], (row, tag, last)
        assert (end % (GR * CH) == 0) == (tag == "boundary")
    return out


def apart(row):
    """-> (ns, payload, chains that survive the first group) of the `apart` stream of a row"""
    pl = ir.plan(*row, 0)
    L = pl.prefix + 4 + 3 * APART_BYTE * pl.scalar
    ns = 1024 if pl.CH == 8192 else 4096
    pay = bytes([APART_BYTE]) * (ns * L)
    assert len(pay) > 2 * ir.IDX_GROUP * pl.CH + pl.E
    starts, end = ir.walk(pay, len(pay), ns, pl.prefix, pl.scalar)
    assert end == len(pay) and (np.diff(starts) == L).all()
    survivors, data = [], np.frombuffer(pay, np.uint8).astype(np.int64)
    for g in range(2):                                                   # from every entry offset of a group's anchor to the group's end
        pos, stop = g * ir.IDX_GROUP * pl.CH + np.arange(0, pl.E, pl.G), (g + 1) * ir.IDX_GROUP * pl.CH
        while (pos < stop).any():                                        # one hop of every walk that is still inside the group
            on = pos < stop
            q = pos[on] + pl.prefix + 1
            for _ in range(3):
                q = q + 1 + data[q] * pl.scalar
            pos[on] = q
        survivors.append(np.unique(pos).size)
    assert min(survivors) >= 100 and survivors[0] == L // pl.G, (row, survivors, L)
    return ns, pay, min(survivors)


_MADE = {}


def made(fn, *args):
    if (fn.__name__,) + args not in _MADE:
        _MADE[(fn.__name__,) + args] = fn(*args)
    return _MADE[(fn.__name__,) + args]


# ---------------------------------------------------------------------------------------------------------------------
# through vc2hip_hq_unpack and vc2hip_decode_batch_dev
# ---------------------------------------------------------------------------------------------------------------------
def check_unpack(hip, oracle, row, ns, pay, what):
    data = np.frombuffer(pay, np.uint8)
    ls, cs, ys, xs = ir.shapes(ns)
    ref = oracle.hq_unpack(data, ls, cs, 1, ys, xs, *row)
    got = hip.hq_unpack(data, ls, cs, 1, ys, xs, *row)
    assert ref[4] == data.size and got[4] == ref[4], f"{what}: consumed {got[4]}, the oracle {ref[4]} of {data.size}"
    assert np.array_equal(got[3], ref[3]), f"{what}: {int((got[3] != ref[3]).sum())} quantiser indices differ"
    for c in range(3):
        bad = np.argwhere(got[c] != ref[c])
        assert not bad.size, f"{what}: component {c}: {len(bad)} coefficients differ, the first at {bad[0].tolist()}"


@pytest.mark.parametrize("row", ROWS, ids=str)
def test_edges(ctxs, oracle, row):
    ns, pay = made(edges, row)
    check_unpack(ctxs(), oracle, row, ns, pay, f"{row} edges")
    gi.check_batch(ctxs(), oracle, gi.case_of(oracle, ns, *row), [(row + ("edges", ns), pay)], f"{row} edges")


@pytest.mark.parametrize("row", END_ROWS, ids=str)
def test_ends(ctxs, oracle, row):
    """the three ends side by side in one call, each also alone through vc2hip_hq_unpack (there the slot ends with the payload)"""
    ns = 256 if row[1] < 8 else 64
    items = made(ends, row, ns)
    for tag, pay in items:
        check_unpack(ctxs(), oracle, row, ns, pay, f"{row} ends in {tag}")
    gi.check_batch(ctxs(), oracle, gi.case_of(oracle, ns, *row), [(row + ("ends", tag, ns), pay) for tag, pay in items], f"{row} ends")


def test_length_beyond_the_stride_raises(ctxs, oracle):
    """the three ends of scalar 2 in one call, the middle picture's length one byte beyond the slot stride: the call reports
    the stream error, and the pictures beside it are the oracle's"""
    import torch
    row, ns = (0, 2), 256
    items = made(ends, row, ns)
    hip, case = ctxs(), gi.case_of(oracle, ns, *row)
    fmt, cp = case.fmt_cp(hip.lib)
    stride = (max(len(p) for _, p in items) + 64 + 255) // 256 * 256
    d_pay = torch.full((3 * stride,), 0xA5, dtype=torch.uint8, device="cuda:0")
    for i, (_, p) in enumerate(items):
        d_pay[i * stride:i * stride + len(p)] = torch.from_numpy(np.frombuffer(p, np.uint8).copy()).to("cuda:0")
    d_len = torch.tensor([len(items[0][1]), stride + 1, len(items[2][1])], dtype=torch.int64, device="cuda:0")
    step = case.raw_bytes()
    d_out = torch.zeros(3 * step, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), 3, fmt, cp, d_out.data_ptr())
    with pytest.raises(Exception):
        hip.sync()
    out = d_out.cpu().numpy().tobytes()
    for i in (0, 2):
        assert out[i * step:(i + 1) * step] == gi.picture(oracle, case, row + ("ends", items[i][0], ns), items[i][1]), items[i][0]
    # the context is usable afterwards
    gi.check_batch(hip, oracle, case, [(row + ("ends", tag, ns), pay) for tag, pay in items], f"{row} ends, after the error")


@pytest.mark.parametrize("row", APART_ROWS, ids=str)
def test_chains_that_never_meet(ctxs, oracle, row):
    ns, pay, survivors = made(apart, row)
    what = f"{row} apart, {survivors} chains"
    check_unpack(ctxs(), oracle, row, ns, pay, what)
    gi.check_batch(ctxs(), oracle, gi.case_of(oracle, ns, *row), [(row + ("apart", ns), pay)], what)


def side_by_side():
    row, ns = (0, 1), 1024
    n, pay = made(edges, row)
    assert n == ns
    items = [(row + ("edges", ns), pay)] + [(row + ("ends", tag, ns), p) for tag, p in made(ends, row, ns)]
    items.append((row + ("ends", "first anchor", ns), ending_at(row, 6000, ns)))
    assert len({len(p) for _, p in items}) == len(items) == 5 and len(items[-1][1]) < ir.plan(*row, 0).CH
    return row, ns, items


@pytest.mark.parametrize("lanes", [1, 2])
def test_batch_of_different_chains(ctxs, oracle, lanes):
    """scalar 1: the edges chain (33 chunks), the three ends and a payload that ends in the first anchor in one call"""
    row, ns, items = side_by_side()
    gi.check_batch(ctxs((), lanes), oracle, gi.case_of(oracle, ns, *row), items, f"{row} side by side, {lanes} lanes")


@pytest.mark.parametrize("stride", [None, ir.THIRD_LEVEL_STRIDE], ids=["two levels", "three levels"])
def test_chain_levels(oracle, stride):
    """the same call in slots of its own size (3 groups: followed directly) and in slots of 2048 chunks (129 groups: composed
    into super-groups); which kernels ran, by name from the profile"""
    from vc2hip_py import Vc2Hip
    row, ns, items = side_by_side()
    pl = ir.plan(*row, stride or (max(len(p) for _, p in items) + 64 + 255) // 256 * 256)
    assert pl.kind == "tables" and (pl.n_groups, pl.n_supers) == ((129, 9) if stride else (3, 0))
    hip = Vc2Hip()
    try:
        seen = gi.profiled(hip, lambda: gi.check_batch(hip, oracle, gi.case_of(oracle, ns, *row), items, f"{pl.n_groups} groups", stride))
    finally:
        hip.close()
    assert gi.GENERAL <= seen and "slice_index_serial" not in seen, sorted(seen)
