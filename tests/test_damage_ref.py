"""The conditions that keep tests/test_gpu_damaged.py from being empty, checked against the oracle alone (no GPU): a
comparison of "both refuse" proves little, so every class has to be accepted, or refused, as often and in the way
tests/damage.py says, on every geometry's input; damage that is accepted has to be SEEN in the picture; the long codes and
the wide escape have to be reached; and every generator has to give the same list for the same seed."""
import numpy as np
import pytest

import damage as dm
import proxy_ref as pr

CASES = [(name, cls) for name in dm.INPUTS for cls in dm.input_classes(name)]


@pytest.mark.parametrize("name", list(dm.INPUTS))
def test_the_walk_ends_on_the_payload_and_the_clean_payload_decodes(oracle, name):
    base, _ = dm.load(oracle, name)
    assert base.slices[0].start == 0 and base.slices[-1].end == len(base.payload)
    assert all(a.end == b.start for a, b in zip(base.slices, base.slices[1:]))
    assert len(base.slices) == base.ns
    if base.case.mode != "LD":
        assert dm.hq_walk(base.payload, base.ns, base.case.prefix, base.case.scalar) == base.slices
    # the slice index works on chunks of 8 KiB (scalar 1) or 16 KiB (scalar 2 and more), in groups of 16 chunks: one chunk
    # boundary inside A's payload, many chunks in B1's (16 of 8 KiB: one full group) and E's, more than one group in B2's
    # (19 of 16 KiB)
    chunks = {"A": (8192, 1, 2), "B1": (8192, 15, 16), "B2": (16384, 16, 32), "E": (8192, 3, 4)}
    if name in chunks:
        size, lo, hi = chunks[name]
        assert dm.index_chunk(base.case.prefix, base.case.scalar) == size, name
        assert lo * size < len(base.payload) <= hi * size, (name, len(base.payload))
    if base.chunk:   # the chunk-boundary mutations stand on a boundary of THIS input's chunks, inside the payload
        for cls in ("random", "length"):
            tags = [m.tag for m in dm.mutations(base, cls, dm.SEED) if "chunk boundary" in m.tag]
            assert len(tags) == 2, (name, cls, tags)
            b = int(tags[0].split("chunk boundary ")[1].split()[0])
            assert b % base.chunk == 0 and 0 < b < len(base.payload), (name, cls, b)
    want, n = oracle.decode_stream(base.case.params(), oracle.encode_stream(base.case.params(), base.raw, 1), 1)
    assert n == 1 and dm.clean_picture(oracle, name) == want


@pytest.mark.parametrize("name,cls", CASES, ids=[f"{n}-{c}" for n, c in CASES])
def test_class_conditions(oracle, name, cls):
    base, _ = dm.load(oracle, name)
    refs = dm.references(oracle, name, cls)
    clean = dm.clean_picture(oracle, name)
    ok = [r for r in refs if r[1] == "ok"]
    print(f"{name} {cls}: {len(ok)} of {len(refs)} accepted")
    assert all(len(pic) == base.case.raw_bytes() for _, _, pic in ok)
    if cls in dm.MIN_ACCEPTED:
        assert len(ok) >= dm.MIN_ACCEPTED[cls] * len(refs), f"{name} {cls}: the oracle accepts {len(ok)} of {len(refs)}"
    if cls == "qindex":
        for m, verdict, res in refs:
            v = int(m.tag.rsplit(" ", 1)[1])
            assert (verdict, v <= 119) in (("ok", True), ("refused", False)), (name, m.tag, verdict, res)
            assert verdict == "ok" or res == dm.EQINDEX, (name, m.tag, res)
    if cls == "short":
        assert [(v, code) for _, v, code in refs] == [("refused", dm.ESTREAM)] * len(refs), (name, [(m.tag, v, c) for m, v, c in refs])
    if cls in ("boundary", "run00", "runff"):
        same = [m.tag for m, _, pic in ok if pic == clean]
        assert not same, f"{name} {cls}: damage that the picture does not show: {same}"
    if cls == "long":
        assert all(pic == clean for _, _, pic in ok), name
    if cls == "run00":   # the branch for codes beyond 32 bits and the escape of values far outside +-65534 are reached
        peak = 0
        for m, verdict, _ in refs:
            if verdict == "ok":
                y, u, v, _ = pr.quantised_planes(oracle, base.case, dm.visible(base, m))
                peak = max(peak, max(int(np.abs(p.astype(np.int64)).max()) for p in (y, u, v)))
        assert peak > 65534, f"{name}: no run00 case codes a value beyond +-65534 (largest {peak})"
    if name == "D":
        assert len(refs) <= 12


def test_cbr_claim_holds_on_boundary_and_fails_on_length(oracle):
    """E: what the decoder's check of the HQ_CBR byte budgets (k_cbr_index_check) must decide, restated on the CPU.  The
    clean payload and every `boundary` mutation keep every slice on its budget, so the batch of them decodes from the
    claimed offsets; a changed length byte, and any other d_lens, breaks the claim for its batch, which then goes through
    the general index.  The decision itself is a word in device memory that no call reports: the GPU test cannot see it."""
    base, _ = dm.load(oracle, "E")
    assert dm.cbr_claim_holds(oracle, base, dm.clean(base))
    assert all(dm.cbr_claim_holds(oracle, base, m) for m in dm.mutations(base, "boundary", dm.SEED))
    for cls in ("length", "short", "long"):
        broken = [m for m in dm.mutations(base, cls, dm.SEED) if m.data != base.payload or m.length != len(base.payload)]
        assert len(broken) >= 3 and not any(dm.cbr_claim_holds(oracle, base, m) for m in broken), cls
    # and among the accepted `length` payloads (one batch on the GPU) at least one breaks it: that batch takes the fall-back
    acc = [m for m, verdict, _ in dm.references(oracle, "E", "length") if verdict == "ok"]
    assert any(not dm.cbr_claim_holds(oracle, base, m) for m in acc), [m.tag for m in acc]


def test_ld_headers_reach_the_shifted_slices(oracle):
    """some header mutation the oracle ACCEPTS carries a luma length beyond its slice: the decoder's flag, serial walk and
    second pass then have a picture to get right, not only a refusal.  (F1's slices of 31 bytes leave the length field
    22 values beyond the slice, and none of its accepted mutations lands there; F2's do.)"""
    hits = {}
    for name in ("F1", "F2"):
        base, _ = dm.load(oracle, name)
        assert not dm.ld_shifted(oracle, base, dm.clean(base))
        hits[name] = [m.tag for cls in ("hdr0", "hdr1") for m, verdict, _ in dm.references(oracle, name, cls)
                      if verdict == "ok" and dm.ld_shifted(oracle, base, m)]
    print(f"accepted header mutations with shifted slices: {hits}")
    assert hits["F2"], hits


def test_geometry_d_stays_within_thirty_mutations(oracle):
    base, _ = dm.load(oracle, "D")
    assert sum(len(dm.input_mutations(base, "D", cls)) for cls in dm.D_CLASSES) <= 30


@pytest.mark.parametrize("name", ["A", "B2", "F1"])
def test_generators_are_deterministic(oracle, name):
    base, _ = dm.load(oracle, name)
    other = dm.INPUTS[name](oracle)
    assert other.payload == base.payload and other.slices == base.slices
    for cls in dm.input_classes(name):
        a, b = dm.mutations(base, cls, 7), dm.mutations(other, cls, 7)
        assert a == b, (name, cls)
    assert dm.mutations(base, "random", 7) != dm.mutations(base, "random", 8)


def test_boundary_moves_keep_the_chain(oracle):
    """a moved border changes two length bytes and re-splits the data: same slice ends, same bytes in the same order"""
    base, _ = dm.load(oracle, "B1")
    muts = dm.mutations(base, "boundary", 0)
    assert len(muts) == 45
    for m in muts:
        walk = dm.hq_walk(m.data, base.ns, base.case.prefix, base.case.scalar)
        assert [(s.start, s.end) for s in walk] == [(s.start, s.end) for s in base.slices], m.tag
        changed = [i for i, (a, b) in enumerate(zip(walk, base.slices)) if m.data[a.start:a.end] != base.payload[b.start:b.end]]
        assert len(changed) == 1, m.tag
        a, b = walk[changed[0]], base.slices[changed[0]]
        strip = lambda pay, s: b"".join(pay[p + 1:p + 1 + pay[p] * base.case.scalar] for p in s.lenpos)
        assert strip(m.data, a) == strip(base.payload, b), m.tag
        assert sum(x != y for x, y in zip((m.data[p] for p in a.lenpos), (base.payload[p] for p in b.lenpos))) == 2, m.tag


def test_class_sizes(oracle):
    base, _ = dm.load(oracle, "B1")
    n = {cls: len(dm.mutations(base, cls, dm.SEED)) for cls in dm.HQ_CLASSES}
    assert n == {"random": 26, "boundary": 45, "length": 77, "qindex": 27, "run00": 24, "runff": 12, "short": 6, "long": 3}, n
    base, _ = dm.load(oracle, "F1")
    n = {cls: len(dm.mutations(base, cls, dm.SEED)) for cls in dm.LD_CLASSES}
    assert n == {"random": 24, "hdr0": 16, "hdr1": 16, "body00": 4, "bodyff": 4}, n
