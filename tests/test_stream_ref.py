"""tests/stream_ref.py on its own, no GPU: the walk model against the oracle's streams, the designed accepted streams against the
oracle's decoder, the census of what the designed sets reach, and the wrong copies of the walk the sets must catch.

Designed accepted streams the oracle cannot parse (each case carries the reason as oracle_no; the model's payloads are still
held against the source pictures):
  * the identity asymmetric flags: the oracle reads the two flags as bare bits;
  * streams without a sequence header (the rest of a stream after a first call, and the "version given" cases): the oracle
    assumes major version 2 where the call is given 3;
  * a slice fragment without data whose slice travels in the next fragment: the oracle parses the slices of each fragment.
A stream whose sequence header disagrees with the version given to the call is no such case: the oracle reads the stream's."""
import pytest

import stream_ref as sr
from test_gpu_stream_dev import CASES


@pytest.fixture(scope="module")
def S(oracle):
    return sr.sources(oracle)


@pytest.fixture(scope="module")
def sets(S):
    return sr.accepted(S), sr.refused(S)


ORACLE_STREAMS = [(case, None, 7) for case in CASES] + [("cbr_legall_420_8", 300, 8), ("ld_legall_420_8", 200, 8),
                                                        ("cbr_legall_420_8", 10 ** 6, 8)]


@pytest.mark.parametrize("case,frag,seed", ORACLE_STREAMS)
def test_model_reads_the_oracles_streams(oracle, case, frag, seed):
    """the streams of test_gpu_stream_dev: payloads = the unit bodies behind the transform parameters, numbers, consumed"""
    over = dict(fragment_length=frag) if frag else {}
    cp, p, stream = sr.oracle_stream(oracle, CASES[case], 3, seed, **over)
    plain = sr.oracle_stream(oracle, CASES[case], 3, seed)[2]
    want = sr.want_of(oracle, cp)
    res = sr.walk(stream, len(stream), 3, want)
    assert res.ok, (res.reason, res.at)
    assert res.payloads == sr.oracle_payloads(cp, plain, 3)
    assert res.numbers == [0, 1, 2] and res.consumed == len(stream) - 13 and res.lens == [len(x) for x in res.payloads]
    if frag:
        assert {c for c, _ in sr.units_of(stream)} & {sr.HQ_FRAG, sr.LD_FRAG}
        assert max(len(s) for s in res.segs) > 1 or frag == 10 ** 6
    for n in (1, 2):   # fewer pictures: consumed is the end of the n-th
        part = sr.walk(stream, len(stream), n, want)
        assert part.ok and part.payloads == res.payloads[:n]
        rest = sr.walk(stream[part.consumed:], len(stream) - part.consumed, 3 - n, want, sr.major_of(stream))
        assert rest.ok and rest.payloads == res.payloads[n:] and part.consumed + rest.consumed == res.consumed
    four = sr.walk(stream, len(stream), 4, want)
    assert (four.reason, four.at, four.lens) == (sr.R_FEWER, len(stream) - 13, res.lens + [0])


def test_sources_are_what_the_designs_need(S):
    assert [len(x) % 16 for x in S["mix"].payloads[:3]] == [15, 1, 0]
    assert set(S["mini4"].sizes[0]) == {4} and set(S["mini5"].sizes[0]) == {5} and set(S["ld1"].sizes[0]) == {1}
    for src in S.values():
        assert (src.xs, src.ns) == (6, 24)
        assert len(set(src.payloads)) == len(src.payloads)


def test_accepted_streams_are_accepted_and_carry_their_pictures(sets):
    acc, _ = sets
    assert len({c.name for c in acc}) == len(acc)
    for c in acc:
        res = c.model()
        assert res.ok, (c.name, res.reason, res.at)
        assert len(res.numbers) == c.n and res.lens == [len(x) for x in res.payloads], c.name
        if c.pics is not None:
            assert res.payloads == [c.src.payloads[k] for k in c.pics], c.name
    by = {c.name: c.model() for c in acc}
    assert by["numbers_wrap"].numbers == [0xFFFFFFFE, 0xFFFFFFFF, 0] and by["numbers_wrap_fragmented"].numbers == [0xFFFFFFFF, 0]
    assert by["empty_payload"].lens[0] == 0
    assert by["resume_first_4"].consumed == len([c for c in acc if c.name == "resume_first_4"][0].stream) - 13


def test_accepted_streams_decode_through_the_oracle(oracle, sets):
    """valid to the reference's decoder, not only to the model: the same pictures as the plain stream they derive from"""
    acc, _ = sets
    plain = {}
    checked = skipped = 0
    for c in acc:
        if c.pics is None or c.oracle_no:
            skipped += 1
            assert c.pics is None or c.oracle_no
            continue
        key = (c.src.name, tuple(c.pics))
        if key not in plain:
            plain[key] = oracle.decode_stream(c.src.p, c.src.plain(c.pics), len(c.pics))[0]
        got, frames = oracle.decode_stream(c.src.p, c.bytes()[:c.length - c.start], 8)   # (a stream may go on behind the n-th)
        assert frames >= len(c.pics) and got[:len(plain[key])] == plain[key], c.name
        checked += 1
    assert checked >= 50 and skipped <= 12


def test_refused_streams_are_refused_for_their_reason(sets):
    _, ref = sets
    assert len({c.name for c in ref}) == len(ref)
    for c in ref:
        res = c.model()
        assert not res.ok and res.reason == c.expect, (c.name, res.reason, res.at)
        assert res.lens[len(res.numbers):] == [0] * (c.n - len(res.numbers))
    by = {c.name: c.model() for c in ref}
    # the boundaries show in the offsets: 12 bytes left refuse the unit itself, 13 the one behind it
    assert by["len_leaves_13"].at == by["len_leaves_12"].at + 13
    # the parse codes: eight known, the rest unknown
    codes = [c for c in ref if c.name.startswith("code_")]
    assert len(codes) == 255 and sum(1 for c in codes if c.expect == sr.R_CODE) == 256 - 8


def test_census(S, sets):
    """the generated sets reach every gather form and every reason of the walk"""
    acc, ref = sets
    cs = sr.census(acc)
    every = set(range(16))
    assert cs["src_phase"] == every and cs["dst_phase"] == every and cs["word_phase"] == every, cs
    assert set(sr.SEGMENT_LENGTHS) <= cs["seg_len"], cs["seg_len"]
    assert cs["segments_per_word"] >= 3 and {0, 1, 15} <= cs["payload_mod16"], cs
    assert {o for c in acc for o in c.offs} == set(sr.ALL_OFFS)
    assert {c.model().reason for c in ref} == set(sr.WALK_REASONS)
    exact, longer, longer_f = sr.capacity(S)
    assert exact.model().ok and max(exact.model().lens) == exact.stride
    for c in (longer, longer_f):
        assert c.model().ok and c.model().lens == [c.stride, c.stride + 1, c.stride]


@pytest.mark.parametrize("mutation", sr.MUTATIONS)
def test_wrong_copies_are_caught(sets, mutation):
    acc, ref = sets
    hits = [c.name for c in acc + ref if c.model(mutation).key() != c.model().key()]
    assert hits, mutation


@pytest.mark.parametrize("mutation", sorted(sr.UNCATCHABLE))
def test_uncatchable_copies_are_uncatchable(sets, mutation):
    """listed with the reason, not dropped: no designed stream tells them from the model, and none can"""
    acc, ref = sets
    assert not [c.name for c in acc + ref if c.model(mutation).key() != c.model().key()]
    assert len(sr.MUTATIONS) >= 10 and not set(sr.MUTATIONS) & set(sr.UNCATCHABLE)
