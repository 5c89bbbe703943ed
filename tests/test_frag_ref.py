"""tests/frag_ref.py against the oracle's own fragmented streams (EncodeStream -F), byte for byte: HQ_CBR and LD, the cases
and fragment lengths of tests/test_gpu_stream_fragments.py.  The slots are cut from the oracle's unfragmented stream of the
same pictures; the bytes after the sequence header are compared.  This pins the test reference before it judges the HQ_ConstQ
pictures, which the oracle's encoder does not fragment."""
import pytest

import frag_ref
from synth import synth
from test_gpu_stream_dev import CASES, _major, _seq_len, _units
from vc2lib import make_params

N = 3


def _cp(c):
    import vc2hip_py
    lib = vc2hip_py.load_library()
    wb = c.get("wb", 2)
    fmt = vc2hip_py.picture_format(c["w"], c["h"], c["cf"], c["bits"], wb)
    return lib, vc2hip_py.coding_params(lib, fmt, c["kernel"], c["depth"], c["u"], c["a"], **c["kw"])


def oracle_slots(oracle, c, raw, n, lib, cp):
    """the slice payloads of the oracle's unfragmented stream"""
    import vc2hip_py
    wb = c.get("wb", 2)
    p = make_params(c["w"], c["h"], c["cf"], c["bits"], c["kernel"], c["depth"], c["u"], c["a"], word_bytes=wb, **c["kw"])
    stream = oracle.encode_stream(p, raw, n)
    hl = len(vc2hip_py.picture_header(lib, cp, _major(stream), 0))
    pics = [b for code, b in _units(stream) if code in (0xE8, 0xC8)]
    assert len(pics) == n
    return [b[hl:] for b in pics]


def oracle_fragmented(oracle, c, raw, n, fragment_length):
    """(sequence header, the rest) of the oracle's fragmented stream"""
    wb = c.get("wb", 2)
    p = make_params(c["w"], c["h"], c["cf"], c["bits"], c["kernel"], c["depth"], c["u"], c["a"], word_bytes=wb,
                    fragment_length=fragment_length, **c["kw"])
    stream = oracle.encode_stream(p, raw, n)
    assert _major(stream) == 3
    return stream[:_seq_len(stream)], stream[_seq_len(stream):]


def ld_budgets(oracle, cp):
    return oracle.slice_bytes(cp.y_slices, cp.x_slices, cp.compressed_bytes, 1).ravel().tolist() if cp.mode == frag_ref.LD else None


def slice_sizes(oracle, cp, pay):
    return ld_budgets(oracle, cp) or frag_ref.slice_sizes_hq(pay, cp.y_slices * cp.x_slices, cp.prefix, cp.scalar)


def lengths(oracle, cp, slots):
    """1: every slice alone; several slices per fragment; one fragment per picture (or, for pictures beyond it, the largest
    length a fragment can have); S = the first two slices' bytes (they share a fragment) and S - 1 (they do not): the >
    against >= boundary of the rule"""
    sizes = slice_sizes(oracle, cp, slots[0])
    s = sizes[0] + sizes[1]
    several = 4 * max(sizes) + 1
    assert several < min(len(x) for x in slots)
    return [1, several, min(max(len(x) for x in slots), 65535), s, s - 1]


@pytest.mark.parametrize("case", ["cbr_legall_420_8", "ld_legall_420_8"])
def test_frag_ref_is_the_oracle_stream(oracle, case):
    c = CASES[case]
    lib, cp = _cp(c)
    raw = synth(c["w"], c["h"], c["cf"], c["bits"], 5, frames=N, word_bytes=c.get("wb", 2))
    slots = oracle_slots(oracle, c, raw, N, lib, cp)
    counts = []
    for f in lengths(oracle, cp, slots):
        seq, want = oracle_fragmented(oracle, c, raw, N, f)
        got, offsets = frag_ref.fragment_stream(slots, cp, f, 0, len(seq), True, ld_budgets(oracle, cp))
        assert got == want, (case, f)
        # the unit offsets are the parse-info chain's
        walk, pos = [], 0
        while True:
            walk.append(pos)
            if got[pos + 4] == 0x10:
                break
            pos += int.from_bytes(got[pos + 5:pos + 9], "big")
        assert offsets == walk
        counts.append((len(offsets), int.from_bytes(got[offsets[1] + 19:offsets[1] + 21], "big")))   # units, slices of the first fragment
    ns = cp.y_slices * cp.x_slices
    assert counts[0] == (N * (ns + 1) + 1, 1) and counts[2] == (2 * N + 1, ns)
    assert N * 2 + 1 < counts[1][0] < counts[0][0] and counts[1][1] >= 4
    assert counts[3][1] >= 2 and counts[4][1] == 1


def test_cut_rule():
    assert frag_ref.cut([5, 5, 5], 10) == [(0, 2, 10), (2, 1, 5)]      # exactly the length: shared
    assert frag_ref.cut([5, 5, 5], 9) == [(0, 1, 5), (1, 1, 5), (2, 1, 5)]
    assert frag_ref.cut([50, 1, 1], 10) == [(0, 1, 50), (1, 2, 2)]     # an oversize slice travels alone
    assert frag_ref.cut([1, 50, 1], 10) == [(0, 1, 1), (1, 1, 50), (2, 1, 1)]
    assert frag_ref.cut([3], 1) == [(0, 1, 3)]
