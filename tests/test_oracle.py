"""CPU tests that pin oracle/ (test infrastructure) to the reference:
  * the reference's own unit-test known answers (tests/Quantisation.cpp:6-36)
  * the reference's quant_factor table (tests/golden)
  * the reference's quantMatrix values (tests/golden)
  * the reference's own VLC.cpp compiled into oracle/_ref
  * internal invariants (q=0 lossless for all seven kernels, pack/unpack inverse)."""
import json
import os

import numpy as np
import pytest

from synth import noise_frame, synth
from vc2lib import KERNELS, OracleError, load_ref_vlc, make_params

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_digests.json")))


def test_quant_known_answers(oracle):
    # /root/reference/tests/Quantisation.cpp:30-36
    for v, q, want in GOLD["quant_known_answers"]:
        assert oracle.quant(v, q) == want


def test_quant_index_limit_message(oracle):
    # /root/reference/tests/Quantisation.cpp:6-12
    with pytest.raises(OracleError, match="quantization index exceeds maximum implemented value."):
        oracle.quant(12, 130)
    oracle.quant(12, 119)


def test_quant_factor_table_equals_reference(oracle):
    # the reference's lookup[120] (Quantisation.cpp), recorded in tests/golden/quant_factor_table.json
    table = [int(x, 16) for x in json.load(open(os.path.join(os.path.dirname(__file__), "golden", "quant_factor_table.json")))["quant_factor"]]
    assert len(table) == 120
    for q, want in enumerate(table):
        got = oracle.quant_factor(q) & 0xFFFFFFFF
        assert got == want, (q, hex(got), hex(want))


def test_quant_matrices_equal_reference(oracle):
    qm = GOLD["quant_matrices"]
    for name in ("DD97", "LeGall", "DD137", "Haar1", "Fidelity", "Daub97"):
        for depth in range(1, 6):
            got = oracle.quant_matrix(KERNELS[name], depth).tolist()
            assert got == qm[name][:3 * depth + 1], (name, depth)
    for depth, want in qm["Haar0_by_depth"].items():
        assert oracle.quant_matrix(KERNELS["Haar0"], int(depth)).tolist() == want


def test_scale_inverts_quant_at_q0(oracle):
    for v in (-70000, -513, -1, 0, 1, 7, 512, 65534):
        assert oracle.scale(oracle.quant(v, 0), 0) == v


def test_vlc_against_reference_vlc_cpp(oracle):
    ref = load_ref_vlc()
    if ref is None:
        pytest.skip("oracle/_ref not built (reference checkout absent)")
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 80))
        scale = int(rng.choice([1, 3, 40, 3000, 60000]))
        vals = rng.integers(-scale, scale + 1, size=n).astype(np.int32)
        vals[rng.random(n) < 0.5] = 0
        # one-slice, one-"plane" HQ pack through the oracle: 1 x n plane, depth 0 is not a
        # codec geometry, so drive the oracle's slice writer with a 2x(n) depth-1 tile instead
        w = 2 * ((n + 1) // 2 * 2)
        plane = np.zeros((2, w), np.int32)
        flat = np.zeros(2 * w, np.int32)
        flat[:n] = vals
        # coding order of a depth-1 2 x w tile: LL (y0,x even), HL (y0,x odd), LH (y1,x even), HH
        order = [(0, x) for x in range(0, w, 2)] + [(0, x) for x in range(1, w, 2)] + \
                [(1, x) for x in range(0, w, 2)] + [(1, x) for x in range(1, w, 2)]
        for (yy, xx), v in zip(order, flat):
            plane[yy, xx] = v
        z = np.zeros((2, w), np.int32)
        q = np.zeros((1, 1), np.int32)
        payload = oracle.hq_pack(plane, z, z, 1, q, 0, 1)
        ylen = int(payload[1])
        ydata = payload[2:2 + ylen]
        out = np.empty(max(ylen, 1) + 8, np.uint8)
        nref = ref.ref_svlc_write_bounded(flat, flat.size, 8 * ylen, out, out.size)
        assert nref == ylen
        assert bytes(out[:nref]) == bytes(ydata)
        back = np.empty(flat.size, np.int32)
        ref.ref_svlc_read_bounded(np.ascontiguousarray(ydata if ylen else np.zeros(1, np.uint8)),
                                  ylen, 8 * ylen, flat.size, back)
        assert back.tolist() == flat.tolist()
        y2, _, _, _, _ = oracle.hq_unpack(payload, (2, w), (2, w), 1, 1, 1)
        assert np.array_equal(y2, plane)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_q0_roundtrip_lossless_with_padding(oracle, kernel):
    # q=0 HQ_ConstQ round trip is lossless for all 7 kernels, also padded
    w, h, depth = 80, 44, 3            # pads to 80 x 48 (luma), 40 -> 40 x 48 (chroma)
    raw = noise_frame(w, h, "422", 10, seed=3)
    p = make_params(w, h, "422", 10, kernel, depth, 1, 2, q=0, scalar=4)
    stream = oracle.encode_stream(p, raw, 1)
    dec, n = oracle.decode_stream(p, stream, 1)
    assert n == 1 and dec == raw


def test_dwt_inverse_inverts_forward(oracle):
    rng = np.random.default_rng(5)
    plane = rng.integers(-512, 512, size=(48, 80)).astype(np.int32)
    for name, k in KERNELS.items():
        c = oracle.dwt_forward(plane, k, 3)
        assert np.array_equal(oracle.dwt_inverse(c, k, 3), plane), name


def test_cbr_slices_have_exact_size(oracle):
    w, h, depth = 128, 64, 3
    raw = synth(w, h, "422", 10, 99)
    p = make_params(w, h, "422", 10, "DD97", depth, 1, 2, mode="HQ_CBR", s=6000, scalar=1)
    stream = oracle.encode_stream(p, raw, 1)
    dec, n = oracle.decode_stream(p, stream, 1)
    assert n == 1 and len(dec) == len(raw)
    # picture data unit = 13 + header + sum(slice_bytes)
    sb = oracle.slice_bytes(8, 4, 6000, 1)
    assert abs(int(sb.sum()) - 6000) < 8 * 4 * 1 + 4


def test_ld_roundtrip_selfconsistent(oracle):
    # LD has no reference vectors here ("parity unpinned"): check encode->decode consistency
    w, h, depth = 128, 64, 3
    raw = synth(w, h, "422", 8, 5, word_bytes=1)
    p = make_params(w, h, "422", 8, "LeGall", depth, 1, 2, mode="LD", s=4000, word_bytes=1)
    stream = oracle.encode_stream(p, raw, 1)
    dec, n = oracle.decode_stream(p, stream, 1)
    assert n == 1 and len(dec) == len(raw)
    a = np.frombuffer(raw, np.uint8).astype(int)
    b = np.frombuffer(dec, np.uint8).astype(int)
    assert np.abs(a - b).mean() < 4.0


# ---- stream-level features added for SURVEY 8(f)3: interlace and picture fragments.  No reference output exists
# ---- for them in this container ("parity unpinned"); these are the invariants the syntax itself gives.
def _units(stream):
    pos, out = 0, []
    while pos < len(stream):
        assert stream[pos:pos + 4] == b"BBCD"
        code = stream[pos + 4]
        nxt = int.from_bytes(stream[pos + 5:pos + 9], "big")
        prev = int.from_bytes(stream[pos + 9:pos + 13], "big")
        size = nxt if nxt else 13
        out.append((code, nxt, prev, stream[pos + 13:pos + size]))
        pos += size
    return out


@pytest.mark.parametrize("bff", [False, True])
def test_interlaced_lossless_round_trip(oracle, bff):
    from synth import synth
    from vc2lib import make_params
    w, h = 64, 64
    raw = synth(w, h, "420", 8, 61, frames=2, word_bytes=1)
    p = make_params(w, h, "420", 8, "Haar0", 2, 2, 2, q=0, scalar=4, word_bytes=1, interlaced=True, bottom_field_first=bff)
    stream = oracle.encode_stream(p, raw, 2)
    units = _units(stream)
    assert [u[0] for u in units] == [0x00, 0xE8, 0xE8, 0xE8, 0xE8, 0x10]
    # picture numbers count fields (Utils.cpp:52-63); parse offsets chain
    assert [int.from_bytes(u[3][:4], "big") for u in units[1:5]] == [0, 1, 2, 3]
    for a, b in zip(units, units[1:]):
        assert b[2] == a[1]
    dec, n = oracle.decode_stream(p, stream, 2)
    assert n == 2 and dec == raw
    # the field order decides which rows a picture carries
    q = make_params(w, h, "420", 8, "Haar0", 2, 2, 2, q=0, scalar=4, word_bytes=1, interlaced=True, bottom_field_first=not bff)
    assert oracle.encode_stream(q, raw, 2) != stream


@pytest.mark.parametrize("mode,kw", [("HQ_CBR", dict(s=5000, scalar=2, prefix=1)), ("LD", dict(s=4000))])
@pytest.mark.parametrize("flen", [1, 300, 100000])
def test_fragmented_stream_carries_the_same_slices(oracle, mode, kw, flen):
    from synth import synth
    from vc2lib import make_params
    w, h = 128, 64
    raw = synth(w, h, "422", 10, 62)
    whole = make_params(w, h, "422", 10, "LeGall", 2, 2, 2, mode=mode, **kw)
    frag = make_params(w, h, "422", 10, "LeGall", 2, 2, 2, mode=mode, fragment_length=flen, **kw)
    s0, s1 = oracle.encode_stream(whole, raw, 1), oracle.encode_stream(frag, raw, 1)
    u0, u1 = _units(s0), _units(s1)
    code = 0xEC if mode == "HQ_CBR" else 0xCC
    assert [u[0] for u in u1] == [0x00] + [code] * (len(u1) - 2) + [0x10]
    assert u1[0][3][0] & 0x80 == 0 and u0[0][3] != u1[0][3]        # fragments force major version 3 (DataUnit.cpp:1065)
    first, rest = u1[1][3], [u[3] for u in u1[2:-1]]
    assert int.from_bytes(first[6:8], "big") == 0                    # parameters fragment: slice count 0
    slices, count, nxt = b"", 0, 0
    for body in rest:
        n = int.from_bytes(body[6:8], "big")
        assert int.from_bytes(body[4:6], "big") == len(body) - 12
        assert int.from_bytes(body[10:12], "big") * 16 + int.from_bytes(body[8:10], "big") == nxt   # slice offset (x, y)
        if flen > 1 and n > 1:
            assert len(body) - 12 <= flen
        slices += body[12:]
        count += n
        nxt += n
    assert count == 128
    if flen == 1:
        assert len(rest) == 128          # never an empty fragment: one slice each
    if flen == 100000:
        assert len(rest) == 1
    # same slice bytes as the unfragmented picture (whose transform parameters lack the v3 flags)
    assert s0[:-13].endswith(slices)
    assert oracle.decode_stream(frag, s1, 1) == oracle.decode_stream(whole, s0, 1)


def test_interlaced_fragmented_ld_stream_shape(oracle):
    from synth import synth
    from vc2lib import make_params
    w, h = 128, 64
    raw = synth(w, h, "422", 8, 63, word_bytes=1)
    p = make_params(w, h, "422", 8, "LeGall", 2, 2, 2, mode="LD", s=8000, word_bytes=1, interlaced=True, fragment_length=500)
    units = _units(oracle.encode_stream(p, raw, 1))
    params = [u for u in units if u[0] == 0xCC and int.from_bytes(u[3][6:8], "big") == 0]
    assert [int.from_bytes(u[3][:4], "big") for u in params] == [0, 1]
    # each field gets half the frame budget (EncodeStream.cpp:378)
    for k in (0, 1):
        total = sum(len(u[3]) - 12 for u in units if u[0] == 0xCC and int.from_bytes(u[3][:4], "big") == k and int.from_bytes(u[3][6:8], "big"))
        assert total == 4000
