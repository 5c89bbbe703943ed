"""GPU tests of the device stream calls (vc2hip_stream_write_dev / vc2hip_stream_read_dev): the slots + lengths of the batch
calls to VC-2 stream bytes and back, against the oracle's streams and decodes, with the bounds and syntax errors they report."""
import numpy as np
import pytest

from synth import synth, synth_fast
from vc2lib import make_params

pytestmark = pytest.mark.gpu

ECAP, ESYNTAX = -9, -12

CASES = {
    "constq_dd97_422_10": dict(w=256, h=128, cf="422", bits=10, kernel="DD97", depth=3, u=2, a=2, kw=dict(q=12, scalar=2)),
    "cbr_legall_420_8": dict(w=256, h=128, cf="420", bits=8, kernel="LeGall", depth=3, u=2, a=2, wb=1,
                             kw=dict(mode="HQ_CBR", s=9000, scalar=1)),
    "ld_legall_420_8": dict(w=128, h=64, cf="420", bits=8, kernel="LeGall", depth=3, u=2, a=2, wb=1, kw=dict(mode="LD", s=3000)),
    "fidelity_444_12": dict(w=192, h=96, cf="444", bits=12, kernel="Fidelity", depth=2, u=2, a=2, kw=dict(q=10)),
    "padded_odd_prefix1_scalar3": dict(w=250, h=130, cf="422", bits=10, kernel="DD97", depth=3, u=1, a=2,
                                       kw=dict(q=10, prefix=1, scalar=3)),
}


def _torch():
    return pytest.importorskip("torch")


def _dev(b):
    torch = _torch()
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")


def _setup(hip, c, n=3, seed=5, interlaced=False, **over):
    """(fmt, cp, oracle params, n raw frames) of one case"""
    import vc2hip_py
    kw = dict(c["kw"], **over)
    wb = c.get("wb", 2)
    ph = c["h"] // 2 if interlaced else c["h"]
    fmt = vc2hip_py.picture_format(c["w"], ph, c["cf"], c["bits"], wb)
    ckw = dict(kw)
    ckw.pop("fragment_length", None)
    if interlaced and "s" in ckw:
        ckw["s"] //= 2
    cp = vc2hip_py.coding_params(hip.lib, fmt, c["kernel"], c["depth"], c["u"], c["a"], **ckw)
    p = make_params(c["w"], c["h"], c["cf"], c["bits"], c["kernel"], c["depth"], c["u"], c["a"], word_bytes=wb,
                    interlaced=interlaced, **kw)
    raw = synth(c["w"], c["h"], c["cf"], c["bits"], seed, frames=n, word_bytes=wb)
    return fmt, cp, p, raw


def _stride(hip, fmt, cp):
    return (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256


def _major(stream):
    """major_version: the first exp-Golomb field of the sequence header that opens the stream"""
    pos = 8 * 13
    v = 1
    while True:
        b = stream[pos >> 3] >> (7 - (pos & 7)) & 1
        pos += 1
        if b:
            return v - 1
        v = (v << 1) | (stream[pos >> 3] >> (7 - (pos & 7)) & 1)
        pos += 1


def _seq_len(stream):
    return int.from_bytes(stream[5:9], "big")


def _units(stream):
    out, pos = [], 0
    while True:
        code, nxt = stream[pos + 4], int.from_bytes(stream[pos + 5:pos + 9], "big")
        if code == 0x10:
            out.append((code, b""))
            return out
        out.append((code, stream[pos + 13:pos + nxt]))
        pos += nxt


def _chain(units):
    """the units again, next / prev parse offsets re-chained"""
    out, prev = bytearray(), 0
    for code, body in units:
        nxt = 0 if code == 0x10 else 13 + len(body)
        out += b"BBCD" + bytes([code]) + nxt.to_bytes(4, "big") + prev.to_bytes(4, "big") + body
        prev = 13 + len(body)
    return bytes(out)


def _write(hip, raw, n, fmt, cp, major, first=0, prev=0, eos=True, cap=None, guard=0):
    """encode_batch_dev + stream_write_dev; returns the device buffers (nothing synchronised)"""
    import vc2hip_py
    torch = _torch()
    stride = _stride(hip, fmt, cp)
    d_raw = _dev(raw)
    d_pay = torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    cap = n * (stride + 64) + 64 if cap is None else cap
    d_stream = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_slen = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    hip.encode_batch_dev(d_raw.data_ptr(), n, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    sp = vc2hip_py.stream_params(major, first, prev, eos)
    hip.stream_write_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, cp, sp, d_stream.data_ptr(), cap, d_slen.data_ptr())
    return dict(raw=d_raw, pay=d_pay, len=d_len, stream=d_stream, slen=d_slen, stride=stride)


def _written(hip, raw, n, fmt, cp, major, **kw):
    b = _write(hip, raw, n, fmt, cp, major, **kw)
    hip.sync()
    return b["stream"][:int(b["slen"].item())].cpu().numpy().tobytes()


def _read(hip, stream, n, fmt, cp, major=0, decode=True):
    """stream_read_dev (+ decode_batch_dev): (decoded bytes, lens, picture numbers, consumed); synchronised"""
    import vc2hip_py
    torch = _torch()
    stride = _stride(hip, fmt, cp)
    rb = hip.raw_picture_bytes(fmt)
    d_stream = _dev(stream)
    d_pay = torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    d_pn = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_cons = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_out = torch.zeros(n * rb, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    hip.stream_read_dev(d_stream.data_ptr(), len(stream), n, cp, vc2hip_py.stream_params(major), d_pay.data_ptr(), stride,
                        d_len.data_ptr(), d_pn.data_ptr(), d_cons.data_ptr())
    if decode:
        hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, fmt, cp, d_out.data_ptr())
    hip.sync()
    return (d_out.cpu().numpy().tobytes(), d_len.cpu().tolist(), [v & 0xFFFFFFFF for v in d_pn.cpu().tolist()],
            int(d_cons.item()))


def _fields(raw, c, n):
    """frames -> field pictures (top field first), each plane split by rows"""
    wb = c.get("wb", 2)
    w, h = c["w"], c["h"]
    cw = w if c["cf"] == "444" else w // 2
    ch = h // 2 if c["cf"] == "420" else h
    shapes = [(h, w * wb), (ch, cw * wb), (ch, cw * wb)]
    fb = sum(a * b for a, b in shapes)
    out = []
    for f in range(n):
        frame = np.frombuffer(raw, np.uint8, fb, f * fb)
        planes, at = [], 0
        for r, rw in shapes:
            planes.append(frame[at:at + r * rw].reshape(r, rw))
            at += r * rw
        for first in (0, 1):
            out.append(b"".join(pl[first::2].tobytes() for pl in planes))
    return b"".join(out)


def _frames(fields, c, n):
    """field pictures -> frames: the inverse of _fields"""
    wb = c.get("wb", 2)
    w, h = c["w"], c["h"]
    cw = w if c["cf"] == "444" else w // 2
    ch = h // 2 if c["cf"] == "420" else h
    shapes = [(h, w * wb), (ch, cw * wb), (ch, cw * wb)]
    pb = sum(a * b for a, b in shapes) // 2
    out = []
    for f in range(n):
        parts = []
        for first in (0, 1):
            pic = np.frombuffer(fields, np.uint8, pb, (2 * f + first) * pb)
            at, pl = 0, []
            for r, rw in shapes:
                pl.append(pic[at:at + (r // 2) * rw].reshape(r // 2, rw))
                at += (r // 2) * rw
            parts.append(pl)
        for k, (r, rw) in enumerate(shapes):
            frame = np.empty((r, rw), np.uint8)
            frame[0::2], frame[1::2] = parts[0][k], parts[1][k]
            out.append(frame.tobytes())
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------------
# write: the oracle's sequence header + the device's bytes == the oracle's stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_write_is_the_oracle_stream(hip, oracle, case):
    fmt, cp, p, raw = _setup(hip, CASES[case])
    stream = oracle.encode_stream(p, raw, 3)
    seq = stream[:_seq_len(stream)]
    assert seq + _written(hip, raw, 3, fmt, cp, _major(stream), prev=len(seq)) == stream


@pytest.mark.parametrize("n", [1, 113])
def test_write_one_and_many_pictures(hip, oracle, n):
    c = CASES["constq_dd97_422_10"] if n == 1 else dict(w=64, h=32, cf="420", bits=8, kernel="DD97", depth=2, u=2, a=2, wb=1,
                                                        kw=dict(q=8, scalar=1))
    fmt, cp, p, raw = _setup(hip, c, n=n, seed=9)
    stream = oracle.encode_stream(p, raw, n)
    seq = stream[:_seq_len(stream)]
    assert seq + _written(hip, raw, n, fmt, cp, _major(stream), prev=len(seq)) == stream
    dec, lens, pns, used = _read(hip, stream, n, fmt, cp)
    assert dec == oracle.decode_stream(p, stream, n)[0]
    assert pns == list(range(n)) and used == len(stream) - 13


def test_write_and_read_on_two_streams(oracle):
    import vc2hip_py
    hip = vc2hip_py.Vc2Hip()
    hip.set_streams(2)
    fmt, cp, p, raw = _setup(hip, CASES["constq_dd97_422_10"], n=5, seed=21)
    stream = oracle.encode_stream(p, raw, 5)
    seq = stream[:_seq_len(stream)]
    assert seq + _written(hip, raw, 5, fmt, cp, _major(stream), prev=len(seq)) == stream
    assert _read(hip, stream, 5, fmt, cp)[0] == oracle.decode_stream(p, stream, 5)[0]


def test_interlaced_fields(hip, oracle):
    """fields split in numpy and coded as pictures of half the height, one picture number per field"""
    c = dict(w=128, h=64, cf="422", bits=10, kernel="DD97", depth=2, u=2, a=2, kw=dict(q=10, scalar=2))
    fmt, cp, p, raw = _setup(hip, c, n=2, seed=31, interlaced=True)
    stream = oracle.encode_stream(p, raw, 2)
    seq = stream[:_seq_len(stream)]
    assert seq + _written(hip, _fields(raw, c, 2), 4, fmt, cp, _major(stream), prev=len(seq)) == stream
    dec, _, pns, _ = _read(hip, stream, 4, fmt, cp)
    assert pns == [0, 1, 2, 3]
    assert _frames(dec, c, 2) == oracle.decode_stream(p, stream, 2)[0]


def test_write_picture_numbers_wrap(hip, oracle):
    fmt, cp, p, raw = _setup(hip, CASES["ld_legall_420_8"])
    stream = _written(hip, raw, 3, fmt, cp, 2, first=2 ** 32 - 2, prev=77, eos=False)
    units = _units(stream + b"BBCD\x10" + bytes(8))
    assert [int.from_bytes(b[:4], "big") for _, b in units[:3]] == [2 ** 32 - 2, 2 ** 32 - 1, 0]
    assert int.from_bytes(stream[9:13], "big") == 77
    seq = oracle.encode_stream(p, raw, 1)
    _, _, pns, _ = _read(hip, seq[:_seq_len(seq)] + stream, 3, fmt, cp, decode=False)
    assert pns == [2 ** 32 - 2, 2 ** 32 - 1, 0]


# ---------------------------------------------------------------------------------------------------------------------
# read: stream_read_dev + decode_batch_dev == the oracle's decode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_read_decodes_as_the_oracle(hip, oracle, case):
    fmt, cp, p, raw = _setup(hip, CASES[case], seed=7)
    stream = oracle.encode_stream(p, raw, 3)
    dec, lens, pns, used = _read(hip, stream, 3, fmt, cp)
    assert dec == oracle.decode_stream(p, stream, 3)[0]
    units = _units(stream)
    assert pns == [0, 1, 2] and used == len(stream) - 13
    assert [13 + len(hip.picture_header(cp, _major(stream), 0)) + n for n in lens] == [13 + len(b) for _, b in units[1:4]]


@pytest.mark.parametrize("case,frag", [("cbr_legall_420_8", 300), ("ld_legall_420_8", 200), ("cbr_legall_420_8", 10 ** 6)])
def test_read_fragmented_pictures(hip, oracle, case, frag):
    fmt, cp, p, raw = _setup(hip, CASES[case], seed=8, fragment_length=frag)
    stream = oracle.encode_stream(p, raw, 3)
    assert {c for c, _ in _units(stream)} & {0xEC, 0xCC}
    assert _read(hip, stream, 3, fmt, cp)[0] == oracle.decode_stream(p, stream, 3)[0]


def test_read_skips_padding_auxiliary_and_repeated_sequence_headers(hip, oracle):
    fmt, cp, p, raw = _setup(hip, CASES["constq_dd97_422_10"], seed=11)
    stream = oracle.encode_stream(p, raw, 3)
    u = _units(stream)
    spliced = [u[0], (0x30, bytes(range(37))), u[1], (0x20, b"aux" * 11), (0x30, b""), u[0], u[2], u[0], (0x20, b"x"), u[3], u[4]]
    dec, _, pns, used = _read(hip, _chain(spliced), 3, fmt, cp)
    assert dec == oracle.decode_stream(p, stream, 3)[0] and pns == [0, 1, 2]
    assert used == len(_chain(spliced)) - 13


def test_read_in_two_calls(hip, oracle):
    fmt, cp, p, raw = _setup(hip, CASES["padded_odd_prefix1_scalar3"], seed=12)
    stream = oracle.encode_stream(p, raw, 3)
    want = oracle.decode_stream(p, stream, 3)[0]
    dec2, _, pns2, used = _read(hip, stream, 2, fmt, cp)
    rest = stream[used:]
    assert rest[4] == 0xE8
    dec1, _, pns1, used1 = _read(hip, rest, 1, fmt, cp, major=_major(stream))
    assert dec2 + dec1 == want and pns2 + pns1 == [0, 1, 2] and used + used1 == len(stream) - 13


# ---------------------------------------------------------------------------------------------------------------------
# bounds and errors (malformed input handled cleanly; the context stays usable)
# ---------------------------------------------------------------------------------------------------------------------
def test_write_cap_one_byte_short(hip, oracle):
    import vc2hip_py
    fmt, cp, p, raw = _setup(hip, CASES["ld_legall_420_8"], seed=13)
    full = _written(hip, raw, 3, fmt, cp, 2)
    for cap in (len(full) - 1, len(full) - 14, len(full) // 2 + 3):
        b = _write(hip, raw, 3, fmt, cp, 2, cap=cap, guard=64)
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            hip.sync()
        assert e.value.code == ECAP
        got = b["stream"].cpu().numpy().tobytes()
        assert int(b["slen"].item()) == len(full)
        assert got[:cap] == full[:cap] and got[cap:] == b"\xa5" * 64
    assert _written(hip, raw, 3, fmt, cp, 2) == full


def _skip_uvlc(s, pos):
    while not s[pos >> 3] >> (7 - (pos & 7)) & 1:
        pos += 2
    return pos + 1


def _corrupt(kind, stream, cp):
    s = bytearray(stream)
    seq = _seq_len(stream)
    n, cpx, length = 3, cp, len(s)
    if kind == "truncated":
        length -= 100
    elif kind == "prefix":
        s[seq + 2] = ord("X")
    elif kind == "params":
        import vc2hip_py
        cpx = vc2hip_py.CodingParams(cp.kernel, cp.depth, cp.y_slices, cp.x_slices, cp.mode, cp.q_index, cp.compressed_bytes,
                                     cp.prefix, cp.scalar + 1)
    elif kind == "fewer":
        n = 4
    elif kind == "quant_matrix":   # picture 1: the flag behind its transform parameters
        pos = 8 * (seq + _seq_len(stream[seq:]) + 13 + 4)
        for _ in range(2):
            pos = _skip_uvlc(s, pos)
        pos += 2 if _major(stream) >= 3 else 0
        for _ in range(4):
            pos = _skip_uvlc(s, pos)
        s[pos >> 3] |= 0x80 >> (pos & 7)
    elif kind == "next_zero":
        at = seq
        s[at + 5:at + 9] = bytes(4)
    return bytes(s[:length]), n, cpx


@pytest.mark.parametrize("kind,why", [("truncated", "past the end"), ("prefix", "prefix"), ("params", "differ"),
                                      ("fewer", "end of sequence"), ("quant_matrix", "quantisation matrix"),
                                      ("next_zero", "next_parse_offset")])
def test_read_syntax_errors(hip, oracle, kind, why):
    import vc2hip_py
    fmt, cp, p, raw = _setup(hip, CASES["constq_dd97_422_10"], seed=14)
    stream = oracle.encode_stream(p, raw, 3)
    bad, n, cpx = _corrupt(kind, stream, cp)
    if kind == "quant_matrix":
        assert bad != stream and len(bad) == len(stream)
    with pytest.raises(vc2hip_py.Vc2HipError) as e:
        _read(hip, bad, n, fmt, cpx, decode=False)
    assert e.value.code == ESYNTAX, str(e.value)
    assert why in str(e.value) and "at byte" in str(e.value)
    assert _read(hip, stream, 3, fmt, cp)[0] == oracle.decode_stream(p, stream, 3)[0]


def test_read_needs_a_major_version(hip, oracle):
    import vc2hip_py
    fmt, cp, p, raw = _setup(hip, CASES["constq_dd97_422_10"], seed=15)
    stream = oracle.encode_stream(p, raw, 1)
    with pytest.raises(vc2hip_py.Vc2HipError) as e:
        _read(hip, stream[_seq_len(stream):], 1, fmt, cp, decode=False)
    assert e.value.code == ESYNTAX and "at byte 0" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
# full size: cfg 2 (UHD-1 4:2:2 10-bit DD97 d4 q16 S2), 128 pictures
# ---------------------------------------------------------------------------------------------------------------------
def test_cfg2_128_pictures_write_then_read(oracle):
    import vc2hip_py
    torch = _torch()
    hip = vc2hip_py.Vc2Hip()
    w, h, n = 3840, 2160, 128
    fmt = vc2hip_py.picture_format(w, h, "422", 10)
    cp = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, q=16, scalar=2)
    p = make_params(w, h, "422", 10, "DD97", 4, 1, 2, q=16, scalar=2)
    raws = [synth_fast(w, h, "422", 10, 900 + i) for i in range(3)]
    rb = hip.raw_picture_bytes(fmt)
    stride = _stride(hip, fmt, cp)
    d_raw = _dev(b"".join(raws)).view(3, rb)[torch.arange(n, device="cuda:0") % 3].reshape(-1).contiguous()
    d_pay = torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    cap = n * (stride + 64)
    d_stream = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    d_slen = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    hip.encode_batch_dev(d_raw.data_ptr(), n, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    hip.stream_write_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, cp, vc2hip_py.stream_params(2, 0, 0, True),
                         d_stream.data_ptr(), cap, d_slen.data_ptr())
    hip.sync()
    slen = int(d_slen.item())
    lens = d_len.cpu().tolist()
    hl = len(hip.picture_header(cp, 2, 0))
    assert slen == sum(13 + hl + x for x in lens) + 13
    d_pay2 = torch.zeros_like(d_pay)
    d_len2 = torch.zeros_like(d_len)
    d_pn = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()   # (torch fills on its stream, the library works on its own)
    hip.stream_read_dev(d_stream.data_ptr(), slen, n, cp, vc2hip_py.stream_params(2), d_pay2.data_ptr(), stride, d_len2.data_ptr(),
                        d_pn.data_ptr(), None)
    hip.sync()
    assert d_len2.cpu().tolist() == lens and d_pn.cpu().tolist() == list(range(n))
    for k in range(n):
        assert torch.equal(d_pay[k * stride:k * stride + lens[k]], d_pay2[k * stride:k * stride + lens[k]]), k
    del d_stream
    d_out = torch.zeros(n * rb, dtype=torch.uint8, device="cuda:0")
    d_out2 = torch.zeros_like(d_out)
    torch.cuda.synchronize()
    hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, fmt, cp, d_out.data_ptr())
    hip.decode_batch_dev(d_pay2.data_ptr(), stride, d_len2.data_ptr(), n, fmt, cp, d_out2.data_ptr())
    hip.sync()
    assert torch.equal(d_out, d_out2)
    for k in (0, n - 1):
        stream = oracle.encode_stream(p, raws[k % 3], 1)
        body = d_pay2[k * stride:k * stride + lens[k]].cpu().numpy().tobytes()
        assert body == stream[-13 - lens[k]:-13], k
        assert d_out2[k * rb:(k + 1) * rb].cpu().numpy().tobytes() == oracle.decode_stream(p, stream, 1)[0], k
