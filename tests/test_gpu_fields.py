"""GPU tests of the field-picture batch calls (vc2hip_encode_fields_batch_dev / vc2hip_decode_fields_batch_dev): interlaced
frames in device memory coded as two field pictures each, read and written in place by the transform's edge kernels.
They are checked against the oracle's interlaced streams, against the progressive batch calls on fields split in numpy,
through every transform family in both directions, at full size, on several lanes, and for the arguments they refuse."""
import numpy as np
import pytest

from synth import synth, synth_fast
from vc2lib import make_params

pytestmark = pytest.mark.gpu

EINVAL = -1

# frame sizes: every field height (h / 2, chroma h / 2) is even
CASES = {
    "constq_dd97_422_10": dict(w=256, h=128, cf="422", bits=10, kernel="DD97", depth=3, u=2, a=2, kw=dict(q=12, scalar=2)),
    "cbr_legall_420_8": dict(w=256, h=128, cf="420", bits=8, kernel="LeGall", depth=3, u=2, a=2, wb=1,
                             kw=dict(mode="HQ_CBR", s=9000, scalar=1)),
    "ld_legall_420_8": dict(w=128, h=64, cf="420", bits=8, kernel="LeGall", depth=3, u=2, a=2, wb=1, kw=dict(mode="LD", s=3000)),
    "fidelity_444_12": dict(w=192, h=96, cf="444", bits=12, kernel="Fidelity", depth=2, u=2, a=2, kw=dict(q=10)),
    "padded_prefix1_scalar3": dict(w=250, h=132, cf="422", bits=10, kernel="DD97", depth=3, u=1, a=2,
                                   kw=dict(q=10, prefix=1, scalar=3)),
    "legall_444_w3": dict(w=128, h=64, cf="444", bits=12, kernel="LeGall", depth=2, u=2, a=2, wb=3, kw=dict(q=10)),
}


def _torch():
    return pytest.importorskip("torch")


def _dev(b):
    torch = _torch()
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")


def _shapes(c):
    """(rows, bytes per row) of the three planes of a FRAME"""
    wb = c.get("wb", 2)
    w, h = c["w"], c["h"]
    cw = w if c["cf"] == "444" else w // 2
    ch = h // 2 if c["cf"] == "420" else h
    return [(h, w * wb), (ch, cw * wb), (ch, cw * wb)]


def _fields(raw, c, n, tff=True):
    """frames -> field pictures in stream order, each plane split by rows (the first field: even rows when tff)"""
    shapes = _shapes(c)
    fb = sum(a * b for a, b in shapes)
    out = []
    for f in range(n):
        frame = np.frombuffer(raw, np.uint8, fb, f * fb)
        planes, at = [], 0
        for r, rw in shapes:
            planes.append(frame[at:at + r * rw].reshape(r, rw))
            at += r * rw
        for first in ((0, 1) if tff else (1, 0)):
            out.append(b"".join(pl[first::2].tobytes() for pl in planes))
    return b"".join(out)


def _frames(fields, c, n, tff=True):
    """field pictures in stream order -> frames: the inverse of _fields"""
    shapes = _shapes(c)
    pb = sum(a * b for a, b in shapes) // 2
    out = []
    for f in range(n):
        parts = []
        for k in (0, 1):
            pic = np.frombuffer(fields, np.uint8, pb, (2 * f + k) * pb)
            at, pl = 0, []
            for r, rw in shapes:
                pl.append(pic[at:at + (r // 2) * rw].reshape(r // 2, rw))
                at += (r // 2) * rw
            parts.append(pl)
        top, bottom = (parts[0], parts[1]) if tff else (parts[1], parts[0])
        for k, (r, rw) in enumerate(shapes):
            frame = np.empty((r, rw), np.uint8)
            frame[0::2], frame[1::2] = top[k], bottom[k]
            out.append(frame.tobytes())
    return b"".join(out)


def _raw(w, h, cf, bits, seed, n, wb, fast=False):
    """n frames of synthetic words; words of 3 or 4 bytes hold synth's samples MSB-justified, big-endian"""
    gen = synth_fast if fast else synth
    if wb in (1, 2):
        return gen(w, h, cf, bits, seed, frames=n, word_bytes=wb)
    v = np.frombuffer(gen(w, h, cf, bits, seed, frames=n), ">u2").astype(np.uint32) >> (16 - bits)
    u = v << (8 * wb - bits)
    return np.stack([(u >> (8 * (wb - 1 - k))) & 0xFF for k in range(wb)], axis=1).astype(np.uint8).tobytes()


def _setup(hip, c, n=3, seed=5, tff=True):
    """(frame format, field cp, oracle params of the interlaced stream, n raw frames) of one case"""
    import vc2hip_py
    wb = c.get("wb", 2)
    ffmt = vc2hip_py.picture_format(c["w"], c["h"], c["cf"], c["bits"], wb)
    fmt = vc2hip_py.picture_format(c["w"], c["h"] // 2, c["cf"], c["bits"], wb)
    ckw = dict(c["kw"])
    if "s" in ckw:
        ckw["s"] //= 2                       # the field's budget (EncodeStream: -s / 2)
    cp = vc2hip_py.coding_params(hip.lib, fmt, c["kernel"], c["depth"], c["u"], c["a"], **ckw)
    p = make_params(c["w"], c["h"], c["cf"], c["bits"], c["kernel"], c["depth"], c["u"], c["a"], word_bytes=wb,
                    interlaced=True, bottom_field_first=not tff, **c["kw"])
    raw = _raw(c["w"], c["h"], c["cf"], c["bits"], seed, n, wb)
    return ffmt, fmt, cp, p, raw


def _stride(hip, fmt, cp):
    return (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256


def _seq_len(stream):
    return int.from_bytes(stream[5:9], "big")


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


def _encode_fields(hip, d_frames, n, ffmt, tff, cp, stride):
    torch = _torch()
    d_pay = torch.zeros(2 * n * stride, dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(2 * n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    hip.encode_fields_batch_dev(d_frames.data_ptr(), n, ffmt, tff, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    hip.sync()
    return d_pay, d_len


def _encode_split(hip, d_fields, n_pics, fmt, cp, stride):
    torch = _torch()
    d_pay = torch.zeros(n_pics * stride, dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(n_pics, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    hip.encode_batch_dev(d_fields.data_ptr(), n_pics, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    hip.sync()
    return d_pay, d_len


def _decode_fields(hip, d_pay, d_len, n, ffmt, tff, cp, stride):
    """decode_fields_batch_dev into a buffer full of a sentinel (equality then shows every byte was written)"""
    torch = _torch()
    d_out = torch.full((n * hip.raw_picture_bytes(ffmt),), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    hip.decode_fields_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, ffmt, tff, cp, d_out.data_ptr())
    hip.sync()
    return d_out


def _decode_split(hip, d_pay, d_len, n_pics, fmt, cp, stride):
    torch = _torch()
    d_out = torch.zeros(n_pics * hip.raw_picture_bytes(fmt), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n_pics, fmt, cp, d_out.data_ptr())
    hip.sync()
    return d_out


def _check_against_split(hip, c, raw, n, ffmt, fmt, cp, tff):
    """fields calls == the progressive batch calls on the fields split in numpy, both directions; returns the slots"""
    stride = _stride(hip, fmt, cp)
    pay, lens = _encode_fields(hip, _dev(raw), n, ffmt, tff, cp, stride)
    pay_s, lens_s = _encode_split(hip, _dev(_fields(raw, c, n, tff)), 2 * n, fmt, cp, stride)
    assert lens.tolist() == lens_s.tolist()
    assert bytes(pay.cpu().numpy()) == bytes(pay_s.cpu().numpy())
    dec = _decode_fields(hip, pay, lens, n, ffmt, tff, cp, stride).cpu().numpy().tobytes()
    dec_s = _decode_split(hip, pay, lens, 2 * n, fmt, cp, stride).cpu().numpy().tobytes()
    assert dec == _frames(dec_s, c, n, tff)
    return pay, lens, stride


# ---------------------------------------------------------------------------------------------------------------------
# 1 / 2: the oracle's interlaced streams, both field orders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tff", [True, False], ids=["tff", "bff"])
@pytest.mark.parametrize("case", list(CASES))
def test_fields_are_the_oracle_stream(hip, oracle, case, tff):
    import vc2hip_py
    torch = _torch()
    c = CASES[case]
    n = 2
    ffmt, fmt, cp, p, raw = _setup(hip, c, n=n, seed=11, tff=tff)
    pay, lens, stride = _check_against_split(hip, c, raw, n, ffmt, fmt, cp, tff)
    stream = oracle.encode_stream(p, raw, n)
    seq = stream[:_seq_len(stream)]
    cap = 2 * n * (stride + 64) + 64
    d_stream = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    d_slen = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    hip.stream_write_dev(pay.data_ptr(), stride, lens.data_ptr(), 2 * n, cp, vc2hip_py.stream_params(_major(stream), 0, len(seq), True),
                         d_stream.data_ptr(), cap, d_slen.data_ptr())
    hip.sync()
    assert seq + d_stream[:int(d_slen.item())].cpu().numpy().tobytes() == stream
    if c["kw"].get("mode") == "LD":
        return  # (the oracle's LD stream decode halves the field budget once more: DecodeStream.cpp:331)
    # decode: stream_read_dev of the oracle's stream (2n field pictures), then decode_fields_batch_dev
    d_in = _dev(stream)
    pay2 = torch.zeros_like(pay)
    lens2 = torch.zeros_like(lens)
    hip.stream_read_dev(d_in.data_ptr(), len(stream), 2 * n, cp, vc2hip_py.stream_params(0), pay2.data_ptr(), stride,
                        lens2.data_ptr())
    dec = _decode_fields(hip, pay2, lens2, n, ffmt, tff, cp, stride).cpu().numpy().tobytes()
    assert dec == oracle.decode_stream(p, stream, n)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 3: every transform family reads and writes fields at its edge
# ---------------------------------------------------------------------------------------------------------------------
# (variant, context flags, frame geometry (w, h, cf, depth, u, a, word_bytes, wavelet), edge families expected fwd / inv)
FAMILY_RUNS = [
    ("default", (), (1024, 512, "422", 3, 2, 4, 2, "LeGall"), ("pair",), ("stream",)),
    ("no_pair", ("NO_PAIR",), (1024, 512, "422", 3, 2, 4, 2, "LeGall"), ("stream",), ("stream",)),
    ("no_stream", ("NO_STREAM",), (1024, 512, "422", 3, 2, 4, 2, "LeGall"), ("fast",), ("fast",)),
    ("generic", ("GENERIC_DWT",), (1024, 512, "422", 3, 2, 4, 2, "LeGall"), ("tile",), ("tile",)),
    ("store32", ("STORE32",), (1024, 512, "422", 3, 2, 4, 2, "DD97"), ("stream", "fast"), ("stream", "fast")),
    ("plane", (), (256, 512, "444", 2, 64, 64, 2, "LeGall"), ("plane",), ("plane",)),
    # 1080i at depth 3: 540 field rows padded to 544
    ("padded_1080i", (), (1920, 1080, "422", 3, 1, 4, 2, "LeGall"), ("pair", "stream"), ("stream",)),
    # 3-byte words: the non-edge route (the streaming and two-level edge kernels read 2-byte words only)
    ("w3", (), (1024, 512, "422", 3, 2, 4, 3, "LeGall"), ("fast",), ("fast",)),
    ("w1_tiles", ("NO_STREAM",), (384, 384, "444", 3, 3, 3, 1, "DD97"), ("tile", "fast"), ("tile", "fast")),
]


@pytest.mark.parametrize("run", FAMILY_RUNS, ids=[r[0] for r in FAMILY_RUNS])
def test_every_family_both_directions(run):
    import vc2hip_py
    torch = _torch()
    name, flags, (w, h, cf, depth, u, a, wb, kernel), fwd_fams, inv_fams = run
    hip = vc2hip_py.Vc2Hip(flags=sum(vc2hip_py.FLAGS[f] for f in flags))
    bits = 8 if wb == 1 else 10
    c = dict(w=w, h=h, cf=cf, bits=bits, wb=wb)
    n = 2
    ffmt = vc2hip_py.picture_format(w, h, cf, bits, wb)
    fmt = vc2hip_py.picture_format(w, h // 2, cf, bits, wb)
    scalar = 256 if name == "plane" else 2   # (room in the length bytes for the one 256 x 256 slice)
    cp = vc2hip_py.coding_params(hip.lib, fmt, kernel, depth, u, a, q=24, scalar=scalar)
    raw = _raw(w, h, cf, bits, 77, n, wb, fast=True)
    stride = _stride(hip, fmt, cp)
    for tff in (True, False):
        pay, lens = _encode_fields(hip, _dev(raw), n, ffmt, tff, cp, stride)
        rec = hip.dwt_launches()
        edge = {r["family"] for r in rec if r["edge"] or r["family"] == "plane"}  # (a plane's ingest is its edge)
        assert edge & set(fwd_fams), f"{name}: forward edge launches {rec}"
        assert all(r["pictures"] == 2 * n for r in rec)
        pay_s, lens_s = _encode_split(hip, _dev(_fields(raw, c, n, tff)), 2 * n, fmt, cp, stride)
        assert lens.tolist() == lens_s.tolist() and torch.equal(pay, pay_s), name
        d_out = _decode_fields(hip, pay, lens, n, ffmt, tff, cp, stride)
        rec = hip.dwt_launches()
        edge = {r["family"] for r in rec if r["edge"] or r["family"] == "plane"}
        assert edge & set(inv_fams), f"{name}: inverse edge launches {rec}"
        dec_s = _decode_split(hip, pay, lens, 2 * n, fmt, cp, stride).cpu().numpy().tobytes()
        assert d_out.cpu().numpy().tobytes() == _frames(dec_s, c, n, tff), name


# ---------------------------------------------------------------------------------------------------------------------
# 4: full size -- 1080i, 128 frames (256 field pictures) and LD 1080i at depth 3
# ---------------------------------------------------------------------------------------------------------------------
def _full_size(hip, c, n, tff=True):
    import vc2hip_py
    torch = _torch()
    wb = c.get("wb", 2)
    ffmt = vc2hip_py.picture_format(c["w"], c["h"], c["cf"], c["bits"], wb)
    fmt = vc2hip_py.picture_format(c["w"], c["h"] // 2, c["cf"], c["bits"], wb)
    cp = vc2hip_py.coding_params(hip.lib, fmt, c["kernel"], c["depth"], c["u"], c["a"], **c["kw"])
    uniq = 3
    raw = synth_fast(c["w"], c["h"], c["cf"], c["bits"], 123, frames=uniq, word_bytes=wb)
    fb = hip.raw_picture_bytes(ffmt)
    pb = hip.raw_picture_bytes(fmt)
    pick = torch.arange(n, device="cuda:0") % uniq
    d_frames = _dev(raw).view(uniq, fb)[pick].reshape(-1)
    d_fields = _dev(_fields(raw, c, uniq, tff)).view(uniq, 2, pb)[pick].reshape(-1)   # (the numpy split, frame by frame)
    stride = _stride(hip, fmt, cp)
    pay, lens = _encode_fields(hip, d_frames, n, ffmt, tff, cp, stride)
    pay_s, lens_s = _encode_split(hip, d_fields, 2 * n, fmt, cp, stride)
    assert torch.equal(lens, lens_s)
    for k in range(2 * n):   # slot for slot
        assert torch.equal(pay[k * stride:(k + 1) * stride], pay_s[k * stride:(k + 1) * stride]), k
    del pay_s, d_fields
    d_out = _decode_fields(hip, pay, lens, n, ffmt, tff, cp, stride)
    dec_s = _decode_split(hip, pay, lens, 2 * uniq, fmt, cp, stride).cpu().numpy().tobytes()  # (the first frames' slots)
    want = _dev(_frames(dec_s, c, uniq, tff)).view(uniq, fb)
    got = d_out.view(n, fb)
    for f in range(n):
        assert torch.equal(got[f], want[f % uniq]), f


def test_full_size_1080i_constq(hip):
    c = dict(w=1920, h=1080, cf="422", bits=10, kernel="LeGall", depth=2, u=1, a=4, kw=dict(q=12, scalar=1))
    _full_size(hip, c, 128)


def test_full_size_1080i_ld(hip):
    c = dict(w=1920, h=1080, cf="422", bits=10, kernel="LeGall", depth=3, u=1, a=4, kw=dict(mode="LD", s=1036800 // 2))
    _full_size(hip, c, 16, tff=False)


# ---------------------------------------------------------------------------------------------------------------------
# 5: lanes -- whole frames per lane, identical to one lane
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_lanes_are_one_lane(hip, k):
    import vc2hip_py
    torch = _torch()
    c = CASES["constq_dd97_422_10"]
    n = 5
    ffmt, fmt, cp, _, raw = _setup(hip, c, n=n, seed=41)
    stride = _stride(hip, fmt, cp)
    pay1, lens1 = _encode_fields(hip, _dev(raw), n, ffmt, True, cp, stride)
    dec1 = _decode_fields(hip, pay1, lens1, n, ffmt, True, cp, stride)
    multi = vc2hip_py.Vc2Hip()
    multi.set_streams(k)
    payk, lensk = _encode_fields(multi, _dev(raw), n, ffmt, True, cp, stride)
    deck = _decode_fields(multi, payk, lensk, n, ffmt, True, cp, stride)
    assert torch.equal(lens1, lensk) and torch.equal(pay1, payk)
    assert torch.equal(dec1, deck)


# ---------------------------------------------------------------------------------------------------------------------
# 6: arguments the calls refuse, with nothing launched and the next call unaffected
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(hip):
    import vc2hip_py
    torch = _torch()
    c = CASES["constq_dd97_422_10"]
    ffmt, fmt, cp, _, raw = _setup(hip, c, n=2, seed=3)
    stride = _stride(hip, fmt, cp)
    pay0, lens0 = _encode_fields(hip, _dev(raw), 2, ffmt, True, cp, stride)
    d_raw = _dev(raw + bytes(64))
    d_pay = torch.zeros(4 * stride + 64, dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(4, dtype=torch.int64, device="cuda:0")

    def refused(call):
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            call()
        assert e.value.code == EINVAL and str(e.value)
        return str(e.value)

    odd = vc2hip_py.picture_format(256, 127, "422", 10)
    assert "even" in refused(lambda: hip.encode_fields_batch_dev(d_raw.data_ptr(), 2, odd, 1, cp, d_pay.data_ptr(), stride,
                                                                 d_len.data_ptr()))
    assert "even" in refused(lambda: hip.decode_fields_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), 2, odd, 1, cp,
                                                                 d_raw.data_ptr()))
    f420 = vc2hip_py.picture_format(256, 130, "420", 8, 1)      # chroma 65 rows
    assert "even" in refused(lambda: hip.encode_fields_batch_dev(d_raw.data_ptr(), 2, f420, 1, cp, d_pay.data_ptr(), stride,
                                                                 d_len.data_ptr()))
    refused(lambda: hip.encode_fields_batch_dev(d_raw.data_ptr(), 0, ffmt, 1, cp, d_pay.data_ptr(), stride, d_len.data_ptr()))
    refused(lambda: hip.decode_fields_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), 0, ffmt, 1, cp, d_raw.data_ptr()))
    assert "aligned" in refused(lambda: hip.encode_fields_batch_dev(d_raw.data_ptr() + 8, 2, ffmt, 1, cp, d_pay.data_ptr(),
                                                                    stride, d_len.data_ptr()))
    assert "aligned" in refused(lambda: hip.decode_fields_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), 2, ffmt, 1, cp,
                                                                    d_raw.data_ptr() + 4))
    hip.sync()
    pay, lens = _encode_fields(hip, _dev(raw), 2, ffmt, True, cp, stride)
    assert torch.equal(lens, lens0) and torch.equal(pay, pay0)
    dec = _decode_fields(hip, pay, lens, 2, ffmt, True, cp, stride).cpu().numpy().tobytes()
    dec_s = _decode_split(hip, pay, lens, 4, fmt, cp, stride).cpu().numpy().tobytes()
    assert dec == _frames(dec_s, c, 2)
