"""GPU tests of packed and semi-planar pictures (vc2hip_set_packed_format) on the device batch calls.

Expected payloads and decoded pictures are the oracle's on the same pictures in the file format.  The encoder's input is
laid out by tests/packed_ref.py with random bits in every ignored position (bits 30 - 31 of a v210 word, the fields beyond a
row's width, the bits of a word outside its sample) and lies in a sentinel-filled buffer; every output goes into a
sentinel-filled buffer that is compared WHOLE with the model: sample values, zero bits, whole groups and untouched gaps in one
comparison.  The launch record under a packed format must equal that of the same call on planar little-endian LSB-justified
pictures, field by field.
"""
import numpy as np
import pytest

import layout_ref
import packed_ref
from test_gpu_dwt_paths import GEOMS, _header_bytes, _unit_bytes
from test_gpu_layout import _ctx, _dev, _diff, _pictures, _slots, _stride, _torch
from vc2lib import make_params

pytestmark = pytest.mark.gpu

EINVAL = -1
N = 3
SENTINEL = 0xA5
WAVELET = "DD97"
Q = 24
WIDE = {g[0]: g for g in GEOMS}["wide"]

# label: (width, height, chroma format, bits, word bytes, depth, u, a).  v210: width % 6 = 0, 2 and 4; 384 is eight 48-pixel
# units and nothing else, 416 eight units and a tail of five whole groups and one of two pixels, 1024 twenty-one units and a
# tail; 30 is five groups (the lanes work in pairs) with 15 chroma samples per row (the last chroma dword is half used).
# Semi-planar: 392 wide, so that one-byte Y rows (392 bytes) and 4:2:0 / 4:2:2 UV rows are no multiple of 16 bytes.
SHAPES = {
    "v210-384": (384, 64, "422", 10, 2, 2, 2, 2),
    "v210-416": (416, 64, "422", 10, 2, 2, 2, 2),
    "v210-wide": (WIDE[1], WIDE[2], WIDE[3], 10, 2, WIDE[4], WIDE[5], WIDE[6]),
    "v210-30": (30, 16, "422", 10, 2, 2, 2, 2),   # an odd number of groups and an odd chroma width (15)
}
for _cf in ("420", "422", "444"):
    SHAPES[f"sp-{_cf}-8"] = (392, 64, _cf, 8, 1, 2, 2, 14)
    SHAPES[f"sp-{_cf}-10"] = (392, 64, _cf, 10, 2, 2, 2, 14)


@pytest.fixture(scope="module")
def hip():
    # (16-bit band planes only: launch records of two calls are compared field by field, as in test_gpu_layout.py)
    h = _ctx(("PLANES8_NEVER",))
    yield h
    h.close()


def _pk(x):
    import vc2hip_py
    if x is None or isinstance(x, vc2hip_py.PackedFormat):
        return x
    return vc2hip_py.packed_format(x.packing, x.little_endian, x.lsb_justified, x.pitch, x.plane_offset, x.picture_stride)


_EXPECTED = {}


def _expected(oracle, label):
    """the pictures of a shape, the oracle's payloads and decoded pictures; computed once and left alone"""
    if label not in _EXPECTED:
        w, h, cf, bits, wb, depth, u, a = SHAPES[label]
        pics = _pictures(w, h, cf, bits, wb, N, seed=21, noise=True)
        p = make_params(w, h, cf, bits, WAVELET, depth, u, a, q=Q, scalar=8, word_bytes=wb)
        hb = _header_bytes(oracle, p)
        pays, decs = [], []
        for raw in pics:
            stream = oracle.encode_stream(p, raw, 1)
            want, got_n = oracle.decode_stream(p, stream, 1)
            assert got_n == 1
            pays.append(stream[-13 - (_unit_bytes(stream) - hb):-13])
            decs.append(want)
        _EXPECTED[label] = dict(pics=pics, pays=pays, decs=decs)
    return _EXPECTED[label]


def _fmt_cp(hip, label, **kw):
    import vc2hip_py
    w, h, cf, bits, wb, depth, u, a = SHAPES[label]
    fmt = vc2hip_py.picture_format(w, h, cf, bits, wb)
    assert hip.lib.vc2hip_slice_size_is_valid(depth, h, h // 2 if cf == "420" else h, u) and \
        hip.lib.vc2hip_slice_size_is_valid(depth, w, w if cf == "444" else w // 2, a), label
    return fmt, vc2hip_py.coding_params(hip.lib, fmt, WAVELET, depth, u, a, q=Q, scalar=8, **kw)


def _encode(hip, buf, n, fmt, cp):
    torch = _torch()
    stride = _stride(hip, fmt, cp)
    d_raw = _dev(buf)
    d_pay = torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    hip.encode_batch_dev(d_raw.data_ptr(), n, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    hip.sync()
    rec = hip.dwt_launches()
    lens = d_len.cpu().tolist()
    pay = d_pay.cpu().numpy()
    return [pay[i * stride:i * stride + lens[i]].tobytes() for i in range(n)], rec


def _decode(hip, pays, fmt, cp, out_bytes, call=None):
    torch = _torch()
    d_pay, d_len, stride = _slots(hip, pays, fmt, cp)
    d_out = torch.full((out_bytes,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    if call is None:
        hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), len(pays), fmt, cp, d_out.data_ptr())
    else:
        call(d_pay.data_ptr(), stride, d_len.data_ptr(), d_out.data_ptr())
    hip.sync()
    return d_out.cpu().numpy(), hip.dwt_launches()


def _planar_records(hip, e, fmt, cp):
    """the launch records of the same calls on planar little-endian LSB-justified pictures"""
    import vc2hip_py
    lay = vc2hip_py.sample_layout(1, 1)
    hip.set_packed_format(None)
    hip.set_sample_layout(lay)
    try:
        pays, fwd = _encode(hip, layout_ref.to_layout(b"".join(e["pics"]), fmt, N, lay), N, fmt, cp)
        assert pays == e["pays"]
        out, inv = _decode(hip, e["pays"], fmt, cp, len(b"".join(e["decs"])))
        assert layout_ref.from_layout(out, fmt, N, lay) == b"".join(e["decs"])
    finally:
        hip.set_sample_layout(None)
    return fwd, inv


def _check_against_the_oracle(hip, oracle, label, formats):
    e = _expected(oracle, label)
    fmt, cp = _fmt_cp(hip, label)
    file_raw, file_dec = b"".join(e["pics"]), b"".join(e["decs"])
    rng = np.random.default_rng(5)
    fwd0, inv0 = _planar_records(hip, e, fmt, cp)
    try:
        for name, pf in formats:
            what = f"{label} {name}"
            pf = _pk(pf)
            assert hip.packed_picture_bytes(fmt, pf) == packed_ref.picture_bytes(fmt, pf) > 0, what
            hip.set_packed_format(pf)
            src = packed_ref.to_packed(file_raw, fmt, N, pf, fill=SENTINEL, garbage=rng)
            got, fwd = _encode(hip, src, N, fmt, cp)
            assert [len(p) for p in got] == [len(p) for p in e["pays"]], f"{what}: payload lengths"
            assert got == e["pays"], f"{what}: payload"
            assert fwd == fwd0, f"{what}: the forward launches differ from the planar call's: {fwd} / {fwd0}"
            want = packed_ref.to_packed(file_dec, fmt, N, pf, fill=SENTINEL)
            out, inv = _decode(hip, e["pays"], fmt, cp, want.size)
            assert np.array_equal(out, want), f"{what}: decoded buffer (samples, zero bits, untouched gaps): {_diff(out, want)}"
            assert inv == inv0, f"{what}: the inverse launches differ from the planar call's: {inv} / {inv0}"
    finally:
        hip.set_packed_format(None)


# ------------------------------------------------------------------------------------------------------------------
# 1. encode + decode against the oracle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ("v210-384", "v210-416", "v210-wide", "v210-30"))
def test_v210_against_the_oracle(hip, oracle, label):
    fmt, _ = _fmt_cp(hip, label)
    _check_against_the_oracle(hip, oracle, label, [("tight", packed_ref.v210(fmt)), ("pitched", packed_ref.v210(fmt, True))])


@pytest.mark.parametrize("cf", ("420", "422", "444"))
@pytest.mark.parametrize("bits", (8, 10))
def test_semiplanar_against_the_oracle(hip, oracle, cf, bits):
    label = f"sp-{cf}-{bits}"
    fmt, _ = _fmt_cp(hip, label)
    forms = [(0, 0)] if bits == 8 else [(1, 0), (1, 1)]   # NV12 / NV16 / NV24; P010 / P210 / P410 form, and LE / LSB
    formats = [(f"le{le}-lsb{lsb}-{'pitched' if p else 'tight'}", packed_ref.semiplanar(fmt, le, lsb, p))
               for le, lsb in forms for p in (False, True)]
    _check_against_the_oracle(hip, oracle, label, formats)


# ------------------------------------------------------------------------------------------------------------------
# 2. the remaining calls, once with v210 and once with P210, against the file-format call put through the model
# ------------------------------------------------------------------------------------------------------------------
def _small(hip, kernel="DD97", w=256, h=128, cf="422", bits=10, depth=3, u=2, a=2, wb=2, n=N, seed=3, **kw):
    import vc2hip_py
    fmt = vc2hip_py.picture_format(w, h, cf, bits, wb)
    cp = vc2hip_py.coding_params(hip.lib, fmt, kernel, depth, u, a, **kw)
    raw = b"".join(_pictures(w, h, cf, bits, wb, n, seed))
    return fmt, cp, raw


def _two(fmt):
    """v210 pitched to 128 bytes with a picture gap, and P210 (little-endian, MSB-justified) pitched with a plane gap"""
    return [("v210", _pk(packed_ref.v210(fmt, True))), ("p210", _pk(packed_ref.semiplanar(fmt, 1, 0, True)))]


def test_recon_call(hip):
    torch = _torch()
    fmt, cp, raw = _small(hip, q=20, scalar=2)
    stride = _stride(hip, fmt, cp)
    ns = cp.y_slices * cp.x_slices

    def run(pf, src):
        hip.set_packed_format(pf)
        d_raw = _dev(src)
        d_rec = torch.full((src.size,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        d_pay = torch.zeros(N * stride, dtype=torch.uint8, device="cuda:0")
        d_len = torch.zeros(N, dtype=torch.int64, device="cuda:0")
        d_sse = torch.zeros(3 * N, dtype=torch.int64, device="cuda:0")
        d_q = torch.full((N * ns,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        hip.encode_recon_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr(), d_rec.data_ptr(),
                                   d_sse.data_ptr(), d_q.data_ptr())
        hip.sync()
        return d_rec.cpu().numpy(), d_sse.cpu().tolist(), d_pay.cpu().numpy().tobytes(), d_len.cpu().tolist(), d_q.cpu().tolist()

    try:
        rec0, sse0, pay0, len0, q0 = run(None, np.frombuffer(raw, np.uint8))
        assert any(sse0)
        rng = np.random.default_rng(9)
        for name, pf in _two(fmt):
            rec, sse, pay, lens, q = run(pf, packed_ref.to_packed(raw, fmt, N, pf, fill=SENTINEL, garbage=rng))
            want = packed_ref.to_packed(rec0.tobytes(), fmt, N, pf, fill=SENTINEL)
            assert np.array_equal(rec, want), f"{name}: d_recon: {_diff(rec, want)}"
            assert sse == sse0, f"{name}: d_sse"
            assert q == q0, f"{name}: d_qidx"
            assert (lens, pay) == (len0, pay0), f"{name}: payload"
    finally:
        hip.set_packed_format(None)


@pytest.mark.parametrize("tff", (True, False), ids=("top-first", "bottom-first"))
def test_field_calls(hip, tff):
    import vc2hip_py
    torch = _torch()
    n = 2
    ffmt, _, raw = _small(hip, kernel="LeGall", n=n, q=12, scalar=2)
    field = vc2hip_py.picture_format(256, 64, "422", 10)
    cp = vc2hip_py.coding_params(hip.lib, field, "LeGall", 3, 2, 2, q=12, scalar=2)
    stride = _stride(hip, field, cp)

    def enc(pf, src):
        hip.set_packed_format(pf)
        d = _dev(src)
        d_pay = torch.zeros(2 * n * stride, dtype=torch.uint8, device="cuda:0")
        d_len = torch.zeros(2 * n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        hip.encode_fields_batch_dev(d.data_ptr(), n, ffmt, tff, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
        hip.sync()
        lens = d_len.cpu().tolist()
        pay = d_pay.cpu().numpy()
        return [pay[i * stride:i * stride + lens[i]].tobytes() for i in range(2 * n)]

    call = lambda p, s, l, o: hip.decode_fields_batch_dev(p, s, l, n, ffmt, tff, cp, o)   # noqa: E731
    try:
        pays0 = enc(None, np.frombuffer(raw, np.uint8))
        dec0, _ = _decode(hip, pays0, field, cp, len(raw), call)
        for name, pf in _two(ffmt):   # (the format is the FRAME's)
            pays = enc(pf, packed_ref.to_packed(raw, ffmt, n, pf, fill=SENTINEL, garbage=np.random.default_rng(2)))
            assert pays == pays0, name
            want = packed_ref.to_packed(dec0.tobytes(), ffmt, n, pf, fill=SENTINEL)
            dec, _ = _decode(hip, pays0, field, cp, want.size, call)
            assert np.array_equal(dec, want), f"{name}: {_diff(dec, want)}"
    finally:
        hip.set_packed_format(None)


def test_reduced_call(hip):
    import vc2hip_py
    fmt, cp, raw = _small(hip, q=12, scalar=2)
    rfmt = vc2hip_py.reduced_format(fmt, 1)
    call = lambda p, s, l, o: hip.decode_reduced_batch_dev(p, s, l, N, fmt, cp, 1, o)   # noqa: E731
    try:
        hip.set_packed_format(None)
        pays, _ = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        dec0, inv0 = _decode(hip, pays, fmt, cp, N * hip.raw_picture_bytes(rfmt), call)
        for name, pf in _two(rfmt):   # (the format describes the REDUCED pictures)
            hip.set_packed_format(pf)
            want = packed_ref.to_packed(dec0.tobytes(), rfmt, N, pf, fill=SENTINEL)
            dec, _ = _decode(hip, pays, fmt, cp, want.size, call)
            assert np.array_equal(dec, want), f"{name}: {_diff(dec, want)}"
    finally:
        hip.set_packed_format(None)


def test_lanes_cut_the_batch_at_the_packed_stride():
    hip = _ctx()
    n = 5
    fmt, cp, raw = _small(hip, n=n, q=12, scalar=2)
    try:
        pays0, _ = _encode(hip, np.frombuffer(raw, np.uint8), n, fmt, cp)
        dec0, _ = _decode(hip, pays0, fmt, cp, len(raw))
        hip.set_streams(2)
        for name, pf in _two(fmt):
            hip.set_packed_format(pf)
            pays, _ = _encode(hip, packed_ref.to_packed(raw, fmt, n, pf, fill=SENTINEL, garbage=np.random.default_rng(1)), n, fmt, cp)
            assert pays == pays0, name
            want = packed_ref.to_packed(dec0.tobytes(), fmt, n, pf, fill=SENTINEL)
            dec, _ = _decode(hip, pays0, fmt, cp, want.size)
            assert np.array_equal(dec, want), f"{name}: {_diff(dec, want)}"
    finally:
        hip.close()


@pytest.mark.parametrize("name,kw", [
    ("hq_cbr", dict(mode="HQ_CBR", s=20000, scalar=2)),
    ("ld", dict(kernel="LeGall", mode="LD", s=12000)),
])
def test_other_modes(hip, name, kw):
    fmt, cp, raw = _small(hip, **kw)
    try:
        hip.set_packed_format(None)
        pays0, _ = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        dec0, _ = _decode(hip, pays0, fmt, cp, len(raw))
        for fname, pf in _two(fmt):
            hip.set_packed_format(pf)
            pays, _ = _encode(hip, packed_ref.to_packed(raw, fmt, N, pf, fill=SENTINEL, garbage=np.random.default_rng(4)), N, fmt, cp)
            assert pays == pays0, f"{name} {fname}: payload"
            want = packed_ref.to_packed(dec0.tobytes(), fmt, N, pf, fill=SENTINEL)
            dec, _ = _decode(hip, pays0, fmt, cp, want.size)
            assert np.array_equal(dec, want), f"{name} {fname}: {_diff(dec, want)}"
    finally:
        hip.set_packed_format(None)


# ------------------------------------------------------------------------------------------------------------------
# 3. state, capture, refusals
# ------------------------------------------------------------------------------------------------------------------
def test_clearing_the_format_restores_the_sample_layout(hip):
    """layout, packed format, clear: the call after is the layout's; and the host-buffer calls keep the file format"""
    import vc2hip_py
    fmt, cp, raw = _small(hip, q=12, scalar=2)
    lay = vc2hip_py.sample_layout(*[getattr(layout_ref.pitched(fmt, 1, 1), k) for k in
                                    ("little_endian", "lsb_justified", "pitch", "plane_offset", "picture_stride")])
    pf = _two(fmt)[0][1]
    try:
        hip.set_sample_layout(None)
        pays0, _ = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        dec0, _ = _decode(hip, pays0, fmt, cp, len(raw))
        hip.set_sample_layout(lay)
        hip.set_packed_format(pf)
        pays, _ = _encode(hip, packed_ref.to_packed(raw, fmt, N, pf, fill=SENTINEL), N, fmt, cp)
        assert pays == pays0
        one = len(raw) // N
        host_pay, _ = hip.encode_picture_hq(raw[:one], fmt, cp)
        assert host_pay == pays0[0]
        assert hip.decode_picture(pays0[0], fmt, cp) == dec0.tobytes()[:one]
        hip.set_packed_format(None)
        pays, _ = _encode(hip, layout_ref.to_layout(raw, fmt, N, lay, fill=SENTINEL), N, fmt, cp)
        assert pays == pays0, "the sample layout set before is in force again"
        want = layout_ref.to_layout(dec0.tobytes(), fmt, N, lay, fill=SENTINEL)
        dec, _ = _decode(hip, pays0, fmt, cp, want.size)
        assert np.array_equal(dec, want), _diff(dec, want)
        hip.set_packed_format(vc2hip_py.packed_format("none"))   # packing NONE: off as well
        pays, _ = _encode(hip, layout_ref.to_layout(raw, fmt, N, lay, fill=SENTINEL), N, fmt, cp)
        assert pays == pays0
    finally:
        hip.set_packed_format(None)
        hip.set_sample_layout(None)


@pytest.mark.parametrize("which", (0, 1), ids=("v210", "p210"))
def test_capture_and_replay(which):
    torch = _torch()
    s = torch.cuda.Stream()
    hip = _ctx(("PLANES8_NEVER",), stream=s.cuda_stream)
    fmt, cp, raw = _small(hip, q=12, scalar=2)
    pf = _two(fmt)[which][1]
    stride = _stride(hip, fmt, cp)
    src = packed_ref.to_packed(raw, fmt, N, pf, fill=SENTINEL, garbage=np.random.default_rng(6))
    try:
        with torch.cuda.stream(s):
            d_raw = _dev(src)
            d_pay = torch.zeros(N * stride, dtype=torch.uint8, device="cuda:0")
            d_len = torch.zeros(N, dtype=torch.int64, device="cuda:0")
            d_out = torch.full((src.size,), SENTINEL, dtype=torch.uint8, device="cuda:0")

            def call():
                hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
                hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, d_out.data_ptr())

            hip.set_packed_format(pf)
            call()                       # the warm-up, and the eager results
            s.synchronize()
            hip.sync()
            eager = (d_pay.cpu().numpy().copy(), d_len.cpu().tolist(), d_out.cpu().numpy().copy())
            assert (eager[2] != SENTINEL).any()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=s):
                call()
        except BaseException as e:       # noqa: BLE001 -- whatever ended the capture
            pytest.fail("graph capture failed: %r" % (e,))
        hip.set_packed_format(None)      # the captured calls keep theirs
        with torch.cuda.stream(s):
            for r in range(2):
                d_pay.zero_(); d_len.zero_(); d_out.fill_(SENTINEL)
                g.replay()
                s.synchronize()
                hip.sync()
                assert d_len.cpu().tolist() == eager[1], r
                assert np.array_equal(d_pay.cpu().numpy(), eager[0]), r
                assert np.array_equal(d_out.cpu().numpy(), eager[2]), (r, _diff(d_out.cpu().numpy(), eager[2]))
    finally:
        hip.close()


def test_refusals_touch_nothing_and_keep_the_format(hip):
    import vc2hip_py
    torch = _torch()
    fmt, cp, raw = _small(hip, q=12, scalar=2)
    stride = _stride(hip, fmt, cp)
    good = _two(fmt)[0][1]
    row = packed_ref.v210_row_bytes(fmt.width)
    P = vc2hip_py.packed_format
    setter = [   # what the struct alone shows
        P(3), P(-1), P("semiplanar", 2, 0), P("semiplanar", 0, -1),
        P("v210", 1, 0), P("v210", 0, 1), P("v210", pitch=(768, 768)), P("v210", plane_offset=(16, 0)), P("v210", plane_offset=(0, 4096)),
        P("v210", pitch=(768 + 8, 0)), P("semiplanar", plane_offset=(0, 4100)), P("v210", picture_stride=768 * 128 + 4),
    ]
    caller = [   # the check needs fmt
        P("v210", pitch=(row - 16, 0)),
        P("semiplanar", pitch=(512, 496)),
        P("v210", pitch=(768, 0), picture_stride=(packed_ref.picture_bytes(fmt, P("v210", pitch=(768, 0))) - 1) // 16 * 16),
        P("v210", pitch=(1 << 23, 0)),
        P("v210", pitch=((1 << 31) // fmt.height // 16 * 16 + 16, 0)),
    ]
    src = packed_ref.to_packed(raw, fmt, N, good, fill=SENTINEL)
    ns = cp.y_slices * cp.x_slices

    def outputs():
        return (torch.full((N * stride,), SENTINEL, dtype=torch.uint8, device="cuda:0"), torch.full((N,), -1, dtype=torch.int64, device="cuda:0"),
                torch.full((src.size,), SENTINEL, dtype=torch.uint8, device="cuda:0"), torch.full((3 * N,), -1, dtype=torch.int64, device="cuda:0"))

    def untouched(o):
        hip.sync()
        return bool((o[0] == SENTINEL).all()) and bool((o[1] == -1).all()) and bool((o[2] == SENTINEL).all()) and bool((o[3] == -1).all())

    def refused(call):
        with pytest.raises(vc2hip_py.Vc2HipError) as ei:
            call()
        assert ei.value.code == EINVAL

    try:
        hip.set_packed_format(None)
        pays0, _ = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        hip.set_packed_format(good)
        for bad in setter:
            refused(lambda: hip.set_packed_format(bad))
        pays, _ = _encode(hip, src, N, fmt, cp)          # the format set before is still in force
        assert pays == pays0
        d_raw = _dev(src)
        d_pay, d_len, _ = _slots(hip, pays0, fmt, cp)

        def calls(o, f=fmt, c=cp):
            return [
                lambda: hip.encode_batch_dev(d_raw.data_ptr(), N, f, c, o[0].data_ptr(), stride, o[1].data_ptr()),
                lambda: hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, f, c, o[2].data_ptr()),
                lambda: hip.encode_recon_batch_dev(d_raw.data_ptr(), N, f, c, o[0].data_ptr(), stride, o[1].data_ptr(), o[2].data_ptr(),
                                                   o[3].data_ptr()),
            ]

        for bad in caller:
            hip.set_packed_format(bad)                   # well-formed: accepted here, refused where the format is known
            assert packed_ref.picture_bytes(fmt, bad) == 0 == hip.packed_picture_bytes(fmt, bad)
            o = outputs()
            torch.cuda.synchronize()
            for call in calls(o):
                refused(call)
            assert untouched(o), "a refused call wrote to an output buffer"
        # a fmt the packing does not admit
        o = outputs()
        torch.cuda.synchronize()
        hip.set_packed_format(good)
        # (each with coding parameters of its own that are valid for it, so that the packed format is what refuses the call)
        def own_cp(f):
            return vc2hip_py.coding_params(hip.lib, f, "DD97", 3, 2, 2, q=12, scalar=2)

        for bad_fmt in (vc2hip_py.picture_format(256, 128, "420", 10), vc2hip_py.picture_format(256, 128, "444", 10),
                        vc2hip_py.picture_format(256, 128, "422", 12), vc2hip_py.picture_format(256, 128, "422", 10, 2, 8),
                        vc2hip_py.picture_format(256, 128, "422", 8, 1), vc2hip_py.picture_format(255, 128, "422", 10)):
            for call in calls(o, bad_fmt, own_cp(bad_fmt))[:2]:
                refused(call)
        hip.set_packed_format(P("semiplanar", 1, 0))
        for wb in (3, 4):
            f = vc2hip_py.picture_format(256, 128, "422", 12, wb)
            for call in calls(o, f, own_cp(f))[:2]:
                refused(call)
        # The reduced call.  The issue's case "a reduced width that is odd" cannot be reached on its own: v210 is 4:2:2, and the
        # reduced call itself requires the chroma width (width / 2) to be a multiple of 2^drop_levels, so the reduced width is
        # always even when that rule passes.  (The even-width check of the packed format is pinned by the CPU test
        # test_library_arithmetic_agrees_with_the_model, case "v210 odd width".)  What can be reached: the format describes the
        # REDUCED pictures, so a pitch that holds less than a reduced row is refused.
        hip.set_packed_format(P("v210", pitch=(packed_ref.v210_row_bytes(fmt.width // 2) - 16, 0)))
        refused(lambda: hip.decode_reduced_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, 1, o[2].data_ptr()))
        # the overlap refusal of d_recon / d_raw uses the packed extents
        hip.set_packed_format(good)
        inside = d_raw.data_ptr() + (N - 1) * good.picture_stride + 16
        refused(lambda: hip.encode_recon_batch_dev(d_raw.data_ptr(), N, fmt, cp, o[0].data_ptr(), stride, o[1].data_ptr(), inside))
        assert untouched(o), "a refused call wrote to an output buffer"
        assert np.array_equal(d_raw.cpu().numpy(), src)
        pays, _ = _encode(hip, src, N, fmt, cp)
        assert pays == pays0
    finally:
        hip.set_packed_format(None)


def test_lanes_refuse_a_picture_stride_that_breaks_the_alignment_rule():
    """tight NV24 pictures of 40 x 13 one-byte samples are 3 x 520 = 1560 bytes, no multiple of 16: lane 1's base would break
    the 16-byte rule -- refused before lane 0 is enqueued; without lanes, or with an explicit stride, the call runs"""
    import vc2hip_py
    torch = _torch()
    hip = _ctx()
    try:
        fmt = vc2hip_py.picture_format(40, 13, "444", 8, 1)            # 3 x 520 = 1560 bytes = 97.5 x 16
        cp = vc2hip_py.coding_params(hip.lib, fmt, "LeGall", 2, 1, 1, q=8, scalar=2)
        pf = vc2hip_py.packed_format("semiplanar")
        assert hip.packed_picture_bytes(fmt, pf) % 16 == 8
        stride = _stride(hip, fmt, cp)
        raw = b"".join(_pictures(40, 13, "444", 8, 1, 4, 5))
        hip.set_packed_format(pf)
        src = packed_ref.to_packed(raw, fmt, 4, pf)
        pays0, _ = _encode(hip, src, 4, fmt, cp)
        hip.set_streams(2)
        d_raw = _dev(src)
        o_pay = torch.full((4 * stride,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        o_len = torch.full((4,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(vc2hip_py.Vc2HipError) as ei:
            hip.encode_batch_dev(d_raw.data_ptr(), 4, fmt, cp, o_pay.data_ptr(), stride, o_len.data_ptr())
        assert ei.value.code == EINVAL
        hip.sync()
        assert bool((o_pay == SENTINEL).all()) and bool((o_len == -1).all()), "a refused call wrote to an output buffer"
        hip.set_packed_format(vc2hip_py.packed_format("semiplanar", picture_stride=1568))   # an explicit stride: lanes run
        src = packed_ref.to_packed(raw, fmt, 4, vc2hip_py.packed_format("semiplanar", picture_stride=1568))
        pays, _ = _encode(hip, src, 4, fmt, cp)
        assert pays == pays0
    finally:
        hip.close()
