"""GPU tests of the caller's sample layout (vc2hip_set_sample_layout) on the device batch calls.

Every edge form of the transform (two-level, streaming, fast tile, generic tile, whole planes; 16-byte vector form and byte
loop) reads and writes pictures laid out by tests/layout_ref.py -- little- or big-endian words, the sample in the low or the
top bits, tight or pitched rows, gaps between planes and pictures -- at the smallest shapes tests/test_gpu_dwt_paths.py pins
those forms with (its GEOMS).  Expected payloads and decoded pictures are the oracle's on the same pictures in the file
format.  The encoder's input carries random bits in every ignored position and lies in a sentinel-filled buffer; the decoder
writes into a sentinel-filled buffer that is compared WHOLE with the model: sample values, zero bits and untouched gaps in
one comparison.  The launch record under a layout must equal the file format's, field by field.
"""
import itertools

import numpy as np
import pytest

import layout_ref
from synth import noise_frame, synth, words_frame
from test_gpu_dwt_paths import GEOMS, VARIANTS, _header_bytes, _unit_bytes
from vc2lib import make_params

pytestmark = pytest.mark.gpu

EINVAL = -1
N = 3            # pictures per batch: the picture stride matters
SENTINEL = 0xA5
WAVELET = "DD97"
Q = 24
BITS = {1: 8, 2: 10, 3: 12, 4: 12}
GEOM = {g[0]: g for g in GEOMS}

# (geometry, context): "wide" under the contexts that reach the two-level FIRST / streaming FINAL, the streaming FIRST and the
# fast tile forms; the generic tile, the whole planes and the byte loops under the default context
CASES = [("wide", "default"), ("wide", "levels"), ("wide", "tiles"), ("odd", "default"), ("plane", "default"),
         ("wide-w1", "default"), ("wide-w3", "default"), ("wide-w4", "default"), ("odd-w3", "default"), ("plane-w4", "default")]


def _torch():
    return pytest.importorskip("torch")


def _ctx(flags=(), stream=None):
    from vc2hip_py import FLAGS, Vc2Hip
    return Vc2Hip(stream=stream, flags=sum(FLAGS[f] for f in flags))


@pytest.fixture(scope="module")
def ctxs():
    # (16-bit band planes only: the adaptive choice of the byte form follows the batch before, and the launch records of two
    # calls are compared field by field here.  The edge forms do not depend on it)
    return {name: _ctx(VARIANTS[name] + ("PLANES8_NEVER",)) for name in ("default", "levels", "tiles")}


def _lay(x):
    """a layout_ref / vc2hip_py layout as the binding's structure (None stays None)"""
    import vc2hip_py
    if x is None or isinstance(x, vc2hip_py.SampleLayout):
        return x
    return vc2hip_py.sample_layout(x.little_endian, x.lsb_justified, x.pitch, x.plane_offset, x.picture_stride)


def _layouts(fmt, full):
    """(name, layout): the full cross of byte order x justification x {tight, pitched}, or little-endian LSB tight plus one
    pitched big-endian MSB layout (pure striding)"""
    import vc2hip_py
    if full:
        for le, lsb in itertools.product((0, 1), (0, 1)):
            if le or lsb:
                yield f"le{le}-lsb{lsb}-tight", vc2hip_py.sample_layout(le, lsb)
            yield f"le{le}-lsb{lsb}-pitched", _lay(layout_ref.pitched(fmt, le, lsb))
    else:
        yield "le1-lsb1-tight", vc2hip_py.sample_layout(1, 1)
        yield "le0-lsb0-pitched", _lay(layout_ref.pitched(fmt, 0, 0))


def _pictures(w, h, cf, bits, wb, n, seed=11, noise=False):
    """n file-format pictures: synth's smooth ones and, with noise, uniform noise as the last"""
    out = []
    for i in range(n):
        last = noise and i == n - 1
        if wb <= 2:
            out.append(noise_frame(w, h, cf, bits, seed + i, word_bytes=wb) if last else synth(w, h, cf, bits, seed + i, word_bytes=wb))
        else:
            v = np.frombuffer(synth(w, h, cf, bits, seed + i), ">u2").astype(np.uint32) >> (16 - bits)
            u = v << (8 * wb - bits)
            smooth = np.stack([(u >> (8 * (wb - 1 - k))) & 0xFF for k in range(wb)], axis=1).astype(np.uint8).tobytes()
            out.append(words_frame(w, h, cf, bits, seed + i, wb, "noise") if last else smooth)
    return out


_EXPECTED = {}


def _expected(oracle, label):
    """(fmt, cp arguments, pictures, the oracle's payloads, the oracle's decoded pictures) of a geometry; computed once"""
    if label not in _EXPECTED:
        _, w, h, cf, depth, u, a, wb, _ = GEOM[label]
        bits = BITS[wb]
        scalar = 256 if label.startswith("plane") else 8
        pics = _pictures(w, h, cf, bits, wb, N, noise=not label.startswith("plane"))   # (one slice per picture: no room for noise)
        p = make_params(w, h, cf, bits, WAVELET, depth, u, a, q=Q, scalar=scalar, word_bytes=wb)
        hb = _header_bytes(oracle, p)
        pays, decs = [], []
        for raw in pics:
            stream = oracle.encode_stream(p, raw, 1)
            want, got_n = oracle.decode_stream(p, stream, 1)
            assert got_n == 1
            pays.append(stream[-13 - (_unit_bytes(stream) - hb):-13])
            decs.append(want)
        _EXPECTED[label] = dict(w=w, h=h, cf=cf, bits=bits, wb=wb, depth=depth, u=u, a=a, scalar=scalar, pics=pics, pays=pays, decs=decs)
    return _EXPECTED[label]


def _fmt_cp(hip, e, **kw):
    import vc2hip_py
    fmt = vc2hip_py.picture_format(e["w"], e["h"], e["cf"], e["bits"], e["wb"])
    cp = vc2hip_py.coding_params(hip.lib, fmt, WAVELET, e["depth"], e["u"], e["a"], q=Q, scalar=e["scalar"], **kw)
    return fmt, cp


def _stride(hip, fmt, cp):
    return (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256


def _dev(a):
    torch = _torch()
    return torch.from_numpy(np.array(a, copy=True)).to("cuda:0")


def _encode(hip, buf, n, fmt, cp):
    """buf: the input buffer (numpy uint8).  Returns (payload list, launch record)."""
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


def _slots(hip, pays, fmt, cp):
    torch = _torch()
    stride = _stride(hip, fmt, cp)
    slots = np.zeros(len(pays) * stride, np.uint8)
    for i, p in enumerate(pays):
        slots[i * stride:i * stride + len(p)] = np.frombuffer(p, np.uint8)
    return _dev(slots), torch.tensor([len(p) for p in pays], dtype=torch.int64, device="cuda:0"), stride


def _decode(hip, pays, fmt, cp, out_bytes, call=None):
    """decode into a sentinel-filled buffer of out_bytes; returns (the whole buffer, launch record)"""
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


def _diff(got, want):
    bad = np.flatnonzero(got != want)
    return "equal" if not bad.size else f"{bad.size} bytes differ, the first at {bad[0]}: {got[bad[0]]:#x} for {want[bad[0]]:#x}"


# ------------------------------------------------------------------------------------------------------------------
# 1. every edge form under every layout, against the oracle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,var", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_edge_forms_against_the_oracle(ctxs, oracle, label, var):
    hip = ctxs[var]
    e = _expected(oracle, label)
    fmt, cp = _fmt_cp(hip, e)
    n = N
    file_raw = b"".join(e["pics"])
    file_dec = b"".join(e["decs"])
    rng = np.random.default_rng(5)
    # the file format on this context: the oracle's results, and the launch records to hold every layout to
    hip.set_sample_layout(None)
    pays, fwd0 = _encode(hip, np.frombuffer(file_raw, np.uint8), n, fmt, cp)
    assert pays == e["pays"], f"{label} [{var}] file format: payload"
    out, inv0 = _decode(hip, e["pays"], fmt, cp, len(file_dec))
    assert out.tobytes() == file_dec, f"{label} [{var}] file format: decoded picture"
    assert any(r["edge"] for r in fwd0) or label.startswith("plane"), fwd0
    try:
        for name, lay in _layouts(fmt, full=(label, var) == ("wide", "default")):
            what = f"{label} [{var}] {name}"
            hip.set_sample_layout(lay)
            src = layout_ref.to_layout(file_raw, fmt, n, lay, fill=SENTINEL, garbage=rng)
            got, fwd = _encode(hip, src, n, fmt, cp)
            assert [len(p) for p in got] == [len(p) for p in e["pays"]], f"{what}: payload lengths"
            assert got == e["pays"], f"{what}: payload"
            assert fwd == fwd0, f"{what}: the forward launches differ from the file format's: {fwd} / {fwd0}"
            want = layout_ref.to_layout(file_dec, fmt, n, lay, fill=SENTINEL)
            out, inv = _decode(hip, e["pays"], fmt, cp, want.size)
            assert np.array_equal(out, want), f"{what}: decoded buffer (samples, zero bits, untouched gaps): {_diff(out, want)}"
            assert inv == inv0, f"{what}: the inverse launches differ from the file format's: {inv} / {inv0}"
    finally:
        hip.set_sample_layout(None)


# ------------------------------------------------------------------------------------------------------------------
# 2. every call, against the file-format call's results put through the model
# ------------------------------------------------------------------------------------------------------------------
def _small(hip, kernel="DD97", w=256, h=128, cf="422", bits=10, depth=3, u=2, a=2, wb=2, chroma_bits=0, n=N, seed=3, **kw):
    import vc2hip_py
    fmt = vc2hip_py.picture_format(w, h, cf, bits, wb, chroma_bits)
    cp = vc2hip_py.coding_params(hip.lib, fmt, kernel, depth, u, a, **kw)
    raw = b"".join(_pictures(w, h, cf, bits, wb, n, seed))
    return fmt, cp, raw


def test_recon_call(ctxs):
    """d_recon whole-buffer, d_sse and payload equal to the file-format call's, with luma and chroma garbage bits present"""
    torch = _torch()
    hip = ctxs["default"]
    fmt, cp, raw = _small(hip, q=20, scalar=2)
    stride = _stride(hip, fmt, cp)

    def run(lay, src):
        hip.set_sample_layout(lay)
        d_raw = _dev(src)
        d_rec = torch.full((src.size,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        d_pay = torch.zeros(N * stride, dtype=torch.uint8, device="cuda:0")
        d_len = torch.zeros(N, dtype=torch.int64, device="cuda:0")
        d_sse = torch.zeros(3 * N, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        hip.encode_recon_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr(), d_rec.data_ptr(),
                                   d_sse.data_ptr())
        hip.sync()
        return d_rec.cpu().numpy(), d_sse.cpu().tolist(), d_pay.cpu().numpy().tobytes(), d_len.cpu().tolist()

    try:
        rec0, sse0, pay0, len0 = run(None, np.frombuffer(raw, np.uint8))
        assert any(sse0)
        rng = np.random.default_rng(9)
        for name, lay in _layouts(fmt, full=False):
            src = layout_ref.to_layout(raw, fmt, N, lay, fill=SENTINEL, garbage=rng)
            rec, sse, pay, lens = run(lay, src)
            want = layout_ref.to_layout(rec0.tobytes(), fmt, N, lay, fill=SENTINEL)
            assert np.array_equal(rec, want), f"{name}: d_recon: {_diff(rec, want)}"
            assert sse == sse0, f"{name}: d_sse"
            assert (lens, pay) == (len0, pay0), f"{name}: payload"
    finally:
        hip.set_sample_layout(None)


@pytest.mark.parametrize("tff", (True, False), ids=("top-first", "bottom-first"))
def test_field_calls_on_a_pitched_little_endian_frame_buffer(ctxs, tff):
    import vc2hip_py
    torch = _torch()
    hip = ctxs["default"]
    n = 2
    ffmt, _, raw = _small(hip, kernel="LeGall", n=n, q=12, scalar=2)
    field = vc2hip_py.picture_format(256, 64, "422", 10)
    cp = vc2hip_py.coding_params(hip.lib, field, "LeGall", 3, 2, 2, q=12, scalar=2)
    stride = _stride(hip, field, cp)
    lay = _lay(layout_ref.pitched(ffmt, 1, 1))

    def enc(lay_, src):
        hip.set_sample_layout(lay_)
        d = _dev(src)
        d_pay = torch.zeros(2 * n * stride, dtype=torch.uint8, device="cuda:0")
        d_len = torch.zeros(2 * n, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        hip.encode_fields_batch_dev(d.data_ptr(), n, ffmt, tff, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
        hip.sync()
        lens = d_len.cpu().tolist()
        pay = d_pay.cpu().numpy()
        return [pay[i * stride:i * stride + lens[i]].tobytes() for i in range(2 * n)], hip.dwt_launches()

    try:
        pays0, rec0 = enc(None, np.frombuffer(raw, np.uint8))
        pays, rec = enc(lay, layout_ref.to_layout(raw, ffmt, n, lay, fill=SENTINEL, garbage=np.random.default_rng(2)))
        assert pays == pays0 and rec == rec0
        hip.set_sample_layout(None)
        dec0, inv0 = _decode(hip, pays0, field, cp, len(raw),
                             lambda p, s, l, o: hip.decode_fields_batch_dev(p, s, l, n, ffmt, tff, cp, o))
        hip.set_sample_layout(lay)
        want = layout_ref.to_layout(dec0.tobytes(), ffmt, n, lay, fill=SENTINEL)
        dec, inv = _decode(hip, pays0, field, cp, want.size,
                           lambda p, s, l, o: hip.decode_fields_batch_dev(p, s, l, n, ffmt, tff, cp, o))
        assert np.array_equal(dec, want), _diff(dec, want)
        assert inv == inv0
    finally:
        hip.set_sample_layout(None)


@pytest.mark.parametrize("drop", (1, 2))
def test_reduced_call_into_a_pitched_layout(ctxs, drop):
    import vc2hip_py
    hip = ctxs["default"]
    fmt, cp, raw = _small(hip, q=12, scalar=2)
    rfmt = vc2hip_py.reduced_format(fmt, drop)
    try:
        hip.set_sample_layout(None)
        pays, _ = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        call = lambda p, s, l, o: hip.decode_reduced_batch_dev(p, s, l, N, fmt, cp, drop, o)   # noqa: E731
        dec0, inv0 = _decode(hip, pays, fmt, cp, N * hip.raw_picture_bytes(rfmt), call)
        for lay in (_lay(layout_ref.pitched(rfmt, 1, 1)), _lay(layout_ref.pitched(rfmt, 0, 0))):
            hip.set_sample_layout(lay)
            want = layout_ref.to_layout(dec0.tobytes(), rfmt, N, lay, fill=SENTINEL)
            dec, inv = _decode(hip, pays, fmt, cp, want.size, call)
            assert np.array_equal(dec, want), _diff(dec, want)
            assert inv == inv0
        # the layout describes the REDUCED pictures' buffer: a pitch that holds only part of a reduced row is refused
        hip.set_sample_layout(vc2hip_py.sample_layout(1, 1, pitch=(rfmt.width * 2 - 16, 0, 0)))
        with pytest.raises(vc2hip_py.Vc2HipError) as ei:
            _decode(hip, pays, fmt, cp, 1 << 20, call)
        assert ei.value.code == EINVAL
    finally:
        hip.set_sample_layout(None)


def test_lanes_use_the_contexts_layout(oracle):
    """set_streams(2) with n = 5: every lane reads and writes its pictures at the layout's picture stride"""
    hip = _ctx()
    n = 5
    fmt, cp, raw = _small(hip, n=n, q=12, scalar=2)
    try:
        pays0, _ = _encode(hip, np.frombuffer(raw, np.uint8), n, fmt, cp)
        dec0, _ = _decode(hip, pays0, fmt, cp, len(raw))
        hip.set_streams(2)
        for lay in (_lay(layout_ref.pitched(fmt, 1, 1)), _lay(layout_ref.pitched(fmt, 0, 0))):
            hip.set_sample_layout(lay)
            pays, _ = _encode(hip, layout_ref.to_layout(raw, fmt, n, lay, fill=SENTINEL, garbage=np.random.default_rng(1)), n, fmt, cp)
            assert pays == pays0
            want = layout_ref.to_layout(dec0.tobytes(), fmt, n, lay, fill=SENTINEL)
            dec, _ = _decode(hip, pays0, fmt, cp, want.size)
            assert np.array_equal(dec, want), _diff(dec, want)
    finally:
        hip.close()


@pytest.mark.parametrize("name,kw", [
    ("hq_cbr", dict(mode="HQ_CBR", s=20000, scalar=2)),
    ("ld", dict(kernel="LeGall", cf="420", bits=8, wb=1, mode="LD", s=12000)),
    ("fidelity_444_12", dict(kernel="Fidelity", w=192, h=96, cf="444", bits=12, depth=2, q=10)),   # streaming edge, no two-level kernel
    ("chroma_depth_8_of_10", dict(chroma_bits=8, q=12, scalar=2)),                                 # encode only: the decoder has one depth
])
def test_other_modes_and_formats(ctxs, name, kw):
    hip = ctxs["default"]
    fmt, cp, raw = _small(hip, **kw)
    if fmt.chroma_bit_depth:   # the chroma words hold 8-bit samples
        import vc2hip_py
        c8 = vc2hip_py.picture_format(fmt.width, fmt.height, "422", 8, 2)
        ysz = fmt.width * fmt.height * 2
        raw = b"".join(p[:ysz] + q[ysz:] for p, q in zip(_pictures(256, 128, "422", 10, 2, N, 3), _pictures(256, 128, "422", 8, 2, N, 4)))
        assert hip.raw_picture_bytes(c8) * N == len(raw)
    try:
        hip.set_sample_layout(None)
        pays0, fwd0 = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        dec0 = inv0 = None
        if not fmt.chroma_bit_depth:
            dec0, inv0 = _decode(hip, pays0, fmt, cp, len(raw))
        for lname, lay in _layouts(fmt, full=False):
            hip.set_sample_layout(lay)
            pays, fwd = _encode(hip, layout_ref.to_layout(raw, fmt, N, lay, fill=SENTINEL, garbage=np.random.default_rng(4)), N, fmt, cp)
            assert pays == pays0, f"{name} {lname}: payload"
            assert fwd == fwd0, f"{name} {lname}: forward launches"
            if dec0 is not None:
                want = layout_ref.to_layout(dec0.tobytes(), fmt, N, lay, fill=SENTINEL)
                dec, inv = _decode(hip, pays0, fmt, cp, want.size)
                assert np.array_equal(dec, want), f"{name} {lname}: {_diff(dec, want)}"
                assert inv == inv0, f"{name} {lname}: inverse launches"
    finally:
        hip.set_sample_layout(None)


# ------------------------------------------------------------------------------------------------------------------
# 3. state, capture, refusals, torch_planes
# ------------------------------------------------------------------------------------------------------------------
def test_the_layout_does_not_outlive_its_reset(ctxs):
    """set, call, set_sample_layout(None), call: the second call is the file-format call (nothing of the layout stays in
    cached launch parameters); and the host-buffer picture calls keep the file format while a layout is set"""
    hip = ctxs["default"]
    fmt, cp, raw = _small(hip, q=12, scalar=2)
    try:
        hip.set_sample_layout(None)
        pays0, _ = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        dec0, _ = _decode(hip, pays0, fmt, cp, len(raw))
        lay = _lay(layout_ref.pitched(fmt, 1, 1))
        hip.set_sample_layout(lay)
        pays, _ = _encode(hip, layout_ref.to_layout(raw, fmt, N, lay, fill=SENTINEL), N, fmt, cp)
        assert pays == pays0
        one = len(raw) // N
        host_pay, _ = hip.encode_picture_hq(raw[:one], fmt, cp)         # host buffers: the file format, layout or not
        assert host_pay == pays0[0]
        assert hip.decode_picture(pays0[0], fmt, cp) == dec0.tobytes()[:one]
        hip.set_sample_layout(None)
        pays, _ = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        assert pays == pays0
        dec, _ = _decode(hip, pays0, fmt, cp, len(raw))
        assert np.array_equal(dec, dec0)
    finally:
        hip.set_sample_layout(None)


def test_capture_and_replay_with_a_layout():
    """on a caller's stream, after a warm-up: one encode + decode captured with a layout set, replayed twice; a captured call
    keeps the layout it was captured with (the context is reset to the file format before the replays)"""
    torch = _torch()
    s = torch.cuda.Stream()
    hip = _ctx(("PLANES8_NEVER",), stream=s.cuda_stream)
    fmt, cp, raw = _small(hip, q=12, scalar=2)
    lay = _lay(layout_ref.pitched(fmt, 1, 1))
    stride = _stride(hip, fmt, cp)
    src = layout_ref.to_layout(raw, fmt, N, lay, fill=SENTINEL, garbage=np.random.default_rng(6))
    try:
        with torch.cuda.stream(s):
            d_raw = _dev(src)
            d_pay = torch.zeros(N * stride, dtype=torch.uint8, device="cuda:0")
            d_len = torch.zeros(N, dtype=torch.int64, device="cuda:0")
            d_out = torch.full((src.size,), SENTINEL, dtype=torch.uint8, device="cuda:0")

            def call():
                hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
                hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, d_out.data_ptr())

            hip.set_sample_layout(lay)
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
        hip.set_sample_layout(None)      # the captured calls keep theirs
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


def test_refusals_touch_nothing_and_keep_the_layout(ctxs):
    import vc2hip_py
    torch = _torch()
    hip = ctxs["default"]
    fmt, cp, raw = _small(hip, q=12, scalar=2)
    stride = _stride(hip, fmt, cp)
    good = _lay(layout_ref.pitched(fmt, 1, 1))
    ok = layout_ref.pitched(fmt)
    row = fmt.width * 2
    setter = [   # malformed structs: refused by the setter
        vc2hip_py.sample_layout(2, 0), vc2hip_py.sample_layout(0, -1),
        vc2hip_py.sample_layout(pitch=(ok.pitch[0] + 8, 0, 0)),
        vc2hip_py.sample_layout(pitch=ok.pitch, plane_offset=(0, ok.plane_offset[1] + 4, ok.plane_offset[2])),
        vc2hip_py.sample_layout(pitch=ok.pitch, plane_offset=ok.plane_offset, picture_stride=ok.picture_stride + 2),
    ]
    caller = [   # the check needs fmt: refused by the batch calls
        vc2hip_py.sample_layout(1, 1, pitch=(row - 16, 0, 0)),
        vc2hip_py.sample_layout(1, 1, pitch=ok.pitch, plane_offset=ok.plane_offset,
                                picture_stride=(layout_ref.picture_bytes(fmt, ok) - 1) // 16 * 16),
        vc2hip_py.sample_layout(1, 1, pitch=(1 << 23, 0, 0)),
        vc2hip_py.sample_layout(1, 1, pitch=((1 << 31) // fmt.height // 16 * 16 + 16, 0, 0)),
    ]
    src = layout_ref.to_layout(raw, fmt, N, good, fill=SENTINEL)
    try:
        hip.set_sample_layout(None)
        pays0, _ = _encode(hip, np.frombuffer(raw, np.uint8), N, fmt, cp)
        hip.set_sample_layout(good)
        for bad in setter:
            with pytest.raises(vc2hip_py.Vc2HipError) as ei:
                hip.set_sample_layout(bad)
            assert ei.value.code == EINVAL
        pays, _ = _encode(hip, src, N, fmt, cp)          # the previous layout is still in force
        assert pays == pays0
        d_raw = _dev(src)
        d_pay, d_len, _ = _slots(hip, pays0, fmt, cp)
        for bad in caller:
            hip.set_sample_layout(bad)                   # well-formed: accepted here, refused where the format is known
            assert layout_ref.picture_bytes(fmt, bad) == 0 == hip.layout_picture_bytes(fmt, bad)
            o_pay = torch.full((N * stride,), SENTINEL, dtype=torch.uint8, device="cuda:0")
            o_len = torch.full((N,), -1, dtype=torch.int64, device="cuda:0")
            o_raw = torch.full((src.size,), SENTINEL, dtype=torch.uint8, device="cuda:0")
            o_sse = torch.full((3 * N,), -1, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            calls = [
                lambda: hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, o_pay.data_ptr(), stride, o_len.data_ptr()),
                lambda: hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, o_raw.data_ptr()),
                lambda: hip.encode_recon_batch_dev(d_raw.data_ptr(), N, fmt, cp, o_pay.data_ptr(), stride, o_len.data_ptr(),
                                                   o_raw.data_ptr(), o_sse.data_ptr()),
            ]
            for call in calls:
                with pytest.raises(vc2hip_py.Vc2HipError) as ei:
                    call()
                assert ei.value.code == EINVAL
            hip.sync()
            assert bool((o_pay == SENTINEL).all()) and bool((o_len == -1).all()) and bool((o_raw == SENTINEL).all()) and \
                bool((o_sse == -1).all()), "a refused call wrote to an output buffer"
        hip.set_sample_layout(good)
        pays, _ = _encode(hip, src, N, fmt, cp)
        assert pays == pays0
    finally:
        hip.set_sample_layout(None)


def test_torch_planes(ctxs, oracle):
    """three int16 views carved from one padded allocation: encode, decode back into views, compare with the oracle"""
    import vc2hip_py
    torch = _torch()
    hip = ctxs["default"]
    e = _expected(oracle, "wide")
    fmt, cp = _fmt_cp(hip, e)
    w, h, cw = e["w"], e["h"], e["w"] // 2
    pitch = w + 40                                              # elements; 80 bytes of padding behind every luma row
    per = 3 * h * pitch + 1024
    samples = layout_ref.file_samples(b"".join(e["pics"]), fmt, N)

    def carve():
        big = torch.full((N * per + 8,), -1, dtype=torch.int16, device="cuda:0")
        start = (-big.data_ptr() % 16) // 2
        view = lambda at, cols: big.as_strided((N, h, cols), (per, pitch, 1), start + at)   # noqa: E731
        return big, view(0, w), view(h * pitch + 512, cw), view(2 * h * pitch + 512 + 64, cw)

    big, y, u, v = carve()
    for k, t in enumerate((y, u, v)):
        t.copy_(torch.from_numpy(np.stack([samples[i][k] for i in range(N)]).astype(np.int16)).to("cuda:0"))
    base, lay = vc2hip_py.torch_planes(y, u, v)
    stride = _stride(hip, fmt, cp)
    d_pay = torch.zeros(N * stride, dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(N, dtype=torch.int64, device="cuda:0")
    big2, y2, u2, v2 = carve()
    base2, lay2 = vc2hip_py.torch_planes(y2, u2, v2)
    assert bytes(lay2) == bytes(lay)
    try:
        hip.set_sample_layout(lay)
        torch.cuda.synchronize()
        hip.encode_batch_dev(base, N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
        hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, base2)
        hip.sync()
    finally:
        hip.set_sample_layout(None)
    lens = d_len.cpu().tolist()
    pay = d_pay.cpu().numpy()
    assert [pay[i * stride:i * stride + lens[i]].tobytes() for i in range(N)] == e["pays"]
    want = layout_ref.file_samples(b"".join(e["decs"]), fmt, N)
    for k, t in enumerate((y2, u2, v2)):
        assert np.array_equal(t.cpu().numpy().astype(np.int64), np.stack([want[i][k] for i in range(N)]).astype(np.int64)), k
    touched = int((big2 != -1).sum().item())               # (no sample is -1: every word outside the views must still be)
    assert touched == N * (h * w + 2 * h * cw), "words outside the views were written"
    with pytest.raises(ValueError):
        vc2hip_py.torch_planes(y[:, :, ::2], u, v)              # a non-unit last stride: no layout expresses it
