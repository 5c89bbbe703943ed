"""GPU tests of vc2hip_set_index_offsets (include/vc2hip.h): every payload, length, index map, decoded
picture and squared error of the three HQ VBR modes under a map of per-slice offsets against the CPU definition
tests/roi_ref.py, which stands on the oracle's quantiser and slice coder.  The caps are cap_ref.caps'.  A picture whose final
encode the oracle refuses (roi_ref.refused) is left out of its batch; test_a_refused_picture runs one alone."""
import numpy as np
import pytest

import cap_ref as cr
import capfill_ref as cf
import layout_ref as lr
import proxy_ref as pr
import qmatrix_ref as qr
import recon_ref as rr
import roi_ref as rf
from test_gpu_cap import DEV, EINVAL, FILL, VARIANTS, Enc, _ctx, _torch, capped, constq
from test_gpu_capfill import fillmode
from test_gpu_fields import _fields

pytestmark = pytest.mark.gpu

FLAGGED_ROWS = (0, 2, 5, rf.ESCAPES, rf.WHOLE_PLANE, rf.NEW)
SMALL = 2         # 512 x 64, 128 slices: the general form
MATRIX_PATTERNS = ("ramp", "roi", "extremes")
SETTINGS = ((0, None), (cr.MODE, "mid"), (cr.MODE, "none"), (cf.MODE, "mid-1"))   # (mode, cap name)
LEAD = 61         # the map starts this many bytes into its tensor: no alignment


@pytest.fixture(scope="module")
def variants():
    out = {name: _ctx(*flags) for name, flags in VARIANTS.items()}
    yield out
    for hip in out.values():
        hip.close()


class Map:
    """offsets on the device between two guards, at an odd address"""

    def __init__(self, rows, stride):
        """rows: one int8 array per picture (stride 0: one row for all); stride: bytes from picture to picture"""
        torch = _torch()
        rows = [np.asarray(r, np.int8).reshape(-1) for r in rows]
        ns = rows[0].size
        assert stride == 0 and len(rows) == 1 or stride >= ns
        body = np.full(max(stride, ns) * len(rows), FILL, np.uint8)
        for k, r in enumerate(rows):
            body[k * stride:k * stride + ns] = r.view(np.uint8)
        self.host = np.concatenate([np.full(LEAD, FILL, np.uint8), body, np.full(64, FILL, np.uint8)])
        self.t = torch.from_numpy(self.host.copy()).to(DEV)
        self.ptr, self.stride = self.t.data_ptr() + LEAD, stride
        torch.cuda.synchronize()

    def rewrite(self, rows):
        """other CONTENTS at the same address (queued on the current stream)"""
        other = Map(rows, self.stride)
        assert other.host.size == self.host.size
        self.host = other.host
        self.t.copy_(other.t, non_blocking=True)

    def unwritten(self):
        return bool((self.t.cpu().numpy() == self.host).all())


def mode_cp(cp, i, mode, cap, name="ramp"):
    if mode == 0:
        return constq(cp, 0 if name == "absolute" else rf.constq_index(i))
    return capped(cp, cap) if mode == cr.MODE else fillmode(cp, cap)


def decoded(oracle, m, qmap, pay):
    """(the decoder's picture of the definition's payload, its squared errors), once per map"""
    cache = m.__dict__.setdefault("_decoded", {})
    key = qmap.tobytes()
    if key not in cache:
        pic = qr.decode(oracle, m.case, pay, m.pic.qm)
        cache[key] = (pic, rr.squared_errors(m.case, m.pic.raw, pic))
    return cache[key]


def check(oracle, enc, want, payload, recon, tag):
    """want: [(Mapped, index map, payload)] per picture of the batch"""
    case = enc.case
    if payload:
        got = enc.payloads()
        for j, (m, qmap, pay) in enumerate(want):
            assert len(got[j]) == len(pay), (tag, j, "length", len(got[j]), len(pay))
            assert cf.slice_indices(got[j], enc.ns, case.prefix, case.scalar) == list(qmap.reshape(-1)), (tag, j, "index bytes")
            assert got[j] == pay, (tag, j, "payload")
    elif recon:
        assert enc.untouched(), tag
    if recon:
        q = enc.d_q.cpu().numpy().reshape(enc.n, enc.ns)
        rec, sse = enc.d_rec.cpu().numpy(), enc.d_sse.cpu().numpy().reshape(enc.n, 3)
        for j, (m, qmap, pay) in enumerate(want):
            assert (q[j] == qmap.reshape(-1)).all(), (tag, j, "d_qidx")
            pic, sums = decoded(oracle, m, qmap, pay)
            assert rec[j * enc.rb:(j + 1) * enc.rb].tobytes() == pic, (tag, j, "d_recon")
            assert [int(x) for x in sse[j]] == sums, (tag, j, "d_sse")
        assert (rec[enc.n * enc.rb:] == FILL).all(), tag


def wanted(oracle, i, name, mode, cname):
    """[(Mapped, map, payload)] of the pictures of row i the oracle codes under (pattern, mode, cap)"""
    out = []
    for k in range(3):
        qmap, pay = rf.expected(oracle, i, name, k, mode, cname)
        if pay is not rf.NOT_CODABLE:
            out.append((rf.mapped(oracle, i, name, k), qmap, pay))
    return out


def run(oracle, hip, i, name, mode, cname, payload=True, recon=True, tag=None):
    """one call on the codable pictures of the row under a broadcast map; returns the Enc (None: nothing codable)"""
    case, _ = cf.batch(oracle, i)
    want = wanted(oracle, i, name, mode, cname)
    if not want:
        return None
    omap = Map([rf.pattern(name, case.ys, case.xs)], 0)
    hip.set_index_offsets(omap.ptr, 0)
    try:
        enc = Enc(hip, case, [m.pic.raw for m, _, _ in want], recon=recon)
        cp = mode_cp(enc.cp, i, mode, rf.caps(oracle, i)[cname][0] if cname else 0, name)
        if recon:
            enc.recon(cp, payload)
        else:
            enc.encode(cp)
    finally:
        hip.set_index_offsets(None)
    check(oracle, enc, want, payload, recon, tag or (rf.IDS[i], name, mode, cname, payload))
    assert omap.unwritten(), (tag, "the map was written")
    return enc


@pytest.mark.parametrize("i", range(len(rf.MATRIX)), ids=rf.IDS)
def test_matrix(variants, oracle, i):
    """every row x pattern x (ConstQ, CAPPED at mid and none, FILL at mid-1) on the default context, through
    vc2hip_encode_recon_batch_dev with and without a payload; the launch profile shows the row's measuring form"""
    hip = variants["default"]
    hip.profile_enable(True)
    hip.profile_reset()
    calls = {0: 0, cr.MODE: 0, cf.MODE: 0}
    mixed = 0
    for name in MATRIX_PATTERNS:
        for mode, cname in SETTINGS:
            for payload in (True, False):
                enc = run(oracle, hip, i, name, mode, cname, payload)
                calls[mode] += enc is not None
            if enc is not None:
                mixed += any(len(set(q.reshape(-1).tolist())) > 1 for _, q, _ in wanted(oracle, i, name, mode, cname))
    prof = hip.profile()
    hip.profile_enable(False)
    assert calls[0] and calls[cr.MODE] and calls[cf.MODE], calls
    assert mixed or cf.batch(oracle, i)[0].ys * cf.batch(oracle, i)[0].xs == 1
    per = 2 if i in rf.FAST else 1     # the register kernel, then the general one over the slices it handed back
    assert prof["q_offsets"][0] == calls[0], prof
    assert prof["cap_measure1"][0] == prof["cap_measure2"][0] == per * (calls[cr.MODE] + calls[cf.MODE]), prof
    assert prof["cap_measure3"][0] == per * calls[cf.MODE] and prof["cap_fill"][0] == calls[cf.MODE], prof
    assert prof["cap_pick"][0] == 2 * (calls[cr.MODE] + calls[cf.MODE]), prof
    if i == rf.WHOLE_PLANE:
        assert any("plane" in x for x in prof), sorted(prof)


@pytest.mark.parametrize("name", ["store32", "general", "onepass", "twopass"])
@pytest.mark.parametrize("i", FLAGGED_ROWS, ids=lambda i: rf.IDS[i])
def test_flagged_contexts_give_the_same_bytes(variants, oracle, i, name):
    for pat in MATRIX_PATTERNS:
        for mode, cname in SETTINGS:
            run(oracle, variants[name], i, pat, mode, cname, recon=False, tag=(name, rf.IDS[i], pat, mode, cname))


def _plain(oracle, hip, i, mode, cname, offs):
    """(payload bytes, lengths, indices, pictures, errors, profile) of one recon call on row i; offs: None or a Map"""
    case, pics = cf.batch(oracle, i)
    want = wanted(oracle, i, "zero", mode, cname)
    enc = Enc(hip, case, [m.pic.raw for m, _, _ in want], recon=True)
    hip.set_index_offsets(offs.ptr if offs else None, offs.stride if offs else 0)
    hip.profile_enable(True)
    hip.profile_reset()
    enc.recon(mode_cp(enc.cp, i, mode, rf.caps(oracle, i)[cname][0] if cname else 0))
    prof = {k: v[0] for k, v in hip.profile().items()}
    hip.profile_enable(False)
    hip.set_index_offsets(None)
    return enc, prof


@pytest.mark.parametrize("i", [0, SMALL, rf.NEW], ids=lambda i: rf.IDS[i])
def test_zero_offsets_are_the_call_without_offsets(oracle, i):
    torch = _torch()
    case, _ = cf.batch(oracle, i)
    hip = _ctx()
    zero = Map([rf.pattern("zero", case.ys, case.xs)], 0)
    for mode, cname in SETTINGS:
        before, prof0 = _plain(oracle, hip, i, mode, cname, None)
        with_zero, prof1 = _plain(oracle, hip, i, mode, cname, zero)
        after, prof2 = _plain(oracle, hip, i, mode, cname, None)
        for a in (with_zero, after):
            for t in ("d_pay", "d_len", "d_q", "d_rec", "d_sse"):
                assert torch.equal(getattr(before, t), getattr(a, t)), (mode, cname, t)
        assert prof0 == prof2, (prof0, prof2)                       # set_index_offsets(None): the launches of before
        assert "q_offsets" not in prof0 and ("q_offsets" in prof1) == (mode == 0)
        swap = dict(prof1)
        if mode == 0:
            swap["fill"] = swap.get("fill", 0) + swap.pop("q_offsets")
        assert swap == prof0, (prof0, prof1)                        # the same rounds under the same names
        check(oracle, before, wanted(oracle, i, "zero", mode, cname), True, True, ("zero", mode, cname))
    assert zero.unwritten()
    hip.close()


def _small(oracle):
    case, pics = cf.batch(oracle, SMALL)
    return case, pics


def _per_picture_rows(case):
    return [rf.pattern(n, case.ys, case.xs) for n in ("ramp", "roi", "extremes")]


def _expect_rows(oracle, case, pics, rows, mode, cap):
    """[(Mapped, map, payload)] of pictures under their OWN rows of offsets"""
    out = []
    for p, r in zip(pics, rows):
        m = rf.Mapped(p, r)
        if mode == 0:
            b = rf.constq_index(SMALL)
            out.append((m, m.qmap(b), m.payload(b)))
        elif mode == cr.MODE:
            b = m.base(case.q, cap)
            out.append((m, m.qmap(b), m.payload(b)))
        else:
            f = rf.fill(m, case.q, cap)
            out.append((m, f.qmap, f.payload()))
    assert all(pay is not rf.NOT_CODABLE for _, _, pay in out)
    return out


def test_an_absolute_map(oracle):
    hip = _ctx()
    enc = run(oracle, hip, SMALL, "absolute", 0, None)
    assert enc is not None
    q = enc.d_q.cpu().numpy().reshape(enc.n, enc.ns)
    assert (q == rf.pattern("absolute", enc.case.ys, enc.case.xs)).all() and q.min() == 0 and q.max() == cr.Q_TOP
    hip.close()


@pytest.mark.parametrize("mode,cname", SETTINGS)
def test_a_map_per_picture_against_broadcast(oracle, mode, cname):
    """three patterns in one batch with picture_stride = ns + 3 (odd, unaligned); the same rows as three broadcast calls"""
    torch = _torch()
    case, pics = _small(oracle)
    ns = case.ys * case.xs
    cap = rf.caps(oracle, SMALL)[cname][0] if cname else 0
    rows = _per_picture_rows(case)
    # (extremes: the smooth picture codes at index 0 -- the noise pictures would not)
    order = [1, 2, 0]
    use = [pics[k] for k in order]
    want = _expect_rows(oracle, case, use, rows, mode, cap)
    hip = _ctx()
    omap = Map(rows, ns + 3)
    hip.set_index_offsets(omap.ptr, ns + 3)
    enc = Enc(hip, case, [p.raw for p in use], recon=True)
    cp = mode_cp(enc.cp, SMALL, mode, cap)
    enc.recon(cp)
    check(oracle, enc, want, True, True, ("per picture", mode, cname))
    pays = enc.payloads()
    for j in range(3):
        one = Map([rows[j]], 0)
        hip.set_index_offsets(one.ptr, 0)
        alone = Enc(hip, case, [use[j].raw]).encode(cp)
        assert alone.payloads() == [pays[j]], (j, "broadcast")
        assert one.unwritten()
    assert omap.unwritten()
    hip.set_index_offsets(None)
    hip.close()


@pytest.mark.parametrize("stride0", [True, False])
def test_two_lanes(oracle, stride0):
    torch = _torch()
    case, pics = _small(oracle)
    ns = case.ys * case.xs
    cap = rf.caps(oracle, SMALL)["mid-1"][0]
    use = [pics[1], pics[2], pics[0]]
    rows = [rf.pattern("ramp", case.ys, case.xs)] if stride0 else _per_picture_rows(case)
    stride = 0 if stride0 else ns + 3
    want = _expect_rows(oracle, case, use, rows * 3 if stride0 else rows, cf.MODE, cap)
    hip = _ctx()
    omap = Map(rows, stride)
    hip.set_index_offsets(omap.ptr, stride)
    one = Enc(hip, case, [p.raw for p in use], recon=True)
    cp = fillmode(one.cp, cap)
    check(oracle, one.recon(cp), want, True, True, "one stream")
    hip.set_streams(2)
    two = Enc(hip, case, [p.raw for p in use], recon=True).recon(cp)
    for t in ("d_pay", "d_len", "d_q", "d_rec", "d_sse"):
        assert torch.equal(getattr(one, t), getattr(two, t)), t
    hip.set_streams(1)
    assert omap.unwritten()
    hip.close()


def test_fields(oracle):
    """interlaced frames: the map is indexed by coded picture, 2 per frame, in slot order"""
    import vc2hip_py
    torch = _torch()
    from synth import noise_frame, synth
    c = dict(w=512, h=128, cf="422", bits=10)
    case = pr.Case(oracle, 512, 64, "422", 10, "DD97", 3, 1, 2, q=3, scalar=1)          # cap_ref.MATRIX[2]: a field
    ns = case.ys * case.xs
    frames = synth(512, 128, "422", 10, 91) + synth(512, 128, "422", 10, 93)
    fields = _fields(frames, c, 2)
    fb = case.raw_bytes()
    pics = [cr.Picture(oracle, case, fields[k * fb:(k + 1) * fb]) for k in range(4)]
    rows = _per_picture_rows(case) + [rf.pattern("zero", case.ys, case.xs)]
    cap = cf.caps(case, pics[0])["mid-1"][0]
    want = _expect_rows(oracle, case, pics, rows, cf.MODE, cap)
    hip = _ctx()
    omap = Map(rows, ns + 3)
    hip.set_index_offsets(omap.ptr, ns + 3)
    split = Enc(hip, case, [p.raw for p in pics]).encode(fillmode(case.fmt_cp(hip.lib)[1], cap))
    check(oracle, split, want, True, False, "split fields")
    ffmt = vc2hip_py.picture_format(512, 128, "422", 10)
    d_frames = torch.frombuffer(bytearray(frames), dtype=torch.uint8).to(DEV)
    d_pay, d_len = torch.full_like(split.d_pay, FILL), torch.full_like(split.d_len, -1)
    torch.cuda.synchronize()
    hip.encode_fields_batch_dev(d_frames.data_ptr(), 2, ffmt, True, fillmode(split.cp, cap), d_pay.data_ptr(), split.stride, d_len.data_ptr())
    hip.sync()
    assert torch.equal(d_len, split.d_len) and torch.equal(d_pay, split.d_pay)
    assert omap.unwritten()
    hip.close()


def test_a_little_endian_lsb_justified_layout(oracle):
    import vc2hip_py
    torch = _torch()
    case, pics = _small(oracle)
    cap = rf.caps(oracle, SMALL)["mid-1"][0]
    want = wanted(oracle, SMALL, "ramp", cf.MODE, "mid-1")
    assert len(want) == 3
    hip = _ctx()
    enc = Enc(hip, case, [p.raw for p in pics])
    layout = vc2hip_py.sample_layout(little_endian=True, lsb_justified=True)
    buf = lr.to_layout(b"".join(p.raw for p in pics), enc.fmt, 3, layout)
    enc.d_raw = torch.frombuffer(bytearray(np.asarray(buf, np.uint8).tobytes()), dtype=torch.uint8).to(DEV)
    torch.cuda.synchronize()
    hip.set_sample_layout(layout)
    omap = Map([rf.pattern("ramp", case.ys, case.xs)], 0)
    hip.set_index_offsets(omap.ptr)
    check(oracle, enc.encode(fillmode(enc.cp, cap)), want, True, False, "layout")
    hip.close()


def test_a_callers_quantisation_matrix(oracle):
    from test_gpu_capfill import MatrixPicture
    case, base = _small(oracle)
    qm = qr.matrix(oracle, "ragged", case.kernel, case.depth)
    pics = [MatrixPicture(oracle, case, p.raw, qm) for p in base]
    cap = cf.caps(case, pics[0])["mid-1"][0]
    rows = [rf.pattern("ramp", case.ys, case.xs)] * 3
    want = _expect_rows(oracle, case, pics, rows, cf.MODE, cap)
    hip = _ctx()
    hip.set_quant_matrix(qm)
    omap = Map(rows[:1], 0)
    hip.set_index_offsets(omap.ptr)
    enc = Enc(hip, case, [p.raw for p in pics], recon=True)
    check(oracle, enc.recon(fillmode(enc.cp, cap)), want, True, True, "matrix")
    hip.close()


def test_on_a_callers_stream_and_under_capture(oracle):
    """a warm-up, then: the call returns while a filler still runs in front of it (no wait); captured once and replayed after
    the map's CONTENTS were changed in place: every replay codes with the bytes it finds"""
    from test_gpu_caller_stream import Filler, _capture
    torch = _torch()
    case, pics = _small(oracle)
    cap = rf.caps(oracle, SMALL)["mid-1"][0]
    contents = ["ramp", "roi", "zero"]
    s = torch.cuda.Stream()
    hip = _ctx(stream=s.cuda_stream)
    with torch.cuda.stream(s):
        enc = Enc(hip, case, [p.raw for p in pics])
        cp = fillmode(enc.cp, cap)
        omap = Map([rf.pattern(contents[0], case.ys, case.xs)], 0)
        hip.set_index_offsets(omap.ptr)
        rings = [(torch.empty_like(enc.d_pay, device="cpu").pin_memory(), torch.empty_like(enc.d_len, device="cpu").pin_memory()) for _ in contents]

        def call():
            hip.encode_batch_dev(enc.d_raw.data_ptr(), 3, enc.fmt, cp, enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr())

        def store(r):
            rings[r][0].copy_(enc.d_pay, non_blocking=True)
            rings[r][1].copy_(enc.d_len, non_blocking=True)

        def verify(r, tag):
            enc2 = Enc.__new__(Enc)
            enc2.__dict__.update(enc.__dict__)
            enc2.d_pay, enc2.d_len = rings[r]
            check(oracle, enc2, wanted(oracle, SMALL, contents[r], cf.MODE, "mid-1"), True, False, (tag, contents[r]))

        call()                                  # the warm-up
        s.synchronize()
        hip.sync()
        e_fill = Filler(s).run()
        call()
        e = torch.cuda.Event()
        e.record(s)
        waited, filler_done = e.query(), e_fill.query()
        store(0)
        s.synchronize()
        hip.sync()
        verify(0, "behind the filler")
        assert not waited and not filler_done, "the call waited for the stream"
    g, _ = _capture(torch, s, hip, call)
    with torch.cuda.stream(s):
        for r in (1, 2):
            omap.rewrite([rf.pattern(contents[r], case.ys, case.xs)])
            g.replay()
            store(r)
        s.synchronize()
        hip.sync()
    for r in (1, 2):
        verify(r, "replay")
    assert omap.unwritten()
    hip.close()


def test_encode_batch_dev_itself(oracle):
    hip = _ctx()
    for mode, cname in SETTINGS:
        assert run(oracle, hip, SMALL, "roi", mode, cname, recon=False) is not None
    hip.close()


def test_stream_round_trip(oracle):
    """the payloads of a call under offsets are a plain HQ stream: written, read back to the same slots, decoded"""
    import vc2hip_py
    torch = _torch()
    hip = _ctx()
    enc = run(oracle, hip, SMALL, "ramp", cf.MODE, "mid-1")
    assert enc.n == 3
    pays = enc.payloads()
    scap = (sum(len(p) for p in pays) + 3 * 64 + 64 + 255) // 256 * 256
    d_stream = torch.full((scap,), FILL, dtype=torch.uint8, device=DEV)
    d_slen = torch.zeros(1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    cp0 = constq(enc.cp, enc.case.q)
    hip.stream_write_dev(enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr(), 3, cp0, vc2hip_py.stream_params(2, 0, 0, True), d_stream.data_ptr(),
                         scap, d_slen.data_ptr())
    hip.sync()
    slen = int(d_slen.cpu()[0])
    d_pay2, d_len2 = torch.full_like(enc.d_pay, FILL), torch.full_like(enc.d_len, -1)
    torch.cuda.synchronize()
    hip.stream_read_dev(d_stream.data_ptr(), slen, 3, cp0, vc2hip_py.stream_params(2), d_pay2.data_ptr(), enc.stride, d_len2.data_ptr())
    hip.sync()
    pay2, len2 = d_pay2.cpu().numpy().reshape(3, enc.stride), d_len2.cpu().numpy()
    assert [pay2[k, :int(len2[k])].tobytes() for k in range(3)] == pays
    out = torch.full((3 * enc.rb + 16,), FILL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    hip.decode_batch_dev(d_pay2.data_ptr(), enc.stride, d_len2.data_ptr(), 3, enc.fmt, cp0, out.data_ptr())
    hip.sync()
    assert torch.equal(out, enc.d_rec), "the decoder's picture"
    hip.close()


def test_ignored_by_the_host_buffer_call_and_the_transcoder(oracle):
    """with offsets set, vc2hip_encode_picture_hq and vc2hip_transcode_batch_dev give their offset-free bytes"""
    import vc2hip_py
    torch = _torch()
    case, pics = _small(oracle)
    cap = rf.caps(oracle, SMALL)["mid-1"][0]
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    q_in = next(q for q in range(case.q, cr.Q_TOP + 1) if all(p.table[q] is not cr.NOT_CODABLE for p in pics))
    src = Enc(hip, case, [p.raw for p in pics]).encode(constq(cp, q_in))      # the transcoder's input: coded without offsets
    tp = vc2hip_py.TranscodeParams(q_in + 9, 0)
    omap = Map([rf.pattern("extremes", case.ys, case.xs)], 0)
    outs = []
    for ptr in (None, omap.ptr):
        hip.set_index_offsets(ptr)
        d_out, d_len = torch.full_like(src.d_pay, FILL), torch.full_like(src.d_len, -1)
        torch.cuda.synchronize()
        hip.transcode_batch_dev(src.d_pay.data_ptr(), src.stride, src.d_len.data_ptr(), 3, src.fmt, constq(cp, q_in), tp, d_out.data_ptr(), src.stride,
                                d_len.data_ptr())
        hip.sync()
        host = [hip.encode_picture_hq(p.raw, fmt, fillmode(cp, cap)) for p in pics]
        outs.append((d_out, d_len, host))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and int(outs[0][1].min()) > 0
    for k, p in enumerate(pics):
        f = cf.fill(p, case.q, cap)
        for _, _, host in outs:
            assert host[k][0] == f.payload() and (np.asarray(host[k][1]).reshape(-1) == f.qmap.reshape(-1)).all(), k
    assert omap.unwritten()
    hip.close()


def test_a_refused_picture(oracle):
    """row 1's noise picture under `extremes` in ConstQ, alone in its batch: the oracle's error surfaces at vc2hip_sync"""
    from vc2hip_py import Vc2HipError
    from vc2lib import OracleError
    i, k = 1, 1
    assert k in rf.refused(oracle, i, "extremes", 0)
    case, pics = cf.batch(oracle, i)
    m = rf.mapped(oracle, i, "extremes", k)
    qmap = m.qmap(rf.constq_index(i))
    with pytest.raises(OracleError) as oe:
        y, u, v = (oracle.quantise_np(pl, case.depth, qmap, m.pic.qm) for pl in m.pic.planes)
        oracle.hq_pack(y, u, v, case.depth, qmap, case.prefix, case.scalar)
    hip = _ctx()
    omap = Map([rf.pattern("extremes", case.ys, case.xs)], 0)
    hip.set_index_offsets(omap.ptr)
    enc = Enc(hip, case, [pics[k].raw])
    with pytest.raises(Vc2HipError) as e:
        enc.encode(constq(enc.cp, rf.constq_index(i)))
    assert e.value.code == oe.value.code, (e.value.code, oe.value.code)
    hip.close()


def test_refusals_launch_nothing_and_touch_nothing(oracle):
    import vc2hip_py
    from vc2hip_py import Vc2HipError
    torch = _torch()
    case, pics = _small(oracle)
    ns = case.ys * case.xs
    cap = rf.caps(oracle, SMALL)["mid-1"][0]
    hip = _ctx()
    use = [pics[1], pics[2], pics[0]]             # (`extremes` on the smooth picture: the noise does not code at index 0)
    raws = [p.raw for p in use]
    omap = Map(_per_picture_rows(case), ns + 3)
    hip.set_index_offsets(omap.ptr, ns + 3)
    good = Enc(hip, case, raws, recon=True).recon(fillmode(case.fmt_cp(hip.lib)[1], cap))
    check(oracle, good, _expect_rows(oracle, case, use, _per_picture_rows(case), cf.MODE, cap), True, True, "before the refusals")
    before = hip.dwt_launches()
    hip.profile_enable(True)
    hip.profile_reset()
    enc = Enc(hip, case, raws, recon=True)
    fmt, cbr = case.fmt_cp(hip.lib)[0], type(enc.cp).from_buffer_copy(enc.cp)
    cbr.mode, cbr.compressed_bytes = 1, 3 * 20000
    ld = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 3, 1, 2, mode="LD", s=20000)
    tries = {"CBR": (cbr, ns + 3), "LD": (ld, ns + 3), "ConstQ 116": (constq(enc.cp, 116), ns + 3), "ConstQ -1": (constq(enc.cp, -1), ns + 3),
             "CAPPED 116": (capped(enc.cp, cap, 116), ns + 3), "FILL 116": (fillmode(enc.cp, cap, 116), ns + 3),
             "stride ns - 1": (fillmode(enc.cp, cap), ns - 1), "stride 1": (constq(enc.cp, 20), 1)}
    for what, (cp, stride) in tries.items():
        hip.set_index_offsets(omap.ptr, stride)
        calls = [lambda: hip.encode_batch_dev(enc.d_raw.data_ptr(), 3, enc.fmt, cp, enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr()),
                 lambda: hip.encode_recon_batch_dev(enc.d_raw.data_ptr(), 3, enc.fmt, cp, enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr(),
                                                    enc.d_rec.data_ptr(), enc.d_sse.data_ptr(), enc.d_q.data_ptr())]
        for call in calls:
            with pytest.raises(Vc2HipError) as e:
                call()
            assert e.value.code == EINVAL, (what, e.value.code)
            if what in ("CBR", "LD"):
                assert all(t in str(e.value) for t in ("HQ_CONSTQ", "HQ_CAPPED", "HQ_CAPPED_FILL")), str(e.value)
        hip.sync()
        assert enc.untouched() and (enc.d_rec == FILL).all() and (enc.d_q == -1).all() and (enc.d_sse == -1).all(), what
        assert hip.dwt_launches() == before and not sum(n for n, _ in hip.profile().values()), (what, hip.profile())
    # the fields call refuses the same
    d_frames = torch.zeros(2 * enc.rb * 2, dtype=torch.uint8, device=DEV)
    ffmt = vc2hip_py.picture_format(case.w, 2 * case.h, case.cf, case.bits)
    hip.set_index_offsets(omap.ptr, ns - 1)
    with pytest.raises(Vc2HipError) as e:
        hip.encode_fields_batch_dev(d_frames.data_ptr(), 1, ffmt, True, fillmode(enc.cp, cap), enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr())
    assert e.value.code == EINVAL and not sum(n for n, _ in hip.profile().values())
    hip.profile_enable(False)
    hip.set_index_offsets(omap.ptr, ns + 3)
    again = Enc(hip, case, raws, recon=True).recon(fillmode(enc.cp, cap))
    assert torch.equal(good.d_pay, again.d_pay) and torch.equal(good.d_q, again.d_q)
    assert omap.unwritten()
    hip.close()


@pytest.mark.parametrize("i", [SMALL, rf.NEW], ids=lambda i: rf.IDS[i])
def test_nothing_is_written_outside_the_outputs(oracle, i):
    """guards behind the n payload slots, d_lens, d_qidx, d_sse and d_recon and around the map keep their bytes"""
    torch = _torch()
    case, _ = cf.batch(oracle, i)
    hip = _ctx()
    guard = 4096
    for mode, cname in SETTINGS:
        want = wanted(oracle, i, "ramp", mode, cname)
        n = len(want)
        enc = Enc(hip, case, [m.pic.raw for m, _, _ in want], recon=True)
        enc.d_pay = torch.full((n * enc.stride + guard,), FILL, dtype=torch.uint8, device=DEV)
        enc.d_len = torch.full((n + guard,), -1, dtype=torch.int64, device=DEV)
        enc.d_q = torch.full((n * enc.ns + guard,), -1, dtype=torch.int32, device=DEV)
        enc.d_sse = torch.full((3 * n + guard,), -1, dtype=torch.int64, device=DEV)
        omap = Map([rf.pattern("ramp", case.ys, case.xs)], 0)
        hip.set_index_offsets(omap.ptr)
        torch.cuda.synchronize()
        enc.recon(mode_cp(enc.cp, i, mode, rf.caps(oracle, i)[cname][0] if cname else 0))
        assert (enc.d_pay[n * enc.stride:] == FILL).all() and (enc.d_len[n:] == -1).all()
        assert (enc.d_q[n * enc.ns:] == -1).all() and (enc.d_sse[3 * n:] == -1).all()
        assert (enc.d_rec[n * enc.rb:] == FILL).all() and omap.unwritten()
        lens = enc.d_len[:n].cpu().numpy()
        pay = enc.d_pay[:n * enc.stride].cpu().numpy().reshape(n, enc.stride)
        for j, (m, qmap, p) in enumerate(want):
            assert pay[j, :int(lens[j])].tobytes() == p, (mode, cname, j)
            assert (enc.d_q[j * enc.ns:(j + 1) * enc.ns].cpu().numpy() == qmap.reshape(-1)).all(), (mode, cname, j)
    hip.close()
