"""GPU tests of VC2HIP_HQ_CAPPED_FILL (include/vc2hip.h): every payload, length, index map, decoded
picture and squared error against the CPU definition tests/capfill_ref.py, which stands on the oracle's quantiser and slice
coder.  The caps come from picture 0's own table of lengths at run time (cap_ref.caps)."""
import numpy as np
import pytest

import cap_ref as cr
import capfill_ref as cf
import layout_ref as lr
import proxy_ref as pr
import qmatrix_ref as qr
import recon_ref as rr
from test_gpu_cap import DEV, EINVAL, FILL, VARIANTS, Enc, _ctx, _torch, capped, constq
from test_gpu_fields import _fields

pytestmark = pytest.mark.gpu

FLAGGED_ROWS = (0, 2, 5, cf.ESCAPES, cf.WHOLE_PLANE, cf.NEW)
SMALL = 2     # the smallest row with a mixed map: 512 x 64, 128 slices


@pytest.fixture(scope="module")
def variants():
    out = {name: _ctx(*flags) for name, flags in VARIANTS.items()}
    yield out
    for hip in out.values():
        hip.close()


def fillmode(cp, cap, floor=None):
    """cp with mode = VC2HIP_HQ_CAPPED_FILL, the cap and (optionally) another floor"""
    out = capped(cp, cap, floor)
    out.mode = cf.MODE
    return out


def decoded(oracle, f):
    """(the decoder's picture of the definition's payload, its squared errors), once per Filled"""
    if "_decoded" not in f.__dict__:
        case = f.pic.case
        pic = qr.decode(oracle, case, f.payload(), f.pic.qm)
        f._decoded = (pic, rr.squared_errors(case, f.pic.raw, pic))
    return f._decoded


def mixed_cap(pics, floor, caps):
    """the first of the five caps at which some picture of the batch gets a mixed map"""
    for name in cf.CAPS:
        fills = [cf.fill(p, floor, caps[name][0]) for p in pics]
        if any(0 < len(f.promoted) < f.ns for f in fills):
            return caps[name][0]
    raise AssertionError("no cap of this batch mixes two indices in one picture")


def check_payloads(enc, pics, floor, cap, tag):
    """payload bytes, lengths and every slice header's index byte; returns the Filled of every picture"""
    case, got = enc.case, enc.payloads()
    fills = [cf.fill(p, floor, cap) for p in pics]
    for i, f in enumerate(fills):
        want = f.payload()
        assert want is not cr.NOT_CODABLE, (tag, i)
        assert len(got[i]) == len(want), (tag, i, "length", len(got[i]), len(want), "q_i", f.q_i, "promoted", len(f.promoted))
        assert cf.slice_indices(got[i], enc.ns, case.prefix, case.scalar) == list(f.qmap.reshape(-1)), (tag, i, "indices")
        assert got[i] == want, (tag, i, "payload")
        if f.pic.fits(f.q_i, cap):
            assert f.pic.table[f.q_i] <= len(got[i]) <= cap, (tag, i)
    return fills


def check_recon(oracle, enc, fills, tag):
    """d_qidx = the map; d_recon and d_sse the decoder's picture of the definition's payload and its squared errors"""
    q = enc.d_q.cpu().numpy().reshape(enc.n, enc.ns)
    rec, sse = enc.d_rec.cpu().numpy(), enc.d_sse.cpu().numpy().reshape(enc.n, 3)
    for k, f in enumerate(fills):
        assert (q[k] == f.qmap.reshape(-1)).all(), (tag, k, "d_qidx")
        pic, sums = decoded(oracle, f)
        assert rec[k * enc.rb:(k + 1) * enc.rb].tobytes() == pic, (tag, k, "d_recon")
        assert [int(x) for x in sse[k]] == sums, (tag, k, "d_sse")
    assert (rec[enc.n * enc.rb:] == FILL).all(), tag


def expected_launches(i, name, calls):
    """per profile label: the fast form is two launches per round (the register kernel, then the general one over the slices
    it handed back), the general form one"""
    fast = i in cf.FAST and name in ("default", "onepass", "twopass")
    return calls * (2 if fast else 1)


@pytest.mark.parametrize("i", range(len(cf.MATRIX)), ids=cf.IDS)
def test_matrix(variants, oracle, i):
    """every row and cap on the default context, through vc2hip_encode_recon_batch_dev with and without a payload"""
    case, pics = cf.batch(oracle, i)
    caps = cf.caps(case, pics[0])
    raws = [p.raw for p in pics]
    hip = variants["default"]
    hip.profile_enable(True)
    hip.profile_reset()
    mixed = 0
    for cname in cf.CAPS:
        cap = caps[cname][0]
        for payload in (True, False):
            enc = Enc(hip, case, raws, recon=True)
            enc.recon(fillmode(enc.cp, cap), payload)
            if payload:
                fills = check_payloads(enc, pics, case.q, cap, (cname, "payload"))
            else:
                assert enc.untouched(), cname
            check_recon(oracle, enc, fills, (cname, payload))
        mixed += sum(0 < len(f.promoted) < f.ns for f in fills)
        if cname == "none":
            assert all(not f.filled and f.q_i == cr.Q_TOP for f in fills)
    prof = hip.profile()
    hip.profile_enable(False)
    assert mixed or enc.ns == 1, "no picture of this row mixes two indices"
    calls = 2 * len(cf.CAPS)
    want = expected_launches(i, "default", calls)   # (row ESCAPES is a fast row: both forms in the third round)
    assert prof["cap_measure1"][0] == prof["cap_measure2"][0] == prof["cap_measure3"][0] == want, prof
    assert prof["cap_pick"][0] == 2 * calls and prof["cap_fill"][0] == calls, prof
    if i == cf.WHOLE_PLANE:
        assert any("plane" in x for x in prof), sorted(prof)


@pytest.mark.parametrize("name", ["store32", "general", "onepass", "twopass"])
@pytest.mark.parametrize("i", FLAGGED_ROWS, ids=lambda i: cf.IDS[i])
def test_flagged_contexts_give_the_same_bytes(variants, oracle, i, name):
    case, pics = cf.batch(oracle, i)
    caps = cf.caps(case, pics[0])
    hip = variants[name]
    hip.profile_enable(True)
    hip.profile_reset()
    for cname in cf.CAPS:
        enc = Enc(hip, case, [p.raw for p in pics])
        check_payloads(enc.encode(fillmode(enc.cp, caps[cname][0])), pics, case.q, caps[cname][0], (name, cname))
    prof = hip.profile()
    hip.profile_enable(False)
    assert prof["cap_measure3"][0] == expected_launches(i, name, len(cf.CAPS)) and prof["cap_fill"][0] == len(cf.CAPS), (name, prof)


def _small(oracle):
    case, pics = cf.batch(oracle, SMALL)
    return case, pics, mixed_cap(pics, case.q, cf.caps(case, pics[0]))


def test_two_lanes_give_identical_bytes(oracle):
    torch = _torch()
    case, pics, cap = _small(oracle)
    raws = [p.raw for p in pics]
    hip = _ctx()
    one = Enc(hip, case, raws)
    check_payloads(one.encode(fillmode(one.cp, cap)), pics, case.q, cap, "one stream")
    hip.set_streams(2)
    two = Enc(hip, case, raws).encode(fillmode(one.cp, cap))
    assert torch.equal(one.d_pay, two.d_pay) and torch.equal(one.d_len, two.d_len)
    hip.set_streams(1)
    hip.close()


def test_fields(oracle):
    """interlaced frames: the cap is per field, and the fields' payloads are those of the filled encode of the split fields"""
    import vc2hip_py
    torch = _torch()
    from synth import noise_frame, synth
    c = dict(w=512, h=128, cf="422", bits=10)
    case = pr.Case(oracle, 512, 64, "422", 10, "DD97", 3, 1, 2, q=3, scalar=1)          # cap_ref.MATRIX[2]: a field
    frames = synth(512, 128, "422", 10, 91) + noise_frame(512, 128, "422", 10, 92)
    fields = _fields(frames, c, 2)
    fb = case.raw_bytes()
    pics = [cr.Picture(oracle, case, fields[k * fb:(k + 1) * fb]) for k in range(4)]
    cap = mixed_cap(pics, case.q, cf.caps(case, pics[0]))
    hip = _ctx()
    split = Enc(hip, case, [p.raw for p in pics]).encode(fillmode(case.fmt_cp(hip.lib)[1], cap))
    check_payloads(split, pics, case.q, cap, "split fields")
    ffmt = vc2hip_py.picture_format(512, 128, "422", 10)
    d_frames = torch.frombuffer(bytearray(frames), dtype=torch.uint8).to(DEV)
    d_pay, d_len = torch.full_like(split.d_pay, FILL), torch.full_like(split.d_len, -1)
    torch.cuda.synchronize()
    hip.encode_fields_batch_dev(d_frames.data_ptr(), 2, ffmt, True, fillmode(split.cp, cap), d_pay.data_ptr(), split.stride, d_len.data_ptr())
    hip.sync()
    assert torch.equal(d_len, split.d_len) and torch.equal(d_pay, split.d_pay)
    hip.close()


def test_a_little_endian_lsb_justified_layout_gives_the_same_payload(oracle):
    import vc2hip_py
    torch = _torch()
    case, pics, cap = _small(oracle)
    hip = _ctx()
    enc = Enc(hip, case, [p.raw for p in pics])
    layout = vc2hip_py.sample_layout(little_endian=True, lsb_justified=True)
    buf = lr.to_layout(b"".join(p.raw for p in pics), enc.fmt, 3, layout)
    enc.d_raw = torch.frombuffer(bytearray(np.asarray(buf, np.uint8).tobytes()), dtype=torch.uint8).to(DEV)
    torch.cuda.synchronize()
    hip.set_sample_layout(layout)
    check_payloads(enc.encode(fillmode(enc.cp, cap)), pics, case.q, cap, "layout")
    hip.close()


class MatrixPicture(cr.Picture):
    """cap_ref.Picture under a caller's quantisation matrix"""

    def __init__(self, oracle, case, raw, qm):
        self.oracle, self.case, self.raw = oracle, case, raw
        self.planes = rr.transform_planes(oracle, case, raw)
        self.qm = np.ascontiguousarray(qm, np.int32)
        self._pay = {}
        self.table = [self._len(q) for q in range(cr.Q_TOP + 1)]


def test_a_callers_quantisation_matrix(oracle):
    case, base, _ = _small(oracle)
    qm = qr.matrix(oracle, "ragged", case.kernel, case.depth)
    assert list(qm) != list(base[0].qm)
    pics = [MatrixPicture(oracle, case, p.raw, qm) for p in base]
    cap = mixed_cap(pics, case.q, cf.caps(case, pics[0]))
    hip = _ctx()
    hip.set_quant_matrix(qm)
    enc = Enc(hip, case, [p.raw for p in pics], recon=True)
    fills = check_payloads(enc.recon(fillmode(enc.cp, cap)), pics, case.q, cap, "matrix")
    check_recon(oracle, enc, fills, "matrix")
    hip.set_quant_matrix(None)
    hip.close()


def test_on_a_callers_stream_and_under_capture(oracle):
    """a warm-up, then: the call returns while a filler still runs in front of it (no wait); captured once and replayed on two
    other inputs, every replay gives each picture its own map"""
    from test_gpu_caller_stream import Filler, _capture
    torch = _torch()
    case, pics, cap = _small(oracle)
    orders = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    s = torch.cuda.Stream()
    hip = _ctx(stream=s.cuda_stream)
    with torch.cuda.stream(s):
        enc = Enc(hip, case, [pics[k].raw for k in orders[0]])
        cp = fillmode(enc.cp, cap)
        inputs = [torch.frombuffer(bytearray(b"".join(pics[k].raw for k in o)), dtype=torch.uint8).pin_memory() for o in orders]
        rings = [(torch.empty_like(enc.d_pay, device="cpu").pin_memory(), torch.empty_like(enc.d_len, device="cpu").pin_memory()) for _ in orders]

        def call():
            hip.encode_batch_dev(enc.d_raw.data_ptr(), 3, enc.fmt, cp, enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr())

        def check(r, tag):
            enc2 = Enc.__new__(Enc)
            enc2.__dict__.update(enc.__dict__)
            enc2.d_pay, enc2.d_len = rings[r]
            check_payloads(enc2, [pics[k] for k in orders[r]], case.q, cap, (tag, r))

        call()                                  # the warm-up
        s.synchronize()
        hip.sync()
        enc.d_raw.copy_(inputs[1], non_blocking=True)
        s.synchronize()
        e_fill = Filler(s).run()
        call()
        e = torch.cuda.Event()
        e.record(s)
        waited, filler_done = e.query(), e_fill.query()
        rings[1][0].copy_(enc.d_pay, non_blocking=True)
        rings[1][1].copy_(enc.d_len, non_blocking=True)
        s.synchronize()
        hip.sync()
        check(1, "behind the filler")
        assert not waited and not filler_done, "the call waited for the stream"
    g, _ = _capture(torch, s, hip, call)
    with torch.cuda.stream(s):
        for r in (2, 0):
            enc.d_raw.copy_(inputs[r], non_blocking=True)
            g.replay()
            rings[r][0].copy_(enc.d_pay, non_blocking=True)
            rings[r][1].copy_(enc.d_len, non_blocking=True)
        s.synchronize()
        hip.sync()
    for r in (2, 0):
        check(r, "replay")
    hip.close()


def test_the_host_buffer_call(oracle):
    case, pics, cap = _small(oracle)
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    for p in pics:
        f = cf.fill(p, case.q, cap)
        payload, qidx = hip.encode_picture_hq(p.raw, fmt, fillmode(cp, cap))
        assert payload == f.payload()
        assert (np.asarray(qidx).reshape(-1) == f.qmap.reshape(-1)).all()
    hip.close()


def test_stream_round_trip_and_decode_under_mode_4(oracle):
    """the stream of a filled batch is the plain HQ stream of its payloads: byte for byte what the calls write under HQ_CONSTQ,
    read back to the same slots; the decoder under mode 4 shows d_recon"""
    import vc2hip_py
    torch = _torch()
    case, pics, cap = _small(oracle)
    hip = _ctx()
    enc = Enc(hip, case, [p.raw for p in pics], recon=True)
    cp4 = fillmode(enc.cp, cap)
    enc.recon(cp4)
    pays = enc.payloads()
    check_payloads(enc, pics, case.q, cap, "stream")
    scap = (sum(len(p) for p in pays) + 3 * 64 + 64 + 255) // 256 * 256
    sp_w = vc2hip_py.stream_params(2, 0, 0, True)
    streams = []
    for cp in (cp4, constq(enc.cp, case.q)):
        d_stream = torch.full((scap,), FILL, dtype=torch.uint8, device=DEV)
        d_slen = torch.zeros(1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        hip.stream_write_dev(enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr(), 3, cp, sp_w, d_stream.data_ptr(), scap, d_slen.data_ptr())
        hip.sync()
        streams.append((d_stream, int(d_slen.cpu()[0])))
    assert streams[0][1] == streams[1][1] and torch.equal(streams[0][0], streams[1][0])
    d_stream, slen = streams[0]
    body = d_stream.cpu().numpy()[:slen].tobytes()
    assert body.count(b"BBCD") >= 4 and all(p in body for p in pays)
    d_pay2, d_len2 = torch.full_like(enc.d_pay, FILL), torch.full_like(enc.d_len, -1)
    torch.cuda.synchronize()
    hip.stream_read_dev(d_stream.data_ptr(), slen, 3, cp4, vc2hip_py.stream_params(2), d_pay2.data_ptr(), enc.stride, d_len2.data_ptr())
    hip.sync()
    pay2, len2 = d_pay2.cpu().numpy().reshape(3, enc.stride), d_len2.cpu().numpy()
    assert [pay2[k, :int(len2[k])].tobytes() for k in range(3)] == pays
    out = torch.full((3 * enc.rb + 16,), FILL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    hip.decode_batch_dev(enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr(), 3, enc.fmt, cp4, out.data_ptr())
    hip.sync()
    assert torch.equal(out, enc.d_rec), "the decoder's picture under mode 4"
    hip.close()


def test_the_old_modes_after_a_filled_call(oracle):
    """HQ_CAPPED and HQ_CONSTQ on the context of a filled call give their own bytes: nothing stays in the index buffer, the
    table or the cost buffer; and a filled call after them is still the definition's"""
    from test_gpu_cap import check_against_definition
    case, pics, cap = _small(oracle)
    raws = [p.raw for p in pics]
    hip = _ctx()
    first = Enc(hip, case, raws)
    check_payloads(first.encode(fillmode(first.cp, cap)), pics, case.q, cap, "filled")
    check_against_definition(Enc(hip, case, raws).encode(capped(first.cp, cap)), pics, case.q, cap, "HQ_CAPPED after")
    q = next(q for q in range(case.q, cr.Q_TOP + 1) if all(p.table[q] is not cr.NOT_CODABLE for p in pics))  # (scalar 1: the noise)
    assert Enc(hip, case, raws).encode(constq(first.cp, q)).payloads() == [p.payload(q) for p in pics]
    check_payloads(Enc(hip, case, raws).encode(fillmode(first.cp, cap)), pics, case.q, cap, "filled again")
    hip.close()


def test_a_picture_not_codable_at_the_floor(oracle):
    """row 1: the noise picture is not codable near the floor.  Under a cap everything codable meets it gets the smallest
    codable index, and every slice that codes one index below it is promoted; trying raises nothing"""
    case, pics = cf.batch(oracle, 1)
    assert pics[1].table[case.q] is cr.NOT_CODABLE
    big = max(p.table[cr.Q_TOP] for p in pics) + (1 << 30)
    for flags in ((), ("CAP_GENERAL",)):
        hip = _ctx(*flags)
        enc = Enc(hip, case, [p.raw for p in pics])
        fills = check_payloads(enc.encode(fillmode(enc.cp, big)), pics, case.q, big, "a cap everything codable meets")
        f = fills[1]
        assert f.filled and f.q_i > case.q and None in f.len_below
        assert len(f.promoted) == f.ns - f.len_below.count(None) > 0
        hip.close()


def test_refusals_launch_nothing_and_touch_nothing(oracle):
    from vc2hip_py import Vc2HipError
    case, pics, cap = _small(oracle)
    hip = _ctx()
    raws = [p.raw for p in pics]
    good = Enc(hip, case, raws).encode(fillmode(case.fmt_cp(hip.lib)[1], cap))
    before = hip.dwt_launches()
    enc = Enc(hip, case, raws)
    tries = {"index 116": fillmode(enc.cp, cap, 116), "index -1": fillmode(enc.cp, cap, -1), "cap 0": fillmode(enc.cp, 0),
             "cap -5": fillmode(enc.cp, -5)}
    for what, cp in tries.items():
        with pytest.raises(Vc2HipError) as e:
            hip.encode_batch_dev(enc.d_raw.data_ptr(), 3, enc.fmt, cp, enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr())
        assert e.value.code == EINVAL, (what, e.value.code)
        hip.sync()
        assert enc.untouched() and hip.dwt_launches() == before, what
    again = Enc(hip, case, raws).encode(fillmode(enc.cp, cap))
    assert _torch().equal(good.d_pay, again.d_pay)
    hip.close()


@pytest.mark.parametrize("i", [SMALL, cf.NEW], ids=lambda i: cf.IDS[i])
def test_nothing_is_written_outside_the_outputs(oracle, i):
    """guards behind the n payload slots, d_lens, d_qidx, d_sse and d_recon keep their bytes"""
    torch = _torch()
    case, pics = cf.batch(oracle, i)
    cap = mixed_cap(pics, case.q, cf.caps(case, pics[0]))
    hip = _ctx()
    enc = Enc(hip, case, [p.raw for p in pics], recon=True)
    guard = 4096
    enc.d_pay = torch.full((3 * enc.stride + guard,), FILL, dtype=torch.uint8, device=DEV)
    enc.d_len = torch.full((3 + guard,), -1, dtype=torch.int64, device=DEV)
    enc.d_q = torch.full((3 * enc.ns + guard,), -1, dtype=torch.int32, device=DEV)
    enc.d_sse = torch.full((9 + guard,), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    enc.recon(fillmode(enc.cp, cap))
    assert (enc.d_pay[3 * enc.stride:] == FILL).all() and (enc.d_len[3:] == -1).all()
    assert (enc.d_q[3 * enc.ns:] == -1).all() and (enc.d_sse[9:] == -1).all()
    lens = enc.d_len[:3].cpu().numpy()
    pay = enc.d_pay[:3 * enc.stride].cpu().numpy().reshape(3, enc.stride)
    for k, f in enumerate(cf.fill(p, case.q, cap) for p in pics):
        assert int(lens[k]) == len(f.payload()) and pay[k, :int(lens[k])].tobytes() == f.payload(), k
        assert (enc.d_q[k * enc.ns:(k + 1) * enc.ns].cpu().numpy() == f.qmap.reshape(-1)).all(), k
    assert (enc.d_rec[3 * enc.rb:] == FILL).all()
    hip.close()
