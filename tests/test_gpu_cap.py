"""GPU tests of VC2HIP_HQ_CAPPED (include/vc2hip.h): every payload, length and index against the CPU
definition tests/cap_ref.py, which stands on the oracle's quantiser and slice coder.  The caps come from picture 0's own
table of lengths at run time (cap_ref.caps)."""
import numpy as np
import pytest

import cap_ref as cr
import layout_ref as lr
import proxy_ref as pr
from test_gpu_fields import _fields

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5
EINVAL = -1
VARIANTS = {"default": (), "store32": ("STORE32",), "general": ("CAP_GENERAL",), "onepass": ("SINGLE_PASS_VBR",), "twopass": ("TWO_PASS_VBR",)}
CAPS = ("floor", "mid", "mid-1", "empty", "none")


def _torch():
    import torch
    return torch


def _ctx(*flags, stream=None):
    from vc2hip_py import FLAGS, Vc2Hip
    return Vc2Hip(stream=stream, flags=sum(FLAGS[f] for f in flags))


@pytest.fixture(scope="module")
def variants():
    out = {name: _ctx(*flags) for name, flags in VARIANTS.items()}
    yield out
    for hip in out.values():
        hip.close()


def capped(cp, cap, floor=None):
    """cp with mode = VC2HIP_HQ_CAPPED, the cap and (optionally) another floor"""
    out = type(cp).from_buffer_copy(cp)
    out.mode, out.compressed_bytes = cr.MODE, cap
    if floor is not None:
        out.q_index = floor
    return out


def constq(cp, q):
    out = type(cp).from_buffer_copy(cp)
    out.mode, out.q_index, out.compressed_bytes = 0, q, 0
    return out


def slice_indices(pay, ns, prefix, scalar):
    """the index byte of every slice header, by a walk over the length bytes"""
    pos, out = 0, []
    for _ in range(ns):
        pos += prefix
        out.append(pay[pos])
        pos += 1
        for _ in range(3):
            pos += 1 + pay[pos] * scalar
    assert pos == len(pay)
    return out


class Enc:
    """one batch on the device, every output pre-filled"""

    def __init__(self, hip, case, raws, recon=False):
        torch = _torch()
        self.torch, self.hip, self.case, self.n = torch, hip, case, len(raws)
        self.fmt, self.cp = case.fmt_cp(hip.lib)
        self.rb, self.ns = case.raw_bytes(), case.ys * case.xs
        assert self.rb % 16 == 0
        self.d_raw = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(DEV)
        self.stride = (hip.max_payload_bytes(self.fmt, self.cp) + 64 + 255) // 256 * 256
        self.d_pay = torch.full((self.n * self.stride,), FILL, dtype=torch.uint8, device=DEV)
        self.d_len = torch.full((self.n,), -1, dtype=torch.int64, device=DEV)
        if recon:
            self.d_rec = torch.full((self.n * self.rb + 16,), FILL, dtype=torch.uint8, device=DEV)
            self.d_sse = torch.full((self.n * 3,), -1, dtype=torch.int64, device=DEV)
            self.d_q = torch.full((self.n * self.ns,), -1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()

    def encode(self, cp):
        self.hip.encode_batch_dev(self.d_raw.data_ptr(), self.n, self.fmt, cp, self.d_pay.data_ptr(), self.stride, self.d_len.data_ptr())
        self.hip.sync()
        return self

    def recon(self, cp, payload=True):
        self.hip.encode_recon_batch_dev(self.d_raw.data_ptr(), self.n, self.fmt, cp, self.d_pay.data_ptr() if payload else None,
                                        self.stride if payload else 0, self.d_len.data_ptr() if payload else None,
                                        self.d_rec.data_ptr(), self.d_sse.data_ptr(), self.d_q.data_ptr())
        self.hip.sync()
        return self

    def payloads(self):
        pay, lens = self.d_pay.cpu().numpy().reshape(self.n, self.stride), self.d_len.cpu().numpy()
        return [pay[i, :int(lens[i])].tobytes() for i in range(self.n)]

    def untouched(self):
        return bool((self.d_pay == FILL).all() and (self.d_len == -1).all())


def check_against_definition(enc, pics, floor, cap, tag):
    """payload bytes, lengths and every slice header's index byte of a capped call; returns the indices"""
    case, got = enc.case, enc.payloads()
    want_q = [p.chosen(floor, cap) for p in pics]
    for i, (p, q) in enumerate(zip(pics, want_q)):
        want = p.payload(q)
        assert want is not cr.NOT_CODABLE, (tag, i, q, "the definition's index must be codable in this matrix")
        assert len(got[i]) == len(want), (tag, i, "length", len(got[i]), len(want), "index", q)
        assert slice_indices(got[i], enc.ns, case.prefix, case.scalar) == [q] * enc.ns, (tag, i, "indices", q)
        assert got[i] == want, (tag, i, "payload")
        assert (len(got[i]) <= cap) == p.fits(q, cap), (tag, i)
    return want_q


@pytest.mark.parametrize("i", range(len(cr.MATRIX)), ids=cr.IDS)
def test_matrix(variants, oracle, i):
    """every row and cap on every context variant"""
    case, pics = cr.batch(oracle, i)
    caps = cr.caps(case, pics[0])
    raws = [p.raw for p in pics]
    for name, hip in variants.items():
        hip.profile_enable(True)
        hip.profile_reset()
        for cname in CAPS:
            cap, want0 = caps[cname]
            enc = Enc(hip, case, raws)
            qs = check_against_definition(enc.encode(capped(enc.cp, cap)), pics, case.q, cap, (name, cname))
            assert qs[0] == want0, (name, cname, qs)
            if cname == "mid":
                assert len(set(qs)) >= 2, (name, qs)
            if cname == "none":
                assert qs == [cr.Q_TOP] * 3 and all(len(p) > cap for p in enc.payloads())
        prof = hip.profile()
        hip.profile_enable(False)
        # the row takes the path its comment in cap_ref.MATRIX names: the fast form is two launches per round (the register
        # kernel, then the general one over the slices it handed back), the general form one
        fast = i in cr.FAST and name in ("default", "onepass", "twopass")
        assert prof["cap_measure1"][0] == prof["cap_measure2"][0] == len(CAPS) * (2 if fast else 1), (name, prof)
        assert prof["cap_pick"][0] == 2 * len(CAPS), (name, prof)
        if i == cr.WHOLE_PLANE:
            assert any("plane" in x for x in prof), (name, sorted(prof))


@pytest.mark.parametrize("i", [0, 2, cr.ESCAPES], ids=lambda i: cr.IDS[i])
def test_recon_with_and_without_a_payload(variants, oracle, i):
    """d_qidx = q_i in every slice, d_recon and d_sse those of the ConstQ call at q_i on that picture alone, and the decoder
    shows d_recon for the capped payload under mode 3"""
    torch = _torch()
    case, pics = cr.batch(oracle, i)
    cap = cr.caps(case, pics[0])["mid"][0]
    raws = [p.raw for p in pics]
    want_q = [p.chosen(case.q, cap) for p in pics]
    for name in ("default", "general"):
        hip = variants[name]
        alone = []
        for p, q in zip(pics, want_q):
            one = Enc(hip, case, [p.raw], recon=True)
            one.recon(constq(one.cp, q))
            assert one.payloads()[0] == p.payload(q)
            alone.append(one)
        for payload in (True, False):
            enc = Enc(hip, case, raws, recon=True)
            enc.recon(capped(enc.cp, cap), payload)
            q = enc.d_q.cpu().numpy().reshape(3, enc.ns)
            for k in range(3):
                assert (q[k] == want_q[k]).all(), (name, payload, k, q[k], want_q[k])
                assert torch.equal(enc.d_rec[k * enc.rb:(k + 1) * enc.rb], alone[k].d_rec[:enc.rb]), (name, payload, k, "picture")
                assert torch.equal(enc.d_sse[3 * k:3 * k + 3], alone[k].d_sse), (name, payload, k, "sums")
            assert (enc.d_rec[3 * enc.rb:] == FILL).all()
            if payload:
                check_against_definition(enc, pics, case.q, cap, (name, "recon"))
                out = torch.full((3 * enc.rb + 16,), FILL, dtype=torch.uint8, device=DEV)
                torch.cuda.synchronize()
                hip.decode_batch_dev(enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr(), 3, enc.fmt, capped(enc.cp, cap), out.data_ptr())
                hip.sync()
                assert torch.equal(out, enc.d_rec), (name, "the decoder's picture")
            else:
                assert enc.untouched()


def test_set_streams_gives_identical_bytes(oracle):
    torch = _torch()
    case, pics = cr.batch(oracle, 0)
    cap = cr.caps(case, pics[0])["mid"][0]
    raws = [p.raw for p in pics]
    hip = _ctx()
    one = Enc(hip, case, raws).encode(capped(pics[0].case.fmt_cp(hip.lib)[1], cap))
    check_against_definition(one, pics, case.q, cap, "one stream")
    hip.set_streams(2)
    two = Enc(hip, case, raws).encode(capped(one.cp, cap))
    assert torch.equal(one.d_pay, two.d_pay) and torch.equal(one.d_len, two.d_len)
    hip.set_streams(1)
    hip.close()


def test_fields(oracle):
    """interlaced frames: the cap is per field, and the fields' payloads are those of the capped encode of the split fields"""
    import vc2hip_py
    torch = _torch()
    from synth import noise_frame, synth
    c = dict(w=512, h=128, cf="422", bits=10)
    case = pr.Case(oracle, 512, 64, "422", 10, "DD97", 3, 1, 2, q=3, scalar=1)          # cap_ref.MATRIX[2]: a field
    frames = synth(512, 128, "422", 10, 91) + noise_frame(512, 128, "422", 10, 92)
    fields = _fields(frames, c, 2)
    fb = case.raw_bytes()
    pics = [cr.Picture(oracle, case, fields[k * fb:(k + 1) * fb]) for k in range(4)]
    cap = cr.caps(case, pics[0])["mid"][0]
    hip = _ctx()
    split = Enc(hip, case, [p.raw for p in pics]).encode(capped(case.fmt_cp(hip.lib)[1], cap))
    qs = check_against_definition(split, pics, case.q, cap, "split fields")
    assert len(set(qs)) >= 2, qs
    ffmt = vc2hip_py.picture_format(512, 128, "422", 10)
    d_frames = torch.frombuffer(bytearray(frames), dtype=torch.uint8).to(DEV)
    d_pay, d_len = torch.full_like(split.d_pay, FILL), torch.full_like(split.d_len, -1)
    torch.cuda.synchronize()
    hip.encode_fields_batch_dev(d_frames.data_ptr(), 2, ffmt, True, capped(split.cp, cap), d_pay.data_ptr(), split.stride, d_len.data_ptr())
    hip.sync()
    assert torch.equal(d_len, split.d_len) and torch.equal(d_pay, split.d_pay)
    hip.close()


def test_a_little_endian_lsb_justified_layout_gives_the_same_payload(oracle):
    import vc2hip_py
    torch = _torch()
    case, pics = cr.batch(oracle, 0)
    cap = cr.caps(case, pics[0])["mid"][0]
    hip = _ctx()
    enc = Enc(hip, case, [p.raw for p in pics])
    layout = vc2hip_py.sample_layout(little_endian=True, lsb_justified=True)
    buf = lr.to_layout(b"".join(p.raw for p in pics), enc.fmt, 3, layout)
    enc.d_raw = torch.frombuffer(bytearray(np.asarray(buf, np.uint8).tobytes()), dtype=torch.uint8).to(DEV)
    torch.cuda.synchronize()
    hip.set_sample_layout(layout)
    check_against_definition(enc.encode(capped(enc.cp, cap)), pics, case.q, cap, "layout")
    hip.close()


@pytest.mark.parametrize("i", [0, 2], ids=lambda i: cr.IDS[i])
def test_on_a_callers_stream_and_under_capture(oracle, i):
    """a warm-up, then: the call returns while a filler still runs in front of it (no wait); captured once and replayed on two
    other inputs, every replay gives each picture its own index"""
    from test_gpu_caller_stream import Filler, _capture
    torch = _torch()
    case, pics = cr.batch(oracle, i)
    cap = cr.caps(case, pics[0])["mid"][0]
    orders = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    s = torch.cuda.Stream()
    hip = _ctx(stream=s.cuda_stream)
    with torch.cuda.stream(s):
        enc = Enc(hip, case, [pics[k].raw for k in orders[0]])
        cp = capped(enc.cp, cap)
        inputs = [torch.frombuffer(bytearray(b"".join(pics[k].raw for k in o)), dtype=torch.uint8).pin_memory() for o in orders]
        rings = [(torch.empty_like(enc.d_pay, device="cpu").pin_memory(), torch.empty_like(enc.d_len, device="cpu").pin_memory()) for _ in orders]

        def call():
            hip.encode_batch_dev(enc.d_raw.data_ptr(), 3, enc.fmt, cp, enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr())

        def check(r, tag):
            enc2 = Enc.__new__(Enc)
            enc2.__dict__.update(enc.__dict__)
            enc2.d_pay, enc2.d_len = rings[r]
            check_against_definition(enc2, [pics[k] for k in orders[r]], case.q, cap, (tag, r))

        call()                                  # the warm-up
        s.synchronize()
        hip.sync()
        # never waits
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
    case, pics = cr.batch(oracle, 0)
    cap = cr.caps(case, pics[0])["mid"][0]
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    for p in pics[:2]:
        q = p.chosen(case.q, cap)
        payload, qidx = hip.encode_picture_hq(p.raw, fmt, capped(cp, cap))
        assert payload == p.payload(q)
        assert (np.asarray(qidx) == q).all()
    hip.close()


def test_stream_write_and_read_round_trip_under_mode_3(oracle):
    """the stream of a capped batch is the plain HQ stream of its payloads: byte for byte what the calls write under
    HQ_CONSTQ, and read back to the same slots"""
    import vc2hip_py
    torch = _torch()
    case, pics = cr.batch(oracle, 2)
    cap = cr.caps(case, pics[0])["mid"][0]
    hip = _ctx()
    enc = Enc(hip, case, [p.raw for p in pics])
    cp3 = capped(enc.cp, cap)
    enc.encode(cp3)
    pays = enc.payloads()
    scap = (sum(len(p) for p in pays) + 3 * 64 + 64 + 255) // 256 * 256
    sp_w = vc2hip_py.stream_params(2, 0, 0, True)
    streams = []
    for cp in (cp3, constq(enc.cp, case.q)):
        d_stream = torch.full((scap,), FILL, dtype=torch.uint8, device=DEV)
        d_slen = torch.zeros(1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        hip.stream_write_dev(enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr(), 3, cp, sp_w, d_stream.data_ptr(), scap, d_slen.data_ptr())
        hip.sync()
        streams.append((d_stream, int(d_slen.cpu()[0])))
    assert streams[0][1] == streams[1][1] and torch.equal(streams[0][0], streams[1][0])
    d_stream, slen = streams[0]
    body = d_stream.cpu().numpy()[:slen].tobytes()
    assert body.count(b"BBCD") >= 4 and all(p in body for p in pays)   # three pictures and the end of sequence
    d_pay2, d_len2 = torch.full_like(enc.d_pay, FILL), torch.full_like(enc.d_len, -1)
    torch.cuda.synchronize()
    hip.stream_read_dev(d_stream.data_ptr(), slen, 3, cp3, vc2hip_py.stream_params(2), d_pay2.data_ptr(), enc.stride, d_len2.data_ptr())
    hip.sync()
    pay2, len2 = d_pay2.cpu().numpy().reshape(3, enc.stride), d_len2.cpu().numpy()
    assert [pay2[k, :int(len2[k])].tobytes() for k in range(3)] == pays
    hip.close()


def test_a_cap_nothing_meets_is_no_error(oracle):
    case, pics = cr.batch(oracle, 1)
    hip = _ctx()
    enc = Enc(hip, case, [p.raw for p in pics])
    enc.encode(capped(enc.cp, 1))               # (vc2hip_sync inside raises on any device-side error)
    got = enc.payloads()
    for p, g in zip(pics, got):
        assert g == p.payload(cr.Q_TOP) and len(g) > 1
        assert slice_indices(g, enc.ns, case.prefix, case.scalar) == [cr.Q_TOP] * enc.ns
    hip.close()


def test_constq_after_a_capped_call_and_trials_raise_nothing(oracle):
    """row 1: the noise picture is not codable near the floor (VC2HIP_ESCALAR under HQ_CONSTQ there) -- the capped call tries
    those indices and raises nothing; a ConstQ call on the same context afterwards gives the oracle's bytes: nothing stays in
    the index buffer or the table"""
    from vc2hip_py import Vc2HipError
    case, pics = cr.batch(oracle, 1)
    assert pics[1].table[case.q] is cr.NOT_CODABLE
    big = max(p.table[cr.Q_TOP] for p in pics) + (1 << 30)
    for flags in ((), ("CAP_GENERAL",)):
        hip = _ctx(*flags)
        enc = Enc(hip, case, [p.raw for p in pics])
        qs = check_against_definition(enc.encode(capped(enc.cp, big)), pics, case.q, big, "a cap everything codable meets")
        assert qs[0] == case.q and qs[1] > case.q            # the smallest CODABLE index, not the floor
        q = 40
        again = Enc(hip, case, [p.raw for p in pics]).encode(constq(enc.cp, q))
        assert again.payloads() == [p.payload(q) for p in pics]
        bad = Enc(hip, case, [p.raw for p in pics])
        with pytest.raises(Vc2HipError) as e:
            bad.encode(constq(enc.cp, case.q))               # what the capped call's trial met, as an encode
        assert e.value.code == -3
        check_against_definition(Enc(hip, case, [p.raw for p in pics]).encode(capped(enc.cp, big)), pics, case.q, big, "after the error")
        hip.close()


def test_refusals_launch_nothing_and_touch_nothing(oracle):
    from vc2hip_py import Vc2HipError
    case, pics = cr.batch(oracle, 0)
    hip = _ctx()
    good = Enc(hip, case, [p.raw for p in pics]).encode(capped(case.fmt_cp(hip.lib)[1], 100000))
    before = hip.dwt_launches()
    enc = Enc(hip, case, [p.raw for p in pics])
    tries = {"index 116": capped(enc.cp, 100000, 116), "index -1": capped(enc.cp, 100000, -1), "cap 0": capped(enc.cp, 0),
             "cap -5": capped(enc.cp, -5)}
    bad_scalar = capped(enc.cp, 100000)
    bad_scalar.scalar = 0
    tries["scalar 0"] = bad_scalar
    for what, cp in tries.items():
        with pytest.raises(Vc2HipError) as e:
            hip.encode_batch_dev(enc.d_raw.data_ptr(), 3, enc.fmt, cp, enc.d_pay.data_ptr(), enc.stride, enc.d_len.data_ptr())
        assert e.value.code == EINVAL, (what, e.value.code)
        hip.sync()
        assert enc.untouched() and hip.dwt_launches() == before, what
    ok = Enc(hip, case, [p.raw for p in pics]).encode(capped(enc.cp, 100000, 115))   # the top index is allowed
    assert all(slice_indices(p, enc.ns, case.prefix, case.scalar) == [115] * enc.ns for p in ok.payloads())
    again = Enc(hip, case, [p.raw for p in pics]).encode(capped(enc.cp, 100000))
    assert _torch().equal(good.d_pay, again.d_pay)
    hip.close()
