"""GPU tests of vc2hip_encode_recon_batch_dev (the encode, the decoder's picture, the squared error, the indices): every
comparison byte for byte against the CPU definition tests/recon_ref.py, which stands on the oracle's encoder and decoder."""
import hashlib
import json
import os

import numpy as np
import pytest

import proxy_ref as pr
import recon_ref as rr
from synth import noise_frame, synth, synth_fast
from test_gpu_reduced import VARIANTS as REDUCED_VARIANTS

pytestmark = pytest.mark.gpu

VARIANTS = dict(REDUCED_VARIANTS, onepass=("SINGLE_PASS_VBR",))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_digests.json")))
COMBOS = ("all", "recon", "payload")   # everything; d_recon + d_sse only; payload + d_qidx only
CODER = ("hq_pack", "slice_offsets_scan", "slice_compact", "ld_pack")
DECODER = ("slice_index_", "hq_unpack", "ld_unpack")
FILL = 0xA5


def _ctx(*flags):
    from vc2hip_py import FLAGS, Vc2Hip
    return Vc2Hip(flags=sum(FLAGS[f] for f in flags))


@pytest.fixture(scope="module")
def variants():
    out = {name: _ctx(*flags) for name, flags in VARIANTS.items()}
    for hip in out.values():
        hip.profile_enable(True)
    return out


class Call:
    """one call's buffers: the input on the device, every output pre-filled"""

    def __init__(self, hip, case, raw, n, combo="all"):
        import torch
        self.torch, self.hip, self.case, self.n, self.combo = torch, hip, case, n, combo
        self.fmt, self.cp = case.fmt_cp(hip.lib)
        self.rb, self.ns = case.raw_bytes(), case.ys * case.xs
        assert len(raw) % self.rb == 0
        pics = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(-1, self.rb)
        self.d_raw = pics[torch.arange(n) % pics.shape[0]].reshape(-1).contiguous().to("cuda:0")
        self.stride = (hip.max_payload_bytes(self.fmt, self.cp) + 64 + 255) // 256 * 256
        dev = "cuda:0"
        self.d_pay = torch.full((n * self.stride,), FILL, dtype=torch.uint8, device=dev)
        self.d_len = torch.full((n,), -1, dtype=torch.int64, device=dev)
        self.d_rec = torch.full((n * self.rb + 16,), FILL, dtype=torch.uint8, device=dev)
        self.d_sse = torch.full((n * 3,), -1, dtype=torch.int64, device=dev)
        self.d_q = torch.full((n * self.ns,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()   # (torch fills on its stream, the library works on its own)

    def args(self):
        pay = self.combo in ("all", "payload")
        rec = self.combo in ("all", "recon")
        return dict(d_payload=self.d_pay.data_ptr() if pay else None, stride=self.stride if pay else 0,
                    d_lens=self.d_len.data_ptr() if pay else None, d_recon=self.d_rec.data_ptr() if rec else None,
                    d_sse=self.d_sse.data_ptr() if rec else None, d_qidx=self.d_q.data_ptr() if self.combo != "recon" else None)

    def run(self):
        self.hip.encode_recon_batch_dev(self.d_raw.data_ptr(), self.n, self.fmt, self.cp, **self.args())
        self.hip.sync()
        return self

    def untouched(self):
        return bool((self.d_pay == FILL).all() and (self.d_len == -1).all() and (self.d_rec == FILL).all() and (self.d_sse == -1).all()
                    and (self.d_q == -1).all())

    def check(self, want, tag):
        """want: recon_ref.recon's list, cycled over the n pictures"""
        pay, lens = self.d_pay.cpu().numpy().reshape(self.n, self.stride), self.d_len.cpu().numpy()
        rec = self.d_rec.cpu().numpy()[:self.n * self.rb].reshape(self.n, self.rb)
        sse, q = self.d_sse.cpu().numpy().reshape(self.n, 3), self.d_q.cpu().numpy().reshape(self.n, self.ns)
        for i in range(self.n):
            w_pay, w_pic, w_sse, w_q = want[i % len(want)]
            if self.combo in ("all", "payload"):
                assert int(lens[i]) == len(w_pay), (tag, i, int(lens[i]), len(w_pay))
                assert pay[i, :len(w_pay)].tobytes() == w_pay, (tag, i, "payload")
                assert np.array_equal(q[i], w_q.reshape(-1)), (tag, i, "indices")
            else:
                assert (pay[i] == FILL).all() and lens[i] == -1 and (q[i] == -1).all(), (tag, i, "outputs not asked for were written")
            if self.combo in ("all", "recon"):
                assert rec[i].tobytes() == w_pic, (tag, i, "picture")
                assert [int(x) for x in sse[i].astype(np.uint64)] == w_sse, (tag, i, "sums", sse[i], w_sse)
            else:
                assert (rec[i] == FILL).all() and (sse[i] == -1).all(), (tag, i, "outputs not asked for were written")
        assert (self.d_rec[self.n * self.rb:] == FILL).all(), (tag, "wrote past the pictures")


def _profile_facts(hip, combo, tag):
    names = set(hip.profile())
    hip.profile_reset()
    assert not [x for x in names if x.startswith(DECODER)], (tag, names)   # the call never decodes its own payload
    if combo == "recon":
        assert not [x for x in names if x in CODER], (tag, names)          # and without a payload it runs no slice coder
    if combo != "payload":
        assert "squared_error" in names, (tag, names)
    return names


@pytest.mark.parametrize("i", range(len(rr.MATRIX)), ids=lambda i: "-".join(str(x) for x in rr.MATRIX[i][:9]) + "-" + rr.MATRIX[i][9].get("mode", "HQ_ConstQ"))
def test_matrix(variants, oracle, i):
    row = rr.MATRIX[i]
    case = rr.matrix_case(oracle, row)
    raw = rr.matrix_raw(case, row)
    want = rr.recon(oracle, case, raw, 2)
    seen = set()
    for name, hip in variants.items():
        hip.profile_reset()
        for combo in COMBOS:
            Call(hip, case, raw, 2, combo).run().check(want, (name, combo))
            seen |= _profile_facts(hip, combo, (name, combo))
            if combo != "payload":
                rec = hip.dwt_launches()
                k = next(j for j, r in enumerate(rec) if r["inverse"])
                assert k > 0 and all(not r["inverse"] for r in rec[:k]) and all(r["inverse"] for r in rec[k:]), (name, rec)
    if case.mode != "LD":
        assert "requantise" in seen, seen


@pytest.mark.parametrize("mode", ["HQ_ConstQ", "HQ_CBR", "LD"])
def test_distinct_pictures_keep_their_sums(oracle, mode):
    """five distinct pictures, some of them lossless: no sum leaks into a neighbour's"""
    kw = dict(q=14, scalar=2, prefix=1) if mode == "HQ_ConstQ" else dict(mode=mode, s=9000, scalar=1)
    case = pr.Case(oracle, 256, 64, "422", 10, "LeGall", 3, 1, 2, **kw)
    flat = bytes(case.raw_bytes())   # all-zero words: every mode codes it without loss
    raw = b"".join([synth(256, 64, "422", 10, 60), flat, noise_frame(256, 64, "422", 10, 61), flat, synth(256, 64, "422", 10, 62)])
    want = rr.recon(oracle, case, raw, 5)
    assert want[1][2] == [0, 0, 0] and want[3][2] == [0, 0, 0] and all(want[k][2][0] > 0 for k in (0, 2, 4))
    hip = _ctx()
    for combo in COMBOS:
        Call(hip, case, raw, 5, combo).run().check(want, (mode, combo))
    hip.close()


def test_small_pictures_beyond_the_one_pass_threshold_and_set_streams(oracle):
    """120 pictures per call (the one-pass coder's side of the threshold), then the same batch over 2 and 3 streams"""
    case = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=7, scalar=2)
    assert case.raw_bytes() % 16 == 0
    raw = synth(1024, 64, "422", 10, 21, frames=3)
    want = rr.recon(oracle, case, raw, 3)
    hip = _ctx()
    one = Call(hip, case, raw, 120).run()
    one.check(want, "one stream")
    for k in (2, 3):
        hip.set_streams(k)
        many = Call(hip, case, raw, 120).run()
        for a, b in ((one.d_pay, many.d_pay), (one.d_len, many.d_len), (one.d_rec, many.d_rec), (one.d_sse, many.d_sse), (one.d_q, many.d_q)):
            assert one.torch.equal(a, b), k
        for combo in ("recon", "payload"):
            Call(hip, case, raw, 7, combo).run().check(want, (k, combo))
    hip.set_streams(1)
    hip.close()


def test_alternating_with_the_other_batch_calls(oracle):
    """one context: this call between encode_batch_dev, decode_batch_dev and decode_reduced_batch_dev on other geometries;
    every result as on a fresh context"""
    import torch
    a = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=7, scalar=2)
    b = pr.Case(oracle, 512, 128, "420", 8, "LeGall", 2, 2, 4, mode="HQ_CBR", s=30000, scalar=1, word_bytes=1)
    c = pr.Case(oracle, 512, 64, "444", 10, "Haar1", 2, 2, 2, mode="LD", s=30000)
    raws = {x: synth(x.w, x.h, x.cf, x.bits, 90 + k, frames=2, word_bytes=x.word_bytes) for k, x in enumerate((a, b, c))}
    wants = {x: rr.recon(oracle, x, raws[x], 2) for x in (a, b, c)}
    hip = _ctx()

    def other(x, k=0):
        fmt, cp = x.fmt_cp(hip.lib)
        call = Call(hip, x, raws[x], 2)
        hip.encode_batch_dev(call.d_raw.data_ptr(), 2, fmt, cp, call.d_pay.data_ptr(), call.stride, call.d_len.data_ptr())
        out = torch.zeros(2 * x.raw_bytes(k) + 16, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        if k:
            hip.decode_reduced_batch_dev(call.d_pay.data_ptr(), call.stride, call.d_len.data_ptr(), 2, fmt, cp, k, out.data_ptr())
        else:
            hip.decode_batch_dev(call.d_pay.data_ptr(), call.stride, call.d_len.data_ptr(), 2, fmt, cp, out.data_ptr())
        hip.sync()
        got = out.cpu().numpy()[:2 * x.raw_bytes(k)].reshape(2, -1)
        for i in range(2):
            want = pr.reduced_picture(oracle, x, wants[x][i][0], k) if k else wants[x][i][1]
            assert got[i].tobytes() == want, (x.mode, k, i)
            assert call.d_pay.cpu().numpy().reshape(2, -1)[i, :len(wants[x][i][0])].tobytes() == wants[x][i][0]

    for rep in range(2):
        for x, y, k in ((a, b, 0), (b, c, 1), (c, a, 1), (a, c, 0), (b, a, 0)):
            for combo in COMBOS:
                Call(hip, x, raws[x], 2, combo).run().check(wants[x], (rep, x.mode, combo))
                other(y, k)
    hip.close()


def test_refusals_launch_nothing_and_touch_nothing(oracle):
    from vc2hip_py import Vc2HipError, picture_format
    case = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=7, scalar=2)
    raw = synth(1024, 64, "422", 10, 22, frames=2)
    hip = _ctx()
    good = Call(hip, case, raw, 2).run()
    before = hip.dwt_launches()
    base = Call(hip, case, raw, 2)
    A = base.args()
    none = dict(d_payload=None, stride=0, d_lens=None, d_recon=None, d_sse=None, d_qidx=None)
    fmt_c = picture_format(case.w, case.h, case.cf, case.bits, 2, chroma_bits=8)
    bad_mode = type(base.cp).from_buffer_copy(base.cp); bad_mode.mode = 7
    bad_kernel = type(base.cp).from_buffer_copy(base.cp); bad_kernel.kernel = 9
    bad_scalar = type(base.cp).from_buffer_copy(base.cp); bad_scalar.scalar = 0
    inside = base.d_raw.data_ptr() + 16 * ((base.rb // 2) // 16)
    tries = {
        "no output": (none, {}),
        "sums without a picture": (dict(none, d_sse=A["d_sse"]), {}),
        "payload without lengths": (dict(A, d_lens=None), {}),
        "payload without a stride": (dict(A, stride=0), {}),
        "stride without a payload": (dict(A, d_payload=None, d_lens=None), {}),
        "lengths alone": (dict(none, d_lens=A["d_lens"], d_qidx=A["d_qidx"]), {}),
        "picture inside the input": (dict(A, d_recon=inside), {}),
        "picture on the input": (dict(A, d_recon=base.d_raw.data_ptr()), {}),
        "misaligned picture": (dict(A, d_recon=A["d_recon"] + 8), {}),
        "misaligned payload": (dict(A, d_payload=A["d_payload"] + 8), {}),
        "misaligned stride": (dict(A, stride=A["stride"] + 8), {}),
        "misaligned lengths": (dict(A, d_lens=A["d_lens"] + 4), {}),
        "misaligned sums": (dict(A, d_sse=A["d_sse"] + 4), {}),
        "misaligned indices": (dict(A, d_qidx=A["d_qidx"] + 2), {}),
        "misaligned input": (A, dict(raw_off=8)),
        "chroma depth": (A, dict(fmt=fmt_c)),
        "mode": (A, dict(cp=bad_mode)),
        "wavelet": (A, dict(cp=bad_kernel)),
        "scalar": (A, dict(cp=bad_scalar)),
        "no pictures": (A, dict(n=0)),
    }
    for what, (args, over) in tries.items():
        with pytest.raises(Vc2HipError) as e:
            hip.encode_recon_batch_dev(base.d_raw.data_ptr() + over.get("raw_off", 0), over.get("n", 2), over.get("fmt", base.fmt),
                                       over.get("cp", base.cp), **args)
        assert e.value.code == -1, (what, e.value.code)   # VC2HIP_EINVAL
        hip.sync()
        assert base.untouched(), what
        assert hip.dwt_launches() == before, what
    # a chroma depth of its own is the encoder's business alone: without d_recon the call takes it
    ok = Call(hip, case, raw, 2, "payload")
    hip.encode_recon_batch_dev(ok.d_raw.data_ptr(), 2, fmt_c, ok.cp, **ok.args())
    hip.sync()
    # the context is usable afterwards
    again = Call(hip, case, raw, 2).run()
    assert good.torch.equal(good.d_rec, again.d_rec) and good.torch.equal(good.d_pay, again.d_pay) and good.torch.equal(good.d_sse, again.d_sse)
    hip.close()


def test_escalar_surfaces_with_and_without_a_payload(oracle):
    """noise at q = 0 with scalar 1: a component needs more than 255 bytes.  encode_batch_dev reports VC2HIP_ESCALAR at sync;
    so does this call, whether or not it was asked for a payload.  (Ordinary data the library refuses cleanly.)"""
    from vc2hip_py import Vc2HipError
    case = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=0, scalar=1)
    raw = noise_frame(1024, 64, "422", 10, 3)
    hip = _ctx()
    call = Call(hip, case, raw, 2)
    hip.encode_batch_dev(call.d_raw.data_ptr(), 2, call.fmt, call.cp, call.d_pay.data_ptr(), call.stride, call.d_len.data_ptr())
    with pytest.raises(Vc2HipError) as e:
        hip.sync()
    assert e.value.code == -3
    for combo in COMBOS + ("indices",):
        c2 = Call(hip, case, raw, 2, combo if combo != "indices" else "payload")
        args = c2.args() if combo != "indices" else dict(d_qidx=c2.d_q.data_ptr())
        hip.encode_recon_batch_dev(c2.d_raw.data_ptr(), 2, c2.fmt, c2.cp, **args)
        with pytest.raises(Vc2HipError) as e:
            hip.sync()
        assert e.value.code == -3, (combo, e.value.code)
    # and the context goes on
    ok = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=0, scalar=8)
    Call(hip, ok, raw, 1).run().check(rr.recon(oracle, ok, raw), "after the error")
    hip.close()


def _reference_case(oracle, cfg):
    p = GOLD[cfg]["params"]
    kw = {k: p[k] for k in ("mode", "q", "s", "scalar") if k in p}
    return pr.Case(oracle, p["width"], p["height"], p["cf"], p["bits"], p["kernel"], p["depth"], p["u"], p["a"], **kw), GOLD[cfg]["frames"]


@pytest.mark.parametrize("cfg", ["cfg1", "cfg2", "cfg3"])
def test_the_references_own_decoded_pictures(oracle, cfg):
    """the synthetic inputs of tests/synth.py: d_recon hashes to the digest of the reference's DecodeStream output, the
    payload is the reference stream's"""
    case, frames = _reference_case(oracle, cfg)
    raw = synth_fast(case.w, case.h, case.cf, case.bits, 1234, frames=frames)
    stream = oracle.encode_stream(case.params(), raw, frames)
    assert hashlib.sha256(stream).hexdigest() == GOLD[cfg]["stream"]["sha256"]
    hip = _ctx()
    for combo in ("all", "recon"):
        call = Call(hip, case, raw, frames, combo).run()
        rec = call.d_rec.cpu().numpy()[:frames * call.rb].tobytes()
        assert hashlib.sha256(rec).hexdigest() == GOLD[cfg]["decoded"]["sha256"], (cfg, combo)
    call = Call(hip, case, raw, frames, "payload").run()
    pay, lens = call.d_pay.cpu().numpy(), call.d_len.cpu().tolist()
    pos = len(stream) - 13
    for k in reversed(range(frames)):   # (as test_gpu_parity.py takes it: the payloads are the tails of the picture data units)
        assert stream[pos - lens[k]:pos] == pay[k * call.stride:k * call.stride + lens[k]].tobytes(), (cfg, k)
        pos = stream.rfind(b"BBCD", 0, pos - lens[k])
    hip.close()


def test_cfg2_sixteen_pictures_per_call(oracle):
    """cfg 2's two frames cycled to 16 per call: picture, digest and the sums against recon_ref"""
    case, frames = _reference_case(oracle, "cfg2")
    raw = synth_fast(case.w, case.h, case.cf, case.bits, 1234, frames=frames)
    rb = case.raw_bytes()
    dec, n = oracle.decode_stream(case.params(), oracle.encode_stream(case.params(), raw, frames), frames)
    assert n == frames and hashlib.sha256(dec).hexdigest() == GOLD["cfg2"]["decoded"]["sha256"]
    sums = [rr.squared_errors(case, raw[k * rb:(k + 1) * rb], dec[k * rb:(k + 1) * rb]) for k in range(frames)]
    hip = _ctx()
    for combo in ("all", "recon"):
        call = Call(hip, case, raw, 16, combo).run()
        rec = call.d_rec[:16 * rb].view(16, rb)
        sse = call.d_sse.cpu().numpy().reshape(16, 3)
        for k in range(frames):
            want = call.torch.frombuffer(bytearray(dec[k * rb:(k + 1) * rb]), dtype=call.torch.uint8).to("cuda:0")
            for j in range(k, 16, frames):
                assert call.torch.equal(rec[j], want), (combo, j)
                assert [int(x) for x in sse[j]] == sums[k], (combo, j)
    hip.close()
