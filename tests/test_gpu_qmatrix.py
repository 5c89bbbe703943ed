"""GPU tests of vc2hip_set_quant_matrix (include/vc2hip.h): every call that takes coding parameters
against the compositions of tests/qmatrix_ref.py, which hand the oracle's primitives the same matrix; the stream calls
against that module's header and stream models.  Where a composition itself refuses (the oracle raises), the call must refuse
with the same code at vc2hip_sync."""
import ctypes as C

import numpy as np
import pytest

import cap_ref as cr
import proxy_ref as pr
import qmatrix_ref as qr
import transcode_cbr_ref as tcr
import transcode_ref as tr
from vc2lib import OracleError

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5
EINVAL, ESYNTAX = -1, -12
VARIANTS = {"default": (), "store32": ("STORE32",), "records": ("NO_BANDPLANES",), "cbr_general": ("CBR_GENERAL",),
            "cap_general": ("CAP_GENERAL",), "onepass": ("SINGLE_PASS_VBR",), "bytes": ("PLANES8_ALWAYS",)}
ROWS = qr.ROWS   # A, G, E, C and one LD picture, with E and L again at budgets their searches meet under `edge`


def _torch():
    import torch
    return torch


def _ctx(*flags, stream=None):
    from vc2hip_py import FLAGS, Vc2Hip
    return Vc2Hip(stream=stream, flags=sum(FLAGS[f] for f in flags))


@pytest.fixture(scope="module")
def variants():
    v = {name: _ctx(*flags) for name, flags in VARIANTS.items()}
    yield v
    for h in v.values():
        h.close()


@pytest.fixture(scope="module")
def hip(variants):
    return variants["default"]


def _dev(b):
    torch = _torch()
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


case_of = qr.case_of


def _try(fn):
    """a composition's result, or the OracleError it refuses with (returned)"""
    try:
        return fn()
    except OracleError as e:
        return e


_REF = {}


def ref(oracle, name, mname):
    """the compositions of one row under one matrix, once per session: per picture the payload, indices and decoded picture"""
    key = (name, mname)
    if key not in _REF:
        case = case_of(oracle, name)
        qm = qr.matrix(oracle, mname, case.kernel, case.depth)
        raws = cr.pictures(case)
        enc = [_try(lambda r=r: qr.encode(oracle, case, r, qm)) for r in raws]
        dec = [None if isinstance(e, OracleError) else qr.decode(oracle, case, e[0], qm) for e in enc]
        # checked here on the CPU: the composition refuses where it is meant to (every picture, that code) and nowhere else
        codes = {e.code if isinstance(e, OracleError) else None for e in enc}
        assert codes == {qr.REFUSES.get(key)}, (key, "the composition's refusals are not the expected ones", codes)
        _REF[key] = dict(case=case, qm=qm, raws=raws, enc=enc, dec=dec)
    return _REF[key]


def _refusal(items):
    return next((e.code for e in items if isinstance(e, OracleError)), None)


def _sync_expect(hip, code, tag):
    import vc2hip_py
    if code is None:
        hip.sync()
        return True
    with pytest.raises(vc2hip_py.Vc2HipError) as e:
        hip.sync()
    assert e.value.code == code, (tag, str(e.value))
    return False


class Batch:
    """n pictures on the device, payload slots and lengths pre-filled"""

    def __init__(self, hip, fmt, cp, raws, stride=None):
        torch = _torch()
        self.hip, self.fmt, self.cp, self.n = hip, fmt, cp, len(raws)
        self.rb = len(raws[0])
        self.d_raw = _dev(b"".join(raws) + bytes(64))
        self.stride = stride or (hip.max_payload_bytes(fmt, cp) + 64 + 255) // 256 * 256
        self.d_pay = torch.full((self.n * self.stride,), FILL, dtype=torch.uint8, device=DEV)
        self.d_len = torch.full((self.n,), -1, dtype=torch.int64, device=DEV)
        self.d_out = torch.full((self.n * self.rb + 64,), FILL, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()

    def encode(self, hip=None):
        (hip or self.hip).encode_batch_dev(self.d_raw.data_ptr(), self.n, self.fmt, self.cp, self.d_pay.data_ptr(), self.stride, self.d_len.data_ptr())

    def decode(self, hip=None):
        (hip or self.hip).decode_batch_dev(self.d_pay.data_ptr(), self.stride, self.d_len.data_ptr(), self.n, self.fmt, self.cp, self.d_out.data_ptr())

    def load(self, payloads):
        torch = _torch()
        slots = np.full((self.n, self.stride), FILL, np.uint8)
        for i, p in enumerate(payloads):
            slots[i, :len(p)] = np.frombuffer(p, np.uint8)
        self.d_pay.copy_(torch.from_numpy(slots.reshape(-1)))
        self.d_len.copy_(torch.tensor([len(p) for p in payloads], dtype=torch.int64))
        torch.cuda.synchronize()

    def payloads(self):
        lens = self.d_len.cpu().tolist()
        pay = self.d_pay.cpu().numpy().reshape(self.n, self.stride)
        return [pay[i, :max(int(lens[i]), 0)].tobytes() for i in range(self.n)]

    def pictures(self, rb=None):
        rb = rb or self.rb
        out = self.d_out.cpu().numpy()
        return [out[i * rb:(i + 1) * rb].tobytes() for i in range(self.n)]

    def untouched(self):
        return bool((self.d_pay == FILL).all() and (self.d_len == -1).all() and (self.d_out == FILL).all())


def _cp(hip, case, **over):
    import vc2hip_py
    fmt = vc2hip_py.picture_format(case.w, case.h, case.cf, case.bits, case.word_bytes)
    kw = dict(mode=case.mode, q=case.q, s=case.s, prefix=case.prefix, scalar=case.scalar)
    kw.update(over)
    return fmt, vc2hip_py.coding_params(hip.lib, fmt, case.kernel, case.depth, case.u, case.a, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# every covered call is the composition, under every context variant
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mname", qr.MATRICES)
@pytest.mark.parametrize("name", list(ROWS))
def test_encode_and_decode_batches(variants, oracle, name, mname):
    r = ref(oracle, name, mname)
    case, code = r["case"], _refusal(r["enc"])
    for vname, hip in variants.items():
        tag = (name, mname, vname)
        fmt, cp = _cp(hip, case)
        hip.set_quant_matrix(r["qm"])
        assert hip.quant_matrix().tolist() == r["qm"].tolist()
        b = Batch(hip, fmt, cp, r["raws"])
        b.encode()
        ok = _sync_expect(hip, code, tag)
        if ok:
            assert b.payloads() == [e[0] for e in r["enc"]], (tag, "payload")
            b.decode()
            hip.sync()
            assert b.pictures() == r["dec"], (tag, "decode")
        hip.set_quant_matrix(None)
        assert hip.quant_matrix().size == 0


@pytest.mark.parametrize("mname", qr.MATRICES)
def test_capped_recon_reduced_and_fields(variants, oracle, mname):
    """row A: HQ_CAPPED, vc2hip_encode_recon_batch_dev (d_recon, d_sse, d_qidx), the reduced decoder at one drop level and the
    two fields calls"""
    import vc2hip_py
    torch = _torch()
    r = ref(oracle, "A", mname)
    case, qm, raws = r["case"], r["qm"], r["raws"]
    assert _refusal(r["enc"]) is None, "row A is not meant to refuse"
    n, ns = len(raws), case.ys * case.xs
    cap = sorted(len(e[0]) for e in r["enc"])[1] * 2 // 3
    capped = [qr.encode_capped(oracle, case, raw, qm, case.q, cap) for raw in raws]
    assert any(t > case.q for _, t in capped)
    capped_dec = [qr.recon(oracle, case, raw, pay, qm) for raw, (pay, _) in zip(raws, capped)]
    reduced = [qr.decode(oracle, case, e[0], qm, 1) for e in r["enc"]]
    sse = [qr.recon(oracle, case, raw, e[0], qm)[1] for raw, e in zip(raws, r["enc"])]
    # fields: every picture of the row as a frame, its two fields coded as pictures of half the height
    fcase = pr.Case(oracle, case.w, case.h // 2, case.cf, case.bits, case.kernel, case.depth, case.u, case.a, q=case.q,
                    scalar=case.scalar, prefix=case.prefix, word_bytes=case.word_bytes)
    fields = [f for raw in raws for f in qr.split_fields(case, raw)]
    fenc = [qr.encode(oracle, fcase, f, qm)[0] for f in fields]
    fdec = [qr.decode(oracle, fcase, p, qm) for p in fenc]
    frames = [qr.merge_fields(case, fdec[2 * i], fdec[2 * i + 1]) for i in range(n)]
    for vname, hip in variants.items():
        tag = (mname, vname)
        hip.set_quant_matrix(qm)
        # HQ_CAPPED through the recon call: payload, recon, sse, indices
        fmt, cpc = _cp(hip, case, mode="HQ_Capped", s=cap)
        b = Batch(hip, fmt, cpc, raws)
        d_sse = torch.zeros(3 * n, dtype=torch.int64, device=DEV)
        d_q = torch.full((n * ns,), -1, dtype=torch.int32, device=DEV)
        hip.encode_recon_batch_dev(b.d_raw.data_ptr(), n, fmt, cpc, b.d_pay.data_ptr(), b.stride, b.d_len.data_ptr(),
                                   b.d_out.data_ptr(), d_sse.data_ptr(), d_q.data_ptr())
        hip.sync()
        assert b.payloads() == [p for p, _ in capped], (tag, "capped payload")
        assert d_q.cpu().numpy().reshape(n, ns).tolist() == [[t] * ns for _, t in capped], (tag, "capped d_qidx")
        assert b.pictures() == [p for p, _ in capped_dec], (tag, "capped d_recon")
        assert d_sse.cpu().numpy().reshape(n, 3).tolist() == [s for _, s in capped_dec], (tag, "capped d_sse")
        b = Batch(hip, fmt, cpc, raws)
        b.encode()
        hip.sync()
        assert b.payloads() == [p for p, _ in capped], (tag, "capped encode_batch_dev")
        # HQ_ConstQ recon without a payload, then the reduced decoder on the composition's payloads
        fmt, cp = _cp(hip, case)
        b = Batch(hip, fmt, cp, raws)
        hip.encode_recon_batch_dev(b.d_raw.data_ptr(), n, fmt, cp, None, 0, None, b.d_out.data_ptr(), d_sse.data_ptr(), d_q.data_ptr())
        hip.sync()
        assert b.pictures() == r["dec"], (tag, "d_recon")
        assert d_sse.cpu().numpy().reshape(n, 3).tolist() == sse, (tag, "d_sse")
        assert (d_q.cpu().numpy() == case.q).all()
        b.load([e[0] for e in r["enc"]])
        hip.decode_reduced_batch_dev(b.d_pay.data_ptr(), b.stride, b.d_len.data_ptr(), n, fmt, cp, 1, b.d_out.data_ptr())
        hip.sync()
        assert b.pictures(case.raw_bytes(1)) == reduced, (tag, "reduced")
        # the fields calls: frames in, 2 n slots, frames out
        _, fcp = _cp(hip, fcase)
        stride = (hip.max_payload_bytes(fmt, fcp) + 64 + 255) // 256 * 256
        d_pay = torch.full((2 * n * stride,), FILL, dtype=torch.uint8, device=DEV)
        d_len = torch.zeros(2 * n, dtype=torch.int64, device=DEV)
        d_frames = torch.full((n * b.rb + 64,), FILL, dtype=torch.uint8, device=DEV)
        hip.encode_fields_batch_dev(b.d_raw.data_ptr(), n, fmt, True, fcp, d_pay.data_ptr(), stride, d_len.data_ptr())
        hip.decode_fields_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, fmt, True, fcp, d_frames.data_ptr())
        hip.sync()
        lens, pay = d_len.cpu().tolist(), d_pay.cpu().numpy().reshape(2 * n, stride)
        assert [pay[i, :lens[i]].tobytes() for i in range(2 * n)] == fenc, (tag, "fields payload")
        out = d_frames.cpu().numpy()
        assert [out[i * b.rb:(i + 1) * b.rb].tobytes() for i in range(n)] == frames, (tag, "fields decode")
        hip.set_quant_matrix(None)


@pytest.mark.parametrize("mname", qr.MATRICES)
def test_both_transcodes(variants, oracle, mname):
    """row A coded by the composition under the matrix: to a coarser index, under a cap, and to a per-slice budget"""
    import vc2hip_py
    torch = _torch()
    r = ref(oracle, "A", mname)
    case, qm = r["case"], r["qm"]
    pics = [qr.Coded(oracle, case, e[0], qm) for e in r["enc"]]
    n, ns = len(pics), case.ys * case.xs
    t = case.q + 7
    fixed = [p.transcode(t) for p in pics]
    assert all(f is not tr.NOT_CODABLE for f in fixed)
    cap = sorted(len(f) for f in fixed)[1] * 3 // 4
    chosen = [p.chosen(case.q, cap) for p in pics]
    assert any(c > case.q for c in chosen)
    s_out = tcr.budget_mixed(case, pics, case.scalar)
    outs = [_try(lambda p=p: tcr.Out(oracle, p, s_out, case.prefix, case.scalar)) for p in pics]
    cbr_code = _refusal(outs)
    for vname, hip in variants.items():
        tag = (mname, vname)
        hip.set_quant_matrix(qm)
        fmt, cp = _cp(hip, case)
        b = Batch(hip, fmt, cp, r["raws"])
        b.load([e[0] for e in r["enc"]])
        vbr = ns * (case.prefix + 4 + 3 * 255 * case.scalar)
        stride_out = (max(hip.max_payload_bytes(fmt, cp), vbr) + 64 + 255) // 256 * 256
        d_out = torch.full((n * stride_out,), FILL, dtype=torch.uint8, device=DEV)
        d_len = torch.zeros(n, dtype=torch.int64, device=DEV)
        d_q = torch.full((n * ns,), -1, dtype=torch.int32, device=DEV)

        def got():
            lens, pay = d_len.cpu().tolist(), d_out.cpu().numpy().reshape(n, stride_out)
            return [pay[i, :lens[i]].tobytes() for i in range(n)], d_q.cpu().numpy().reshape(n, ns)

        hip.transcode_batch_dev(b.d_pay.data_ptr(), b.stride, b.d_len.data_ptr(), n, fmt, cp, vc2hip_py.transcode_params(t),
                                d_out.data_ptr(), stride_out, d_len.data_ptr(), d_q.data_ptr())
        hip.sync()
        pay, q = got()
        assert pay == fixed, (tag, "transcode")
        assert all((q[i] == pics[i].indices(t).ravel()).all() for i in range(n)), (tag, "transcode d_qidx")
        hip.transcode_batch_dev(b.d_pay.data_ptr(), b.stride, b.d_len.data_ptr(), n, fmt, cp, vc2hip_py.transcode_params(case.q, cap),
                                d_out.data_ptr(), stride_out, d_len.data_ptr(), d_q.data_ptr())
        hip.sync()
        pay, q = got()
        assert pay == [p.transcode(c) for p, c in zip(pics, chosen)], (tag, "capped transcode", chosen)
        _, cp_out = _cp(hip, case, mode="HQ_CBR", s=s_out)
        hip.transcode_cbr_batch_dev(b.d_pay.data_ptr(), b.stride, b.d_len.data_ptr(), n, fmt, cp, cp_out, d_out.data_ptr(), stride_out,
                                    d_len.data_ptr(), d_q.data_ptr())
        if _sync_expect(hip, cbr_code, tag):
            pay, q = got()
            assert pay == [o.payload for o in outs], (tag, "transcode to HQ_CBR")
            assert all((q[i] == outs[i].q.ravel()).all() for i in range(n)), (tag, "transcode to HQ_CBR d_qidx")
        hip.set_quant_matrix(None)


@pytest.mark.parametrize("mname", ["steep", "ragged"])
def test_host_buffer_and_pipelined_calls(hip, oracle, mname):
    for name in ("A", "L"):
        r = ref(oracle, name, mname)
        assert _refusal(r["enc"]) is None, "not meant to refuse (the LD search under `edge` is: test_encode_and_decode_batches)"
        fmt, cp = _cp(hip, r["case"])
        hip.set_quant_matrix(r["qm"])
        pay, q = hip.encode_picture_hq(r["raws"][1], fmt, cp)
        assert pay == r["enc"][1][0] and (q == r["enc"][1][1]).all()
        assert hip.decode_picture(pay, fmt, cp) == r["dec"][1]
        assert hip.encode_pictures_pipelined(r["raws"], fmt, cp) == [e[0] for e in r["enc"]]
        assert hip.decode_pictures_pipelined([e[0] for e in r["enc"]], fmt, cp) == r["dec"]
        hip.set_quant_matrix(None)
        assert hip.encode_picture_hq(r["raws"][1], fmt, cp)[0] == ref(oracle, name, "default")["enc"][1][0]


# ---------------------------------------------------------------------------------------------------------------------
# the default matrix set explicitly, and NULL after a matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "G", "E", "C", "L"])   # (the roomy rows E2 and L2 reach index 0, where no matrix matters)
def test_default_set_explicitly_and_null_again(oracle, name):
    r = ref(oracle, name, "default")
    case = r["case"]
    fresh, hip = _ctx("PLANES8_NEVER"), _ctx("PLANES8_NEVER")   # (one band-plane form, however many batches a context has decoded)
    fmt, cp = _cp(hip, case)

    def run(h):
        b = Batch(h, fmt, cp, r["raws"])
        b.encode()
        b.decode()
        h.sync()
        return b.payloads(), b.pictures(), h.dwt_launches()

    unset = run(fresh)
    assert unset[0] == [e[0] for e in r["enc"]]
    hip.set_quant_matrix(r["qm"])
    assert run(hip) == unset
    hip.set_quant_matrix(qr.matrix(oracle, "ragged", case.kernel, case.depth))
    other = run(hip)
    assert other[0] == [e[0] for e in ref(oracle, name, "ragged")["enc"]] and other[0] != unset[0]
    hip.set_quant_matrix(None)
    assert run(hip) == unset
    fresh.close()
    hip.close()


def test_the_benchmarks_path_launches_the_same_kernels(oracle):
    """a context that never saw the setter, one whose matrix was set and taken back, and one set to the default: the same
    transform launches (vc2hip_dwt_launches) and the same kernels by name and launch count (vc2hip_profile_*) for the
    benchmark's coding parameters (HQ_ConstQ DD97 depth 4, 32 x 16 slices, 4:2:2 10-bit, q 16, scalar 2) on a small picture"""
    case = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 4, 1, 2, q=16, scalar=2)
    from synth import synth
    rb = case.raw_bytes()
    two = synth(case.w, case.h, case.cf, case.bits, 21, frames=2)   # (the benchmark's generator: noise does not fit scalar 2)
    raws = [two[:rb], two[rb:]]
    qm = qr.matrix(oracle, "default", case.kernel, case.depth)
    seen = []
    for how in ("never", "set and taken back", "default set"):
        hip = _ctx()
        if how != "never":
            hip.set_quant_matrix(qr.matrix(oracle, "ragged", case.kernel, case.depth) if how != "default set" else qm)
        if how == "set and taken back":
            hip.set_quant_matrix(None)
        fmt, cp = _cp(hip, case)
        b = Batch(hip, fmt, cp, raws)
        hip.profile_enable(True)
        b.encode()
        enc_rec = hip.dwt_launches()
        b.decode()
        hip.sync()
        prof = {k: v[0] for k, v in hip.profile().items()}
        seen.append((b.payloads(), b.pictures(), enc_rec, hip.dwt_launches(), prof))
        hip.close()
    assert seen[0][4] and seen[1] == seen[0] and seen[2] == seen[0]


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------
def _stream_call(hip, b, cp, frag, eos=True, first=3, prev=17):
    import vc2hip_py
    torch = _torch()
    cap = b.n * (b.stride + 4096) + 64
    d_stream = torch.full((cap,), FILL, dtype=torch.uint8, device=DEV)
    d_slen = torch.zeros(1, dtype=torch.int64, device=DEV)
    sp = vc2hip_py.stream_params(3, first, prev, eos)
    if frag:
        hip.stream_write_fragments_dev(b.d_pay.data_ptr(), b.stride, b.d_len.data_ptr(), b.n, cp, sp, frag, d_stream.data_ptr(), cap,
                                       d_slen.data_ptr())
    else:
        hip.stream_write_dev(b.d_pay.data_ptr(), b.stride, b.d_len.data_ptr(), b.n, cp, sp, d_stream.data_ptr(), cap, d_slen.data_ptr())
    hip.sync()
    return d_stream[:int(d_slen.item())].cpu().numpy().tobytes()


def _read(hip, stream, b, cp):
    """stream_read_dev into b's slots (pre-filled); returns (payloads, picture numbers)"""
    import vc2hip_py
    torch = _torch()
    b.d_pay.fill_(FILL)
    b.d_len.fill_(-1)
    d_stream = _dev(stream + bytes(16))
    d_pn = torch.zeros(b.n, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    hip.stream_read_dev(d_stream.data_ptr(), len(stream), b.n, cp, vc2hip_py.stream_params(3), b.d_pay.data_ptr(), b.stride,
                        b.d_len.data_ptr(), d_pn.data_ptr())
    hip.sync()
    return b.payloads(), [v & 0xFFFFFFFF for v in d_pn.cpu().tolist()]


@pytest.mark.parametrize("name", ["A", "L"])
@pytest.mark.parametrize("mname", ["ragged", "edge", "default"])
def test_stream_writers_are_the_model_and_read_back(hip, oracle, name, mname):
    r = ref(oracle, name, mname)
    case, qm = r["case"], r["qm"]
    # (the stream calls move payload bytes only: where the composition refuses the row under this matrix -- the LD search
    # under `edge` -- the default matrix's payloads travel under this matrix's header)
    pays = [e[0] for e in (r if _refusal(r["enc"]) is None else ref(oracle, name, "default"))["enc"]]
    fmt, cp = _cp(hip, case)
    sb = oracle.slice_bytes(case.ys, case.xs, case.s, 1).ravel() if case.mode == "LD" else None
    hip.set_quant_matrix(qm)
    b = Batch(hip, fmt, cp, r["raws"])
    b.load(pays)
    whole = _stream_call(hip, b, cp, 0)
    assert whole == qr.picture_stream(pays, cp, 3, qm, 3, 17, True), (name, mname, "stream_write_dev")
    frag = _stream_call(hip, b, cp, 300)
    assert frag == qr.fragment_stream(pays, cp, 300, qm, 3, 17, True, sb), (name, mname, "stream_write_fragments_dev")
    for s in (whole, frag):
        assert _read(hip, s, b, cp) == (pays, [3, 4, 5])
    hip.set_quant_matrix(None)
    plain = _stream_call(hip, b, cp, 0)
    assert plain == qr.picture_stream(pays, cp, 3, None, 3, 17, True), "an unset context writes no matrix"


def test_stream_reader_compares_effective_matrices(hip, oracle):
    import vc2hip_py
    r = ref(oracle, "A", "ragged")
    case, x = r["case"], r["qm"]
    pays = [e[0] for e in r["enc"]]
    fmt, cp = _cp(hip, case)
    b = Batch(hip, fmt, cp, r["raws"])
    y = qr.matrix(oracle, "steep", case.kernel, case.depth)
    dflt = qr.matrix(oracle, "default", case.kernel, case.depth)
    with_x = qr.picture_stream(pays, cp, 3, x, 0, 0, True)
    frag_x = qr.fragment_stream(pays, cp, 200, x, 0, 0, True)
    with_d = qr.picture_stream(pays, cp, 3, dflt, 0, 0, True)
    plain = qr.picture_stream(pays, cp, 3, None, 0, 0, True)

    def refused(stream, why):
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            _read(hip, stream, b, cp)
        assert e.value.code == ESYNTAX and why in str(e.value) and "at byte" in str(e.value), str(e.value)

    hip.set_quant_matrix(x)
    assert _read(hip, with_x, b, cp)[0] == pays and _read(hip, frag_x, b, cp)[0] == pays
    refused(plain, "differs from the context's")
    refused(with_d, "differs from the context's")
    hip.set_quant_matrix(y)
    refused(with_x, "differs from the context's")
    refused(frag_x, "differs from the context's")
    hip.set_quant_matrix(None)
    refused(with_x, "differs from the context's")
    assert _read(hip, with_d, b, cp)[0] == pays, "the default matrix carried explicitly is read by an unset context"
    assert _read(hip, plain, b, cp)[0] == pays
    hip.set_quant_matrix(dflt)
    assert _read(hip, plain, b, cp)[0] == pays and _read(hip, with_d, b, cp)[0] == pays
    big = x.copy()
    big[5] = 256
    hip.set_quant_matrix(x)
    refused(qr.picture_stream(pays, cp, 3, big, 0, 0, True), "255")
    refused(qr.fragment_stream(pays, cp, 200, big, 0, 0, True), "255")
    refused(qr.picture_stream(pays, cp, 3, x, 0, 0, True)[:40], "past the end")
    hip.set_quant_matrix(None)
    assert _read(hip, plain, b, cp)[0] == pays


# ---------------------------------------------------------------------------------------------------------------------
# graph capture and lanes
# ---------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_keeps_its_matrix(oracle):
    torch = _torch()
    rx, ry = ref(oracle, "A", "ragged"), ref(oracle, "A", "steep")
    case = rx["case"]
    s = torch.cuda.Stream()
    hip = _ctx(stream=s.cuda_stream)
    fmt, cp = _cp(hip, case)
    with torch.cuda.stream(s):
        b = Batch(hip, fmt, cp, rx["raws"])
        hip.set_quant_matrix(rx["qm"])
        b.encode()                       # the warm-up: one eager call with the same fmt, cp and n, and a sync
        s.synchronize()
        hip.sync()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=s):
            b.encode()
    except BaseException as e:           # noqa: BLE001 -- whatever ended the capture; no further GPU call
        pytest.fail("graph capture failed: %r" % (e,))
    hip.set_quant_matrix(ry["qm"])       # pure host state: the graph holds X by value
    with torch.cuda.stream(s):
        b.d_pay.fill_(FILL)
        g.replay()
        s.synchronize()
        hip.sync()
        assert b.payloads() == [e[0] for e in rx["enc"]], "the replay codes with the matrix it was captured with"
        b.encode()
        s.synchronize()
        hip.sync()
        assert b.payloads() == [e[0] for e in ry["enc"]], "an eager call codes with the context's matrix"
    hip.close()


@pytest.mark.parametrize("name", ["A", "E", "L"])
def test_lanes_use_the_contexts_matrix(oracle, name):
    r = ref(oracle, name, "ragged")
    if _refusal(r["enc"]) is not None:
        pytest.fail("the composition refuses this row under the ragged matrix")
    hip = _ctx()
    hip.set_streams(2)
    fmt, cp = _cp(hip, r["case"])
    hip.set_quant_matrix(r["qm"])
    b = Batch(hip, fmt, cp, r["raws"])
    b.encode()
    b.decode()
    hip.sync()
    assert b.payloads() == [e[0] for e in r["enc"]] and b.pictures() == r["dec"]
    hip.set_quant_matrix(qr.matrix(oracle, "flat", r["case"].kernel, r["case"].depth))
    b.encode()
    hip.sync()
    assert b.payloads() == [e[0] for e in ref(oracle, name, "flat")["enc"]]
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing_and_keep_the_matrix(oracle):
    import vc2hip_py
    r = ref(oracle, "A", "ragged")
    case, qm = r["case"], r["qm"]
    hip = _ctx()
    fmt, cp = _cp(hip, case)
    hip.set_quant_matrix(qm)
    b = Batch(hip, fmt, cp, r["raws"])

    def setter(entries, depth):
        m = np.ascontiguousarray(entries, np.int32)
        return hip.lib.vc2hip_set_quant_matrix(hip.h, m.ctypes.data_as(C.c_void_p), depth)

    low, high = qm.copy(), qm.copy()
    low[3], high[-1] = -1, 256
    assert setter(low, case.depth) == EINVAL and setter(high, case.depth) == EINVAL
    assert setter(np.zeros(22, np.int32), 0) == EINVAL and setter(np.zeros(25, np.int32), 8) == EINVAL
    assert hip.quant_matrix().tolist() == qm.tolist(), "a refused setter leaves the matrix as it was"
    # a call whose cp->depth is not the matrix's: every covered call once, HQ and LD where the call has both
    other = pr.Case(oracle, case.w, case.h, case.cf, case.bits, case.kernel, 2, 2, 4, q=case.q, scalar=case.scalar)
    fmt2, cp2 = _cp(hip, other)
    _, cp2_cbr = _cp(hip, other, mode="HQ_CBR", s=40000)
    _, cp2_ld = _cp(hip, other, mode="LD", s=12000)
    _, cp2_field = _cp(hip, pr.Case(oracle, case.w, case.h // 2, case.cf, case.bits, case.kernel, 2, 2, 4, q=case.q, scalar=case.scalar))
    sp = vc2hip_py.stream_params(3)
    d8 = b.d_len.data_ptr()
    calls = [lambda: hip.encode_batch_dev(b.d_raw.data_ptr(), b.n, fmt2, cp2, b.d_pay.data_ptr(), b.stride, d8),
             lambda: hip.decode_batch_dev(b.d_pay.data_ptr(), b.stride, d8, b.n, fmt2, cp2, b.d_out.data_ptr()),
             lambda: hip.decode_reduced_batch_dev(b.d_pay.data_ptr(), b.stride, d8, b.n, fmt2, cp2, 1, b.d_out.data_ptr()),
             lambda: hip.encode_recon_batch_dev(b.d_raw.data_ptr(), b.n, fmt2, cp2, b.d_pay.data_ptr(), b.stride, d8, b.d_out.data_ptr()),
             lambda: hip.transcode_batch_dev(b.d_raw.data_ptr(), 256, d8, 1, fmt2, cp2, vc2hip_py.transcode_params(9), b.d_pay.data_ptr(),
                                             b.stride, d8),
             lambda: hip.stream_write_dev(b.d_raw.data_ptr(), 256, d8, 1, cp2, sp, b.d_pay.data_ptr(), 4096, d8),
             lambda: hip.stream_read_dev(b.d_raw.data_ptr(), 256, 1, cp2, sp, b.d_pay.data_ptr(), b.stride, d8),
             lambda: hip.encode_picture_hq(r["raws"][0], fmt2, cp2),
             lambda: hip.decode_picture(r["enc"][0][0], fmt2, cp2),
             lambda: hip.encode_pictures_pipelined(r["raws"][:1], fmt2, cp2),
             lambda: hip.decode_pictures_pipelined([r["enc"][0][0]], fmt2, cp2),
             lambda: hip.encode_picture_hq(r["raws"][0], fmt2, cp2_ld),      # (vc2hip_encode_picture_ld: the binding picks it by mode)
             lambda: hip.decode_picture(r["enc"][0][0], fmt2, cp2_ld),       # (vc2hip_decode_picture_ld)
             lambda: hip.encode_batch_dev(b.d_raw.data_ptr(), b.n, fmt2, cp2_ld, b.d_pay.data_ptr(), b.stride, d8),
             lambda: hip.decode_batch_dev(b.d_pay.data_ptr(), b.stride, d8, b.n, fmt2, cp2_ld, b.d_out.data_ptr()),
             lambda: hip.transcode_cbr_batch_dev(b.d_raw.data_ptr(), 256, d8, 1, fmt2, cp2, cp2_cbr, b.d_pay.data_ptr(), b.stride, d8),
             lambda: hip.encode_fields_batch_dev(b.d_raw.data_ptr(), 1, fmt2, True, cp2_field, b.d_pay.data_ptr(), b.stride, d8),
             lambda: hip.decode_fields_batch_dev(b.d_pay.data_ptr(), b.stride, d8, 1, fmt2, True, cp2_field, b.d_out.data_ptr()),
             lambda: hip.stream_write_fragments_dev(b.d_raw.data_ptr(), 256, d8, 1, cp2, sp, 300, b.d_pay.data_ptr(), 4096, d8),
             lambda: hip.stream_write_fragments_dev(b.d_raw.data_ptr(), 256, d8, 1, cp2_ld, sp, 300, b.d_pay.data_ptr(), 4096, d8)]
    for k, call in enumerate(calls):
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            call()
        assert e.value.code == EINVAL and "depth" in str(e.value), (k, str(e.value))
    hip.sync()
    assert b.untouched(), "a refused call wrote an output byte"
    assert hip.quant_matrix().tolist() == qm.tolist()
    b.encode()
    hip.sync()
    assert b.payloads() == [e[0] for e in r["enc"]], "the context codes on with its matrix after the refusals"
    hip.close()
