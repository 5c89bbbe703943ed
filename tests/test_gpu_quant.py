"""GPU tests of every copy of the quantiser (and of the dequantisers behind them) at its boundaries, exactly: the designed
values of tests/quant_ref.py through the fine-grained calls and, as designed pictures, through the slice coders, the LD
quantiser, both transcoders and the recon call.  Expected values come from the Python definition and the oracle only
(tests/test_quant_ref.py shows on the CPU that the two agree on every designed value and what each design reaches).

  copy 1        quant_core: vc2hip_quantise_np on sheets that hold every index 0 .. 119 (mixed wavefronts and all-slow ones)
  copy 2        load8_tab: designed pictures on the int32 store (P32; P16 under STORE32)
  copy 3, heads p16_group, the pack16 kernels' heads and p16_general: P16 (slots and one pass) and P16W on the 16-bit store
  copies 5, 6   the LD quantisers on a fast and a general slice geometry, indices given
  copy 4        k_cbr_search: vc2hip_cbr_qindices on the tight search sheets under CBR_GENERAL
  copy 9        the register searches and the cap's measure: the same sheets on the default context, one HQ_CBR picture and one
                HQ_CAPPED batch on P16; copy 5's search half: vc2hip_ld_qindices at budgets tight on the 2^K boundaries
  copy 7        tc_quant_c: requantise pairs through both transcoders
  copy 8        rq_quant: vc2hip_encode_recon_batch_dev on the P16 and P32 designs
  dequantisers  the literal ones on the dequantiser sheets; the fused ones (and, under PLANES8_ALWAYS, the byte planes' table) by
                decoding every designed payload
The library's own records say which path ran: hip.dwt_launches() the store, hip.profile() slots or one pass,
hip.band_plane_bits() the band planes' form; which pack kernel a geometry gets is pack16_plan's rule, restated in
quant_ref.pack_kernel and asserted on the CPU."""
import numpy as np
import pytest

import qmatrix_ref as qmr
import quant_ref as qr
import transcode_cbr_ref as tcr
import transcode_ref as tr
from vc2lib import KERNELS, OracleError, make_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5
ECODE32 = -11
SCALAR = 4
QM0 = np.zeros(7, np.int32)
VARIANTS = {"default": (), "store32": ("STORE32",), "onepass": ("SINGLE_PASS_VBR",), "bytes": ("PLANES8_ALWAYS",),
            "cbr_general": ("CBR_GENERAL",), "cap_general": ("CAP_GENERAL",)}


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def variants():
    from vc2hip_py import FLAGS, Vc2Hip
    v = {name: Vc2Hip(flags=sum(FLAGS[f] for f in flags)) for name, flags in VARIANTS.items()}
    yield v
    for h in v.values():
        h.close()


@pytest.fixture(scope="module")
def hip(variants):
    return variants["default"]


def _dev(b):
    torch = _torch()
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(DEV)


def _cp(hip, case, **over):
    import vc2hip_py
    fmt = vc2hip_py.picture_format(case.w, case.h, case.cf, case.bits, case.word_bytes)
    kw = dict(mode=case.mode, q=case.q, s=case.s, prefix=case.prefix, scalar=case.scalar)
    kw.update(over)
    return fmt, vc2hip_py.coding_params(hip.lib, fmt, case.kernel, case.depth, case.u, case.a, **kw)


def _first_diff(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    bad = np.flatnonzero(a != b)
    return None if bad.size == 0 else (int(bad[0]), int(a[bad[0]]), int(b[bad[0]]), int(bad.size))


# ---------------------------------------------------------------------------------------------------------------------
# copy 1 and the literal dequantisers: the fine-grained calls on the sheets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "slow"])
def test_quantise_np_on_the_sheets(hip, oracle, kind):
    mixed, slow = qr.quant_sheets()
    qi = qr.sheet_qidx()
    for k, plane in enumerate(mixed if kind == "mixed" else slow):
        want = qr.sheet_want(plane, qr.quant_np)
        assert np.array_equal(oracle.quantise_np(plane, qr.SHEET_DEPTH, qi, QM0), want)
        got = hip.quantise_np(plane, qr.SHEET_DEPTH, qi, QM0)
        bad = _first_diff(got, want)
        assert bad is None, (kind, k, "at, got, want, count", bad, "index", int(qi.ravel()[bad[0] // plane.shape[1] // qr.SHEET_SH * qr.SHEET_XS
                                                                                   + bad[0] % plane.shape[1] // qr.SHEET_SW]))


def test_quantise_np_refuses_index_120_with_the_reference_s_message(hip, oracle):
    from vc2hip_py import Vc2HipError
    plane = qr.quant_sheets()[0][0]
    qi = qr.sheet_qidx().copy()
    qi[-1, -1] = 120
    with pytest.raises(Vc2HipError, match="quantization index exceeds maximum implemented value."):
        hip.quantise_np(plane, qr.SHEET_DEPTH, qi, QM0)
    with pytest.raises(OracleError, match="quantization index exceeds maximum implemented value."):
        oracle.quantise_np(plane, qr.SHEET_DEPTH, qi, QM0)


def test_dequantise_np_and_ld_on_the_sheets(hip, oracle):
    qi = qr.sheet_qidx()
    for k, plane in enumerate(qr.dequant_sheets()):
        want = qr.sheet_want(plane, qr.scale_np)
        assert np.array_equal(oracle.dequantise_np(plane, qr.SHEET_DEPTH, qi, QM0), want)
        bad = _first_diff(hip.dequantise_np(plane, qr.SHEET_DEPTH, qi, QM0), want)
        assert bad is None, (k, "dequantise_np: at, got, want, count", bad)
        bad = _first_diff(hip.dequantise_ld(plane, qr.SHEET_DEPTH, qi, QM0), oracle.dequantise_ld(plane, qr.SHEET_DEPTH, qi, QM0))
        assert bad is None, (k, "dequantise_ld: at, got, want, count", bad)


# ---------------------------------------------------------------------------------------------------------------------
# copies 2 and 3, the heads, p16_general and the fused dequantisers: designed pictures
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(oracle, name, q, seed=None):
    """the composition's payload and decoded picture of a designed picture under its ladder matrix, once per session"""
    key = (name, q, seed)
    if key not in _REF:
        d = qr.design(oracle, name, q) if seed is None else qr.build_design(oracle, qr.GEOMS[name], q, seed=seed)
        case = d.geom.case(oracle, q, SCALAR)
        payload, qidx = qmr.encode(oracle, case, d.raw, d.qm)
        _REF[key] = dict(d=d, case=case, payload=payload, dec=qmr.decode(oracle, case, payload, d.qm))
    return _REF[key]


class Batch:
    """n pictures on the device, payload slots and lengths pre-filled"""

    def __init__(self, hip, fmt, cp, raws):
        torch = _torch()
        self.hip, self.fmt, self.cp, self.n, self.rb = hip, fmt, cp, len(raws), len(raws[0])
        self.d_raw = _dev(b"".join(raws) + bytes(64))
        self.stride = (hip.max_payload_bytes(fmt, cp) + 64 + 255) // 256 * 256
        self.d_pay = torch.full((self.n * self.stride,), FILL, dtype=torch.uint8, device=DEV)
        self.d_len = torch.full((self.n,), -1, dtype=torch.int64, device=DEV)
        self.d_out = torch.full((self.n * self.rb + 64,), FILL, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()

    def payloads(self):
        lens = self.d_len.cpu().tolist()
        pay = self.d_pay.cpu().numpy().reshape(self.n, self.stride)
        return [pay[i, :max(int(lens[i]), 0)].tobytes() for i in range(self.n)]

    def pictures(self):
        out = self.d_out.cpu().numpy()
        return [out[i * self.rb:(i + 1) * self.rb].tobytes() for i in range(self.n)]


def _store_bits(hip):
    return {r["store_bits"] for r in hip.dwt_launches() if not r["inverse"]}


# which contexts a geometry runs on, and what the library's records must say there: (store bits, slots behind the coder)
CONTEXTS = {"P32": {"default": (32, True)},
            "P16": {"default": (16, True), "store32": (32, True), "onepass": (16, False), "bytes": (16, True)},
            "P16W": {"default": (16, True), "bytes": (16, True)}}
PICTURES = [(name, q) for name, g in qr.GEOMS.items() for q in qr.picture_indices(g)]


@pytest.mark.parametrize("name,q", PICTURES, ids=lambda v: str(v))
def test_designed_pictures(variants, oracle, name, q):
    """one designed picture through vc2hip_encode_picture_hq, and three (the design, a second design of the same index, the
    design again) through vc2hip_encode_batch_dev and vc2hip_decode_batch_dev, on every context the geometry has"""
    a, b = _reference(oracle, name, q), _reference(oracle, name, q, seed=5000 + q)
    assert a["payload"] != b["payload"]
    case, qm = a["case"], a["d"].qm
    raws, pays, decs = [r["d"].raw for r in (a, b, a)], [r["payload"] for r in (a, b, a)], [r["dec"] for r in (a, b, a)]
    for vname, (bits, slots) in CONTEXTS[name].items():
        hip = variants[vname]
        tag = (name, q, vname)
        fmt, cp = _cp(hip, case)
        hip.set_quant_matrix(qm)
        try:
            payload, qidx = hip.encode_picture_hq(a["d"].raw, fmt, cp)
            assert _store_bits(hip) == {bits}, (tag, _store_bits(hip))
            assert len(payload) == len(a["payload"]) and payload == a["payload"], (tag, "payload", len(payload), len(a["payload"]))
            assert (qidx == q).all()
            assert hip.decode_picture(a["payload"], fmt, cp) == a["dec"], (tag, "decode_picture")
            bt = Batch(hip, fmt, cp, raws)
            hip.profile_reset()
            hip.profile_enable(True)
            hip.encode_batch_dev(bt.d_raw.data_ptr(), 3, fmt, cp, bt.d_pay.data_ptr(), bt.stride, bt.d_len.data_ptr())
            assert _store_bits(hip) == {bits}, (tag, _store_bits(hip))        # (the record of the launches just made)
            hip.decode_batch_dev(bt.d_pay.data_ptr(), bt.stride, bt.d_len.data_ptr(), 3, fmt, cp, bt.d_out.data_ptr())
            hip.sync()
            hip.profile_enable(False)
            seen = {k for k, v in hip.profile().items() if v[0] > 0}
            assert "hq_pack" in seen and ("slice_compact" in seen) == slots, (tag, seen)
            if vname == "bytes":
                assert hip.band_plane_bits() == 8, (tag, hip.band_plane_bits())
            assert bt.d_len.cpu().tolist() == [len(p) for p in pays], (tag, "lengths")
            assert bt.payloads() == pays, (tag, "batch payloads")
            assert bt.pictures() == decs, (tag, "batch decode")
        finally:
            hip.set_quant_matrix(None)


@pytest.mark.parametrize("name,q", [("P32", 15), ("P16", 24), ("P16W", 30)], ids=lambda v: str(v))
def test_designed_pictures_under_the_default_matrix(variants, oracle, name, q):
    """the same designs without a matrix of the context's: payload and lengths against oracle.encode_stream, the decoded
    picture against oracle.decode_stream"""
    d = qr.design(oracle, name, q)
    g = d.geom
    p = make_params(g.w, g.h, g.cf, g.bits, g.wavelet, g.depth, g.u, g.a, q=q, scalar=SCALAR)
    stream = oracle.encode_stream(p, d.raw, 1)
    dec, n = oracle.decode_stream(p, stream, 1)
    assert n == 1
    case = g.case(oracle, q, SCALAR)
    for vname in CONTEXTS[name]:
        hip = variants[vname]
        fmt, cp = _cp(hip, case)
        payload, _ = hip.encode_picture_hq(d.raw, fmt, cp)
        assert payload == stream[-13 - len(payload):-13] and len(payload) > 1000, (name, q, vname)
        assert hip.decode_picture(payload, fmt, cp) == dec, (name, q, vname)


@pytest.mark.parametrize("name", ["P32", "P16"])
def test_a_design_with_the_first_uncodable_quotient_is_refused(variants, oracle, name):
    """k = 65535 (a code of 34 bits): the library refuses the picture with VC2HIP_ECODE32 on every context; on the reference's
    side the value lies outside its 32-bit code words (VLC.h:27 -- the oracle's writer has no such check, so the definition's
    rule, transcode_ref.in_domain, stands for it).  The neighbour 65534 is coded: it is part of every ordinary design at the
    index 0 (tests/test_quant_ref.py)"""
    from vc2hip_py import Vc2HipError
    q = qr.GEOMS[name].body_lo - 1
    d = qr.design(oracle, name, q, refused=True)
    case = d.geom.case(oracle, q, 64)
    qi = np.full((case.ys, case.xs), q, np.int32)
    planes = [oracle.quantise_np(p, case.depth, qi, d.qm) for p in qr.design_planes(d)]
    assert max(int(np.abs(p).max()) for p in planes) == qr.CODE_MAX + 1 and not tr.in_domain(planes, qi)
    for vname in CONTEXTS[name]:
        hip = variants[vname]
        fmt, cp = _cp(hip, case)
        hip.set_quant_matrix(d.qm)
        try:
            with pytest.raises(Vc2HipError, match="exceeds 65534") as e:
                hip.encode_picture_hq(d.raw, fmt, cp)
            assert e.value.code == ECODE32, (name, vname)
        finally:
            hip.set_quant_matrix(None)


@pytest.mark.parametrize("scalar,one_pass", [(45, True), (46, False), (100, False)])
def test_single_pass_flag_keeps_the_slots_for_long_slices(variants, oracle, scalar, one_pass):
    """Found by the refused design above, which asks for a slice scalar of 64: under VC2HIP_FLAG_SINGLE_PASS_VBR the look-back
    of k_hq_pack counts tiles of four slices, but from a scalar of 46 on four slice images no longer fit in LDS and a
    workgroup holds two slices (from 96 on: one) -- twice or four times as many tiles as status words, an access beyond
    their buffer.  The flag now keeps the slots there.  A designed P16 picture at the last scalar of the one-pass form and
    at the first ones of both long forms: payloads, lengths and decoded pictures, and what the profile says ran"""
    q = 24
    d, d2 = qr.design(oracle, "P16", q), qr.build_design(oracle, qr.P16, q, seed=5000 + q)
    case = d.geom.case(oracle, q, scalar)
    pays = [qmr.encode(oracle, case, x.raw, d.qm)[0] for x in (d, d2)]
    decs = [qmr.decode(oracle, case, p, d.qm) for p in pays]
    hip = variants["onepass"]
    fmt, cp = _cp(hip, case)
    hip.set_quant_matrix(d.qm)
    try:
        payload, _ = hip.encode_picture_hq(d.raw, fmt, cp)
        assert payload == pays[0], (scalar, len(payload), len(pays[0]))
        bt = Batch(hip, fmt, cp, [d.raw, d2.raw])
        hip.profile_reset()
        hip.profile_enable(True)
        hip.encode_batch_dev(bt.d_raw.data_ptr(), 2, fmt, cp, bt.d_pay.data_ptr(), bt.stride, bt.d_len.data_ptr())
        hip.decode_batch_dev(bt.d_pay.data_ptr(), bt.stride, bt.d_len.data_ptr(), 2, fmt, cp, bt.d_out.data_ptr())
        hip.sync()
        hip.profile_enable(False)
        seen = {k for k, v in hip.profile().items() if v[0] > 0}
        assert "hq_pack" in seen and ("slice_compact" in seen) == (not one_pass), (scalar, seen)
        assert bt.d_len.cpu().tolist() == [len(p) for p in pays], scalar
        assert bt.payloads() == pays and bt.pictures() == decs, scalar
    finally:
        hip.set_quant_matrix(None)


# ---------------------------------------------------------------------------------------------------------------------
# copy 8: the recon call on the designs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,q", [(n, q) for n in ("P32", "P16") for q in qr.picture_indices(qr.GEOMS[n])[::2]] + [("P32", 119)], ids=lambda v: str(v))
def test_recon_call_on_the_designs(variants, oracle, name, q):
    """every second design of P32 and P16, and P32 at 119: adjusted indices 110 .. 119, the wrapped factors among them, where
    the small values between the designed ones must quantise to 0 (the reciprocal multiply has no domain there)"""
    torch = _torch()
    a = _reference(oracle, name, q)
    case, qm, raw = a["case"], a["d"].qm, a["d"].raw
    pic, sse = qmr.recon(oracle, case, raw, a["payload"], qm)
    assert pic == a["dec"]
    ns = case.ys * case.xs
    for vname in ("default", "store32"):
        hip = variants[vname]
        fmt, cp = _cp(hip, case)
        hip.set_quant_matrix(qm)
        try:
            bt = Batch(hip, fmt, cp, [raw, raw])
            d_sse = torch.zeros(6, dtype=torch.int64, device=DEV)
            d_q = torch.full((2 * ns,), -1, dtype=torch.int32, device=DEV)
            hip.encode_recon_batch_dev(bt.d_raw.data_ptr(), 2, fmt, cp, bt.d_pay.data_ptr(), bt.stride, bt.d_len.data_ptr(),
                                       bt.d_out.data_ptr(), d_sse.data_ptr(), d_q.data_ptr())
            hip.sync()
            assert bt.payloads() == [a["payload"]] * 2, (name, q, vname, "payload")
            assert bt.pictures() == [pic] * 2, (name, q, vname, "d_recon")
            assert d_sse.cpu().numpy().reshape(2, 3).tolist() == [sse] * 2, (name, q, vname, "d_sse")
            assert (d_q.cpu().numpy() == q).all()
            # without a payload: the call's own quantise / dequantise round trip alone
            bt2 = Batch(hip, fmt, cp, [raw, raw])
            hip.encode_recon_batch_dev(bt2.d_raw.data_ptr(), 2, fmt, cp, None, 0, None, bt2.d_out.data_ptr(), d_sse.data_ptr(), None)
            hip.sync()
            assert bt2.pictures() == [pic] * 2, (name, q, vname, "d_recon without a payload")
            assert d_sse.cpu().numpy().reshape(2, 3).tolist() == [sse] * 2
        finally:
            hip.set_quant_matrix(None)


# ---------------------------------------------------------------------------------------------------------------------
# copies 5 and 6: the LD quantisers with given indices
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(qr.LD_GEOMS))
def test_quantise_ld_on_designed_planes(hip, oracle, geom):
    depth, ys, xs, lshape, cshape, fast = qr.LD_GEOMS[geom]
    assert qr.ld_fast(depth, ys, xs, lshape, cshape) == fast
    qm = oracle.quant_matrix(KERNELS["LeGall"], depth)
    for sheet, (planes, qidx) in enumerate(qr.ld_planes(geom)):
        hip.profile_reset()
        hip.profile_enable(True)
        got = [hip.quantise_ld(p, depth, qidx, qm) for p in planes]
        hip.profile_enable(False)
        # one launch per anti-diagonal of slices and plane, on both kernels (which of them: ld_fast, vc2_launch_ld_quantise's rule)
        assert hip.profile().get("ld_quantise", (0, 0.0))[0] == 3 * (ys + xs - 1), hip.profile()
        for c, (g, p) in enumerate(zip(got, planes)):
            want = oracle.quantise_ld(p, depth, qidx, qm)
            # behind LL the LD quantiser is quant at the slice's adjusted index: the definition is the third witness
            aq = qr.band_index_plane(p.shape, depth, ys, xs, qidx, qm)
            behind = np.ones(p.shape, bool)
            behind[::1 << depth, ::1 << depth] = False
            assert np.array_equal(want[behind], qr.quant_np(p, aq)[behind])
            assert want[0, 0] == qr.quant(int(p[0, 0]), int(aq[0, 0]))       # the LL sample whose prediction is 0
            bad = _first_diff(g, want)
            assert bad is None, (geom, sheet, c, "at, got, want, count", bad)


# ---------------------------------------------------------------------------------------------------------------------
# copy 7: requantise pairs through both transcoders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", qr.REQUANT_TARGETS)
def test_requantise_pairs_through_both_transcoders(variants, oracle, t):
    import vc2hip_py
    torch = _torch()
    case, qm, pays = qr.requant_inputs(oracle, t)
    pics = [qmr.Coded(oracle, case, p, qm) for p in pays]
    n, ns = len(pics), case.ys * case.xs
    fixed = [p.transcode(t) for p in pics]
    assert all(f is not tr.NOT_CODABLE for f in fixed) and all(p.in_domain for p in pics)
    # the definition is the third witness of the requantised planes
    for p in pics:
        y2 = p.requantised(t)[0]
        aq_s = np.repeat(np.repeat(p.q, y2.shape[0] // case.ys, axis=0), y2.shape[1] // case.xs, axis=1)
        want = qr.quant_np(qr.scale_np(p.planes[0], aq_s), np.maximum(aq_s, t))
        assert np.array_equal(np.where(aq_s >= t, p.planes[0], want), y2)
    cap = len(fixed[0])
    chosen = [p.chosen(0, cap) for p in pics]
    assert chosen[0] == t and pics[0].table()[t - 1] > cap        # tight: one index lower does not fit
    # a budget that half of picture 0's slices meet as they are: the others are searched and requantised
    s_out = ns * (int(np.median(tcr.slice_need(case, pics[0].planes, case.scalar)[0])) + 4)
    outs = [tcr.Out(oracle, p, s_out, case.prefix, case.scalar) for p in pics]
    for vname in ("default", "store32"):
        hip = variants[vname]
        tag = (t, vname)
        hip.set_quant_matrix(qm)
        try:
            fmt, cp = _cp(hip, case)
            stride_in = (max(hip.max_payload_bytes(fmt, cp), max(len(p) for p in pays)) + 64 + 255) // 256 * 256
            slots = np.full((n, stride_in), FILL, np.uint8)
            for i, p in enumerate(pays):
                slots[i, :len(p)] = np.frombuffer(p, np.uint8)
            d_in = torch.from_numpy(slots.reshape(-1)).to(DEV)
            d_lin = torch.tensor([len(p) for p in pays], dtype=torch.int64, device=DEV)
            vbr = ns * (case.prefix + 4 + 3 * 255 * case.scalar)
            stride_out = (max(hip.max_payload_bytes(fmt, cp), vbr) + 64 + 255) // 256 * 256
            d_out = torch.full((n * stride_out,), FILL, dtype=torch.uint8, device=DEV)
            d_len = torch.zeros(n, dtype=torch.int64, device=DEV)
            d_q = torch.full((n * ns,), -1, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()

            def got():
                lens, pay = d_len.cpu().tolist(), d_out.cpu().numpy().reshape(n, stride_out)
                return [pay[i, :lens[i]].tobytes() for i in range(n)], d_q.cpu().numpy().reshape(n, ns), lens

            hip.transcode_batch_dev(d_in.data_ptr(), stride_in, d_lin.data_ptr(), n, fmt, cp, vc2hip_py.transcode_params(t),
                                    d_out.data_ptr(), stride_out, d_len.data_ptr(), d_q.data_ptr())
            hip.sync()
            pay, q, lens = got()
            assert lens == [len(f) for f in fixed], (tag, "d_lens_out")
            assert pay == fixed, (tag, "transcode")
            assert all((q[i] == pics[i].indices(t).ravel()).all() for i in range(n)), (tag, "d_qidx")
            # the capped form, whose measure kernel holds tc_quant_c: the cap is picture 0's length at t, so the smallest
            # index that fits is found among lengths measured with the transcoder's own quantiser
            hip.transcode_batch_dev(d_in.data_ptr(), stride_in, d_lin.data_ptr(), n, fmt, cp, vc2hip_py.transcode_params(0, cap),
                                    d_out.data_ptr(), stride_out, d_len.data_ptr(), d_q.data_ptr())
            hip.sync()
            pay, q, lens = got()
            assert all((q[i] == pics[i].indices(chosen[i]).ravel()).all() for i in range(n)), (tag, "capped d_qidx", chosen)
            assert pay == [p.transcode(c) for p, c in zip(pics, chosen)], (tag, "capped transcode", chosen)
            _, cp_out = _cp(hip, case, mode="HQ_CBR", s=s_out)
            hip.transcode_cbr_batch_dev(d_in.data_ptr(), stride_in, d_lin.data_ptr(), n, fmt, cp, cp_out, d_out.data_ptr(), stride_out,
                                        d_len.data_ptr(), d_q.data_ptr())
            hip.sync()
            pay, q, lens = got()
            assert lens == [len(o.payload) for o in outs], (tag, "HQ_CBR d_lens_out")
            assert pay == [o.payload for o in outs], (tag, "transcode to HQ_CBR")
            assert all((q[i] == outs[i].q.ravel()).all() for i in range(n)), (tag, "HQ_CBR d_qidx")
        finally:
            hip.set_quant_matrix(None)


# ---------------------------------------------------------------------------------------------------------------------
# copies 4 and 9 and the LD search: budgets that the longer code just overflows
# ---------------------------------------------------------------------------------------------------------------------
def _searches(hip, call):
    hip.profile_reset()
    hip.profile_enable(True)
    try:
        res = call()
    finally:
        hip.profile_enable(False)
    return res, hip.profile().get("cbr_search", (0, 0.0))[0]


def test_cbr_qindices_on_the_tight_sheets(variants, oracle):
    """512 slices, each tight on a boundary 2^K - 1 at its own index (tests/test_quant_ref.py): the register kernel on int32
    planes (float form; two launches: it and the pass over what it marked), the general kernel alone under CBR_GENERAL (the
    integer form, eight at a time; one launch) and the int32 store"""
    g, planes, qm, sb, spec = qr.search_planes()
    want = oracle.cbr_qindices(*planes, g.depth, qm, sb, 1)
    for vname, launches in (("default", 2), ("cbr_general", 1), ("store32", 2)):
        hip = variants[vname]
        got, n = _searches(hip, lambda: hip.cbr_qindices(*planes, g.depth, qm, sb, 1))
        assert n == launches, (vname, n)
        bad = np.flatnonzero((got != want).ravel())
        assert bad.size == 0, (vname, bad.size, [(int(s), spec[s], int(got.ravel()[s]), int(want.ravel()[s])) for s in bad[:6]])


def test_hq_cbr_picture_on_p16(variants, oracle):
    """a designed P16 picture under HQ_CBR (k_cbr_search16 on the 16-bit store, the general kernel, the register kernel on the
    int32 store): payload and indices against oracle.encode_stream"""
    import cbr_ref as cr
    d = qr.design(oracle, "P16", 24)
    g = d.geom
    s_total = 1024 * 28 + 333          # 28 bytes a slice: the designed slices end at 50 different indices, 13 .. 68
    p = make_params(g.w, g.h, g.cf, g.bits, g.wavelet, g.depth, g.u, g.a, mode="HQ_CBR", s=s_total, scalar=2)
    stream = oracle.encode_stream(p, d.raw, 1)
    geo = g.geometry(oracle)
    sb = oracle.slice_bytes(geo.ys, geo.xs, s_total, 2)
    want = stream[-13 - int(sb.sum()):-13]
    widx = cr.payload_indices(want, sb, 0)
    assert len(set(widx.tolist())) > 8
    case = g.case(oracle, 24, 2)
    for vname, (bits, launches) in (("default", (16, 2)), ("cbr_general", (16, 1)), ("store32", (32, 2))):
        hip = variants[vname]
        fmt, cp = _cp(hip, case, mode="HQ_CBR", s=s_total)
        (payload, qidx), n = _searches(hip, lambda: hip.encode_picture_hq(d.raw, fmt, cp))
        assert _store_bits(hip) == {bits} and n == launches, (vname, _store_bits(hip), n)
        assert np.array_equal(qidx.ravel(), widx), (vname, _first_diff(qidx, widx))
        assert payload == want, vname


def test_hq_capped_batch_on_p16(variants, oracle):
    """three designed P16 pictures under a cap that picture 0 meets exactly at its sixth index from the floor and misses by
    bytes one index lower: a length measured one code too long or too short moves its index.  Expected: the definition
    that looks at every index (qmatrix_ref.encode_capped with the wavelet's own matrix -- tests/test_qmatrix_ref.py holds it
    equal to cap_ref's model)"""
    torch = _torch()
    floor = 20
    ds = [qr.design(oracle, "P16", 24), qr.design(oracle, "P16", 18), qr.build_design(oracle, qr.P16, 24, seed=5024)]
    case = qr.P16.case(oracle, floor, SCALAR)
    qm = oracle.quant_matrix(KERNELS[case.kernel], case.depth)
    lens = [len(qmr.encode(oracle, pr_case, ds[0].raw, qm)[0]) for pr_case in (qr.P16.case(oracle, q, SCALAR) for q in range(floor, floor + 6))]
    cap = lens[5]
    assert lens[4] > cap and lens[0] > lens[5]
    want = [qmr.encode_capped(oracle, case, d.raw, qm, floor, cap) for d in ds]
    assert want[0][1] == floor + 5 and len(want[0][0]) == cap
    ns = case.ys * case.xs
    for vname in ("default", "cap_general", "store32"):
        hip = variants[vname]
        fmt, cp = _cp(hip, case, mode="HQ_Capped", s=cap)
        bt = Batch(hip, fmt, cp, [d.raw for d in ds])
        d_q = torch.full((3 * ns,), -1, dtype=torch.int32, device=DEV)
        hip.profile_reset()
        hip.profile_enable(True)
        hip.encode_recon_batch_dev(bt.d_raw.data_ptr(), 3, fmt, cp, bt.d_pay.data_ptr(), bt.stride, bt.d_len.data_ptr(), None, None, d_q.data_ptr())
        hip.sync()
        hip.profile_enable(False)
        seen = {k for k, v in hip.profile().items() if v[0] > 0}
        assert "cap_pick" in seen, (vname, seen)
        assert d_q.cpu().numpy().reshape(3, ns)[:, 0].tolist() == [t for _, t in want], (vname, "indices")
        assert bt.payloads() == [p for p, _ in want], (vname, "payloads")


@pytest.mark.parametrize("geom", list(qr.LD_GEOMS))
def test_ld_qindices_at_tight_budgets(hip, oracle, geom):
    """the LD search (the fast kernels' ld_diag_body::eval; the general kernel) at the least budget that holds each slice's
    designed index and one byte below it; every eighth slice climbs to 116, where the small values of a subband with matrix
    entry 0 meet the wrapped factors and must quantise to 0"""
    depth, ys, xs, lshape, cshape, fast = qr.LD_GEOMS[geom]
    qm = oracle.quant_matrix(KERNELS["LeGall"], depth)
    planes, spec = qr.ld_search_planes(geom)
    budgets, at, below = qr.ld_tight_budgets(oracle, geom, planes, spec)
    for name, sb, want in (("tight", budgets, at), ("one byte less", (budgets - 1).astype(np.int32), below)):
        got = hip.ld_qindices(*planes, depth, qm, sb)
        bad = np.flatnonzero((got != want).ravel())
        assert bad.size == 0, (geom, name, [(int(s), spec[s], int(got.ravel()[s]), int(want.ravel()[s])) for s in bad[:6]])
