"""GPU tests of the HQ slice writer k_hq_pack at the edges of its own bit strings, exactly: the designed coefficients of
tests/writer_ref.py through vc2hip_hq_pack (planes that are quantised already: load8<false> and codes8) on the eight
geometries that reach its forms -- four, two and one slice a wavefront, one round, rounds with a short last one, two and
five rounds -- at the scalars 1, 2, 3, 7 and, on one small geometry, at the scalars on both sides of every change of lanes
and of image mode; VBR through the slots, VBR in one pass (SINGLE_PASS_VBR: k_hq_pack's own look-back) and HQ_CBR.
Three of the generators also run as pictures through vc2hip_encode_batch_dev: k_hq_pack's quantising loads and the 16-bit
store's k_hq_pack16 and k_hq_pack16w (at the end of this file).

Expected payloads are oracle.hq_pack's; tests/test_writer_ref.py shows on the CPU that the oracle writes exactly what the
definition writer_ref.plain does on every one of these inputs, and what each input reaches.  Every comparison is exact, every
refusal is matched to the reference's words and the library's code.  The call copies exactly the payload's length to the
host, so a byte beyond it would show only as a wrong length; the host buffer is filled with 0xA5 all the same and asserted
untouched behind the length.

Which instantiation of k_hq_pack ran is not recorded by the library: that rests on writer_ref.pack_form, the launcher's rule
restated.  The profile does say whether a call went through the slots (slice_compact) or not."""
import ctypes as C

import numpy as np
import pytest

import writer_ref as wr
from vc2lib import OracleError

pytestmark = pytest.mark.gpu

FILL = 0xA5
SMALL_SCALARS = ((0, 1), (1, 2), (2, 3), (3, 7))        # (prefix, scalar): every byte phase of the first data bit
LARGE_SCALARS = tuple(s for pair in wr.lane_scalars(wr.GEOS[wr.SMALL]) + wr.mode_scalars() for s in pair)


@pytest.fixture(scope="module")
def variants():
    from vc2hip_py import FLAGS, Vc2Hip
    v = {"slots": Vc2Hip(), "onepass": Vc2Hip(flags=FLAGS["SINGLE_PASS_VBR"])}
    yield v
    for h in v.values():
        h.close()


def _pack(hip, planes, geo, qidx, prefix, scalar, budgets=None):
    """vc2hip_hq_pack into a buffer of 0xA5: the payload, with the bytes behind it asserted untouched"""
    y, u, v = planes
    ns = qidx.size
    g = hip.geom(y, u, geo.depth, geo.ys, geo.xs)
    cap = ns * (prefix + 4 + 3 * 255 * scalar) + 64
    cbr_p = None
    if budgets is not None:
        budgets = np.ascontiguousarray(budgets, np.int32)
        cap = int(budgets.sum()) + ns * prefix + 64
        cbr_p = budgets.ctypes.data_as(C.c_void_p)
    out = np.full(cap + 256, FILL, np.uint8)
    n = C.c_size_t()
    hip._chk(hip.lib.vc2hip_hq_pack(hip.h, y, u, v, C.byref(g), qidx, prefix, scalar, cbr_p, out, cap, C.byref(n)))
    assert (out[n.value:] == FILL).all()
    return out[:n.value].tobytes()


def _first_diff(a, b):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return k, a[k:k + 4].hex(), b[k:k + 4].hex()


def _check(variants, oracle, inp, prefix, scalar, forms):
    """one input on the given forms (slots, onepass: VBR; cbr: under its budgets): payloads or refusals as the oracle's"""
    from vc2hip_py import Vc2HipError
    geo = inp.geo
    planes = wr.planes(geo, inp.recs)
    qidx = np.ascontiguousarray(inp.qidx.reshape(geo.ys, geo.xs))
    for form in forms:
        hip = variants["onepass" if form == "onepass" else "slots"]
        budgets = None if form != "cbr" else inp.budgets.reshape(geo.ys, geo.xs)
        tag = (geo.name, inp.gen, inp.tag, prefix, scalar, form)
        if inp.refused:
            words, code = wr.REFUSALS[inp.refused]
            with pytest.raises(OracleError, match=words):
                oracle.hq_pack(*planes, geo.depth, qidx, prefix, scalar, cbr=budgets)
            with pytest.raises(Vc2HipError, match=words) as e:
                _pack(hip, planes, geo, qidx, prefix, scalar, budgets)
            assert e.value.code == code, tag
            continue
        want = oracle.hq_pack(*planes, geo.depth, qidx, prefix, scalar, cbr=budgets).tobytes()
        got = _pack(hip, planes, geo, qidx, prefix, scalar, budgets)
        assert len(got) == len(want) and got == want, (tag, len(got), len(want), "first difference at, got, want", _first_diff(got, want))


def _forms(inp):
    return ("cbr",) if inp.budgets is not None else ("slots", "onepass")


@pytest.mark.parametrize("prefix,scalar", SMALL_SCALARS)
@pytest.mark.parametrize("gen", list(wr.GENERATORS))
@pytest.mark.parametrize("gname", list(wr.GEOS))
def test_designed_inputs(variants, oracle, gname, gen, prefix, scalar):
    """every designed input of a generator on a geometry: VBR through the slots and in one pass, the inputs of `cbr` under
    their budgets; the accepted VBR inputs of `last`, `units`, `tiles` and `random` once more under HQ_CBR with seeded remainders"""
    ins = wr.inputs(gen, gname, prefix, scalar)
    assert ins
    for inp in ins:
        _check(variants, oracle, inp, prefix, scalar, _forms(inp))
        if gen in ("last", "units", "tiles", "random") and not inp.refused:
            _check(variants, oracle, wr.with_budgets(inp, scalar), prefix, scalar, ("cbr",))


@pytest.mark.parametrize("scalar", LARGE_SCALARS)
def test_large_scalars(variants, oracle, scalar):
    """the scalars on both sides of every change of form on the small geometry: the lanes a slice (four slices a wavefront,
    two, one), then four, two and one wavefront a workgroup and the slice images in global memory"""
    for gen in wr.LARGE_GENERATORS:
        for inp in wr.inputs(gen, wr.SMALL, 1, scalar):
            _check(variants, oracle, inp, 1, scalar, _forms(inp))
            if gen in ("last", "random") and not inp.refused:
                _check(variants, oracle, wr.with_budgets(inp, scalar), 1, scalar, ("cbr",))


def test_the_profile_says_slots_or_not(variants, oracle):
    """what the library records of the form: slice_compact runs for VBR through the slots, not in one pass and not under
    HQ_CBR; from the first scalar of image mode 2 on the one-pass context goes through the slots too, and from the first of
    mode -1 on HQ_CBR does"""
    (_, m2), _, (_, gimg) = wr.mode_scalars()
    rows = [("slots", 1, False, True), ("onepass", 1, False, False), ("slots", 1, True, False),
            ("onepass", m2, False, True), ("slots", gimg, True, True)]
    for ctx, scalar, cbr, slots in rows:
        hip = variants[ctx]
        one = wr.inputs("random", wr.SMALL, 0, scalar)[0]
        one = wr.with_budgets(one, scalar) if cbr else one
        hip.profile_reset()
        hip.profile_enable(True)
        try:
            _check({"slots": hip, "onepass": hip}, oracle, one, 0, scalar, ("cbr",) if cbr else ("slots",))
        finally:
            hip.profile_enable(False)
        seen = {k for k, v in hip.profile().items() if v[0] > 0}
        assert "hq_pack" in seen and ("slice_compact" in seen) == slots, (ctx, scalar, cbr, seen)


def test_the_longest_slice_under_cbr(variants, oracle):
    """Y, U and V at 255 units each and a remainder in V's room: 4 + 3 * 255 * scalar + scalar - 1 bytes, the longest slice the
    reference writes.  Five rounds of luma hold 255 units up to a scalar of 36, three rounds of chroma up to 18"""
    ins = [i for i in wr.inputs("cbr", "r2304", 0, 16) if i.tag.startswith("longest")]
    assert [i.tag for i in ins] == ["longest", "longest_dense"] and all(int(i.budgets.max()) == 4 + 3 * 255 * 16 + 15 for i in ins)
    for inp in wr.inputs("cbr", "r2304", 0, 16):
        _check(variants, oracle, inp, 0, 16, ("cbr",))


def test_the_longest_slice_with_the_images_in_global_memory(variants, oracle):
    """the same at the first scalar whose slice images live in the slots: two slices of 3 x 16384 coefficients, the second
    with the remainder; the slot holds the remainder's bytes and they are zeros, not the next slot's head"""
    gimg = wr.mode_scalars()[2][1]
    inp = wr.longest(wr.HUGE, gimg)
    assert wr.pack_form(wr.HUGE, 0, gimg, cbr=True).gimg and inp.budgets.tolist() == [4 + 765 * gimg, 4 + 765 * gimg + gimg - 1]
    _check(variants, oracle, inp, 0, gimg, ("cbr",))
    _check(variants, oracle, wr.longest(wr.HUGE, gimg, dense=True), 0, gimg, ("cbr",))


# ---------------------------------------------------------------------------------------------------------------------
# the quantising path: the same designs as pictures through vc2hip_encode_batch_dev
# ---------------------------------------------------------------------------------------------------------------------
# which pictures a geometry of tests/quant_ref.py takes (the oracle needs a second for a P16W picture), on which contexts, and
# what the library's records must say there: (store bits, slots behind the coder)
BATCH = {"S16": (("strings", "last", "random"), None, {"slots": (32, True)}),
         "M1024": (("strings", "last", "random"), None, {"slots": (32, True)}),
         "M2048": (("strings", "last", "random"), None, {"slots": (32, True)}),
         "P32": (("strings", "last", "random"), None, {"slots": (32, True)}),
         "P16": (("strings", "last", "random", "last16"), None, {"slots": (16, True), "onepass": (16, False)}),
         "P16W": (("strings", "random", "last16"), ("A63.0", "A64.0", "A65.0", "r0", "r1", "h0", "h1", "h2"), {"slots": (16, True)})}


def _torch():
    import torch
    return torch


CBR_BYTES = 1000            # a slice under HQ_CBR: every designed slice fits at index 0, so the search stays there


@pytest.mark.parametrize("name,gen,mode", [(n, g, "HQ_ConstQ") for n, (gens, _, _) in BATCH.items() for g in gens]
                         + [(n, "strings", "HQ_CBR") for n in ("P32", "P16", "P16W")])
def test_designed_pictures_through_the_batch_encoder(variants, oracle, name, gen, mode):
    """k_hq_pack's quantising loads (P32: load8_tab on the int32 store) and the 16-bit store's k_hq_pack16 (P16: slots and
    one pass) and k_hq_pack16w (P16W) on designed strings, last places and random fields: Haar0 pictures whose transform is
    the designed field (asserted), a flat matrix and index 0, three pictures a call.  S16: four slices a wavefront and shared
    slots on the quantising path; M1024, M2048: the MID form, two rounds in registers and the bits8_tab measuring pass.
    HQ_CBR (k_hq_pack's, k_hq_pack16<P16_CBR>, k_hq_pack16w<true>): 1000 bytes a slice, where the search keeps index 0 (the
    payload's index bytes say so).  Expected payloads are the oracle's composition (tests/qmatrix_ref.py); the slots are 0xA5
    behind their lengths inside a larger allocation"""
    import proxy_ref as pr
    import qmatrix_ref as qmr
    import vc2hip_py
    torch = _torch()
    _, tags, contexts = BATCH[name]
    pg = wr.BATCH_GEOMS[name]
    case = pg.case(oracle, 0, wr.BATCH_SCALAR)
    if mode == "HQ_CBR":
        case = pr.Case(oracle, pg.w, pg.h, pg.cf, pg.bits, pg.wavelet, pg.depth, pg.u, pg.a, mode="HQ_CBR", s=case.ys * case.xs * CBR_BYTES,
                       scalar=wr.BATCH_SCALAR)
        contexts = {"slots": (contexts["slots"][0], False)}
    raws, pays = [], []
    for inp in wr.batch_inputs(oracle, name, (gen,)):
        if tags and inp.tag not in tags:
            continue
        raw, d = wr.batch_picture(oracle, name, inp)
        if raw is None:
            continue
        raws.append(raw)
        pay, qi = qmr.encode(oracle, case, raw, d.qm)
        assert (qi == 0).all()
        pays.append(pay)
    assert len(raws) >= 2 and len(set(pays)) == len(pays)
    for ctx, (bits, slots) in contexts.items():
        hip = variants[ctx]
        fmt = vc2hip_py.picture_format(case.w, case.h, case.cf, case.bits, case.word_bytes)
        cp = vc2hip_py.coding_params(hip.lib, fmt, case.kernel, case.depth, case.u, case.a, mode=case.mode, q=0, s=case.s, prefix=case.prefix, scalar=case.scalar)
        stride = (hip.max_payload_bytes(fmt, cp) + 64 + 255) // 256 * 256
        hip.set_quant_matrix(np.zeros(3 * case.depth + 1, np.int32))
        try:
            for at in range(0, len(raws), 3):
                part, want = raws[at:at + 3], pays[at:at + 3]
                n = len(part)
                d_raw = torch.frombuffer(bytearray(b"".join(part) + bytes(64)), dtype=torch.uint8).to("cuda:0")
                d_pay = torch.full((n * stride + 4096,), FILL, dtype=torch.uint8, device="cuda:0")
                d_len = torch.full((n + 8,), -1, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                hip.profile_reset()
                hip.profile_enable(True)
                hip.encode_batch_dev(d_raw.data_ptr(), n, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
                hip.sync()
                hip.profile_enable(False)
                tag = (name, gen, mode, ctx, at)
                assert {r["store_bits"] for r in hip.dwt_launches() if not r["inverse"]} == {bits}, tag
                seen = {k for k, v in hip.profile().items() if v[0] > 0}
                assert "hq_pack" in seen and ("slice_compact" in seen) == slots, (tag, seen)
                lens = d_len.cpu().tolist()
                assert lens[:n] == [len(p) for p in want] and lens[n:] == [-1] * 8, (tag, lens)      # (the words behind d_lens untouched)
                got = d_pay.cpu().numpy()
                for i in range(n):
                    slot = got[i * stride:(i + 1) * stride]
                    assert slot[:lens[i]].tobytes() == want[i], (tag, i, _first_diff(slot[:lens[i]].tobytes(), want[i]))
                    assert (slot[lens[i]:] == FILL).all(), (tag, i, "bytes behind the payload's length")
                assert (got[n * stride:] == FILL).all(), tag
        finally:
            hip.set_quant_matrix(None)


@pytest.mark.parametrize("name", list(BATCH))
def test_a_designed_picture_under_the_default_matrix(variants, oracle, name):
    """the first `strings` picture of every geometry without a matrix of the context's: the payload is oracle.encode_stream's"""
    import vc2hip_py
    from vc2lib import make_params
    pg = wr.BATCH_GEOMS[name]
    raw, _ = wr.batch_picture(oracle, name, wr.batch_inputs(oracle, name, ("strings",))[0])
    p = make_params(pg.w, pg.h, pg.cf, pg.bits, pg.wavelet, pg.depth, pg.u, pg.a, q=0, scalar=wr.BATCH_SCALAR)
    stream = oracle.encode_stream(p, raw, 1)
    case = pg.case(oracle, 0, wr.BATCH_SCALAR)
    for ctx in BATCH[name][2]:
        hip = variants[ctx]
        fmt = vc2hip_py.picture_format(case.w, case.h, case.cf, case.bits, case.word_bytes)
        cp = vc2hip_py.coding_params(hip.lib, fmt, case.kernel, case.depth, case.u, case.a, mode=case.mode, q=0, s=case.s, prefix=case.prefix, scalar=case.scalar)
        payload, _ = hip.encode_picture_hq(raw, fmt, cp)
        assert len(payload) > 1000 and payload == stream[-13 - len(payload):-13], (name, ctx)
