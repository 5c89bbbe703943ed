"""GPU tests of vc2hip_transcode_cbr_batch_dev (include/vc2hip.h): every payload, length and index
against the CPU definition tests/transcode_cbr_ref.py, which stands on the oracle's slice reader, dequantiser, HQ_CBR search,
quantiser and CBR slice writer.  The inputs are the rows of tests/transcode_ref.py (coded by oracle primitives), the budgets
those of transcode_cbr_ref.budgets; tests/test_transcode_cbr_ref.py shows on the CPU that they exercise both kinds of slice.

Every output is pre-filled, and lies between guards that must come back unchanged (test_gpu_transcode.Slots)."""
import ctypes as C

import numpy as np
import pytest

import damage as dm
import proxy_ref as pr
import recon_ref as rr
import transcode_cbr_ref as tc
import transcode_ref as tr
from test_gpu_cap import VARIANTS, slice_indices
from test_gpu_damaged import _pick
from test_gpu_transcode import DEV, FILL, GUARD, Slots, _ctx, _tp, _torch
from vc2lib import KERNELS, OracleError

pytestmark = pytest.mark.gpu

EINVAL, ECAP = -1, -9
ROWS = ("A", "C", "D", "E", "G", "H", "I")
BUDGETS = ("mixed", "roomy", "tight")
CODES = (tr.ESTREAM, tr.EQINDEX, tr.ESCALAR, tr.ECODE32, tc.ECBR_TOOBIG, tc.ECBR_LEN)


@pytest.fixture(scope="module")
def hip():
    h = _ctx()
    yield h
    h.close()


def cp_out_of(hip, case, s_out, prefix=None, scalar=None):
    import vc2hip_py
    fmt = vc2hip_py.picture_format(case.w, case.h, case.cf, case.bits, case.word_bytes)
    return vc2hip_py.coding_params(hip.lib, fmt, case.kernel, case.depth, case.u, case.a, mode="HQ_CBR", s=s_out,
                                   prefix=case.prefix if prefix is None else prefix, scalar=case.scalar if scalar is None else scalar)


def total_bytes(oracle, case, cp_out):
    ns = case.ys * case.xs
    return int(oracle.slice_bytes(case.ys, case.xs, cp_out.compressed_bytes, cp_out.scalar).sum()) + ns * cp_out.prefix


class CbrSlots(Slots):
    """test_gpu_transcode.Slots with the output slots sized for cp_out's budgets, and the HQ_CBR call"""

    def __init__(self, hip, oracle, case, payloads, cp_out, **kw):
        self.cp_out = cp_out
        self.total = total_bytes(oracle, case, cp_out)
        super().__init__(hip, case, payloads, **kw)
        self.stride_out = (self.total + 64 + 255) // 256 * 256
        self.fresh()

    def call(self, tp=None, hip=None, n=None):
        (hip or self.hip).transcode_cbr_batch_dev(self.d_in.data_ptr(), self.stride_in, self.d_len_in.data_ptr(), n or self.n, self.fmt,
                                                  self.cp, self.cp_out, self.out_ptr, self.stride_out, self.len_ptr, self.q_ptr)

    def run(self, tp=None, hip=None):
        return super().run(tp, hip)


def wanted(oracle, pics, cp_out):
    return [tc.transcode_cbr(oracle, p, cp_out.compressed_bytes, cp_out.prefix, cp_out.scalar) for p in pics]


def check(slots, oracle, pics, tag, only=None):
    got, lens, q = slots.results()
    cp = slots.cp_out
    for i, want in enumerate(wanted(oracle, pics, cp)):
        if only is not None and i not in only:
            continue
        assert not isinstance(want, OracleError), (tag, i, "the definition refuses", want.code)
        assert lens[i] == want.total == slots.total, (tag, i, "length", lens[i], want.total)
        assert (q[i] == want.q.ravel()).all(), (tag, i, "d_qidx")
        assert slice_indices(got[i], slots.ns, cp.prefix, cp.scalar) == q[i].tolist(), (tag, i, "index bytes")
        assert got[i] == want.payload, (tag, i, "payload")


def sync_code(hip):
    import vc2hip_py
    try:
        hip.sync()
    except vc2hip_py.Vc2HipError as e:
        return e.code
    return 0


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the rows at three budgets; a changed prefix and scalar
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", ROWS)
def test_rows_at_three_budgets(hip, oracle, name, budget):
    case, pics = tr.batch(oracle, name)
    cp_out = cp_out_of(hip, case, tc.budgets(oracle, name)[budget])
    slots = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out)
    if (name, budget) == ("I", "roomy"):      # the designed refusal: every slice kept, V's padding passes 255 * scalar
        slots.call()
        assert sync_code(hip) == tc.ECBR_LEN
        assert slots.guards_intact()
        return
    check(slots.run(), oracle, pics, (name, budget))


@pytest.mark.parametrize("name", tc.ROWS_CHANGED)
def test_changed_prefix_and_scalar(hip, oracle, name):
    case, pics = tr.batch(oracle, name)
    prefix, scalar = tc.changed(case)
    cp_out = cp_out_of(hip, case, tc.budgets(oracle, name, scalar)["mixed"], prefix, scalar)
    slots = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out)
    check(slots.run(), oracle, pics, (name, "prefix + 1, scalar x 2"))


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4: stability across generations
# ---------------------------------------------------------------------------------------------------------------------
def test_hq_cbr_input_comes_back_from_its_own_cp(hip, oracle):
    case, pics = tr.batch(oracle, "E")
    slots = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out_of(hip, case, case.s)).run()
    got, lens, q = slots.results()
    assert got == [p.payload for p in pics]
    assert all((q[i] == p.q.ravel()).all() for i, p in enumerate(pics))
    check(slots, oracle, pics, "E to its own cp")


@pytest.mark.parametrize("name,change", [("A", False), ("E", False), ("C", True)])
def test_the_output_fed_to_the_call_again(hip, oracle, name, change):
    case, pics = tr.batch(oracle, name)
    prefix, scalar = tc.changed(case) if change else (case.prefix, case.scalar)
    s_out = tc.budgets(oracle, name, scalar)["mixed"]
    cp_out = cp_out_of(hip, case, s_out, prefix, scalar)
    first = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out).run()
    check(first, oracle, pics, (name, "first generation"))
    out = first.results()[0]
    case2 = pr.Case(oracle, case.w, case.h, case.cf, case.bits, case.kernel, case.depth, case.u, case.a, mode="HQ_CBR", s=s_out,
                    scalar=scalar, prefix=prefix, word_bytes=case.word_bytes)
    second = CbrSlots(hip, oracle, case2, out, cp_out).run()
    got, lens, q = second.results()
    assert got == out, (name, "the second generation differs")
    assert (q == first.results()[2]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5: the decoder on the output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "E"])
def test_decoder_shows_the_definitions_picture(hip, oracle, name):
    torch = _torch()
    case, pics = tr.batch(oracle, name)
    s_out = tc.budgets(oracle, name)["mixed"]
    cp_out = cp_out_of(hip, case, s_out)
    slots = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out).run()
    check(slots, oracle, pics, (name, "decode"))
    rb = case.raw_bytes()
    out = torch.full((3 * rb + 16,), FILL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    hip.decode_batch_dev(slots.out_ptr, slots.stride_out, slots.len_ptr, 3, slots.fmt, cp_out, out.data_ptr())
    hip.sync()
    got = out.cpu().numpy()
    cbr = pr.Case(oracle, case.w, case.h, case.cf, case.bits, case.kernel, case.depth, case.u, case.a, mode="HQ_CBR", s=s_out,
                  scalar=case.scalar, prefix=case.prefix, word_bytes=case.word_bytes)
    for i, want in enumerate(wanted(oracle, pics, cp_out)):
        assert got[i * rb:(i + 1) * rb].tobytes() == pr.full_picture(oracle, cbr, want.payload), (name, i)
    assert (got[3 * rb:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6: the profile
# ---------------------------------------------------------------------------------------------------------------------
def test_profile_holds_no_transform(oracle):
    case, pics = tr.batch(oracle, "A")
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    pic = hip.decode_picture(pics[0].payload, fmt, cp)        # a call that runs a transform
    assert pic == pr.full_picture(oracle, case, pics[0].payload)
    before = hip.dwt_launches()
    assert before
    slots = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out_of(hip, case, tc.budgets(oracle, "A")["mixed"]))
    hip.profile_reset()
    hip.profile_enable(True)
    slots.run()
    hip.profile_enable(False)
    prof = hip.profile()
    for stage in ("hq_unpack", "transcode_fit", "hq_pack"):
        assert prof[stage][0] == 1, (stage, prof)
    assert prof["cbr_search"][0] in (1, 2), prof      # (the register kernel and the general one behind it, or the general one alone)
    allowed = ("slice_index_", "cbr_index", "transcode_", "hq_unpack", "cbr_search", "hq_pack", "slice_offsets_scan", "slice_compact", "fill")
    others = [k for k in prof if not k.startswith(allowed)]
    assert not others, prof
    assert hip.dwt_launches() == before, "the call before's launch record changed"
    check(slots, oracle, pics, "profiled")
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7: HQ_CBR in, HQ_CBR out at a smaller budget -- two budget tables in one call
# ---------------------------------------------------------------------------------------------------------------------
def _smaller_budget(oracle):
    return tc.budgets(oracle, "E")["mixed"]


def test_two_tables_eager(hip, oracle):
    case, pics = tr.batch(oracle, "E")
    s_out = _smaller_budget(oracle)
    assert s_out < case.s
    slots = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out_of(hip, case, s_out))
    for k in range(3):      # (the second and third call find both tables warm)
        check(slots.fresh().run(), oracle, pics, ("E smaller", k))


def test_two_tables_on_a_callers_stream_and_under_capture(oracle):
    """a warm-up, then: the call returns while a filler still runs in front of it (no wait, though it holds two budget tables);
    captured once and replayed on other inputs"""
    from test_gpu_caller_stream import Filler, _capture
    torch = _torch()
    case, pics = tr.batch(oracle, "E")
    s_out = _smaller_budget(oracle)
    orders = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    s = torch.cuda.Stream()
    for lanes in (1, 2):
        hip = _ctx(stream=s.cuda_stream, lanes=lanes)
        cp_out = cp_out_of(hip, case, s_out)
        with torch.cuda.stream(s):
            a = CbrSlots(hip, oracle, case, [pics[k].payload for k in orders[0]], cp_out)
            ins = []
            for o in orders:
                x = Slots(hip, case, [pics[k].payload for k in o], stride_in=a.stride_in)
                ins.append((x.d_in.cpu().pin_memory(), x.d_len_in.cpu().pin_memory()))

            def load(r):
                a.d_in.copy_(ins[r][0], non_blocking=True)
                a.d_len_in.copy_(ins[r][1], non_blocking=True)

            def snapshot():
                return (a.buf.clone(), a.len_buf.clone(), a.q_buf.clone())

            def check_snap(snap, r, tag):
                y = CbrSlots.__new__(CbrSlots)
                y.__dict__.update(a.__dict__)
                y.buf, y.len_buf, y.q_buf = snap
                check(y, oracle, [pics[k] for k in orders[r]], (lanes, tag, r))

            a.call()                                    # the warm-up: both tables are uploaded here
            s.synchronize()
            hip.sync()
            check_snap(snapshot(), 0, "warm-up")
            load(1)
            s.synchronize()
            e_fill = Filler(s).run()
            a.call()
            e = torch.cuda.Event()
            e.record(s)
            waited, filler_done = e.query(), e_fill.query()
            snap = snapshot()
            s.synchronize()
            hip.sync()
            check_snap(snap, 1, "behind the filler")
            assert not waited and not filler_done, "the call waited for the stream"
        g, _ = _capture(torch, s, hip, a.call)          # (a call that does not return VC2HIP_OK raises)
        with torch.cuda.stream(s):
            snaps = {}
            for r in (2, 0):
                load(r)
                g.replay()
                snaps[r] = snapshot()
            s.synchronize()
            hip.sync()
        for r in (2, 0):
            check_snap(snaps[r], r, "replay")
        hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8: lanes, one picture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [2, 3])
def test_lanes_give_identical_bytes(hip, oracle, lanes):
    torch = _torch()
    for name in ("A", "E"):
        case, pics = tr.batch(oracle, name)
        order = [0, 1, 2, 1, 0]
        pays, ps = [pics[k].payload for k in order], [pics[k] for k in order]
        s_out = tc.budgets(oracle, name)["mixed"]
        one = CbrSlots(hip, oracle, case, pays, cp_out_of(hip, case, s_out)).run()
        hl = _ctx(lanes=lanes)
        two = CbrSlots(hl, oracle, case, pays, cp_out_of(hl, case, s_out)).run()
        check(two, oracle, ps, (name, lanes))
        assert one.results()[0] == two.results()[0] and torch.equal(one.q_buf, two.q_buf) and torch.equal(one.len_buf, two.len_buf)
        hl.close()


def test_one_picture(hip, oracle):
    case, pics = tr.batch(oracle, "A")
    cp_out = cp_out_of(hip, case, tc.budgets(oracle, "A")["mixed"])
    for k in (1, 2):
        check(CbrSlots(hip, oracle, case, [pics[k].payload], cp_out).run(), oracle, [pics[k]], ("n = 1", k))


# ---------------------------------------------------------------------------------------------------------------------
# 9: every context flag gives the same bytes; the 16-bit store
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS) + ["CBR_GENERAL", "NO_CBR_INDEX"])
def test_flags_give_the_same_bytes(oracle, variant):
    flags = VARIANTS.get(variant, (variant,))
    hip = _ctx(*flags)
    for name in (["E"] if variant == "NO_CBR_INDEX" else ["A", "E"]):
        case, pics = tr.batch(oracle, name)
        cp_out = cp_out_of(hip, case, tc.budgets(oracle, name)["mixed"])
        check(CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out).run(), oracle, pics, (variant, name))
    hip.close()


_WIDE = {}


def _store16_batch(oracle):
    """1024 x 128 LeGall depth 3, 32 x 16 slices: the smallest 4:2:2 picture the library keeps in its 16-bit store
    (tests/cap_ref.py); indices in a checkerboard of 6 and 30, the 16-bit noise picture's values escape the 16-bit elements
    once dequantised"""
    if not _WIDE:
        import cap_ref as cr
        case = pr.Case(oracle, 1024, 128, "422", 16, "LeGall", 3, 2, 4, q=6, scalar=8)
        qm = oracle.quant_matrix(KERNELS[case.kernel], case.depth)
        yy, xx = np.mgrid[0:case.ys, 0:case.xs]
        qi = np.where((yy + xx) % 2 == 0, 20, 34).astype(np.int32)
        pics = []
        for raw in cr.pictures(case):
            planes = rr.transform_planes(oracle, case, raw)
            y, u, v = (oracle.quantise_np(p, case.depth, qi, qm) for p in planes)
            pics.append(tr.Coded(oracle, case, oracle.hq_pack(y, u, v, case.depth, qi, case.prefix, case.scalar).tobytes()))
        _WIDE["b"] = (case, pics)
    return _WIDE["b"]


@pytest.mark.parametrize("variant", ["default", "store32"])
def test_the_16_bit_store(oracle, variant):
    case, pics = _store16_batch(oracle)
    ns = case.ys * case.xs
    s_out = tc.budget_mixed(case, pics, case.scalar)
    outs = [tc.transcode_cbr(oracle, p, s_out) for p in pics]
    assert not any(isinstance(o, OracleError) for o in outs), outs
    kept = int(outs[2].keep.sum())
    assert 4 * kept >= ns and 4 * (ns - kept) >= ns, (kept, ns)
    assert max(int(np.abs(d).max()) for p in pics for d in p.deq) > 32767, "no dequantised value leaves the 16-bit elements"
    hip = _ctx(*VARIANTS[variant])
    check(CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out_of(hip, case, s_out)).run(), oracle, pics, ("16-bit store", variant))
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10: mixing with the other calls on one context
# ---------------------------------------------------------------------------------------------------------------------
def test_mixed_with_decode_transcode_and_encode(oracle):
    torch = _torch()
    import cap_ref as cr
    case, pics = tr.batch(oracle, "A")
    hip = _ctx()
    rb = case.raw_bytes()
    want_pics = [pr.full_picture(oracle, case, p.payload) for p in pics]
    pays = [p.payload for p in pics]
    vbr = Slots(hip, case, pays)
    cbr = CbrSlots(hip, oracle, case, pays, cp_out_of(hip, case, tc.budgets(oracle, "A")["mixed"]))
    t = tr.mid_target(pics[0], tr.floor_of(pics))
    raws = cr.pictures(case)

    def decode():
        out = torch.full((3 * rb + 16,), FILL, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        hip.decode_batch_dev(vbr.d_in.data_ptr(), vbr.stride_in, vbr.d_len_in.data_ptr(), 3, vbr.fmt, vbr.cp, out.data_ptr())
        hip.sync()
        got = out.cpu().numpy()
        assert [got[i * rb:(i + 1) * rb].tobytes() for i in range(3)] == want_pics and (got[3 * rb:] == FILL).all()

    def transcode():
        from test_gpu_transcode import check_fixed
        check_fixed(vbr.fresh().run(_tp(t)), pics, t, "mixed: transcode")

    def encode():
        d_raw = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(DEV)
        d_pay = torch.full((3 * vbr.stride_out,), FILL, dtype=torch.uint8, device=DEV)
        d_len = torch.full((3,), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        hip.encode_batch_dev(d_raw.data_ptr(), 3, vbr.fmt, vbr.cp, d_pay.data_ptr(), vbr.stride_out, d_len.data_ptr())
        hip.sync()
        pay, lens = d_pay.cpu().numpy().reshape(3, -1), d_len.cpu().numpy()
        assert [pay[i, :int(lens[i])].tobytes() for i in range(3)] == pays      # (a ConstQ row: the input itself)

    decode()
    transcode()
    check(cbr.fresh().run(), oracle, pics, "mixed: first")
    encode()
    check(cbr.fresh().run(), oracle, pics, "mixed: behind the encoder")
    transcode()
    decode()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 11: the designed refusals at vc2hip_sync
# ---------------------------------------------------------------------------------------------------------------------
def test_refusal_of_the_cbr_writer(hip, oracle):
    """row I, roomy: every picture of the row is refused with ECBR_LEN; alone and in a batch"""
    case, pics = tr.batch(oracle, "I")
    cp_out = cp_out_of(hip, case, tc.budgets(oracle, "I")["roomy"])
    assert all(isinstance(w, OracleError) and w.code == tc.ECBR_LEN for w in wanted(oracle, pics, cp_out))
    for pays in ([pics[0].payload], [p.payload for p in pics]):
        slots = CbrSlots(hip, oracle, case, pays, cp_out)
        slots.call()
        assert sync_code(hip) == tc.ECBR_LEN
        assert slots.guards_intact()
    check(CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out_of(hip, case, tc.budgets(oracle, "I")["mixed"])).run(), oracle, pics,
          "the context after the refusal")


def test_refusal_of_the_search(hip, oracle):
    """row F, mixed: picture 1's one slice is refused by a search trial (ESCALAR); the other pictures of the batch are what
    the definition codes"""
    case, pics = tr.batch(oracle, "F")
    cp_out = cp_out_of(hip, case, tc.budgets(oracle, "F")["mixed"])
    want = wanted(oracle, pics, cp_out)
    assert isinstance(want[1], OracleError) and want[1].code == tr.ESCALAR
    coded = [i for i, w in enumerate(want) if not isinstance(w, OracleError)]
    assert coded, "no other picture of the batch is coded"
    slots = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out)
    slots.call()
    assert sync_code(hip) == tr.ESCALAR
    check(slots, oracle, pics, "F beside the refused picture", only=coded)


# ---------------------------------------------------------------------------------------------------------------------
# 12: refusals on the host
# ---------------------------------------------------------------------------------------------------------------------
def _raw_call(hip, a):
    return hip.lib.vc2hip_transcode_cbr_batch_dev(hip.h, a["in"], a["stride_in"], a["lens_in"], a["n"], a["fmt"], a["cp_in"], a["cp_out"],
                                                  a["out"], a["stride_out"], a["lens_out"], a["qidx"])


@pytest.mark.parametrize("lanes", [1, 3])
def test_refusals_launch_nothing_and_touch_nothing(oracle, lanes):
    import vc2hip_py
    case, pics = tr.batch(oracle, "A")
    hip = _ctx(lanes=lanes)
    cp_out = cp_out_of(hip, case, tc.budgets(oracle, "A")["mixed"])
    slots = CbrSlots(hip, oracle, case, [p.payload for p in pics], cp_out)
    check(slots.run(), oracle, pics, "before the refusals")
    slots.fresh()
    good = dict(stride_in=slots.stride_in, n=3, fmt=C.byref(slots.fmt), cp_in=C.byref(slots.cp), cp_out=C.byref(cp_out),
                stride_out=slots.stride_out, lens_in=slots.d_len_in.data_ptr(), lens_out=slots.len_ptr, qidx=slots.q_ptr, out=slots.out_ptr)
    good["in"] = slots.d_in.data_ptr()

    def cp_with(base, **kw):
        cp = type(base).from_buffer_copy(base)
        for k, v in kw.items():
            setattr(cp, k, v)
        return C.byref(cp)

    fmt_bad = type(slots.fmt).from_buffer_copy(slots.fmt)
    fmt_bad.width = 0
    ld = vc2hip_py.MODES["LD"]
    tries = {
        "fmt null": dict(fmt=None), "cp_in null": dict(cp_in=None), "cp_out null": dict(cp_out=None), "input null": {"in": None},
        "lens_in null": dict(lens_in=None), "output null": dict(out=None), "lens_out null": dict(lens_out=None),
        "n 0": dict(n=0), "n -1": dict(n=-1),
        "cp_in LD": dict(cp_in=cp_with(slots.cp, mode=ld, compressed_bytes=20000)), "cp_out LD": dict(cp_out=cp_with(cp_out, mode=ld)),
        "cp_in mode 7": dict(cp_in=cp_with(slots.cp, mode=7)),
        "cp_out ConstQ": dict(cp_out=cp_with(cp_out, mode=vc2hip_py.MODES["HQ_ConstQ"])),
        "cp_out Capped": dict(cp_out=cp_with(cp_out, mode=vc2hip_py.MODES["HQ_Capped"])),
        "cp_out kernel": dict(cp_out=cp_with(cp_out, kernel=(cp_out.kernel + 1) % 7)), "cp_out depth": dict(cp_out=cp_with(cp_out, depth=cp_out.depth - 1)),
        "cp_out y_slices": dict(cp_out=cp_with(cp_out, y_slices=cp_out.y_slices // 2)),
        "cp_out x_slices": dict(cp_out=cp_with(cp_out, x_slices=cp_out.x_slices // 2)),
        "cp_out bytes 0": dict(cp_out=cp_with(cp_out, compressed_bytes=0)), "cp_out bytes -1": dict(cp_out=cp_with(cp_out, compressed_bytes=-1)),
        "cp_out scalar 0": dict(cp_out=cp_with(cp_out, scalar=0)), "cp_out prefix -1": dict(cp_out=cp_with(cp_out, prefix=-1)),
        "input misaligned": {"in": good["in"] + 8}, "input stride misaligned": dict(stride_in=slots.stride_in + 8),
        "output misaligned": dict(out=good["out"] + 8), "output stride misaligned": dict(stride_out=slots.stride_out + 8),
        "lens_in misaligned": dict(lens_in=good["lens_in"] + 4), "lens_out misaligned": dict(lens_out=good["lens_out"] + 4),
        "qidx misaligned": dict(qidx=good["qidx"] + 2),
        "output on the input": dict(out=good["in"]), "output inside the input": dict(out=good["in"] + 2 * slots.stride_in),
        "output ends in the input": dict(out=good["in"] - slots.stride_out),
        "cp_in scalar 0": dict(cp_in=cp_with(slots.cp, scalar=0)), "cp_in prefix -1": dict(cp_in=cp_with(slots.cp, prefix=-1)),
        "depth 0": dict(cp_in=cp_with(slots.cp, depth=0), cp_out=cp_with(cp_out, depth=0)),
        "no slices": dict(cp_in=cp_with(slots.cp, y_slices=0), cp_out=cp_with(cp_out, y_slices=0)),
        "width 0": dict(fmt=C.byref(fmt_bad)),
        "kernel 9": dict(cp_in=cp_with(slots.cp, kernel=9), cp_out=cp_with(cp_out, kernel=9)),
    }
    for what, change in tries.items():
        rc = _raw_call(hip, {**good, **change})
        assert rc == EINVAL, (what, rc)
        hip.sync()
        assert slots.untouched(), what
    rc = _raw_call(hip, {**good, "stride_out": (slots.total - 1) // 16 * 16})
    assert rc == ECAP, rc
    hip.sync()
    assert slots.untouched()
    assert _raw_call(hip, {**good, "qidx": None}) == 0          # d_qidx is optional
    hip.sync()
    assert (slots.q_buf == -1).all()
    assert slots.results()[0] == [w.payload for w in wanted(oracle, pics, cp_out)]
    check(slots.fresh().run(), oracle, pics, "after the refusals")
    slots.stride_out = (slots.total + 15) // 16 * 16            # the budgets' sum is enough
    check(slots.fresh().run(), oracle, pics, "the budgets' sum as the stride")
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 13: damaged input
# ---------------------------------------------------------------------------------------------------------------------
REFUSED_PER_INPUT = 12


def _damaged_call(hip, oracle, case, muts, cp_out):
    slots = CbrSlots(hip, oracle, case, [m.data for m in muts], cp_out, lengths=[m.length for m in muts],
                     zero_tail=any(m.cls == "long" for m in muts))
    slots.call()
    return sync_code(hip), slots


@pytest.mark.parametrize("name", ["A", "B2"])
def test_damaged_input(oracle, name):
    base, _ = dm.load(oracle, name)
    case = base.case
    hip = _ctx()
    clean_m = dm.clean(base)
    clean = tc.Unpacked(oracle, case, base.payload)
    s_out = tc.budget_mixed(case, [clean] * 3, case.scalar)
    cp_out = cp_out_of(hip, case, s_out)
    args = (s_out, case.prefix, case.scalar)
    ref = tc.reference(oracle, case, base.payload, *args)
    assert ref[0] == "ok" and ref[3]
    clean_out, clean_q = ref[1], ref[2].ravel()
    kept = int(tc.Out(oracle, clean, *args).keep.sum())
    assert 0 < kept < case.ys * case.xs, "the clean picture has only one kind of slice"

    def pictures_are_clean(slots, where):
        buf = slots.buf.cpu().numpy()[GUARD:].reshape(-1)
        lens, q = slots.len_buf.cpu().numpy()[1:-1], slots.q_buf.cpu().numpy()[1:-1].reshape(slots.n, -1)
        for i in where:
            assert lens[i] == len(clean_out) and buf[i * slots.stride_out:i * slots.stride_out + len(clean_out)].tobytes() == clean_out, i
            assert (q[i] == clean_q).all(), i

    refused_run = compared = 0
    for cls in dm.input_classes(name):
        refs = [(m, tc.reference(oracle, case, dm.visible(base, m), *args)) for m in dm.input_mutations(base, name, cls)]
        ok = [(m, r) for m, r in refs if r[0] == "ok" and r[3]]
        outside = [(m, r) for m, r in refs if not r[-1]]        # (whether the composition codes or refuses them)
        refused = [(m, r) for m, r in refs if r[0] == "refused" and r[2]]
        assert all(r[1] in CODES for _, r in refused), (name, cls, [r[1] for _, r in refused])
        # in the encoder's domain: one call, every damaged slot between two clean ones
        if ok:
            row = [clean_m]
            for m, _ in ok:
                row += [m, clean_m]
            code, slots = _damaged_call(hip, oracle, case, row, cp_out)
            assert code == 0, (name, cls, "payloads the composition accepts", code)
            got, lens, q = slots.results()
            pictures_are_clean(slots, range(0, len(row), 2))
            for k, (m, r) in enumerate(ok):
                i = 2 * k + 1
                assert got[i] == r[1] and (q[i] == r[2].ravel()).all(), (name, cls, m.tag)
                compared += 1
        # outside the domain: the memory and isolation rules, OK or one of the composition's codes
        for m, r in outside:
            code, slots = _damaged_call(hip, oracle, case, [clean_m, m, clean_m], cp_out)
            assert code == 0 or code in CODES, (name, cls, m.tag, code)
            assert slots.guards_intact(), (name, cls, m.tag)
            pictures_are_clean(slots, (0, 2))
        # refused: the composition's code at sync, the neighbours their own transcode, the context usable afterwards
        quota = {"short": 4, "qindex": 3, "length": 4, "random": 1}.get(cls, 0)
        for m, r in _pick(refused, quota):
            refused_run += 1
            for row, where in (([clean_m, m, clean_m], (0, 2)), ([m], ())):
                code, slots = _damaged_call(hip, oracle, case, row, cp_out)
                assert code == r[1], (name, cls, m.tag, "composition", r[1], "library", code)
                assert slots.guards_intact(), (name, cls, m.tag)
                pictures_are_clean(slots, where)
            code, slots = _damaged_call(hip, oracle, case, [clean_m, clean_m], cp_out)
            assert code == 0
            pictures_are_clean(slots, (0, 1))
        print(f"{name} {cls}: {len(ok)} in domain compared, {len(outside)} outside it, {len(refused)} refused")
    assert 0 < refused_run <= REFUSED_PER_INPUT and compared > 0
    hip.close()
