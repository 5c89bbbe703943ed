"""GPU tests of vc2hip_transcode_batch_dev (include/vc2hip.h): every payload, length and index against
the CPU definition tests/transcode_ref.py, which stands on the oracle's slice reader, quantiser and slice writer.  The
inputs are coded by oracle primitives, so nothing here depends on the library's own encoder; the caps and the mid targets
come from picture 0's own table of transcoded lengths.

Every output is pre-filled, and lies between guards that must come back unchanged: 4096 bytes before and after the output
slots, one element before and after d_lens_out and d_qidx."""
import ctypes as C

import numpy as np
import pytest

import damage as dm
import proxy_ref as pr
import transcode_ref as tr
from test_gpu_cap import VARIANTS, slice_indices
from test_gpu_damaged import _pick

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = 0xA5
GUARD = 4096
EINVAL, ECAP = -1, -9
CAPS = ("floor", "mid", "mid-1", "empty", "none")
FOUR_CODES = (tr.ESTREAM, tr.EQINDEX, tr.ESCALAR, tr.ECODE32)


def _torch():
    import torch
    return torch


def _ctx(*flags, stream=None, lanes=1):
    from vc2hip_py import FLAGS, Vc2Hip
    hip = Vc2Hip(stream=stream, flags=sum(FLAGS[f] for f in flags))
    if lanes > 1:
        hip.set_streams(lanes)
    return hip


@pytest.fixture(scope="module")
def hip():
    h = _ctx()
    yield h
    h.close()


class Slots:
    """n coded pictures in device slots (0xA5 behind every length; `lengths`: what d_lens_in says, the payloads' by default)
    and every output of one call, pre-filled, between guards"""

    def __init__(self, hip, case, payloads, lengths=None, stride_in=None, zero_tail=False):
        torch = _torch()
        self.torch, self.hip, self.case, self.n = torch, hip, case, len(payloads)
        self.fmt, self.cp = case.fmt_cp(hip.lib)
        self.ns = case.ys * case.xs
        lengths = [len(p) for p in payloads] if lengths is None else list(lengths)
        need = max(max(len(p) for p in payloads), max(lengths))
        self.stride_in = stride_in or (need + 64 + 255) // 256 * 256
        slots = np.full((self.n, self.stride_in), 0 if zero_tail else FILL, np.uint8)
        for i, p in enumerate(payloads):
            slots[i, :len(p)] = np.frombuffer(p, np.uint8)
        self.d_in = torch.from_numpy(slots.reshape(-1)).to(DEV)
        self.d_len_in = torch.tensor(lengths, dtype=torch.int64).to(DEV)
        # the output is a VBR payload whatever coded the input: the bound is what three length bytes a slice can describe
        self.vbr_bound = self.ns * (case.prefix + 4 + 3 * 255 * case.scalar)
        self.stride_out = (max(hip.max_payload_bytes(self.fmt, self.cp), self.vbr_bound) + 64 + 255) // 256 * 256
        self.fresh()

    def fresh(self):
        torch = self.torch
        self.buf = torch.full((GUARD + self.n * self.stride_out + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.len_buf = torch.full((self.n + 2,), -1, dtype=torch.int64, device=DEV)
        self.q_buf = torch.full((self.n * self.ns + 2,), -1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        return self

    @property
    def out_ptr(self):
        return self.buf.data_ptr() + GUARD

    @property
    def len_ptr(self):
        return self.len_buf.data_ptr() + 8

    @property
    def q_ptr(self):
        return self.q_buf.data_ptr() + 4

    def call(self, tp, hip=None, n=None):
        (hip or self.hip).transcode_batch_dev(self.d_in.data_ptr(), self.stride_in, self.d_len_in.data_ptr(), n or self.n, self.fmt, self.cp,
                                              tp, self.out_ptr, self.stride_out, self.len_ptr, self.q_ptr)

    def run(self, tp, hip=None):
        self.call(tp, hip)
        (hip or self.hip).sync()
        return self

    def results(self):
        """([payload bytes], lengths, indices n x ns); the guards are asserted"""
        buf, lens, q = self.buf.cpu().numpy(), self.len_buf.cpu().numpy(), self.q_buf.cpu().numpy()
        assert self.guards_intact(buf, lens, q), "bytes outside the output slots, d_lens_out or d_qidx were written"
        pay = buf[GUARD:GUARD + self.n * self.stride_out].reshape(self.n, self.stride_out)
        lens = lens[1:-1]
        assert (lens >= 0).all() and (lens <= self.stride_out).all(), lens
        return [pay[i, :int(lens[i])].tobytes() for i in range(self.n)], lens.tolist(), q[1:-1].reshape(self.n, self.ns)

    def guards_intact(self, buf=None, lens=None, q=None):
        buf = self.buf.cpu().numpy() if buf is None else buf
        lens = self.len_buf.cpu().numpy() if lens is None else lens
        q = self.q_buf.cpu().numpy() if q is None else q
        return bool((buf[:GUARD] == FILL).all() and (buf[GUARD + self.n * self.stride_out:] == FILL).all()
                    and lens[0] == -1 and lens[-1] == -1 and q[0] == -1 and q[-1] == -1)

    def untouched(self):
        return bool((self.buf == FILL).all() and (self.len_buf == -1).all() and (self.q_buf == -1).all())


def _tp(q, cap=0):
    import vc2hip_py
    return vc2hip_py.transcode_params(q, cap)


def check_fixed(slots, pics, t, tag):
    got, lens, q = slots.results()
    case = slots.case
    for i, p in enumerate(pics):
        want = p.transcode(t)
        assert want is not tr.NOT_CODABLE, (tag, i, t)
        assert lens[i] == len(want), (tag, i, "length", lens[i], len(want), "target", t)
        assert (q[i] == p.indices(t).ravel()).all(), (tag, i, "d_qidx", t)
        assert slice_indices(got[i], slots.ns, case.prefix, case.scalar) == q[i].tolist(), (tag, i, "index bytes", t)
        assert got[i] == want, (tag, i, "payload", t)


def check_capped(slots, pics, floor, cap, tag):
    got, lens, q = slots.results()
    case = slots.case
    chosen = [p.chosen(floor, cap) for p in pics]
    for i, (p, qi) in enumerate(zip(pics, chosen)):
        want = p.transcode(qi)
        assert want is not tr.NOT_CODABLE, (tag, i, qi)
        assert lens[i] == len(want), (tag, i, "length", lens[i], len(want), "index", qi, "cap", cap)
        assert (q[i] == p.indices(qi).ravel()).all(), (tag, i, "d_qidx", qi)
        assert slice_indices(got[i], slots.ns, case.prefix, case.scalar) == q[i].tolist(), (tag, i, "index bytes", qi)
        assert got[i] == want, (tag, i, "payload", qi)
        assert (lens[i] <= cap) == p.fits(qi, cap), (tag, i)
    return chosen


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: every row, fixed targets and caps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tr.ROWS)
def test_fixed_target(hip, oracle, name):
    case, pics = tr.batch(oracle, name)
    slots = Slots(hip, case, [p.payload for p in pics])
    for t in tr.fixed_targets(pics):
        check_fixed(slots.fresh().run(_tp(t)), pics, t, (name, "fixed"))


@pytest.mark.parametrize("name", tr.ROWS)
def test_caps(hip, oracle, name):
    case, pics = tr.batch(oracle, name)
    floor = tr.floor_of(pics)
    caps = tr.caps(pics[0], floor)
    slots = Slots(hip, case, [p.payload for p in pics])
    for cname in CAPS:
        cap, want0 = caps[cname]
        chosen = check_capped(slots.fresh().run(_tp(floor, cap)), pics, floor, cap, (name, cname))   # (run: vc2hip_sync raises on any device error)
        assert chosen[0] == want0, (name, cname, chosen)
        if cname == "mid":
            assert len(set(chosen)) >= 2, (name, chosen)
        if cname == "none":
            assert chosen == [tr.Q_TOP] * 3 and all(n > cap for n in slots.results()[1])
    # another floor than the inputs' own: above every kept slice of row I's coarse half, a cap from the middle of the table
    fl = min(floor + 3, tr.Q_TOP)
    cap = pics[0].table()[min(fl + 20, tr.Q_TOP)]
    check_capped(slots.fresh().run(_tp(fl, cap)), pics, fl, cap, (name, "floor + 3"))


# ---------------------------------------------------------------------------------------------------------------------
# 3: the decoder on the output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "E"])
def test_decoder_shows_the_definitions_picture(hip, oracle, name):
    torch = _torch()
    case, pics = tr.batch(oracle, name)
    t = tr.mid_target(pics[0], tr.floor_of(pics))
    slots = Slots(hip, case, [p.payload for p in pics]).run(_tp(t))
    check_fixed(slots, pics, t, (name, "decode"))
    rb = case.raw_bytes()
    out = torch.full((3 * rb + 16,), FILL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    # the output is a plain VBR payload: read under an HQ_CONSTQ cp, whatever coded the input
    vbr = pr.Case(oracle, case.w, case.h, case.cf, case.bits, case.kernel, case.depth, case.u, case.a, scalar=case.scalar, prefix=case.prefix,
                  word_bytes=case.word_bytes)
    fmt, cp = vbr.fmt_cp(hip.lib)
    hip.decode_batch_dev(slots.out_ptr, slots.stride_out, slots.len_ptr, 3, fmt, cp, out.data_ptr())
    hip.sync()
    got = out.cpu().numpy()
    for i, p in enumerate(pics):
        assert got[i * rb:(i + 1) * rb].tobytes() == pr.full_picture(oracle, vbr, p.transcode(t)), (name, i)
    assert (got[3 * rb:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4: the profile
# ---------------------------------------------------------------------------------------------------------------------
def test_profile_holds_no_transform(oracle):
    case, pics = tr.batch(oracle, "A")
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    pic = hip.decode_picture(pics[0].payload, fmt, cp)        # a call that runs a transform
    assert pic == pr.full_picture(oracle, case, pics[0].payload)
    before = hip.dwt_launches()
    assert before
    floor = tr.floor_of(pics)
    slots = Slots(hip, case, [p.payload for p in pics])
    hip.profile_reset()
    hip.profile_enable(True)
    slots.run(_tp(floor + 6))
    slots.fresh().run(_tp(floor, tr.caps(pics[0], floor)["mid"][0]))
    hip.profile_enable(False)
    prof = hip.profile()
    # the fixed call: slice index, the decoder's slice reader, the scale step, the encoder's slice coder; the capped call adds two
    # measuring passes and two picks.  The writing stage of this call IS the encoder's slice coder (hq_pack and, in its two-pass
    # form, the scan and the compaction).
    assert prof["transcode_scale"][0] == 2 and prof["hq_unpack"][0] == 2 and prof["hq_pack"][0] == 2, prof
    assert prof["transcode_measure"][0] == 2 and prof["transcode_pick"][0] == 2, prof
    # no transform (dwt_*, idwt_*, plane_*), nothing of the decoder behind its slice reader, nothing of the encoder before its coder
    allowed = ("slice_index_", "transcode_", "hq_unpack", "hq_pack", "slice_offsets_scan", "slice_compact", "fill")
    others = [k for k in prof if not k.startswith(allowed)]
    assert not others, prof
    assert hip.dwt_launches() == before, "the call before's launch record changed"
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5: lanes and streams
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "E"])
@pytest.mark.parametrize("lanes", [2, 3])
def test_lanes_give_identical_bytes(hip, oracle, name, lanes):
    torch = _torch()
    case, pics = tr.batch(oracle, name)
    floor = tr.floor_of(pics)
    order = [0, 1, 2, 1, 0]
    pays, ps = [pics[k].payload for k in order], [pics[k] for k in order]
    t, cap = tr.mid_target(pics[0], floor), tr.caps(pics[0], floor)["mid"][0]
    one_f = Slots(hip, case, pays).run(_tp(t))
    one_c = Slots(hip, case, pays).run(_tp(floor, cap))
    hl = _ctx(lanes=lanes)
    two_f = Slots(hl, case, pays).run(_tp(t))
    check_fixed(two_f, ps, t, (name, lanes, "fixed"))
    two_c = Slots(hl, case, pays).run(_tp(floor, cap))
    check_capped(two_c, ps, floor, cap, (name, lanes, "capped"))
    for a, b in ((one_f, two_f), (one_c, two_c)):
        la, lb = a.results()[1], b.results()[1]
        assert la == lb and a.results()[0] == b.results()[0] and torch.equal(a.q_buf, b.q_buf)
    hl.close()


def test_one_picture_and_seventy(hip, oracle):
    case, pics = tr.batch(oracle, "A")
    floor = tr.floor_of(pics)
    t, cap = tr.mid_target(pics[0], floor), tr.caps(pics[0], floor)["mid"][0]
    for k in (1, 2):
        check_fixed(Slots(hip, case, [pics[k].payload]).run(_tp(t)), [pics[k]], t, ("n = 1", k))
        check_capped(Slots(hip, case, [pics[k].payload]).run(_tp(floor, cap)), [pics[k]], floor, cap, ("n = 1 capped", k))
    # 70 pictures of row G: past the 64 pictures of one workgroup of the pick
    case, pics = tr.batch(oracle, "G")
    floor = tr.floor_of(pics)
    cap = tr.caps(pics[0], floor)["mid"][0]
    order = [i % 3 for i in range(70)]
    ps = [pics[k] for k in order]
    slots = Slots(hip, case, [p.payload for p in ps])
    chosen = check_capped(slots.run(_tp(floor, cap)), ps, floor, cap, "70 pictures")
    assert len(set(chosen[64:])) >= 2 and len(set(chosen)) >= 2, chosen
    check_fixed(slots.fresh().run(_tp(floor + 5)), ps, floor + 5, "70 pictures fixed")


@pytest.mark.parametrize("name", ["A", "E"])
def test_on_a_callers_stream_and_under_capture(oracle, name):
    """a warm-up, then: the call returns while a filler still runs in front of it (no wait); captured once and replayed on
    other inputs and another batch's lengths, fixed and capped in one graph"""
    from test_gpu_caller_stream import Filler, _capture
    torch = _torch()
    case, pics = tr.batch(oracle, name)
    floor = tr.floor_of(pics)
    t, cap = tr.mid_target(pics[0], floor), tr.caps(pics[0], floor)["mid"][0]
    orders = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    s = torch.cuda.Stream()
    for lanes in (1, 2):
        hip = _ctx(stream=s.cuda_stream, lanes=lanes)
        with torch.cuda.stream(s):
            a = Slots(hip, case, [pics[k].payload for k in orders[0]])
            b = Slots(hip, case, [pics[k].payload for k in orders[0]], stride_in=a.stride_in)
            b.d_in, b.d_len_in = a.d_in, a.d_len_in         # one input, two outputs: the fixed and the capped call
            ins = []
            for o in orders:
                x = Slots(hip, case, [pics[k].payload for k in o], stride_in=a.stride_in)
                ins.append((x.d_in.cpu().pin_memory(), x.d_len_in.cpu().pin_memory()))

            def call():
                a.call(_tp(t))
                b.call(_tp(floor, cap))

            def load(r):
                a.d_in.copy_(ins[r][0], non_blocking=True)
                a.d_len_in.copy_(ins[r][1], non_blocking=True)

            def snapshot():
                return [(x.buf.clone(), x.len_buf.clone(), x.q_buf.clone()) for x in (a, b)]

            def check(snap, r, tag):
                ps = [pics[k] for k in orders[r]]
                for x, (buf, lens, q) in zip((a, b), snap):
                    y = Slots.__new__(Slots)
                    y.__dict__.update(x.__dict__)
                    y.buf, y.len_buf, y.q_buf = buf, lens, q
                    if x is a:
                        check_fixed(y, ps, t, (name, lanes, tag, r))
                    else:
                        check_capped(y, ps, floor, cap, (name, lanes, tag, r))

            call()                                      # the warm-up
            s.synchronize()
            hip.sync()
            check(snapshot(), 0, "warm-up")
            load(1)
            s.synchronize()
            e_fill = Filler(s).run()
            call()
            e = torch.cuda.Event()
            e.record(s)
            waited, filler_done = e.query(), e_fill.query()
            snap = snapshot()
            s.synchronize()
            hip.sync()
            check(snap, 1, "behind the filler")
            assert not waited and not filler_done, "the call waited for the stream"
        g, _ = _capture(torch, s, hip, call)
        with torch.cuda.stream(s):
            snaps = {}
            for r in (2, 0):
                load(r)
                g.replay()
                snaps[r] = snapshot()
            s.synchronize()
            hip.sync()
        for r in (2, 0):
            check(snaps[r], r, "replay")
        hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6: mixing with the other calls on one context
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C"])
def test_mixed_with_decode_and_encode(oracle, name):
    torch = _torch()
    case, pics = tr.batch(oracle, name)
    hip = _ctx()
    floor = tr.floor_of(pics)
    t, cap = tr.mid_target(pics[0], floor), tr.caps(pics[0], floor)["mid"][0]
    rb = case.raw_bytes()
    want_pics = [pr.full_picture(oracle, case, p.payload) for p in pics]
    slots = Slots(hip, case, [p.payload for p in pics])
    import cap_ref as cr
    raws = cr.pictures(case)

    def decode():
        out = torch.full((3 * rb + 16,), FILL, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        hip.decode_batch_dev(slots.d_in.data_ptr(), slots.stride_in, slots.d_len_in.data_ptr(), 3, slots.fmt, slots.cp, out.data_ptr())
        hip.sync()
        got = out.cpu().numpy()
        assert [got[i * rb:(i + 1) * rb].tobytes() for i in range(3)] == want_pics and (got[3 * rb:] == FILL).all()

    def encode():
        d_raw = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(DEV)
        d_pay = torch.full((3 * slots.stride_out,), FILL, dtype=torch.uint8, device=DEV)
        d_len = torch.full((3,), -1, dtype=torch.int64, device=DEV)
        torch.cuda.synchronize()
        hip.encode_batch_dev(d_raw.data_ptr(), 3, slots.fmt, slots.cp, d_pay.data_ptr(), slots.stride_out, d_len.data_ptr())
        hip.sync()
        pay, lens = d_pay.cpu().numpy().reshape(3, -1), d_len.cpu().numpy()
        assert [pay[i, :int(lens[i])].tobytes() for i in range(3)] == [p.payload for p in pics]   # (ConstQ rows: the input itself)

    decode()
    check_fixed(slots.fresh().run(_tp(t)), pics, t, (name, "mixed fixed"))
    encode()
    check_capped(slots.fresh().run(_tp(floor, cap)), pics, floor, cap, (name, "mixed capped"))
    decode()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7: every context flag gives the same bytes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS) + ["NO_CBR_INDEX"])
def test_flags_give_the_same_bytes(oracle, variant):
    flags = VARIANTS.get(variant, (variant,))
    hip = _ctx(*flags)
    for name in (["E"] if variant == "NO_CBR_INDEX" else ["A", "E"]):
        case, pics = tr.batch(oracle, name)
        floor = tr.floor_of(pics)
        t, cap = tr.mid_target(pics[0], floor), tr.caps(pics[0], floor)["mid"][0]
        slots = Slots(hip, case, [p.payload for p in pics])
        check_fixed(slots.run(_tp(t)), pics, t, (variant, name))
        check_capped(slots.fresh().run(_tp(floor, cap)), pics, floor, cap, (variant, name))
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8: refusals
# ---------------------------------------------------------------------------------------------------------------------
def _raw_call(hip, a):
    return hip.lib.vc2hip_transcode_batch_dev(hip.h, a["in"], a["stride_in"], a["lens_in"], a["n"], a["fmt"], a["cp"], a["tp"], a["out"],
                                              a["stride_out"], a["lens_out"], a["qidx"])


@pytest.mark.parametrize("lanes", [1, 3])
def test_refusals_launch_nothing_and_touch_nothing(oracle, lanes):
    import vc2hip_py
    case, pics = tr.batch(oracle, "A")
    hip = _ctx(lanes=lanes)
    floor = tr.floor_of(pics)
    slots = Slots(hip, case, [p.payload for p in pics])
    check_fixed(slots.run(_tp(floor + 6)), pics, floor + 6, "before the refusals")
    slots.fresh()
    tp = _tp(floor + 6)
    good = dict(stride_in=slots.stride_in, n=3, fmt=C.byref(slots.fmt), cp=C.byref(slots.cp), tp=C.byref(tp), stride_out=slots.stride_out,
                lens_in=slots.d_len_in.data_ptr(), lens_out=slots.len_ptr, qidx=slots.q_ptr, out=slots.out_ptr)
    good["in"] = slots.d_in.data_ptr()

    def cp_with(**kw):
        cp = type(slots.cp).from_buffer_copy(slots.cp)
        for k, v in kw.items():
            setattr(cp, k, v)
        return C.byref(cp)

    def tp_with(q, cap=0):
        return C.byref(vc2hip_py.transcode_params(q, cap))

    fmt_bad = type(slots.fmt).from_buffer_copy(slots.fmt)
    fmt_bad.width = 0
    tries = {
        "tp null": dict(tp=None), "fmt null": dict(fmt=None), "cp null": dict(cp=None), "input null": {"in": None},
        "lens_in null": dict(lens_in=None), "output null": dict(out=None), "lens_out null": dict(lens_out=None),
        "n 0": dict(n=0), "n -1": dict(n=-1),
        "LD": dict(cp=cp_with(mode=vc2hip_py.MODES["LD"], compressed_bytes=20000)), "mode 7": dict(cp=cp_with(mode=7)),
        "index -1": dict(tp=tp_with(-1)), "index 116": dict(tp=tp_with(116)), "cap -1": dict(tp=tp_with(floor, -1)),
        "input misaligned": {"in": good["in"] + 8}, "input stride misaligned": dict(stride_in=slots.stride_in + 8),
        "output misaligned": dict(out=good["out"] + 8), "output stride misaligned": dict(stride_out=slots.stride_out + 8),
        "lens_in misaligned": dict(lens_in=good["lens_in"] + 4), "lens_out misaligned": dict(lens_out=good["lens_out"] + 4),
        "qidx misaligned": dict(qidx=good["qidx"] + 2),
        "output on the input": dict(out=good["in"]), "output inside the input": dict(out=good["in"] + 2 * slots.stride_in),
        "output ends in the input": dict(out=good["in"] - slots.stride_out),
        "scalar 0": dict(cp=cp_with(scalar=0)), "prefix -1": dict(cp=cp_with(prefix=-1)), "depth 0": dict(cp=cp_with(depth=0)),
        "no slices": dict(cp=cp_with(y_slices=0)), "width 0": dict(fmt=C.byref(fmt_bad)), "kernel 9": dict(cp=cp_with(kernel=9)),
    }
    for what, change in tries.items():
        rc = _raw_call(hip, {**good, **change})
        assert rc == EINVAL, (what, rc)
        hip.sync()
        assert slots.untouched(), what
    rc = _raw_call(hip, {**good, "stride_out": (slots.vbr_bound - 1) // 16 * 16})
    assert rc == ECAP, rc
    hip.sync()
    assert slots.untouched()
    assert _raw_call(hip, {**good, "qidx": None}) == 0          # d_qidx is optional
    hip.sync()
    assert (slots.q_buf == -1).all()
    got = slots.results()
    assert got[0] == [p.transcode(floor + 6) for p in pics]
    check_fixed(slots.fresh().run(_tp(floor + 6)), pics, floor + 6, "after the refusals")
    check_fixed(slots.fresh().run(_tp(tr.Q_TOP)), pics, tr.Q_TOP, "the top index is allowed")
    hip.close()


def test_a_budget_sized_stride_is_refused_under_hq_cbr(oracle):
    """row E: under an HQ_CBR cp vc2hip_max_payload_bytes is the budget's bound, below that of the VBR payload the call writes;
    a stride between the two is refused on the host and nothing is touched, the VBR bound is accepted"""
    case, pics = tr.batch(oracle, "E")
    hip = _ctx()
    slots = Slots(hip, case, [p.payload for p in pics])
    small = (hip.max_payload_bytes(slots.fmt, slots.cp) + 15) // 16 * 16
    assert small < slots.vbr_bound
    tp = _tp(tr.floor_of(pics) + 4)
    rc = hip.lib.vc2hip_transcode_batch_dev(hip.h, slots.d_in.data_ptr(), slots.stride_in, slots.d_len_in.data_ptr(), 3, C.byref(slots.fmt),
                                            C.byref(slots.cp), C.byref(tp), slots.out_ptr, small, slots.len_ptr, slots.q_ptr)
    assert rc == ECAP, rc
    hip.sync()
    assert slots.untouched()
    slots.stride_out = (slots.vbr_bound + 15) // 16 * 16
    check_fixed(slots.fresh().run(tp), pics, tr.floor_of(pics) + 4, "the VBR bound")
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9: damaged input
# ---------------------------------------------------------------------------------------------------------------------
REFUSED_PER_INPUT = 12
MIN_IN_DOMAIN = {"boundary": 1.0, "long": 1.0, "runff": 1.0, "random": 2 / 3, "run00": 0.5}


def _damaged_call(hip, case, muts, t):
    """one call over mutations; (the error of vc2hip_sync or None, the Slots)"""
    import vc2hip_py
    slots = Slots(hip, case, [m.data for m in muts], lengths=[m.length for m in muts], zero_tail=any(m.cls == "long" for m in muts))
    slots.call(_tp(t))
    err = None
    try:
        hip.sync()
    except vc2hip_py.Vc2HipError as e:
        err = e
    return err, slots


@pytest.mark.parametrize("name", ["A", "B2"])
def test_damaged_input(oracle, name):
    base, _ = dm.load(oracle, name)
    case = base.case
    t = case.q + 6
    hip = _ctx()
    clean_m = dm.clean(base)
    clean = tr.Coded(oracle, case, base.payload)
    clean_out, clean_q = clean.transcode(t), clean.indices(t).ravel()

    def neighbours_ok(slots, where):
        got, lens, q = slots.results()     # (asserts the guards)
        for i in where:
            assert got[i] == clean_out and (q[i] == clean_q).all(), "a clean neighbour is not its own transcode"

    refused_run = 0
    for cls in dm.input_classes(name):
        refs = [(m, tr.damaged_reference(oracle, case, dm.visible(base, m), t)) for m in dm.input_mutations(base, name, cls)]
        ok = [(m, r) for m, r in refs if r[0] == "ok" and r[3]]
        outside = [(m, r) for m, r in refs if r[0] == "ok" and not r[3]]
        refused = [(m, r) for m, r in refs if r[0] == "refused"]
        if cls in MIN_IN_DOMAIN:
            assert len(ok) >= MIN_IN_DOMAIN[cls] * len(refs) - 1e-9, (name, cls, len(ok), len(refs))
        assert all(r[1] in (tr.ESTREAM, tr.EQINDEX) for _, r in refused), (name, cls, [r[1] for _, r in refused])
        # (a) in the encoder's domain: one call, every damaged slot between two clean ones
        if ok:
            row = [clean_m]
            for m, _ in ok:
                row += [m, clean_m]
            err, slots = _damaged_call(hip, case, row, t)
            assert err is None, (name, cls, "payloads the composition accepts", err.code, str(err))
            got, lens, q = slots.results()
            neighbours_ok(slots, range(0, len(row), 2))
            for k, (m, r) in enumerate(ok):
                i = 2 * k + 1
                assert got[i] == r[1] and (q[i] == r[2].ravel()).all(), (name, cls, m.tag)
            # (b) each on its own
            for m, r in ok:
                err, one = _damaged_call(hip, case, [m], t)
                assert err is None, (name, cls, m.tag, err)
                got, lens, q = one.results()
                assert got[0] == r[1] and (q[0] == r[2].ravel()).all(), (name, cls, m.tag, "alone")
        # outside the domain: the memory and isolation rules, OK or one of the four codes
        for m, r in outside:
            for row, where in (([clean_m, m, clean_m], (0, 2)), ([m], ())):
                err, slots = _damaged_call(hip, case, row, t)
                assert err is None or err.code in FOUR_CODES, (name, cls, m.tag, err.code)
                assert slots.guards_intact(), (name, cls, m.tag)
                if where:
                    buf = slots.buf.cpu().numpy()[GUARD:].reshape(-1)
                    lens, q = slots.len_buf.cpu().numpy()[1:-1], slots.q_buf.cpu().numpy()[1:-1].reshape(len(row), -1)
                    for i in where:
                        assert lens[i] == len(clean_out) and buf[i * slots.stride_out:i * slots.stride_out + len(clean_out)].tobytes() == clean_out
                        assert (q[i] == clean_q).all()
        # refused: the composition's code at sync, the neighbours their own transcode, the context usable afterwards
        quota = {"short": 4, "qindex": 3, "length": 4, "random": 1}.get(cls, 0)
        for m, r in _pick(refused, quota):
            refused_run += 1
            for row, where in (([clean_m, m, clean_m], (0, 2)), ([m], ())):
                err, slots = _damaged_call(hip, case, row, t)
                assert err is not None, (name, cls, m.tag, "the composition refuses with", r[1])
                assert err.code == r[1], (name, cls, m.tag, "composition", r[1], "library", err.code)
                assert slots.guards_intact(), (name, cls, m.tag)
                if where:
                    buf = slots.buf.cpu().numpy()[GUARD:].reshape(-1)
                    lens, q = slots.len_buf.cpu().numpy()[1:-1], slots.q_buf.cpu().numpy()[1:-1].reshape(len(row), -1)
                    for i in where:
                        assert lens[i] == len(clean_out) and buf[i * slots.stride_out:i * slots.stride_out + len(clean_out)].tobytes() == clean_out
                        assert (q[i] == clean_q).all()
            err, slots = _damaged_call(hip, case, [clean_m, clean_m], t)
            assert err is None
            neighbours_ok(slots, (0, 1))
        print(f"{name} {cls}: {len(ok)} in domain compared, {len(outside)} outside it, {len(refused)} refused")
    assert 0 < refused_run <= REFUSED_PER_INPUT
    hip.close()
