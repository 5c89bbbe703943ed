"""vc2hip_stream_read_dev (k_stream_walk + k_stream_gather) against tests/stream_ref.py's walk model on designed unit chains
(DESIGN.md section 26), exact comparisons only.

Every case runs twice inside a larger device tensor, 64 bytes in front of the stream and 256 behind: once with zeros around
it, once with a valid continuation -- a well-formed picture unit that starts exactly at len, and "BBCD" ending exactly at the
base.  Lengths, picture numbers, consumed, every byte of the slots and their guard, and the error text must be the model's in
both.  The buffers lie well inside one allocation: a dependence on the surroundings shows as a difference, never as a fault."""
import numpy as np
import pytest

import stream_ref as sr
from test_gpu_stream_dev import CASES

pytestmark = pytest.mark.gpu

ECAP, ESYNTAX = -9, -12
FRONT, BACK, GUARD = 64, 256, 256
PARTS = 6


def _torch():
    return pytest.importorskip("torch")


class Env:
    def __init__(self, oracle):
        import vc2hip_py
        self.oracle = oracle
        self.S = sr.sources(oracle)
        self.acc, self.ref = sr.accepted(self.S), sr.refused(self.S)
        m = sr.MINI
        self.fmt = vc2hip_py.picture_format(m["w"], m["h"], m["cf"], m["bits"], m["wb"])
        self.decoded = {}
        good = self.S["mini5"]
        self.good = sr.Case("good", "a good stream after a refusal", good, good.plain([2, 0]), 2, pics=[2, 0])

    def want_pictures(self, c):
        key = (c.src.name, tuple(c.pics))
        if key not in self.decoded:
            self.decoded[key] = self.oracle.decode_stream(c.src.p, c.src.plain(c.pics), len(c.pics))[0]
        return self.decoded[key]


@pytest.fixture(scope="module")
def env(oracle):
    return Env(oracle)


def _stride(hip, fmt, cp):
    return (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256


def _surroundings(c, off, continuation):
    """host bytes of the larger tensor and the stream's position in it"""
    base = FRONT + off
    host = bytearray(base + len(c.stream) + BACK + 16)
    if continuation:
        host[:base] = (b"\xe8" * base)[:base - 4] + b"BBCD"
        cont = sr.chain([c.src.whole(0, 3, 0x01020304), sr.U(sr.EOS)])[0]
        room = len(host) - (base + c.length)
        cont = (cont * (room // len(cont) + 1))[:room]
        host[base + c.length:] = cont
    host[base:base + c.length] = c.stream[:c.length]
    return host, base


def _run(hip, c, fmt, off=0, continuation=False, stride=None, decode=False, cp=None):
    """one stream_read_dev at the given offset from a 16-byte boundary; everything it wrote, and the error at sync"""
    import vc2hip_py
    torch = _torch()
    cp = cp or c.src.cp
    stride = stride or c.stride or _stride(hip, fmt, cp)
    host, base = _surroundings(c, off, continuation)
    big = torch.frombuffer(host, dtype=torch.uint8).to("cuda:0")
    assert big.data_ptr() % 16 == 0
    n = c.n
    d_pay = torch.full((n * stride + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_len = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    d_pn = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d_cons = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    hip.stream_read_dev(big.data_ptr() + base + c.start, c.length - c.start, n, cp, vc2hip_py.stream_params(c.major), d_pay.data_ptr(),
                        stride, d_len.data_ptr(), d_pn.data_ptr(), d_cons.data_ptr())
    code, msg = 0, ""
    try:
        hip.sync()
    except vc2hip_py.Vc2HipError as e:
        code, msg = e.code, str(e)
    out = dict(code=code, msg=msg, lens=d_len.cpu().tolist(), pns=[v & 0xFFFFFFFF for v in d_pn.cpu().tolist()],
               consumed=int(d_cons.item()), pay=d_pay.cpu().numpy().tobytes(), stride=stride)
    if decode and code == 0:
        rb = hip.raw_picture_bytes(fmt)
        d_out = torch.zeros(n * rb, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, fmt, cp, d_out.data_ptr())
        hip.sync()
        out["pictures"] = d_out.cpu().numpy().tobytes()
    return out


def _check_slots(tag, got, res, n):
    """the pictures the model completed are in their slots, zeros up to the 16-byte boundary behind each; every other byte of
    the slots and the guard keeps its fill"""
    stride, pay = got["stride"], got["pay"]
    done = len(res.numbers)
    assert got["lens"] == res.lens, (tag, got["lens"], res.lens)
    assert got["pns"][:done] == res.numbers, (tag, got["pns"], res.numbers)
    for k in range(n):
        slot = pay[k * stride:(k + 1) * stride]
        if k >= done:
            assert slot == b"\xa5" * stride, (tag, k, "a slot behind the pictures completed was written")
            continue
        held = min(res.lens[k], stride)
        edge = min((held + 15) // 16 * 16, stride)
        assert slot[:held] == res.payloads[k][:held], (tag, k, "payload")
        assert slot[held:edge] == bytes(edge - held), (tag, k, "zero fill")
        assert slot[edge:] == b"\xa5" * (stride - edge), (tag, k, "the rest of the slot")
    assert pay[n * stride:] == b"\xa5" * GUARD, (tag, "guard")


def _same(a, b):
    return all(a[k] == b[k] for k in ("code", "msg", "lens", "pns", "consumed", "pay"))


def _accepted(hip, env, c, fmt=None, want_pictures=None, **kw):
    fmt = fmt or env.fmt
    res = c.model()
    assert res.ok, c.name
    first = None
    for off in c.offs:
        runs = [_run(hip, c, fmt, off, cont, decode=(first is None and not cont and c.pics is not None and c.stride is None), **kw)
                for cont in (False, True)]
        for got in runs:
            tag = (c.name, c.edge, off)
            assert got["code"] == 0, (tag, got["msg"])
            assert got["consumed"] == res.consumed, (tag, got["consumed"], res.consumed)
            _check_slots(tag, got, res, c.n)
        assert _same(*runs), (c.name, off, "the result depends on what lies outside the stream")
        if first is None:
            first = runs[0]
            if "pictures" in first:
                assert first["pictures"] == (want_pictures or env.want_pictures(c)), (c.name, "decode")
        else:
            assert first["pay"] == runs[0]["pay"], (c.name, off, "the slots depend on the stream's alignment")


def _refused(hip, env, c, code=ESYNTAX):
    res = c.model()
    assert not res.ok and res.reason == c.expect, c.name
    runs = [_run(hip, c, env.fmt, 0, cont) for cont in (False, True)]
    for got in runs:
        tag = (c.name, c.edge)
        assert got["code"] == code, (tag, got["code"], got["msg"])
        assert "at byte %d: %s" % (res.at, res.reason) in got["msg"], (tag, got["msg"], res.at, res.reason)
        _check_slots(tag, got, res, c.n)
    assert _same(*runs), (c.name, "the result depends on what lies outside the stream")
    good = _run(hip, env.good, env.fmt)
    assert good["code"] == 0 and good["consumed"] == env.good.model().consumed, (c.name, "the context after the refusal")
    _check_slots((c.name, "good stream after"), good, env.good.model(), 2)


@pytest.mark.parametrize("part", range(PARTS))
def test_accepted_streams(hip, env, part):
    for c in env.acc[part::PARTS]:
        _accepted(hip, env, c)


@pytest.mark.parametrize("part", range(PARTS))
def test_refused_streams(hip, env, part):
    """every reason of the walk with its byte offset, on both sides of each boundary (the accepted sides are among the accepted
    streams); pictures completed before the refused unit are delivered; the same context then reads a good stream"""
    cases = env.ref[part::PARTS]
    for c in cases:
        _refused(hip, env, c)
    if part == 0:
        assert {c.expect for c in env.ref} == set(sr.WALK_REASONS)


@pytest.mark.parametrize("case,frag,seed", [(case, None, 7) for case in CASES] +
                         [("cbr_legall_420_8", 300, 8), ("ld_legall_420_8", 200, 8), ("cbr_legall_420_8", 10 ** 6, 8)])
def test_oracle_streams(hip, oracle, env, case, frag, seed):
    """the oracle's own streams (whole pictures and the greedy cut) at two alignments, against the model and the oracle's decode"""
    import vc2hip_py
    g = CASES[case]
    cp, p, stream = sr.oracle_stream(oracle, g, 3, seed, **(dict(fragment_length=frag) if frag else {}))
    src = sr.Source(case, g, cp, p, sr.oracle_payloads(cp, sr.oracle_stream(oracle, g, 3, seed)[2], 3), None, sr.want_of(oracle, cp))
    fmt = vc2hip_py.picture_format(g["w"], g["h"], g["cf"], g["bits"], g.get("wb", 2))
    c = sr.Case(case, "the oracle's stream", src, stream, 3, pics=[0, 1, 2], offs=(0, 7))
    _accepted(hip, env, c, fmt=fmt, want_pictures=oracle.decode_stream(p, stream, 3)[0])


def test_slot_capacity(hip, env):
    """a picture of exactly the stride is read; one of stride + 1 bytes is VC2HIP_ECAP at sync: its length is the true one, its
    slot holds the first stride bytes, the next picture's slot is right and nothing outside the slots is touched"""
    exact, longer, longer_f = sr.capacity(env.S)
    _accepted(hip, env, exact)
    for c in (longer, longer_f):
        res = c.model()
        for cont in (False, True):
            got = _run(hip, c, env.fmt, 1, cont)
            assert got["code"] == ECAP, (c.name, got["code"], got["msg"])
            assert got["lens"] == [c.stride, c.stride + 1, c.stride] and got["consumed"] == res.consumed
            _check_slots((c.name, cont), got, res, 3)
    _accepted(hip, env, env.good)


def test_on_two_lanes(oracle, env):
    import vc2hip_py
    hip = vc2hip_py.Vc2Hip()
    hip.set_streams(2)
    by = {c.name: c for c in env.acc + env.ref}
    for name in ("mix_cut_random_a", "mini4_cut_ones", "resume_rest_2"):
        _accepted(hip, env, by[name])
    _refused(hip, env, by["rows_in_the_wrong_order"])
    hip.close()


def test_on_a_callers_stream_and_under_capture(oracle, env):
    """one context on a caller's stream: a plain call in stream order, then the call captured once and replayed on two
    different streams of equal length"""
    import vc2hip_py
    from test_gpu_caller_stream import _capture, _ctx
    torch = _torch()
    s = torch.cuda.Stream()
    hip = _ctx(s)
    src = env.S["mini5"]
    seq3, eos = sr.sequence_header(3), sr.U(sr.EOS)
    cut = [1, 4, 7, 3, 9]
    streams = [sr.chain([seq3] + src.cut(a, cut) + [src.whole(b, 3)] + [eos])[0] for a, b in ((0, 1), (2, 0))]
    cases = [sr.Case("captured_%d" % i, "replay", src, st, 2) for i, st in enumerate(streams)]
    assert len(streams[0]) == len(streams[1]) and streams[0] != streams[1]
    stride = _stride(hip, env.fmt, src.cp)
    size = FRONT + 7 + len(streams[0])
    pinned = [torch.from_numpy(np.frombuffer(bytes(FRONT + 7) + st, np.uint8).copy()).pin_memory() for st in streams]
    with torch.cuda.stream(s):
        d_stream = torch.zeros(size + BACK, dtype=torch.uint8, device="cuda:0")
        d_pay = torch.full((2 * stride + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        d_len = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        d_pn = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        d_cons = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        outs = [[torch.empty_like(t, device="cpu").pin_memory() for t in (d_pay, d_len, d_pn, d_cons)] for _ in range(3)]

        def call():
            hip.stream_read_dev(d_stream.data_ptr() + FRONT + 7, len(streams[0]), 2, src.cp, vc2hip_py.stream_params(0), d_pay.data_ptr(),
                                stride, d_len.data_ptr(), d_pn.data_ptr(), d_cons.data_ptr())

        def round_(k, which, fn):
            d_stream[:size].copy_(pinned[which], non_blocking=True)
            d_pay.fill_(0xA5)
            fn()
            for o, t in zip(outs[k], (d_pay, d_len, d_pn, d_cons)):
                o.copy_(t, non_blocking=True)

        round_(0, 0, call)             # stream order, the host ahead; also the warm-up the contract asks for
        s.synchronize()
        hip.sync()
    g, _ = _capture(torch, s, hip, call)
    with torch.cuda.stream(s):
        round_(1, 1, g.replay)
        round_(2, 0, g.replay)
        s.synchronize()
        hip.sync()
    for k, which in enumerate((0, 1, 0)):
        res = cases[which].model()
        pay, lens, pns, cons = outs[k]
        got = dict(stride=stride, pay=pay.numpy().tobytes(), lens=lens.tolist(), pns=[v & 0xFFFFFFFF for v in pns.tolist()])
        assert int(cons.item()) == res.consumed
        _check_slots(("capture", k), got, res, 2)
        assert res.payloads == [src.payloads[i] for i in ((0, 1), (2, 0))[which]]
    hip.close()
