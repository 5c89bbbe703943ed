"""GPU tests of the batch calls on a CALLER's stream (vc2hip_create_on_stream / _on_stream_with_flags), the way an integrator
drives the library from PyTorch: stream order with the host running ahead of the GPU (part A), graph capture and replay
(part B), and "the call never waits" measured with an event behind a long filler (part C).  include/vc2hip.h states the
contract.  Every context here is made on torch.cuda.Stream().cuda_stream and all torch work runs under that stream; the
expected bytes come from the CPU oracle (recon_ref.recon, proxy_ref, oracle.encode_stream), never from another run of the
library, except where a test says "equals the own-stream context" in addition.

The filler of parts A and C is FILLER_REPS in-place multiplications of a FILLER_BYTES float32 tensor on the stream.  A call
that waited for the stream would return after the filler; one that does not returns while it runs, and an event recorded
behind the call is then still incomplete.  test_the_filler_outlasts_every_call measures, on every run, the filler's
duration against the host time of every scenario's calls on an idle stream (median of 20, perf_counter around the calls
only) and asserts the factor of 20 the sizing rests on.
Measured on an MI355X, 2026-10-16, working tree over commit eebf9cb: filler 34.3 ms; slowest call whole_plane (encode +
decode of two pictures), median host time 0.390 ms; every other scenario 0.06 - 0.10 ms.  Factor 88.
"""
import time

import numpy as np
import pytest

import proxy_ref as pr
import recon_ref as rr
from synth import noise_frame, synth
from test_gpu_fields import _fields, _frames
from test_gpu_stream_dev import _major, _seq_len

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 4                       # iterations the host issues without a synchronisation (part A)
R = 3                       # replays of a captured graph (part B)
POOL = 5                    # distinct pictures of a scenario; iteration k holds pictures (i + k) % POOL at position i
FILLER_BYTES = 1 << 30
FILLER_REPS = 96
ESCALAR = -3


def _torch():
    import torch
    return torch


def _ctx(s, *flags):
    from vc2hip_py import FLAGS, Vc2Hip
    return Vc2Hip(stream=s.cuda_stream, flags=sum(FLAGS[f] for f in flags))


class Filler:
    """ordinary torch work on a large tensor: keeps the stream busy for tens of milliseconds"""
    _t = None

    def __init__(self, s):
        torch = _torch()
        if Filler._t is None:
            Filler._t = torch.ones(FILLER_BYTES // 4, dtype=torch.float32, device=DEV)
            torch.cuda.synchronize()
        self.s = s

    def run(self):
        """enqueue the filler on the current stream; returns an event recorded behind it"""
        torch = _torch()
        for _ in range(FILLER_REPS):
            Filler._t.mul_(1.0)
        e = torch.cuda.Event()
        e.record(self.s)
        return e


def _pin(arr):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(arr)).pin_memory()


# ---------------------------------------------------------------------------------------------------------------------
# scenarios: the inputs of iteration k in pinned memory, the device buffers, the library calls, the oracle's answers
# ---------------------------------------------------------------------------------------------------------------------
class Scenario:
    """inputs: name -> pinned (iterations, bytes) uint8; dev: name -> device uint8 tensor (inputs and outputs);
    outputs: names copied to the ring after the calls; check(k, got): got[name] is the ring's slot k as numpy uint8"""
    may_wait = False        # the calls may synchronise by contract (a budget table that changes between them)

    def __init__(self, hip, iters):
        self.hip, self.iters = hip, iters
        self.inputs, self.dev, self.outputs, self.ring = {}, {}, [], {}

    def buffers(self, **sizes):
        torch = _torch()
        for name, nbytes in sizes.items():
            self.dev[name] = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=DEV)

    def finish(self, outputs):
        torch = _torch()
        self.outputs = outputs
        for name in outputs:
            self.ring[name] = torch.full((self.iters, self.dev[name].numel()), 0x5A, dtype=torch.uint8).pin_memory()

    def p(self, name):
        return self.dev[name].data_ptr()

    def load(self, k):
        for name, stack in self.inputs.items():
            self.dev[name][:stack.shape[1]].copy_(stack[k], non_blocking=True)

    def store(self, k):
        for name in self.outputs:
            self.ring[name][k].copy_(self.dev[name], non_blocking=True)

    def got(self, k):
        return {name: self.ring[name][k].numpy() for name in self.outputs}

    def sets(self, k, n):
        return [(i + k) % POOL for i in range(n)]


def _pool_raw(case, kind, seed):
    if kind == "noise":
        return b"".join(noise_frame(case.w, case.h, case.cf, case.bits, seed + f, word_bytes=case.word_bytes) for f in range(POOL))
    return synth(case.w, case.h, case.cf, case.bits, seed, frames=POOL, word_bytes=case.word_bytes)


def _check_slots(tag, got_pay, got_len, stride, want_pays):
    lens = got_len[:8 * len(want_pays)].view(np.int64)
    for i, w in enumerate(want_pays):
        assert int(lens[i]) == len(w), (tag, i, "length", int(lens[i]), len(w))
        assert got_pay[i * stride:i * stride + len(w)].tobytes() == w, (tag, i, "payload")


def _check_pictures(tag, got, rb, want_pics):
    for i, w in enumerate(want_pics):
        assert got[i * rb:(i + 1) * rb].tobytes() == w, (tag, i, "picture")
    assert (got[len(want_pics) * rb:] == 0xA5).all(), (tag, "wrote past the pictures")


class EncDec(Scenario):
    """raw pictures -> encode_batch_dev -> decode_batch_dev (or encode_recon_batch_dev with every output when recon)"""

    def __init__(self, hip, oracle, case, n, iters, kind="synth", seed=31, recon=False):
        super().__init__(hip, iters)
        self.case, self.n, self.recon = case, n, recon
        self.fmt, self.cp = case.fmt_cp(hip.lib)
        self.rb, self.ns = case.raw_bytes(), case.ys * case.xs
        assert self.rb % 16 == 0
        raw = _pool_raw(case, kind, seed)
        self.want = rr.recon(oracle, case, raw, POOL)
        pics = np.frombuffer(raw, np.uint8).reshape(POOL, self.rb)
        self.inputs["raw"] = _pin(np.stack([pics[self.sets(k, n)].reshape(-1) for k in range(iters)]))
        self.stride = (hip.max_payload_bytes(self.fmt, self.cp) + 64 + 255) // 256 * 256
        self.buffers(raw=n * self.rb, pay=n * self.stride, len=n * 8, out=n * self.rb, sse=n * 24, q=n * self.ns * 4)
        self.finish(["pay", "len", "out"] + (["sse", "q"] if recon else []))

    def call(self):
        h = self.hip
        if self.recon:
            h.encode_recon_batch_dev(self.p("raw"), self.n, self.fmt, self.cp, self.p("pay"), self.stride, self.p("len"),
                                     self.p("out"), self.p("sse"), self.p("q"))
        else:
            h.encode_batch_dev(self.p("raw"), self.n, self.fmt, self.cp, self.p("pay"), self.stride, self.p("len"))
            h.decode_batch_dev(self.p("pay"), self.stride, self.p("len"), self.n, self.fmt, self.cp, self.p("out"))

    def check(self, k, got, tag):
        w = [self.want[j] for j in self.sets(k, self.n)]
        _check_slots((tag, k), got["pay"], got["len"], self.stride, [x[0] for x in w])
        _check_pictures((tag, k), got["out"], self.rb, [x[1] for x in w])
        if self.recon:
            sse = got["sse"][:self.n * 24].view(np.uint64).reshape(self.n, 3)
            q = got["q"][:self.n * self.ns * 4].view(np.int32).reshape(self.n, self.ns)
            for i, x in enumerate(w):
                assert [int(v) for v in sse[i]] == x[2], (tag, k, i, "sums")
                assert np.array_equal(q[i], x[3].reshape(-1)), (tag, k, i, "indices")


class Decode(Scenario):
    """payload slots -> decode_batch_dev, with reduced decodes at `drops` around it; pool: [(case, payload)], one geometry"""

    def __init__(self, hip, oracle, pool, n, iters, drops=()):
        super().__init__(hip, iters)
        self.pool, self.n, self.drops, self.oracle = pool, n, drops, oracle
        self.case = pool[0][0]
        self.fmt, self.cp = self.case.fmt_cp(hip.lib)
        self.rb = self.case.raw_bytes()
        self.stride = (max(len(p) for _, p in pool) + 64 + 255) // 256 * 256
        slots = np.zeros((len(pool), self.stride), np.uint8)
        for i, (_, p) in enumerate(pool):
            slots[i, :len(p)] = np.frombuffer(p, np.uint8)
        lens = np.array([len(p) for _, p in pool], np.int64)
        idx = [[(i + k) % len(pool) for i in range(n)] for k in range(iters)]
        self.idx = idx
        self.inputs["pay"] = _pin(np.stack([slots[ix].reshape(-1) for ix in idx]))
        self.inputs["len"] = _pin(np.stack([lens[ix].view(np.uint8) for ix in idx]))
        sizes = dict(pay=n * self.stride, len=n * 8, out=n * self.rb)
        for d in drops:
            assert self.case.raw_bytes(d) % 16 == 0
            sizes["red%d" % d] = n * self.case.raw_bytes(d)
        self.buffers(**sizes)
        self.finish(["out"] + ["red%d" % d for d in drops])
        self.full = [pr.full_picture(oracle, c, p) for c, p in pool]
        self.red = {d: [pr.reduced_picture(oracle, c, p, d) for c, p in pool] for d in drops}

    def call(self):
        h = self.hip
        for i, d in enumerate(self.drops):   # reduced, full, reduced: the calls are mixed on one context
            if i == 1:
                h.decode_batch_dev(self.p("pay"), self.stride, self.p("len"), self.n, self.fmt, self.cp, self.p("out"))
            h.decode_reduced_batch_dev(self.p("pay"), self.stride, self.p("len"), self.n, self.fmt, self.cp, d, self.p("red%d" % d))
        if len(self.drops) < 2:
            h.decode_batch_dev(self.p("pay"), self.stride, self.p("len"), self.n, self.fmt, self.cp, self.p("out"))

    def check(self, k, got, tag):
        _check_pictures((tag, k), got["out"], self.rb, [self.full[j] for j in self.idx[k]])
        for d in self.drops:
            _check_pictures((tag, k, d), got["red%d" % d], self.case.raw_bytes(d), [self.red[d][j] for j in self.idx[k]])


class Alternate(Scenario):
    """HQ_CBR and LD decodes in turn on one context: they share the cached budget table, which is uploaded at every change"""
    may_wait = True

    def __init__(self, hip, oracle, a, b, iters):
        super().__init__(hip, iters)
        self.parts = [a, b]
        self.outputs = []

    def load(self, k):
        for s in self.parts:
            s.load(k)

    def store(self, k):
        for s in self.parts:
            s.store(k)

    def call(self):
        for s in self.parts:
            s.call()

    def got(self, k):
        return [s.got(k) for s in self.parts]

    def check(self, k, got, tag):
        for s, g in zip(self.parts, got):
            s.check(k, g, (tag, s.case.mode))


class Fields(Scenario):
    """interlaced frames -> encode_fields_batch_dev -> decode_fields_batch_dev; the oracle codes the split fields"""

    def __init__(self, hip, oracle, c, n, iters, tff=True):
        import vc2hip_py
        super().__init__(hip, iters)
        self.n, self.tff, self.c = n, tff, c
        wb = c.get("wb", 2)
        kw = dict(c["kw"])
        if "s" in kw:
            kw["s"] //= 2
        self.case = pr.Case(oracle, c["w"], c["h"] // 2, c["cf"], c["bits"], c["kernel"], c["depth"], c["u"], c["a"], word_bytes=wb, **kw)
        self.ffmt = vc2hip_py.picture_format(c["w"], c["h"], c["cf"], c["bits"], wb)
        _, self.cp = self.case.fmt_cp(hip.lib)
        self.fb = 2 * self.case.raw_bytes()
        assert self.fb % 16 == 0
        raw = synth(c["w"], c["h"], c["cf"], c["bits"], 17, frames=POOL, word_bytes=wb)
        self.want = rr.recon(oracle, self.case, _fields(raw, c, POOL, tff), 2 * POOL)   # slot 2 f + j: field j of frame f
        frames = np.frombuffer(raw, np.uint8).reshape(POOL, self.fb)
        self.inputs["raw"] = _pin(np.stack([frames[self.sets(k, n)].reshape(-1) for k in range(iters)]))
        self.stride = (hip.max_payload_bytes(self.case.fmt_cp(hip.lib)[0], self.cp) + 64 + 255) // 256 * 256
        self.buffers(raw=n * self.fb, pay=2 * n * self.stride, len=2 * n * 8, out=n * self.fb)
        self.finish(["pay", "len", "out"])

    def call(self):
        h = self.hip
        h.encode_fields_batch_dev(self.p("raw"), self.n, self.ffmt, self.tff, self.cp, self.p("pay"), self.stride, self.p("len"))
        h.decode_fields_batch_dev(self.p("pay"), self.stride, self.p("len"), self.n, self.ffmt, self.tff, self.cp, self.p("out"))

    def check(self, k, got, tag):
        w = [self.want[2 * f + j] for f in self.sets(k, self.n) for j in (0, 1)]
        _check_slots((tag, k), got["pay"], got["len"], self.stride, [x[0] for x in w])
        frames = _frames(b"".join(x[1] for x in w), self.c, self.n, self.tff)
        _check_pictures((tag, k), got["out"], self.fb, [frames[i * self.fb:(i + 1) * self.fb] for i in range(self.n)])


class StreamChain(EncDec):
    """encode_batch_dev -> stream_write_dev -> stream_read_dev -> decode_batch_dev, nothing in between"""

    def __init__(self, hip, oracle, case, n, iters):
        import vc2hip_py
        super().__init__(hip, oracle, case, n, iters)
        raws = [self.inputs["raw"][k].numpy().tobytes() for k in range(iters)]
        self.streams = [oracle.encode_stream(case.params(), r, n) for r in raws]   # sequence header, pictures 0 .. n - 1, end of sequence
        seq = _seq_len(self.streams[0])
        self.cap = (max(len(s) for s in self.streams) + 255) // 256 * 256
        self.sp_w = vc2hip_py.stream_params(_major(self.streams[0]), 0, seq, True)
        self.sp_r = vc2hip_py.stream_params(_major(self.streams[0]))
        self.seq = seq
        self.buffers(stream=self.cap, slen=8, pay2=n * self.stride, len2=n * 8, pn=n * 4, cons=8)
        self.finish(["pay", "len", "out", "stream", "slen", "pay2", "len2", "pn", "cons"])

    def load(self, k):
        super().load(k)
        self.cur_len = len(self.streams[k]) - self.seq   # (the stream's length is the oracle's: the host never reads slen back)

    def call(self):
        h = self.hip
        h.encode_batch_dev(self.p("raw"), self.n, self.fmt, self.cp, self.p("pay"), self.stride, self.p("len"))
        h.stream_write_dev(self.p("pay"), self.stride, self.p("len"), self.n, self.cp, self.sp_w, self.p("stream"), self.cap, self.p("slen"))
        h.stream_read_dev(self.p("stream"), self.cur_len, self.n, self.cp, self.sp_r, self.p("pay2"), self.stride, self.p("len2"),
                          self.p("pn"), self.p("cons"))
        h.decode_batch_dev(self.p("pay2"), self.stride, self.p("len2"), self.n, self.fmt, self.cp, self.p("out"))

    def check(self, k, got, tag):
        super().check(k, got, tag)
        body = self.streams[k][self.seq:]
        assert int(got["slen"][:8].view(np.int64)[0]) == len(body), (tag, k, "stream length")
        assert got["stream"][:len(body)].tobytes() == body, (tag, k, "stream bytes")
        w = [self.want[j] for j in self.sets(k, self.n)]
        _check_slots((tag, k, "read"), got["pay2"], got["len2"], self.stride, [x[0] for x in w])
        assert got["pn"][:4 * self.n].view(np.uint32).tolist() == list(range(self.n)), (tag, k, "picture numbers")
        assert int(got["cons"][:8].view(np.int64)[0]) == len(body) - 13, (tag, k, "consumed")


# the geometries: small pictures (the oracle stays cheap), existing Cases where they exist
def _constq(oracle):
    return pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=7, scalar=2)          # test_gpu_recon / test_gpu_reduced


def _cbr(oracle):
    return pr.Case(oracle, 512, 128, "420", 12, "Fidelity", 2, 2, 4, mode="HQ_CBR", s=30000, scalar=1, prefix=3)   # recon_ref.MATRIX


def _ld(oracle):
    return pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, mode="LD", s=40000)     # recon_ref.MATRIX


def _whole_plane(oracle):
    case = pr.Case(oracle, 1024, 512, "444", 10, "DD97", 3, 512 >> 3, 1024 >> 3, q=24, scalar=4000)   # test_whole_plane_path
    assert (case.ys, case.xs) == (1, 1)
    return case


def _fields_case():
    from test_gpu_fields import CASES
    return CASES["constq_dd97_422_10"]


def _decode_pool(oracle, case, kind="synth", seed=41):
    raw = _pool_raw(case, kind, seed)
    return [(case, p) for p in pr.oracle_payloads(oracle, case, raw, POOL)]


SCENARIOS = ["constq3", "constq120", "cbr", "ld", "whole_plane", "recon", "reduced", "fields", "stream", "alternate",
             "constq3-STORE32", "constq3-NO_STREAM", "constq3-SINGLE_PASS_VBR", "cbr-STORE32", "cbr-NO_STREAM", "cbr-CBR_GENERAL"]
CAPTURED = ["constq3", "constq120", "cbr", "ld", "whole_plane", "recon", "reduced", "fields"]


def _scenario(name, hip, oracle, iters):
    base = name.split("-")[0]
    if base == "constq3":
        return EncDec(hip, oracle, _constq(oracle), 3, iters)
    if base == "constq120":
        return EncDec(hip, oracle, _constq(oracle), 120, iters)
    if base == "cbr":
        return EncDec(hip, oracle, _cbr(oracle), 3, iters, kind="noise")
    if base == "ld":
        return EncDec(hip, oracle, _ld(oracle), 3, iters)
    if base == "whole_plane":
        return EncDec(hip, oracle, _whole_plane(oracle), 2, iters)
    if base == "recon":
        return EncDec(hip, oracle, _constq(oracle), 3, iters, recon=True)
    if base == "reduced":
        return Decode(hip, oracle, _decode_pool(oracle, _constq(oracle)), 3, iters, drops=(1, 2))
    if base == "fields":
        return Fields(hip, oracle, _fields_case(), 3, iters)
    if base == "stream":
        return StreamChain(hip, oracle, _constq(oracle), 3, iters)
    if base == "alternate":
        return Alternate(hip, oracle, Decode(hip, oracle, _decode_pool(oracle, _cbr(oracle), "noise"), 3, iters),
                         Decode(hip, oracle, _decode_pool(oracle, _ld(oracle)), 3, iters), iters)
    raise KeyError(name)


def _make(name, oracle, iters, streams=1):
    torch = _torch()
    s = torch.cuda.Stream()
    hip = _ctx(s, *name.split("-")[1:])
    with torch.cuda.stream(s):
        scen = _scenario(name, hip, oracle, iters)
        if streams > 1:
            hip.set_streams(streams)
        # warm-up: one synchronised call of the same geometry and n -- no workspace growth or table upload after it
        scen.load(0)
        scen.call()
        s.synchronize()
        hip.sync()
    return torch, s, hip, scen


# ---------------------------------------------------------------------------------------------------------------------
# A. stream order with the host running ahead
# ---------------------------------------------------------------------------------------------------------------------
def _run_ahead(torch, s, hip, scen, tag, final_sync=True):
    with torch.cuda.stream(s):
        e_fill = Filler(s).run()
        for k in range(K):
            scen.load(k)
            scen.call()
            scen.store(k)
        ahead = not e_fill.query()   # every call was issued while the GPU had not even reached the first
        done = torch.cuda.Event()
        done.record(s)
        done.synchronize()
        if final_sync:
            hip.sync()
    for k in range(K):
        scen.check(k, scen.got(k), tag)
    if not scen.may_wait:
        assert ahead, (tag, "the host was not ahead of the GPU: a call waited, or the filler is too short")


@pytest.mark.parametrize("name", SCENARIOS)
def test_stream_order_with_the_host_ahead(oracle, name):
    torch, s, hip, scen = _make(name, oracle, K)
    _run_ahead(torch, s, hip, scen, name)
    hip.close()


@pytest.mark.parametrize("streams", [2, 3])
@pytest.mark.parametrize("mode", ["constq", "ld"])
def test_lanes_on_the_callers_stream(oracle, mode, streams):
    """set_streams(k) on a caller's stream: the oracle's bytes, and the caller's stream alone orders the results -- an event
    recorded on it after the calls is waited for, and the copies were enqueued on it; vc2hip_sync comes after the checks"""
    torch = _torch()
    s = torch.cuda.Stream()
    hip = _ctx(s)
    with torch.cuda.stream(s):
        scen = EncDec(hip, oracle, _constq(oracle), 7, K) if mode == "constq" else EncDec(hip, oracle, _ld(oracle), 5, K)
        hip.set_streams(streams)
        scen.load(0)
        scen.call()
        s.synchronize()
        hip.sync()
    _run_ahead(torch, s, hip, scen, (mode, streams), final_sync=False)
    hip.sync()
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# B. graph capture and replay
# ---------------------------------------------------------------------------------------------------------------------
def _capture(torch, s, hip, fn):
    """capture fn() on s once; a failure ends the capture and fails the test, with no further GPU call"""
    g = torch.cuda.CUDAGraph()
    before = hip.band_plane_bits()
    try:
        with torch.cuda.graph(g, stream=s):
            fn()                       # (a call that does not return VC2HIP_OK raises)
    except BaseException as e:         # noqa: BLE001 -- whatever ended the capture
        pytest.fail("graph capture failed: %r" % (e,))
    return g, before


def _replay_and_check(torch, s, hip, scen, g, tag, rounds=R):
    with torch.cuda.stream(s):
        for r in range(rounds):
            scen.load(r)
            g.replay()
            scen.store(r)
        s.synchronize()
        hip.sync()
    for r in range(rounds):
        scen.check(r, scen.got(r), (tag, "replay"))


@pytest.mark.parametrize("name", CAPTURED)
def test_capture_and_replay(oracle, name):
    torch, s, hip, scen = _make(name, oracle, R)
    bits0 = hip.band_plane_bits()
    g, before = _capture(torch, s, hip, scen.call)
    assert hip.band_plane_bits() == before == bits0, (name, "the band-plane form changed during the capture")
    _replay_and_check(torch, s, hip, scen, g, name)
    hip.close()


@pytest.mark.parametrize("streams", [2])
@pytest.mark.parametrize("mode", ["constq", "ld"])
def test_capture_with_lanes(oracle, mode, streams):
    """include/vc2hip.h: lanes under capture are supported -- parallel branches of the graph, exact on every replay"""
    torch = _torch()
    s = torch.cuda.Stream()
    hip = _ctx(s)
    with torch.cuda.stream(s):
        scen = EncDec(hip, oracle, _constq(oracle), 7, R) if mode == "constq" else EncDec(hip, oracle, _ld(oracle), 5, R)
        hip.set_streams(streams)
        scen.load(0)
        scen.call()
        s.synchronize()
        hip.sync()
    g, before = _capture(torch, s, hip, scen.call)
    assert hip.band_plane_bits() == before
    _replay_and_check(torch, s, hip, scen, g, (mode, streams))
    # and an eager call on the same lanes afterwards
    with torch.cuda.stream(s):
        scen.load(1)
        scen.call()
        scen.store(1)
        s.synchronize()
        hip.sync()
    scen.check(1, scen.got(1), (mode, streams, "eager after the capture"))
    hip.close()


def _form_case(oracle, q, bits=16):
    return pr.Case(oracle, 2048, 128, "422", bits, "DD97", 3, 1, 2, q=q, scalar=8)   # test_band_plane_form_follows...'s geometry


@pytest.mark.parametrize("flag,bits", [("PLANES8_ALWAYS", 8), ("PLANES8_NEVER", 16)])
def test_capture_with_a_frozen_plane_form(oracle, flag, bits):
    """vc2hip_create_on_stream_with_flags: the form is fixed, the captured decode is replayed on content the form was not
    chosen for -- 16-bit noise at the lowest index that keeps it inside the reference's code domain (q = 8: quantised values
    up to 65533, beyond a byte and beyond the 16-bit store: both escapes; at q = 0 they pass 65534, which VLC.h:27 excludes)
    and smooth pictures"""
    torch = _torch()
    noise_case, smooth_case = _form_case(oracle, 8), _form_case(oracle, 30)
    planes = pr.quantised_planes(oracle, noise_case, pr.oracle_payloads(oracle, noise_case, noise_frame(2048, 128, "422", 16, 3))[0])[:3]
    assert 32767 < max(int(np.abs(x).max()) for x in planes) <= 65534
    noise = noise_frame(2048, 128, "422", 16, 3)
    smooth = synth(2048, 128, "422", 16, 4)
    pool = [(smooth_case, pr.oracle_payloads(oracle, smooth_case, smooth)[0]), (noise_case, pr.oracle_payloads(oracle, noise_case, noise)[0]),
            (noise_case, pr.oracle_payloads(oracle, noise_case, smooth)[0])]
    s = torch.cuda.Stream()
    hip = _ctx(s, flag)
    with torch.cuda.stream(s):
        scen = Decode(hip, oracle, pool, 2, R)
        scen.load(0)
        scen.call()
        s.synchronize()
        hip.sync()
    assert hip.band_plane_bits() == bits, "the geometry has no band planes of the form asked for: the test would show nothing"
    g, before = _capture(torch, s, hip, scen.call)
    assert hip.band_plane_bits() == before == bits
    _replay_and_check(torch, s, hip, scen, g, flag)
    hip.close()


def test_an_error_in_a_replay_surfaces_at_sync_and_the_next_replay_is_clean(oracle):
    """test_gpu_recon.py::test_escalar_surfaces...'s input: noise at q = 0 with scalar 1 (VC2HIP_ESCALAR, a library error code)"""
    from vc2hip_py import Vc2HipError
    torch = _torch()
    case = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=0, scalar=1)
    s = torch.cuda.Stream()
    hip = _ctx(s)
    with torch.cuda.stream(s):
        scen = EncDec(hip, oracle, case, 2, R, seed=22)
        bad = _pin(np.frombuffer(noise_frame(1024, 64, "422", 10, 3) * 2, np.uint8))
        scen.load(0)
        scen.call()
        s.synchronize()
        hip.sync()
    g, _ = _capture(torch, s, hip, scen.call)
    with torch.cuda.stream(s):
        scen.load(0); g.replay(); scen.store(0)
        s.synchronize()
        hip.sync()
        scen.dev["raw"][:bad.numel()].copy_(bad, non_blocking=True)
        g.replay()
        s.synchronize()
        with pytest.raises(Vc2HipError) as e:
            hip.sync()
        assert e.value.code == ESCALAR
        scen.load(1); g.replay(); scen.store(1)
        s.synchronize()
        hip.sync()                     # clean again
    for r in (0, 1):
        scen.check(r, scen.got(r), ("around the error", r))
    hip.close()


def test_the_adaptive_form_still_follows_the_batches_after_a_capture(oracle):
    """a capture records no look and consumes none; the first eager decode after it takes the look the warm-up left and
    records the next: coarse pictures (few payload bits per sample, by the oracle's lengths) turn the planes to bytes, then
    10-bit noise at q = 0 (ten bits per sample and more) turns them back -- a pending look that stuck would freeze the form"""
    torch = _torch()
    coarse, fine = _form_case(oracle, 24, bits=10), _form_case(oracle, 0, bits=10)
    cpool = [(coarse, p) for p in pr.oracle_payloads(oracle, coarse, synth(2048, 128, "422", 10, 5, frames=3), 3)]
    fpool = [(fine, pr.oracle_payloads(oracle, fine, noise_frame(2048, 128, "422", 10, 8 + i))[0]) for i in range(3)]
    samples = 2 * 2048 * 128
    assert all(8 * len(p) / samples < 5.0 for _, p in cpool) and all(8 * len(p) / samples > 8.0 for _, p in fpool)
    s = torch.cuda.Stream()
    hip = _ctx(s)
    with torch.cuda.stream(s):
        a, b = Decode(hip, oracle, cpool, 3, R), Decode(hip, oracle, fpool, 3, R)

        def eager(scen, r):
            scen.load(r); scen.call(); scen.store(r)
            s.synchronize()
            hip.sync()
            scen.check(r, scen.got(r), "eager")
            return hip.band_plane_bits()

        b.load(0); b.call(); s.synchronize(); hip.sync()      # (sizes the workspace for the larger payloads)
        assert eager(a, 0) in (8, 16)                           # a look is pending behind this call
    g, before = _capture(torch, s, hip, a.call)
    assert hip.band_plane_bits() == before
    _replay_and_check(torch, s, hip, a, g, "adaptive")
    with torch.cuda.stream(s):
        eager(a, 1)                                             # takes the pending look (coarse or noise), records its own
        assert eager(a, 2) == 8, "coarse pictures did not turn the band planes to bytes: the look is stuck"
        eager(b, 0)
        assert eager(b, 1) == 16, "noise did not turn the band planes back to 16 bits: the look is stuck"
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# C. "never waits", measured
# ---------------------------------------------------------------------------------------------------------------------
def _lane_scenarios(oracle, hip, iters):
    return EncDec(hip, oracle, _constq(oracle), 7, iters)


@pytest.mark.parametrize("name", [n for n in SCENARIOS if n != "alternate"] + ["lanes2"])
def test_the_calls_never_wait(oracle, name):
    """filler, the calls, an event: the event must not be complete when the calls have returned.  (`alternate` is absent: the
    budget table changes between its calls, which the contract lets wait.)"""
    if name == "lanes2":
        torch = _torch()
        s = torch.cuda.Stream()
        hip = _ctx(s)
        with torch.cuda.stream(s):
            scen = _lane_scenarios(oracle, hip, 1)
            hip.set_streams(2)
            scen.load(0); scen.call(); s.synchronize(); hip.sync()
    else:
        torch, s, hip, scen = _make(name, oracle, 1)
    with torch.cuda.stream(s):
        scen.load(0)
        s.synchronize()
        e_fill = Filler(s).run()
        scen.call()
        e = torch.cuda.Event()
        e.record(s)
        waited, filler_done = e.query(), e_fill.query()
        scen.store(0)
        s.synchronize()
        hip.sync()
    scen.check(0, scen.got(0), name)
    assert not waited and not filler_done, (name, "the call waited for the stream")
    hip.close()


def test_the_filler_outlasts_every_call(oracle):
    """the sizing of the filler, measured on every run: its duration on the stream against the host time of each scenario's
    calls on an idle stream (median of 20), with the factor of 20 the never-waits assertions rest on"""
    torch = _torch()
    s0 = torch.cuda.Stream()
    with torch.cuda.stream(s0):
        f = Filler(s0)
        f.run(); s0.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s0); f.run(); b.record(s0); s0.synchronize()
    filler_ms = a.elapsed_time(b)
    worst = ("", 0.0)
    for name in [n for n in SCENARIOS if n != "alternate"]:
        torch, s, hip, scen = _make(name, oracle, 1)
        times = []
        with torch.cuda.stream(s):
            for _ in range(20):
                s.synchronize()
                t0 = time.perf_counter()
                scen.call()
                times.append(time.perf_counter() - t0)
            s.synchronize()
            hip.sync()
        med = 1e3 * float(np.median(times))
        print("host time of %-24s median %.3f ms (filler %.1f ms)" % (name, med, filler_ms))
        worst = max(worst, (name, med), key=lambda x: x[1])
        hip.close()
    print("filler %.1f ms; slowest call %s, median %.3f ms; factor %.0f" % (filler_ms, worst[0], worst[1], filler_ms / worst[1]))
    assert filler_ms >= 20 * worst[1], (filler_ms, worst)
