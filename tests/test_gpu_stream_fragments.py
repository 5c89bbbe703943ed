"""GPU tests of vc2hip_stream_write_fragments_dev: the slots + lengths of the batch calls to fragmented pictures in device
memory.  HQ_CBR and LD byte for byte against the oracle's fragmented streams (EncodeStream -F); HQ_ConstQ, which the oracle's
encoder does not fragment, against tests/frag_ref.py (pinned to the oracle by tests/test_frag_ref.py), through
vc2hip_stream_read_dev and through the oracle's decoder; the parse-info chain and the unit table; the bounds, the errors the
kernels report and the arguments the host refuses; field pictures; a caller's stream and graph capture; many pictures; and
pictures of more slices than the cut kernel holds in LDS."""
import functools

import numpy as np
import pytest

import frag_ref
from synth import synth
from test_frag_ref import ld_budgets, lengths, oracle_fragmented, slice_sizes
from test_gpu_stream_dev import CASES, _dev, _major, _seq_len, _setup, _stride
from vc2lib import make_params

pytestmark = pytest.mark.gpu

EINVAL, ECAP, ESTREAM, ESYNTAX = -1, -9, -10, -12
N = 3
DEV = "cuda:0"


def _torch():
    return pytest.importorskip("torch")


def _encode(hip, raw, n, fmt, cp):
    """encode_batch_dev, synchronised: (slots, lens, stride) on the device"""
    torch = _torch()
    stride = _stride(hip, fmt, cp)
    d_raw = _dev(raw)
    d_pay = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    d_len = torch.zeros(n, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    hip.encode_batch_dev(d_raw.data_ptr(), n, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    hip.sync()
    return d_pay, d_len, stride


def _host_slots(d_pay, d_len, stride):
    lens = d_len.cpu().tolist()
    pay = d_pay.cpu().numpy()
    return [pay[k * stride:k * stride + n].tobytes() for k, n in enumerate(lens)]


def _bound(lens, ns, n, tp=16):
    """the header's worst case: (stream bytes, units)"""
    return sum(lens) + n * (21 + tp) + n * ns * 25 + 13, n * (ns + 1) + 1


def _frag(hip, d_pay, stride, d_len, n, cp, flen, first=0, prev=0, eos=True, cap=None, guard=64, unit_cap=None, table=True,
          major=3, bound=None):
    """stream_write_fragments_dev, nothing synchronised: the device buffers (0xA5 behind cap, -1 behind unit_cap)"""
    import vc2hip_py
    torch = _torch()
    ns = cp.y_slices * cp.x_slices
    bytes_, units = bound or _bound([stride] * n, ns, n)
    cap = bytes_ + 64 if cap is None else cap
    unit_cap = units if unit_cap is None else unit_cap
    b = dict(stream=torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device=DEV),
             slen=torch.full((1,), -1, dtype=torch.int64, device=DEV),
             units=torch.full((unit_cap + 8,), -1, dtype=torch.int64, device=DEV),
             count=torch.full((1,), -1, dtype=torch.int64, device=DEV), cap=cap, unit_cap=unit_cap)
    torch.cuda.synchronize()
    sp = vc2hip_py.stream_params(major, first, prev, eos)
    t = (b["units"].data_ptr(), unit_cap, b["count"].data_ptr()) if table else (None, 0, None)
    hip.stream_write_fragments_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, cp, sp, flen, b["stream"].data_ptr(), cap,
                                   b["slen"].data_ptr(), *t)
    return b


def _result(hip, b):
    """after the sync: (stream bytes up to the length, unit offsets up to the count)"""
    hip.sync()
    return (b["stream"][:int(b["slen"].item())].cpu().numpy().tobytes(), b["units"][:int(b["count"].item())].cpu().tolist())


@functools.lru_cache(maxsize=None)
def _case(hip, oracle, name, n=N, seed=5):
    """one case's pictures coded once: (fmt, cp, raw, device slots, device lens, stride, host slots)"""
    fmt, cp, p, raw = _setup(hip, CASES[name], n=n, seed=seed)
    d_pay, d_len, stride = _encode(hip, raw, n, fmt, cp)
    return fmt, cp, raw, d_pay, d_len, stride, _host_slots(d_pay, d_len, stride)


def _walk(stream, eos):
    """the parse-info chain forwards: [(offset, code, next, prev)]"""
    out, pos = [], 0
    while pos < len(stream):
        assert stream[pos:pos + 4] == b"BBCD", pos
        code, nxt, prev = stream[pos + 4], int.from_bytes(stream[pos + 5:pos + 9], "big"), int.from_bytes(stream[pos + 9:pos + 13], "big")
        out.append((pos, code, nxt, prev))
        if code == 0x10:
            assert eos and nxt == 0 and pos + 13 == len(stream)
            break
        pos += nxt
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. HQ_CBR and LD: the oracle's fragmented stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cbr_legall_420_8", "ld_legall_420_8"])
def test_fragments_are_the_oracle_stream(hip, oracle, case):
    fmt, cp, raw, d_pay, d_len, stride, slots = _case(hip, oracle, case)
    for flen in lengths(oracle, cp, slots):
        seq, want = oracle_fragmented(oracle, CASES[case], raw, N, flen)
        got, units = _result(hip, _frag(hip, d_pay, stride, d_len, N, cp, flen, prev=len(seq)))
        assert got == want, (case, flen)
        assert units == [u[0] for u in _walk(got, True)], (case, flen)


# ---------------------------------------------------------------------------------------------------------------------
# 2. HQ_ConstQ: frag_ref, then back through stream_read_dev and through the oracle's decoder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["constq_dd97_422_10", "padded_odd_prefix1_scalar3", "fidelity_444_12"])
def test_constq_fragments_are_frag_ref_and_read_back(hip, oracle, case):
    torch = _torch()
    c = CASES[case]
    fmt, cp, raw, d_pay, d_len, stride, slots = _case(hip, oracle, case)
    big = max(max(slice_sizes(oracle, cp, s)) for s in slots)
    assert big > 2, "a case whose slices carry nothing"
    # the sequence header of an HQ_CBR fragmented stream of the same video format (major version 3); the unfragmented decode
    kw = {k: v for k, v in c["kw"].items() if k in ("scalar", "prefix")}
    p_cbr = make_params(c["w"], c["h"], c["cf"], c["bits"], c["kernel"], c["depth"], c["u"], c["a"], word_bytes=c.get("wb", 2),
                        mode="HQ_CBR", s=len(slots[0]), fragment_length=1000, **kw)
    s_cbr = oracle.encode_stream(p_cbr, raw, 1)
    seq = s_cbr[:_seq_len(s_cbr)]
    assert _major(seq) == 3
    p = make_params(c["w"], c["h"], c["cf"], c["bits"], c["kernel"], c["depth"], c["u"], c["a"], word_bytes=c.get("wb", 2), **c["kw"])
    whole = oracle.encode_stream(p, raw, N)
    want_pictures = oracle.decode_stream(p, whole, N)[0]
    for flen in lengths(oracle, cp, slots) + [big - 1]:      # (below the largest slice: it travels alone)
        want, want_units = frag_ref.fragment_stream(slots, cp, flen, 7, len(seq), True)
        got, units = _result(hip, _frag(hip, d_pay, stride, d_len, N, cp, flen, first=7, prev=len(seq)))
        assert got == want and units == want_units, (case, flen)
        # read: slots up to each length, the lengths, the picture numbers
        d_stream = _dev(got)
        d_pay2 = torch.zeros_like(d_pay)
        d_len2 = torch.zeros_like(d_len)
        d_pn = torch.zeros(N, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        import vc2hip_py
        hip.stream_read_dev(d_stream.data_ptr(), len(got), N, cp, vc2hip_py.stream_params(3), d_pay2.data_ptr(), stride,
                            d_len2.data_ptr(), d_pn.data_ptr(), None)
        hip.sync()
        assert _host_slots(d_pay2, d_len2, stride) == slots and d_pn.cpu().tolist() == [7, 8, 9], (case, flen)
        assert oracle.decode_stream(p, seq + got, N)[0] == want_pictures, (case, flen)


# ---------------------------------------------------------------------------------------------------------------------
# 3. chain and numbering
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eos", [True, False])
def test_chain_numbers_and_unit_table(hip, oracle, eos):
    fmt, cp, raw, d_pay, d_len, stride, slots = _case(hip, oracle, "constq_dd97_422_10")
    flen = lengths(oracle, cp, slots)[1]
    b = _frag(hip, d_pay, stride, d_len, N, cp, flen, first=2 ** 32 - 2, prev=77, eos=eos)
    got, units = _result(hip, b)
    walk = _walk(got, eos)
    assert walk[0][3] == 77
    assert (walk[-1][1] == 0x10) == eos
    for a, u in zip(walk, walk[1:]):          # forwards: every unit names the size of the one before
        assert u[3] == a[2] and u[0] == a[0] + a[2]
    pos, back = walk[-1][0], []               # backwards from the last unit
    while True:
        back.append(pos)
        if pos == 0:
            break
        pos -= int.from_bytes(got[pos + 9:pos + 13], "big")
        assert pos >= 0
    assert back[::-1] == [u[0] for u in walk] == units
    assert int(b["count"].item()) == len(walk)
    end = walk[-1][0] + (13 if eos else walk[-1][2])
    assert int(b["slen"].item()) == end == len(got)
    numbers = [int.from_bytes(got[o + 13:o + 17], "big") for o, code, _, _ in walk if code == 0xEC]
    assert sorted(set(numbers), key=numbers.index) == [2 ** 32 - 2, 2 ** 32 - 1, 0]
    assert got == frag_ref.fragment_stream(slots, cp, flen, 2 ** 32 - 2, 77, eos)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 4. bounds
# ---------------------------------------------------------------------------------------------------------------------
def test_caps(hip, oracle):
    import vc2hip_py
    fmt, cp, raw, d_pay, d_len, stride, slots = _case(hip, oracle, "constq_dd97_422_10")
    flen = lengths(oracle, cp, slots)[1]
    full, units = frag_ref.fragment_stream(slots, cp, flen, 0, 0, True)
    mid = units[len(units) // 2]
    assert full[mid + 4] == 0xEC and int.from_bytes(full[mid + 19:mid + 21], "big") > 0      # a slice fragment
    for cap, unit_cap in [(mid + 7, None), (mid + 16, None), (mid + 25 + 37, None), (len(full) - 5, None), (None, len(units) - 1)]:
        b = _frag(hip, d_pay, stride, d_len, N, cp, flen, cap=cap, unit_cap=unit_cap)
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            hip.sync()
        assert e.value.code == ECAP, (cap, unit_cap)
        assert int(b["slen"].item()) == len(full) and int(b["count"].item()) == len(units)
        got = b["stream"].cpu().numpy().tobytes()
        k = min(b["cap"], len(full))
        assert got[:k] == full[:k], (cap, unit_cap)
        assert got[b["cap"]:] == b"\xa5" * 64, (cap, unit_cap)
        table = b["units"].cpu().tolist()
        k = min(b["unit_cap"], len(units))
        assert table[:k] == units[:k] and table[k:] == [-1] * (len(table) - k), (cap, unit_cap)
    assert _result(hip, _frag(hip, d_pay, stride, d_len, N, cp, flen)) == (full, units)
    # without the unit table
    b = _frag(hip, d_pay, stride, d_len, N, cp, flen, table=False)
    hip.sync()
    assert b["stream"][:int(b["slen"].item())].cpu().numpy().tobytes() == full
    assert int(b["count"].item()) == -1 and b["units"].cpu().tolist() == [-1] * len(b["units"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors the kernels find (each bounded and reported; the context works on the next call)
# ---------------------------------------------------------------------------------------------------------------------
def _last_length_byte(pay, cp):
    """offset of the third length byte of the last slice"""
    sizes = frag_ref.slice_sizes_hq(pay, cp.y_slices * cp.x_slices, cp.prefix, cp.scalar)
    q = sum(sizes[:-1]) + cp.prefix + 1
    for _ in range(2):
        q += 1 + pay[q] * cp.scalar
    return q


def test_errors_found_on_the_device(hip, oracle):
    import vc2hip_py
    torch = _torch()
    fmt, cp, raw, d_pay, d_len, stride, slots = _case(hip, oracle, "constq_dd97_422_10")
    flen = 700
    want = frag_ref.fragment_stream(slots, cp, flen, 0, 0, True)

    def fails(code, pay, lens, cpx=cp, st=stride, n=N, **kw):
        b = _frag(hip, pay, st, lens, n, cpx, flen, **kw)
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            hip.sync()
        assert e.value.code == code, str(e.value)
        assert b["stream"][b["cap"]:].cpu().tolist() == [0xA5] * 64
        assert _result(hip, _frag(hip, d_pay, stride, d_len, N, cp, flen)) == want      # the context works normally
        return str(e.value)

    # the last length byte of picture 1 raised by one: the walk ends behind the length
    bad = d_pay.clone()
    at = _last_length_byte(slots[1], cp)
    assert slots[1][at] < 255
    bad[stride + at] += 1
    fails(ESTREAM, bad, d_len)
    # a length one short: the walk does not end on it
    short = d_len.clone()
    short[2] -= 1
    fails(ESTREAM, d_pay, short)
    # a length beyond the slot
    over = d_len.clone()
    over[0] = stride + 16
    fails(ECAP, d_pay, over)
    # one slice of 1 + 3 * (1 + 255 * 128) = 97,924 bytes, built by hand: no fragment's 16-bit data length holds it
    one = vc2hip_py.CodingParams(cp.kernel, cp.depth, 1, 1, cp.mode, cp.q_index, 0, 0, 128)
    body = bytes([3]) + (bytes([255]) + bytes(255 * 128)) * 3
    assert len(body) == 97924
    st1 = (len(body) + 255) // 256 * 256
    d_one = _dev(body + bytes(st1 - len(body)))
    d_one_len = torch.tensor([len(body)], dtype=torch.int64, device=DEV)
    text = fails(ESYNTAX, d_one, d_one_len, cpx=one, st=st1, n=1, bound=(st1 + 200, 3))
    assert "65535" in text
    # LD: a length that is not the table's sum
    fmt_l, cp_l, raw_l, d_pay_l, d_len_l, stride_l, slots_l = _case(hip, oracle, "ld_legall_420_8")
    short = d_len_l.clone()
    short[1] -= 1
    fails(ESTREAM, d_pay_l, short, cpx=cp_l, st=stride_l)


# ---------------------------------------------------------------------------------------------------------------------
# 6. arguments the host refuses: VC2HIP_EINVAL, nothing launched, no output byte touched
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(hip, oracle):
    import vc2hip_py
    torch = _torch()
    fmt, cp, raw, d_pay, d_len, stride, slots = _case(hip, oracle, "constq_dd97_422_10")
    cap = N * stride + 4096
    d_stream = torch.full((cap + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    d_slen = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    d_units = torch.full((64,), -1, dtype=torch.int64, device=DEV)
    d_count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    sp3 = vc2hip_py.stream_params(3, 0, 0, True)

    def cpx(**kw):
        f = dict(kernel=cp.kernel, depth=cp.depth, y_slices=cp.y_slices, x_slices=cp.x_slices, mode=cp.mode, q_index=cp.q_index,
                 compressed_bytes=cp.compressed_bytes, prefix=cp.prefix, scalar=cp.scalar)
        f.update(kw)
        return vc2hip_py.CodingParams(*[f[k] for k in ("kernel", "depth", "y_slices", "x_slices", "mode", "q_index",
                                                        "compressed_bytes", "prefix", "scalar")])

    good = dict(pay=d_pay.data_ptr(), stride=stride, lens=d_len.data_ptr(), n=N, cp=cp, sp=sp3, flen=1400,
                stream=d_stream.data_ptr(), cap=cap, slen=d_slen.data_ptr(), units=d_units.data_ptr(), unit_cap=64,
                count=d_count.data_ptr())
    refusals = [
        dict(sp=vc2hip_py.stream_params(2, 0, 0, True)), dict(sp=vc2hip_py.stream_params(0, 0, 0, True)),
        dict(flen=0), dict(flen=-1), dict(flen=65536),
        dict(cp=cpx(x_slices=65536)), dict(cp=cpx(y_slices=65536)),
        dict(units=None), dict(count=None), dict(unit_cap=0), dict(units=None, unit_cap=0), dict(units=None, count=None),
        dict(unit_cap=0, count=None),
        dict(stream=d_stream.data_ptr() + 8), dict(pay=d_pay.data_ptr() + 8), dict(stride=stride + 8),
        dict(lens=d_len.data_ptr() + 4), dict(slen=d_slen.data_ptr() + 4),
        # what vc2hip_stream_write_dev refuses
        dict(n=0), dict(pay=None), dict(lens=None), dict(stream=None), dict(slen=None),
        dict(cp=cpx(kernel=9)), dict(cp=cpx(scalar=0)), dict(cp=cpx(x_slices=0)), dict(cp=cpx(mode=2, compressed_bytes=0)),
    ]
    for r in refusals:
        a = dict(good, **r)
        with pytest.raises(vc2hip_py.Vc2HipError) as e:
            hip.stream_write_fragments_dev(a["pay"], a["stride"], a["lens"], a["n"], a["cp"], a["sp"], a["flen"], a["stream"],
                                           a["cap"], a["slen"], a["units"], a["unit_cap"], a["count"])
        assert e.value.code == EINVAL, r
    hip.sync()
    assert bool((d_stream == 0xA5).all()) and d_slen.item() == -1 and d_count.item() == -1 and bool((d_units == -1).all())
    hip.stream_write_fragments_dev(*[good[k] for k in ("pay", "stride", "lens", "n", "cp", "sp", "flen", "stream", "cap", "slen")])
    hip.sync()
    assert d_stream[:int(d_slen.item())].cpu().numpy().tobytes() == frag_ref.fragment_stream(slots, cp, 1400, 0, 0, True)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 7. field pictures
# ---------------------------------------------------------------------------------------------------------------------
def test_interlaced_ld_fields(hip, oracle):
    import vc2hip_py
    torch = _torch()
    w, h, n = 128, 64, 2
    raw = synth(w, h, "422", 8, 63, frames=n, word_bytes=1)
    p = make_params(w, h, "422", 8, "LeGall", 2, 2, 2, mode="LD", s=8000, word_bytes=1, interlaced=True, fragment_length=500)
    stream = oracle.encode_stream(p, raw, n)
    seq = stream[:_seq_len(stream)]
    ffmt = vc2hip_py.picture_format(w, h, "422", 8, 1)
    fmt = vc2hip_py.picture_format(w, h // 2, "422", 8, 1)
    cp = vc2hip_py.coding_params(hip.lib, fmt, "LeGall", 2, 2, 2, mode="LD", s=4000)
    stride = _stride(hip, fmt, cp)
    d_frames = _dev(raw)
    d_pay = torch.zeros(2 * n * stride, dtype=torch.uint8, device=DEV)
    d_len = torch.zeros(2 * n, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    hip.encode_fields_batch_dev(d_frames.data_ptr(), n, ffmt, 1, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    got, units = _result(hip, _frag(hip, d_pay, stride, d_len, 2 * n, cp, 500, prev=len(seq)))
    assert seq + got == stream
    assert units == [u[0] for u in _walk(got, True)]


# ---------------------------------------------------------------------------------------------------------------------
# 8. a caller's stream and graph capture: encode -> write_fragments -> read -> decode with no synchronisation in between
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["constq_dd97_422_10", "ld_legall_420_8"])
def test_callers_stream_and_capture(oracle, case):
    import vc2hip_py
    torch = _torch()
    c = CASES[case]
    s = torch.cuda.Stream()
    hip = vc2hip_py.Vc2Hip(stream=s.cuda_stream, flags=vc2hip_py.FLAGS["PLANES8_NEVER"])
    rounds = 3                                       # eager (the warm-up), then two replays
    fmt, cp, p, raw = _setup(hip, c, n=N * rounds, seed=41)
    rb = hip.raw_picture_bytes(fmt)
    stride = _stride(hip, fmt, cp)
    ns = cp.y_slices * cp.x_slices
    cap, unit_cap = _bound([stride] * N, ns, N)
    flen = 300
    sp = vc2hip_py.stream_params(3, 5, 0, True)
    pinned = torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(rounds, N * rb).pin_memory()
    out = {k: [] for k in ("stream", "slen", "units", "count", "dec", "pay2", "len2")}
    with torch.cuda.stream(s):
        d = dict(raw=torch.zeros(N * rb, dtype=torch.uint8, device=DEV), pay=torch.zeros(N * stride, dtype=torch.uint8, device=DEV),
                 len=torch.zeros(N, dtype=torch.int64, device=DEV), stream=torch.zeros(cap, dtype=torch.uint8, device=DEV),
                 slen=torch.zeros(1, dtype=torch.int64, device=DEV), units=torch.zeros(unit_cap, dtype=torch.int64, device=DEV),
                 count=torch.zeros(1, dtype=torch.int64, device=DEV), pay2=torch.zeros(N * stride, dtype=torch.uint8, device=DEV),
                 len2=torch.zeros(N, dtype=torch.int64, device=DEV), dec=torch.zeros(N * rb, dtype=torch.uint8, device=DEV))

        def chain():
            hip.encode_batch_dev(d["raw"].data_ptr(), N, fmt, cp, d["pay"].data_ptr(), stride, d["len"].data_ptr())
            hip.stream_write_fragments_dev(d["pay"].data_ptr(), stride, d["len"].data_ptr(), N, cp, sp, flen, d["stream"].data_ptr(),
                                           cap, d["slen"].data_ptr(), d["units"].data_ptr(), unit_cap, d["count"].data_ptr())
            # (the reader takes the whole buffer: the units end with the end of sequence, zeros follow)
            hip.stream_read_dev(d["stream"].data_ptr(), cap, N, cp, vc2hip_py.stream_params(3), d["pay2"].data_ptr(), stride,
                                d["len2"].data_ptr(), None, None)
            hip.decode_batch_dev(d["pay2"].data_ptr(), stride, d["len2"].data_ptr(), N, fmt, cp, d["dec"].data_ptr())

        def keep():
            for k in out:
                t = torch.empty(d[k].shape, dtype=d[k].dtype).pin_memory()
                t.copy_(d[k], non_blocking=True)
                out[k].append(t)

        d["raw"].copy_(pinned[0], non_blocking=True)
        chain()                                      # eager, and the warm-up of the capture
        keep()
        s.synchronize()
        hip.sync()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=s):
                chain()
        except BaseException as e:                   # noqa: BLE001 -- whatever ended the capture
            pytest.fail("graph capture failed: %r" % (e,))
        for r in (1, 2):
            d["raw"].copy_(pinned[r], non_blocking=True)
            g.replay()
            keep()
        s.synchronize()
        hip.sync()
    for r in range(rounds):
        pics = raw[r * N * rb:(r + 1) * N * rb]
        whole = oracle.encode_stream(p, pics, N)
        hl = len(hip.picture_header(cp, _major(whole), 0))
        slots = [b[hl:] for code, b in _units_of(whole) if code in (0xE8, 0xC8)]
        want, want_units = frag_ref.fragment_stream(slots, cp, flen, 5, 0, True, ld_budgets(oracle, cp))
        assert int(out["slen"][r].item()) == len(want) and int(out["count"][r].item()) == len(want_units), (case, r)
        assert out["stream"][r][:len(want)].numpy().tobytes() == want, (case, r)
        assert out["units"][r][:len(want_units)].tolist() == want_units, (case, r)
        assert _host_slots(out["pay2"][r], out["len2"][r], stride) == slots, (case, r)
        assert out["dec"][r].numpy().tobytes() == oracle.decode_stream(p, whole, N)[0], (case, r)
    hip.close()


def _units_of(stream):
    from test_gpu_stream_dev import _units
    return _units(stream)


# ---------------------------------------------------------------------------------------------------------------------
# 9. many pictures, small
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ld", "constq"])
def test_seventy_pictures(hip, oracle, case):
    c = (CASES["ld_legall_420_8"] if case == "ld" else
         dict(w=64, h=32, cf="420", bits=8, kernel="DD97", depth=2, u=2, a=2, wb=1, kw=dict(q=8, scalar=1)))
    n = 70
    fmt, cp, p, raw = _setup(hip, c, n=n, seed=9)
    d_pay, d_len, stride = _encode(hip, raw, n, fmt, cp)
    slots = _host_slots(d_pay, d_len, stride)
    for flen in (1, 150):
        want = frag_ref.fragment_stream(slots, cp, flen, 2 ** 32 - 30, 13, True, ld_budgets(oracle, cp))
        assert _result(hip, _frag(hip, d_pay, stride, d_len, n, cp, flen, first=2 ** 32 - 30, prev=13)) == want, (case, flen)


# ---------------------------------------------------------------------------------------------------------------------
# 10. pictures of many slices, built by hand (no encode): every slice is its index byte and three zero lengths, but for a
# few that carry bytes.  198 x 180 slices are the most the cut holds in LDS; 200 x 200 take its path through device memory
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ys,xs", [(180, 198), (200, 200)])
def test_many_slices(hip, ys, xs):
    import vc2hip_py
    torch = _torch()
    cp = vc2hip_py.CodingParams(1, 2, ys, xs, 0, 0, 0, 0, 1)
    ns = ys * xs
    rng = np.random.default_rng(ys)
    slots = []
    for k in range(2):
        parts = []
        for i in range(ns):
            ln = [int(v) for v in rng.integers(0, 40, 3)] if (i + k) % 7 == 0 else [0, 0, 0]
            parts.append(bytes([i & 63]) + b"".join(bytes([v]) + bytes([i & 255]) * v for v in ln))
        slots.append(b"".join(parts))
    stride = (max(len(s) for s in slots) + 255) // 256 * 256
    d_pay = _dev(b"".join(s + bytes(stride - len(s)) for s in slots))
    d_len = torch.tensor([len(s) for s in slots], dtype=torch.int64, device=DEV)
    for flen in (10, 1400, 65535):
        want = frag_ref.fragment_stream(slots, cp, flen, 0, 0, True)
        assert _result(hip, _frag(hip, d_pay, stride, d_len, 2, cp, flen)) == want, flen
