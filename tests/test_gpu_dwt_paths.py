"""Every transform kernel path, pinned by the launch record (vc2hip_dwt_launches) and checked against the oracle.

run_forward / run_inverse choose per level between five kernel families -- two-level (PAIR), streaming (STREAM, with its
TAIL instantiation), fast tile (FAST, with the inverse's element-wise small gather), generic LDS tile (TILE) and whole
planes in HBM (PLANE) -- each with an edge form (raw sample words) and, where it has both, a 16- and a 32-bit store.
The profile names do not tell the tile, fast and stream kernels apart, so coverage here comes from the launch record
only: a cell that no case reached fails the test and is named.  Every case compares the payload, its length and the
decoded picture with the oracle's; the cases that fit the int32 fine-grained calls compare vc2hip_dwt_forward /
_inverse with oracle.dwt_forward / dwt_inverse too.

The segment sweep reaches, through vc2hip_encode_batch_dev / _decode_batch_dev and the batch size alone, one segment per
strip, one per slice row (or the most the two-level plan admits) and a count in between that does not divide the slice
rows, for the streaming kernels (edge and interior, both directions) and the two-level kernels.  Another test pins that
no two-level kernel reads byte band planes; the last one is the benchmark's own call (cfg 2, 128 pictures).
"""
import zlib

import numpy as np
import pytest

from synth import noise_frame, synth, synth_fast, words_frame
from vc2lib import KERNELS, make_params

pytestmark = pytest.mark.gpu

PAIR_WAVELETS = ("DD97", "LeGall", "DD137", "Haar0", "Haar1")   # vc2hip_dwt_pair.hip: not Fidelity, not Daub97
# context switches (vc2hip_create_with_flags) that send the same pictures down the other families
VARIANTS = {"default": (), "levels": ("NO_PAIR",), "store32": ("STORE32",), "tiles": ("NO_STREAM",),
            "tiles32": ("NO_STREAM", "STORE32")}


def _ctx(flags):
    from vc2hip_py import FLAGS, Vc2Hip
    return Vc2Hip(flags=sum(FLAGS[f] for f in flags))


@pytest.fixture(scope="module")
def ctxs():
    return {name: _ctx(flags) for name, flags in VARIANTS.items()}


def _cell(r):
    """what a launch record entry says about the kernel that ran"""
    fam = r["family"]
    if fam == "stream" and r["tail"]:
        fam = "stream-tail"
    if fam == "fast" and r["small_gather"]:
        fam = "fast-small"
    return (fam, "inv" if r["inverse"] else "fwd", "edge" if r["edge"] else "interior", r["store_bits"])


def _name(cell):
    return "%s %s %s %d-bit" % cell


def _path(rec):
    """the cells of a call's launches, level by level (failure messages)"""
    return ", ".join(f"L{r['level']}{'+' + str(r['level'] + 1) if r['levels'] == 2 else ''} {_name(_cell(r))}" for r in rec)


def _forbidden(wavelet, rec, word_bytes, what):
    """the cells the dispatch must never produce"""
    for r in rec:
        c = _cell(r)
        where = f"{what}: {_name(c)} level {r['level']}"
        if r["family"] == "pair":
            assert wavelet in PAIR_WAVELETS, f"{where}: no two-level kernel exists for {wavelet}"
            assert r["store_bits"] == 16, f"{where}: two-level kernels run on the 16-bit store only"
            assert not (r["inverse"] and r["edge"]), f"{where}: the inverse pair that ends at the samples is not used"
            assert r["levels"] == 2 and r["segments"] >= 1, where
        if r["family"] == "stream":
            assert r["segments"] >= 1 and r["levels"] == 1, where
            if r["tail"]:
                assert wavelet != "Fidelity", f"{where}: no TAIL instantiation for Fidelity"
                assert not r["edge"], f"{where}: the TAIL instantiation never runs at an edge"
        if r["family"] in ("stream", "pair") and r["edge"]:
            assert word_bytes == 2, f"{where}: streaming and two-level edge kernels read 2-byte words only"
        if r["band_planes"]:
            assert r["inverse"] and r["family"] in ("stream", "pair"), f"{where}: band planes are read by the streaming kernels"
            assert not (r["family"] == "pair" and r["band_planes"] == 8), f"{where}: two-level kernels never read byte band planes"
        if r["small_gather"]:
            assert r["family"] == "fast" and r["inverse"], where
        if r["family"] not in ("stream", "pair"):
            assert r["segments"] == 0, where


# ------------------------------------------------------------------------------------------------------------------
# 1. the path matrix
# ------------------------------------------------------------------------------------------------------------------
# (label, w, h, cf, depth, u, a, word_bytes, variants): u / a are the reference's slice sizes in units of 2^depth
GEOMS = [
    # luma 1024 / chroma 512 wide, 16 x 32 slices: pair 0+1 forward, pair 1+2 inverse, stream, fast at level 2 (chroma 128
    # wide), its small gather (chroma blocks 2 wide at level 2)
    ("wide", 1024, 256, "422", 3, 2, 4, 2, ("default", "levels", "store32", "tiles", "tiles32")),
    # depth 4 with 16 x 32 slices (cfg 2's slices): two-level kernels over levels 2 + 3 as well
    ("deep", 2048, 512, "422", 4, 1, 2, 2, ("default",)),
    # slice rows of 8: levels 1 and 2 have 196 and 98 rows, pair counts that are not multiples of four (TAIL)
    ("tail", 1024, 392, "422", 3, 1, 4, 2, ("default", "levels", "store32")),
    # 4 samples wide slices: the fast inverse's small gather at the edge and below it
    ("narrow", 512, 128, "444", 2, 2, 1, 2, ("default", "store32")),
    # 24 x 24 slices (not a power of two): the generic LDS tile kernels at every level
    ("odd", 384, 192, "444", 3, 3, 3, 2, ("default",)),
    # one slice for the whole picture: beyond any LDS tile, whole planes in HBM
    ("plane", 256, 256, "444", 2, 64, 64, 2, ("default",)),
    # words of 1, 3 and 4 bytes through every family whose edge form reads them (fast, tile, plane)
    ("wide-w1", 1024, 256, "422", 3, 2, 4, 1, ("default", "store32")),
    ("wide-w3", 1024, 256, "422", 3, 2, 4, 3, ("default", "store32")),
    ("wide-w4", 1024, 256, "422", 3, 2, 4, 4, ("default", "store32")),
    ("odd-w1", 384, 192, "444", 3, 3, 3, 1, ("default",)),
    ("odd-w3", 384, 192, "444", 3, 3, 3, 3, ("default",)),
    ("odd-w4", 384, 192, "444", 3, 3, 3, 4, ("default",)),
    ("plane-w1", 256, 256, "444", 2, 64, 64, 1, ("default",)),
    ("plane-w3", 256, 256, "444", 2, 64, 64, 3, ("default",)),
    ("plane-w4", 256, 256, "444", 2, 64, 64, 4, ("default",)),
]


def _worst_bits(wavelet, word_bytes):
    """the highest bit depth of the worst-case pictures: 16 (8 in 1-byte words; the stream signals 8, 10, 12 and 16 bits
    only), 12 for Daub97, whose 16-bit pictures leave the int32 domain from depth 2 on (tests/test_oracle_dwt_model.py,
    DOMAIN_LIMITS)"""
    return 8 if word_bytes == 1 else 12 if wavelet == "Daub97" else 16


def _pictures(wavelet, label, w, h, cf, wb, seed):
    """(kind, bits, raw): a smooth picture and two worst cases for lifting growth"""
    if wb <= 2:
        bits = 8 if wb == 1 else 10
        yield "smooth", bits, synth(w, h, cf, bits, seed, word_bytes=wb)
    else:   # (3- and 4-byte words: 12-bit noise, shifted by 12 and 20 bits into the word)
        yield "noise", 12, words_frame(w, h, cf, 12, seed, wb, "noise")
    bits = _worst_bits(wavelet, wb)
    if wb <= 2:
        yield "full-scale noise", bits, noise_frame(w, h, cf, bits, seed + 1, word_bytes=wb, full_scale=True)
    else:
        yield "full-scale noise", bits, words_frame(w, h, cf, bits, seed + 1, wb, "extremes")
    yield "checkerboard", bits, words_frame(w, h, cf, bits, seed + 2, wb, "checker")


QS = (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64)


def _encode_lowest_q(hip, fmt_cp, wavelet):
    """the lowest index of QS whose quantised coefficients stay inside the reference's code words (no VC2HIP_ECODE32)
    and whose slices fit their length bytes (no VC2HIP_ESCALAR)"""
    from vc2hip_py import Vc2HipError
    for q in QS:
        fmt, cp = fmt_cp(q)
        try:
            hip.encode_picture_hq(fmt_cp.raw, fmt, cp)
            return q
        except Vc2HipError as e:
            if e.code not in (-11, -3):
                raise
    raise AssertionError(f"{wavelet} {fmt_cp.what}: every index of {QS} overflows the code words or the slices")


def _unit_bytes(stream):
    """bytes of the stream's last picture data unit: the previous-parse-offset field of the end-of-sequence parse info"""
    return int.from_bytes(stream[-4:], "big")


_HEADERS = {}


def _header_bytes(oracle, p):
    """bytes of a picture data unit in front of its slices for these parameters (parse info, picture number, transform
    parameters), from the oracle alone: the same picture coded at two quantiser indices (not part of those parameters)
    gives data units that, behind their parse info (13 bytes, with the unit's size), first differ at the first slice's
    index byte, which opens the payload (no prefix bytes here)"""
    assert p.prefix == 0
    key = bytes(p)
    if key not in _HEADERS:
        ch = p.height // 2 if p.cf == 2 else p.height
        cw = p.width if p.cf == 0 else p.width // 2
        grey = (1 << (p.bit_depth - 1)) << (8 * p.word_bytes - p.bit_depth)   # every coefficient 0: the smallest slices
        flat = grey.to_bytes(p.word_bytes, "big") * (p.width * p.height + 2 * ch * cw)
        p2 = type(p).from_buffer_copy(p)
        p2.q_index = p.q_index + 1 if p.q_index < 100 else p.q_index - 1
        a, b = oracle.encode_stream(p, flat, 1), oracle.encode_stream(p2, flat, 1)
        start = len(a) - 13 - _unit_bytes(a)           # where the picture data unit begins
        assert a[:start] == b[:start] and a[start:start + 4] == b"BBCD"
        k = next(i for i in range(start + 13, min(len(a), len(b))) if a[i] != b[i])
        assert a[k] == p.q_index and b[k] == p2.q_index
        _HEADERS[key] = k - start
    return _HEADERS[key]


def _run_geom(ctxs, oracle, wavelet, geom, seen):
    import vc2hip_py
    label, w, h, cf, depth, u, a, wb, variants = geom
    scalar = 256 if label.startswith("plane") else 8   # (room in the length bytes for the one 256 x 256 slice)
    for kind, bits, raw in _pictures(wavelet, label, w, h, cf, wb, seed=zlib.crc32(f"{label} {wavelet}".encode()) % 1000):
        def fmt_cp(q):
            fmt = vc2hip_py.picture_format(w, h, cf, bits, wb)
            return fmt, vc2hip_py.coding_params(ctxs["default"].lib, fmt, wavelet, depth, u, a, q=q, scalar=scalar)
        fmt_cp.raw, fmt_cp.what = raw, f"{label} {kind} {bits}-bit {wb}-byte"
        q = _encode_lowest_q(ctxs["default"], fmt_cp, wavelet)
        fmt, cp = fmt_cp(q)
        p = make_params(w, h, cf, bits, wavelet, depth, u, a, q=q, scalar=scalar, word_bytes=wb)
        stream = oracle.encode_stream(p, raw, 1)
        want, n = oracle.decode_stream(p, stream, 1)
        assert n == 1
        oracle_payload = stream[-13 - (_unit_bytes(stream) - _header_bytes(oracle, p)):-13]
        for var in variants:
            hip = ctxs[var]
            what = f"{wavelet} {label} {kind} {bits}-bit {wb}-byte q{q} [{var}]"
            payload, _ = hip.encode_picture_hq(raw, fmt, cp)
            fwd = hip.dwt_launches()
            assert len(payload) == len(oracle_payload), f"{what}: payload length after {_path(fwd)}"
            assert payload == oracle_payload, f"{what}: payload after {_path(fwd)}"
            dec = hip.decode_picture(oracle_payload, fmt, cp)
            inv = hip.dwt_launches()
            assert dec == want, f"{what}: decoded picture after {_path(inv)}"
            assert fwd and all(not r["inverse"] for r in fwd), what
            assert inv and all(r["inverse"] for r in inv), what
            for r in fwd + inv:
                assert r["pictures"] == 1, what
                _forbidden(wavelet, [r], wb, what)
                seen.setdefault((_cell(r), wb), what)


def _run_int32_calls(hip, oracle, wavelet, seen):
    """vc2hip_dwt_forward / _inverse (one int32 plane, no raw words): interior kernels on the int32 store"""
    k = KERNELS[wavelet]
    rng = np.random.default_rng(k)
    for h, w, depth in ((256, 1024, 3), (196, 512, 2), (150, 333, 3), (72, 100, 2)):
        bits = _worst_bits(wavelet, 2)
        x = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(h, w)).astype(np.int32)
        what = f"{wavelet} int32 {h}x{w} depth {depth}"
        want = oracle.dwt_forward(x, k, depth)
        got = hip.dwt_forward(x, k, depth)
        assert np.array_equal(got, want), f"{what}: forward after {_path(hip.dwt_launches())}"
        for r in hip.dwt_launches():
            _forbidden(wavelet, [r], 2, what)
            seen.setdefault((_cell(r), 0), what)
        coef = want + rng.integers(-40, 41, size=want.shape).astype(np.int32)
        back = hip.dwt_inverse(coef, k, depth, (h, w))
        assert np.array_equal(back, oracle.dwt_inverse(coef, k, depth, (h, w))), f"{what}: inverse after {_path(hip.dwt_launches())}"
        for r in hip.dwt_launches():
            _forbidden(wavelet, [r], 2, what)
            seen.setdefault((_cell(r), 0), what)


def _required(wavelet):
    """every (family, direction, edge, store) cell the dispatch admits for this wavelet"""
    cells = set()
    for d in ("fwd", "inv"):
        for e in ("edge", "interior"):
            for b in (16, 32):
                cells |= {("stream", d, e, b), ("fast", d, e, b)}
            cells.add(("tile", d, e, 32))
        cells.add(("plane", d, "interior", 32))
    for b in (16, 32):
        cells |= {("fast-small", "inv", "edge", b), ("fast-small", "inv", "interior", b)}
        if wavelet != "Fidelity":
            cells |= {("stream-tail", "fwd", "interior", b), ("stream-tail", "inv", "interior", b)}
    if wavelet in PAIR_WAVELETS:
        cells |= {("pair", "fwd", "edge", 16), ("pair", "fwd", "interior", 16), ("pair", "inv", "interior", 16)}
    return cells


EDGE_WORDS = {1: ("fast", "tile", "plane"), 3: ("fast", "tile", "plane"), 4: ("fast", "tile", "plane")}


@pytest.mark.parametrize("wavelet", list(KERNELS))
def test_path_matrix(ctxs, oracle, wavelet):
    seen = {}
    for geom in GEOMS:
        _run_geom(ctxs, oracle, wavelet, geom, seen)
    _run_int32_calls(ctxs["default"], oracle, wavelet, seen)
    got = {c for c, _ in seen}
    missing = sorted(_required(wavelet) - got)
    assert not missing, f"{wavelet}: cells no case reached: {[_name(c) for c in missing]}; reached: {[_name(c) for c in sorted(got)]}"
    # raw words of 1, 3 and 4 bytes: through every edge form that reads them (a plane's ingest / emit are its edges)
    for wb, fams in EDGE_WORDS.items():
        for fam in fams:
            for d in ("fwd", "inv"):
                e = "interior" if fam == "plane" else "edge"
                assert any(c[0].split("-")[0] == fam and c[1] == d and c[2] == e for c, b in seen if b == wb), \
                    f"{wavelet}: no {fam} {d} {e} launch with {wb}-byte words"
        assert not any(c[0].startswith(("stream", "pair")) and c[2] == "edge" for c, b in seen if b == wb), wb


@pytest.mark.parametrize("wavelet", PAIR_WAVELETS)
def test_pair_kernels_never_read_byte_band_planes(oracle, wavelet):
    """the "wide" geometry's decoder keeps levels 0 and 1 as band planes, and its inverse pair covers levels 1 + 2: with
    16-bit planes the pair runs and reads them; with byte planes (VC2HIP_FLAG_PLANES8_ALWAYS) the pair must give way to
    one launch per level, the streaming kernel reading the bytes at level 1.  Both decode the oracle's payload to the
    oracle's picture."""
    import vc2hip_py
    w, h, cf, depth, u, a = 1024, 256, "422", 3, 2, 4
    raw = synth(w, h, cf, 10, 77)
    p = make_params(w, h, cf, 10, wavelet, depth, u, a, q=8, scalar=8)
    stream = oracle.encode_stream(p, raw, 1)
    want, _ = oracle.decode_stream(p, stream, 1)
    payload = stream[-13 - (_unit_bytes(stream) - _header_bytes(oracle, p)):-13]
    seen = {}
    for var in ("PLANES8_NEVER", "PLANES8_ALWAYS"):
        hip = _ctx((var,))
        fmt = vc2hip_py.picture_format(w, h, cf, 10)
        cp = vc2hip_py.coding_params(hip.lib, fmt, wavelet, depth, u, a, q=8, scalar=8)
        assert hip.decode_picture(payload, fmt, cp) == want, f"{wavelet} [{var}]: decoded picture"
        rec = hip.dwt_launches()
        _forbidden(wavelet, rec, 2, f"{wavelet} [{var}]")
        seen[var] = ([(r["family"], r["level"], r["levels"], r["band_planes"]) for r in rec], hip.band_plane_bits())
        hip.close()
    words, bytes8 = seen["PLANES8_NEVER"], seen["PLANES8_ALWAYS"]
    assert words[1] == 16 and ("pair", 1, 2, 16) in words[0], f"{wavelet}: the pair over levels 1 + 2 on 16-bit planes: {words}"
    assert bytes8[1] == 8 and ("stream", 1, 1, 8) in bytes8[0], f"{wavelet}: level 1 streams from byte planes: {bytes8}"
    assert not any(f == "pair" and bp == 8 for f, _, _, bp in bytes8[0]), f"{wavelet}: a pair read byte planes: {bytes8}"


# ------------------------------------------------------------------------------------------------------------------
# 2. the segment sweep
# ------------------------------------------------------------------------------------------------------------------
# 4 MiB pictures (4096 x 256 4:2:2, depth 4, 8 rows of 32 x 32 slices): planes wide enough that the chip's wavefront
# slots fill within the batch list (one segment per strip then costs least); two-level kernels over levels 0 + 1 and
# 2 + 3 (and, without them, the streaming kernels at levels 0 and 1).
SWEEPS = {"A": dict(w=4096, h=256, cf="422", bits=10, depth=4, u=2, a=2)}
BATCHES = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024)
DISTINCT = 5
# The two-level plan admits a segment boundary only where the segment below it spans at least 3 * OFFL row pairs
# (vc2_pair_applicable), so one segment per slice row needs slice rows of that many row pairs at the pair's first level.
# In this geometry (and in cfg 2) the interior pairs start at level 2, where a slice row is 4 row pairs: too few for DD97
# and DD137.  These are the most segments the plan admits there, reached at one picture per call.
ROW_LIMITED = {("A", "DD97 pair fwd interior"): 7, ("A", "DD97 pair inv interior"): 7, ("A", "DD137 pair fwd interior"): 3,
               ("A", "DD137 pair inv interior"): 3}


def _batch_roundtrip(hip, fmt, cp, d_pics, rb, n, stride, torch):
    """n pictures (the distinct ones of d_pics cycled) through encode_batch_dev and decode_batch_dev twice; the launch
    records of the three calls, the payloads, their lengths and the two decoded batches"""
    k = d_pics.numel() // rb
    idx = torch.arange(n, device=d_pics.device) % k
    d_raw = d_pics.view(k, rb)[idx].reshape(-1).contiguous()
    d_pay = torch.zeros(n * stride, dtype=torch.uint8, device=d_pics.device)
    d_len = torch.zeros(n, dtype=torch.int64, device=d_pics.device)
    torch.cuda.synchronize()
    hip.encode_batch_dev(d_raw.data_ptr(), n, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    hip.sync()
    del d_raw
    recs = [hip.dwt_launches()]
    outs = []
    for _ in range(2):   # the adaptive band planes: the second call decides from the first (16-bit, then bytes)
        d_out = torch.zeros(n * rb, dtype=torch.uint8, device=d_pics.device)
        hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, fmt, cp, d_out.data_ptr())
        hip.sync()
        recs.append(hip.dwt_launches())
        outs.append(d_out)
    return recs, d_pay, d_len, outs


def _check_slots(n, stride, rb, d_pay, d_len, outs, payloads, decoded, what):
    """every slot against the oracle: payload length and bytes, and both decoded batches"""
    k = len(payloads)
    lens = d_len.cpu().numpy()
    pay = d_pay.cpu().numpy().reshape(n, stride)
    for i in range(n):
        assert lens[i] == len(payloads[i % k]), f"{what}: slot {i} payload length"
        assert pay[i, :lens[i]].tobytes() == payloads[i % k], f"{what}: slot {i} payload"
    for j, d_out in enumerate(outs):
        out = d_out.cpu().numpy().reshape(n, rb)
        for i in range(n):
            assert out[i].tobytes() == decoded[i % k], f"{what}: decode {j + 1}, slot {i}"


def _oracle_pictures(oracle, p, raws):
    """the oracle's payload and decoded picture of each raw picture"""
    payloads, decoded = [], []
    for raw in raws:
        stream = oracle.encode_stream(p, raw, 1)
        payloads.append(stream[-13 - (_unit_bytes(stream) - _header_bytes(oracle, p)):-13])
        decoded.append(oracle.decode_stream(p, stream, 1)[0])
    return payloads, decoded


def _segment_targets_met(t, top, ys):
    return 1 in t and top in t and any(1 < g < ys and ys % g for g in t)


def _sweep_phase(oracle_pics, hip, fmt, cp, d_pics, rb, stride, ys, wavelet, fam, forms, limits, torch):
    """batch sizes of BATCHES, ascending, until every form has shown its target counts: {form: {segments: first batch}}.
    Every batch has its payload lengths checked against the oracle; a batch that first gave a target count (and batch 1)
    has every slot's payload and both decoded batches checked too.  One output buffer at a time: at 1024 pictures the
    batch holds 4 GiB of pictures, their payloads and 4 GiB of output."""
    payloads, decoded = oracle_pics
    k = len(payloads)
    want_lens = np.array([len(payloads[i % k]) for i in range(BATCHES[-1])])
    table = {f: {} for f in forms}

    def note(rec, n):
        hit = False
        for r in rec:
            assert r["pictures"] == n
            _forbidden(wavelet, [r], 2, f"{wavelet} batch {n}")
            key = ("inv" if r["inverse"] else "fwd", "edge" if r["edge"] else "interior")
            g = r["segments"]
            if r["family"] == fam and key in table and g not in table[key]:
                t = table[key]
                hit |= g in (1, ys, limits.get(key)) or bool(ys % g and not any(1 < x < ys and ys % x for x in t))
                t[g] = n
        return hit

    for n in BATCHES:
        what = f"{wavelet} {fam} batch {n}"
        idx = torch.arange(n, device=d_pics.device) % k
        d_raw = d_pics.view(k, rb)[idx].reshape(-1).contiguous()
        d_pay = torch.zeros(n * stride, dtype=torch.uint8, device=d_pics.device)
        d_len = torch.zeros(n, dtype=torch.int64, device=d_pics.device)
        torch.cuda.synchronize()
        hip.encode_batch_dev(d_raw.data_ptr(), n, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
        hip.sync()
        del d_raw
        check = note(hip.dwt_launches(), n) or n == 1
        lens = d_len.cpu().numpy()
        bad = np.nonzero(lens != want_lens[:n])[0]
        assert not bad.size, f"{what}: payload lengths of slots {bad[:8].tolist()}"
        if check:
            pay = d_pay.cpu().numpy().reshape(n, stride)
            for i in range(n):
                assert pay[i, :lens[i]].tobytes() == payloads[i % k], f"{what}: slot {i} payload"
            del pay
        d_out = torch.empty(n * rb, dtype=torch.uint8, device=d_pics.device)
        for j in range(2):   # the adaptive band planes: the second call decides from the first (16-bit, then bytes)
            d_out.fill_(0)
            hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, fmt, cp, d_out.data_ptr())
            hip.sync()
            if note(hip.dwt_launches(), n) or check:
                out = d_out.cpu().numpy().reshape(n, rb)
                for i in range(n):
                    assert out[i].tobytes() == decoded[i % k], f"{what}: decode {j + 1}, slot {i}"
                del out
        del d_pay, d_len, d_out
        if all(_segment_targets_met(t, limits.get(f, ys), ys) for f, t in table.items()):
            break
    return table


@pytest.mark.parametrize("wavelet", list(KERNELS))
def test_segment_sweep(ctxs, oracle, wavelet):
    """one segment per strip, one per slice row (or the most the two-level plan admits: ROW_LIMITED) and a count in
    between that does not divide the slice rows, for each streaming form (a context without two-level kernels) and each
    two-level form, reached by the batch size alone.  The table is printed (pytest -s)."""
    torch = pytest.importorskip("torch")
    import vc2hip_py
    report = []
    for geo, s in SWEEPS.items():
        fmt = vc2hip_py.picture_format(s["w"], s["h"], s["cf"], s["bits"])
        cp = vc2hip_py.coding_params(ctxs["default"].lib, fmt, wavelet, s["depth"], s["u"], s["a"], q=16, scalar=4)
        ys = cp.y_slices
        p = make_params(s["w"], s["h"], s["cf"], s["bits"], wavelet, s["depth"], s["u"], s["a"], q=16, scalar=4)
        raws = [synth_fast(s["w"], s["h"], s["cf"], s["bits"], 500 + i) for i in range(DISTINCT)]
        pics = _oracle_pictures(oracle, p, raws)
        rb = ctxs["default"].raw_picture_bytes(fmt)
        stride = (ctxs["default"].max_payload_bytes(fmt, cp) + 255) // 256 * 256
        d_pics = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to("cuda:0")
        phases = [("levels", "stream", [(d, e) for d in ("fwd", "inv") for e in ("edge", "interior")])]
        if wavelet in PAIR_WAVELETS:
            phases.append(("default", "pair", [("fwd", "edge"), ("fwd", "interior"), ("inv", "interior")]))
        for var, fam, forms in phases:
            limits = {f: ROW_LIMITED[(geo, f"{wavelet} {fam} {' '.join(f)}")] for f in forms
                      if (geo, f"{wavelet} {fam} {' '.join(f)}") in ROW_LIMITED}
            table = _sweep_phase(pics, ctxs[var], fmt, cp, d_pics, rb, stride, ys, wavelet, fam, forms, limits, torch)
            report += [(geo, f"{wavelet} {fam} {' '.join(f)}", ys, limits.get(f, ys), t) for f, t in table.items()]
        del d_pics
    print(f"\nsegment sweep {wavelet} (segments @ first batch): " + "; ".join(
        f"[{geo}] {name}: " + ", ".join(f"{g} @ {b}" for g, b in sorted(t.items())) for geo, name, _, _, t in report))
    bad = []
    for geo, name, ys, top, t in report:
        name = f"[{geo}] {name}"
        if 1 not in t:
            bad.append(f"{name}: no batch of {BATCHES} gave one segment per strip: {t}")
        if t.get(top) != 1 or max(t) != top:
            bad.append(f"{name}: one picture per call did not give {top} segments, the most the plan admits: {t}")
        if not any(1 < g < ys and ys % g for g in t):
            bad.append(f"{name}: no count between 1 and {ys} that does not divide it: {t}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# 3. the benchmark's own call
# ------------------------------------------------------------------------------------------------------------------
def test_cfg2_128_pictures_per_call(oracle):
    """cfg 2 (UHD-1 4:2:2 10-bit DD97, depth 4, q 16, scalar 2) at the 128 pictures per call bench.py times, 3 distinct
    pictures cycled: the launch record of the benchmark's kernels, every slot against the oracle"""
    torch = pytest.importorskip("torch")
    import vc2hip_py
    hip = _ctx(())
    w, h, n = 3840, 2160, 128
    fmt = vc2hip_py.picture_format(w, h, "422", 10)
    cp = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, q=16, scalar=2)
    p = make_params(w, h, "422", 10, "DD97", 4, 1, 2, q=16, scalar=2)
    raws = [synth_fast(w, h, "422", 10, 900 + i) for i in range(3)]
    payloads, decoded = _oracle_pictures(oracle, p, raws)
    rb = hip.raw_picture_bytes(fmt)
    stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
    d_pics = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to("cuda:0")
    recs, d_pay, d_len, outs = _batch_roundtrip(hip, fmt, cp, d_pics, rb, n, stride, torch)
    _check_slots(n, stride, rb, d_pay, d_len, outs, payloads, decoded, "cfg2 x 128")
    show = [[(_name(_cell(r)), r["level"], r["segments"]) for r in rec] for rec in recs]
    print("\ncfg2 x 128 launches: forward", show[0], "inverse", show[1], "inverse again", show[2])
    for rec in recs:
        for r in rec:
            assert r["pictures"] == n
            _forbidden("DD97", [r], 2, "cfg2 x 128")
    # forward: two-level kernels over levels 0 + 1 (raw words in) and 2 + 3
    cells = [(_cell(r)[0], _cell(r)[2], r["level"]) for r in recs[0]]
    assert cells == [("pair", "edge", 0), ("pair", "interior", 2)], cells
    for rec in recs[1:]:
        # inverse: levels 3 + 2 in one launch, then 1 and 0 (the pair that ends at the samples keeps two launches)
        cells = [(_cell(r)[0], _cell(r)[2], r["level"]) for r in rec]
        assert cells == [("pair", "interior", 2), ("stream", "interior", 1), ("stream", "edge", 0)], cells
