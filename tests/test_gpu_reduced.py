"""GPU tests of vc2hip_decode_reduced_batch_dev (pictures at 1/2, 1/4, 1/8 size): every comparison byte for byte against
the CPU definition tests/proxy_ref.py, on payloads made by the oracle's encoder."""
import numpy as np
import pytest

import proxy_ref as pr
from synth import noise_frame, synth, synth_fast, words_frame

pytestmark = pytest.mark.gpu

VARIANTS = {"default": (), "store32": ("STORE32",), "tiles": ("NO_STREAM",), "levels": ("NO_PAIR",), "records": ("NO_BANDPLANES",),
            "noheads": ("NO_HEADS",), "generic": ("GENERIC_DWT",), "bytes": ("PLANES8_ALWAYS",), "words": ("PLANES8_NEVER",)}


def _ctx(*flags):
    from vc2hip_py import FLAGS, Vc2Hip
    return Vc2Hip(flags=sum(FLAGS[f] for f in flags))


@pytest.fixture(scope="module")
def variants():
    return {name: _ctx(*flags) for name, flags in VARIANTS.items()}


class Batch:
    """payloads in device slots"""

    def __init__(self, pays, n=None):
        import torch
        self.torch = torch
        n = n or len(pays)
        self.n = n
        self.stride = (max(len(p) for p in pays) + 64 + 255) // 256 * 256
        slots = np.zeros((len(pays), self.stride), np.uint8)
        for i, p in enumerate(pays):
            slots[i, :len(p)] = np.frombuffer(p, np.uint8)
        idx = torch.arange(n, device="cuda:0") % len(pays)
        self.d_pay = torch.from_numpy(slots).to("cuda:0")[idx].reshape(-1).contiguous()
        self.d_len = torch.tensor([len(p) for p in pays], dtype=torch.int64, device="cuda:0")[idx].contiguous()

    def out(self, nbytes, fill=0):
        o = self.torch.full((self.n * nbytes + 16,), fill, dtype=self.torch.uint8, device="cuda:0")
        self.torch.cuda.synchronize()   # (torch fills on its stream, the library works on its own)
        return o

    def reduced(self, hip, fmt, cp, k, nbytes):
        o = self.out(nbytes)
        hip.decode_reduced_batch_dev(self.d_pay.data_ptr(), self.stride, self.d_len.data_ptr(), self.n, fmt, cp, k, o.data_ptr())
        hip.sync()
        return o[:self.n * nbytes].view(self.n, nbytes)

    def full(self, hip, fmt, cp, nbytes):
        o = self.out(nbytes)
        hip.decode_batch_dev(self.d_pay.data_ptr(), self.stride, self.d_len.data_ptr(), self.n, fmt, cp, o.data_ptr())
        hip.sync()
        return o[:self.n * nbytes].view(self.n, nbytes)


def _launch_facts(hip, k, name):
    """what vc2hip_dwt_launches must say of a reduced call; returns the family that wrote the raw words"""
    rec = hip.dwt_launches()
    assert rec and all(r["inverse"] for r in rec), (name, rec)
    assert min(r["level"] for r in rec) == k, (name, k, rec)
    if rec[0]["family"] == "plane":     # whole planes in HBM: one entry per component, the emit is a kernel of its own
        return "plane"
    edges = [r for r in rec if r["edge"]]
    assert len(edges) == 1 and edges[0]["level"] == k, (name, k, rec)
    fam = edges[0]["family"]
    if name == "tiles":
        assert fam in ("fast", "tile"), rec
    if name == "generic":
        assert fam == "tile", rec
    if name == "store32":
        assert all(r["store_bits"] == 32 for r in rec), rec
    return fam


def _check_case(variants, oracle, case, raw, seen=None, names=None):
    pays = pr.oracle_payloads(oracle, case, raw, len(raw) // case.raw_bytes())
    batch = Batch(pays)
    drops = case.drops()
    assert drops
    for k in drops:
        want = [pr.reduced_picture(oracle, case, p, k) for p in pays]
        for name, hip in variants.items():
            if names and name not in names:
                continue
            fmt, cp = case.fmt_cp(hip.lib)
            got = batch.reduced(hip, fmt, cp, k, case.raw_bytes(k)).cpu().numpy()
            fam = _launch_facts(hip, k, name)
            if seen is not None:
                seen.setdefault(name, set()).add(fam)
            for i, wnt in enumerate(want):
                assert got[i].tobytes() == wnt, (name, k, i, fam)


def _raw(c, seed, kind="synth", frames=1):
    w, h, cf, bits, wb = c.w, c.h, c.cf, c.bits, c.word_bytes
    if wb > 2 or kind == "words":
        return b"".join(words_frame(w, h, cf, bits, seed + f, wb) for f in range(frames))
    if kind == "noise":
        return b"".join(noise_frame(w, h, cf, bits, seed + f, word_bytes=wb) for f in range(frames))
    return synth(w, h, cf, bits, seed, frames=frames, word_bytes=wb)


# (w, h, cf, bits, word_bytes, wavelet, depth, u, a, coding, picture): every wavelet, chroma format, bit depth, word size and
# drop count at least twice; all three modes; prefix and scalar other than 0 / 1; pictures padded in height (270 -> 272),
# in width (1004 -> 1008) and in both (1004 x 60 -> 1008 x 64); q = 0 and indices that leave few coefficients
MATRIX = [
    (1024, 96, "422", 10, 2, "DD97", 3, 1, 2, dict(q=7, scalar=2), "noise"),
    (1280, 270, "422", 10, 2, "DD97", 4, 1, 2, dict(q=6, scalar=3, prefix=2), "synth"),
    (2048, 128, "422", 10, 2, "LeGall", 4, 1, 2, dict(q=0, scalar=8), "synth"),
    (1004, 64, "422", 12, 2, "LeGall", 3, 1, 2, dict(q=40, scalar=1, prefix=5), "noise"),
    (1004, 60, "444", 12, 3, "DD137", 3, 1, 1, dict(q=11, scalar=4), "words"),
    (512, 64, "420", 8, 1, "DD137", 2, 2, 4, dict(q=0, scalar=8), "synth"),
    (1280, 128, "420", 8, 1, "Haar0", 3, 2, 4, dict(q=30, scalar=1), "synth"),
    (256, 64, "444", 10, 3, "Haar0", 4, 1, 1, dict(q=3, scalar=6, prefix=1), "words"),
    (1024, 64, "444", 8, 1, "Haar1", 3, 1, 2, dict(q=9, scalar=2), "noise"),
    (2048, 256, "422", 12, 2, "Haar1", 4, 1, 2, dict(mode="HQ_CBR", s=120000, scalar=2), "synth"),
    (1024, 64, "422", 10, 2, "Fidelity", 3, 1, 2, dict(q=5, scalar=3), "synth"),
    (512, 128, "420", 12, 2, "Fidelity", 2, 2, 4, dict(mode="HQ_CBR", s=30000, scalar=1, prefix=3), "noise"),
    (1024, 64, "422", 10, 2, "DD97", 3, 1, 2, dict(mode="LD", s=40000), "synth"),
    (256, 128, "420", 8, 1, "LeGall", 3, 2, 2, dict(mode="LD", s=9000), "synth"),
    (512, 64, "444", 10, 2, "Haar1", 2, 2, 2, dict(mode="LD", s=30000), "noise"),
]

@pytest.mark.parametrize("row", MATRIX, ids=lambda r: "-".join(str(x) for x in r[:9]) + "-" + r[9].get("mode", "HQ_ConstQ"))
def test_matrix(variants, oracle, row):
    w, h, cf, bits, wb, kernel, depth, u, a, kw, kind = row
    case = pr.Case(oracle, w, h, cf, bits, kernel, depth, u, a, word_bytes=wb, **kw)
    _check_case(variants, oracle, case, _raw(case, 40 + w + depth, kind, frames=2))


def test_every_inverse_family_writes_raw_words(variants, oracle):
    """a picture whose reduced planes are still wide enough for the streaming kernels: their edge by default, the fast tile
    kernels' without them, the generic tile kernels' when asked for -- all the same bytes"""
    # (the streaming kernels want slice footprints of 8 samples or more across at the level they run, chroma included:
    # slices of 64 luma samples are 32 / 16 across at level 1)
    case = pr.Case(oracle, 2048, 128, "422", 10, "DD97", 3, 1, 8, q=10, scalar=2)
    seen = {}
    _check_case(variants, oracle, case, _raw(case, 77), seen, names=("default", "tiles", "generic", "store32"))
    assert "stream" in seen["default"] and "fast" in seen["tiles"] and seen["generic"] == {"tile"}, seen


def test_whole_plane_path(variants, oracle):
    """one slice per picture, at k = 1 still 256 x 512 samples: no LDS tile holds it, the transform runs on whole planes and
    its emit normalises (at k = 2 the slice fits the level kernels again)"""
    case = pr.Case(oracle, 1024, 512, "444", 10, "DD97", 3, 512 >> 3, 1024 >> 3, q=24, scalar=4000)
    assert (case.ys, case.xs) == (1, 1)
    seen = {}
    _check_case(variants, oracle, case, _raw(case, 5), seen, names=("default", "generic"))
    assert "plane" in seen["default"], seen


def test_store16_escapes(variants, oracle):
    """16-bit samples whose quantised coefficients pass 32767 (as test_gpu_wide.py::test_store16_escapes_both_directions
    builds them): the escapes of the kept levels reach the reduced picture"""
    w, h, depth, u, a = 1024, 64, 2, 2, 4
    raw = noise_frame(w, h, "422", 16, seed=74)
    hit = None
    for q in (16, 12, 10, 8, 7, 6, 5, 4, 3, 2):
        case = pr.Case(oracle, w, h, "422", 16, "LeGall", depth, u, a, q=q, scalar=8)
        try:
            (pay,) = pr.oracle_payloads(oracle, case, raw)
        except Exception:   # |quantised| > 65534: outside the reference's domain
            break
        planes = pr.quantised_planes(oracle, case, pay)[:3]
        kept = max(int(np.abs(x[::2, ::2]).max()) for x in planes)
        if 32767 < kept <= 65534:
            hit = case
            break
    assert hit is not None, "no quantiser index puts kept quantised values between 32768 and 65534"
    _check_case(variants, oracle, hit, raw)


@pytest.mark.parametrize("mode", ["HQ_ConstQ", "LD"])
def test_the_dropped_tail_is_not_read(variants, oracle, mode):
    """every coefficient of the dropped levels replaced by other small values and the slices packed again with the same
    indices: every slice offset moves, the reduced picture does not"""
    kw = dict(q=8, scalar=4, prefix=1) if mode == "HQ_ConstQ" else dict(mode="LD", s=60000)
    case = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, **kw)
    (pay,) = pr.oracle_payloads(oracle, case, _raw(case, 9))
    y, u, v, q = pr.quantised_planes(oracle, case, pay)
    rng = np.random.default_rng(3)
    for k in (1, 2):
        planes = []
        for p in (y, u, v):
            p2 = p.copy()
            yy, xx = np.mgrid[0:p.shape[0], 0:p.shape[1]]
            tail = ((yy | xx) & ((1 << k) - 1)) != 0
            # (an LD slice has a fixed size and the encoder fills it: a longer luma would push chroma out of it, so the tail is cleared)
            p2[tail] = rng.integers(-2, 3, size=int(tail.sum())) if mode == "HQ_ConstQ" else 0
            planes.append(np.ascontiguousarray(p2))
        pay2 = pr.pack_planes(oracle, case, *planes, q)
        assert pay2 != pay and (mode == "LD" or len(pay2) != len(pay))
        want = pr.reduced_picture(oracle, case, pay, k)
        assert pr.reduced_picture(oracle, case, pay2, k) == want
        for name, hip in variants.items():
            fmt, cp = case.fmt_cp(hip.lib)
            got = Batch([pay, pay2]).reduced(hip, fmt, cp, k, case.raw_bytes(k)).cpu().numpy()
            assert got[0].tobytes() == want and got[1].tobytes() == want, (name, k)


@pytest.mark.parametrize("streams", [2, 3])
def test_set_streams_gives_identical_bytes(oracle, streams):
    case = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=7, scalar=2)
    pays = pr.oracle_payloads(oracle, case, _raw(case, 21, frames=3), 3)
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    batch = Batch(pays, n=7)
    for k in (1, 2):
        assert case.raw_bytes(k) % 16 == 0
        want = [pr.reduced_picture(oracle, case, p, k) for p in pays]
        hip.set_streams(1)
        one = batch.reduced(hip, fmt, cp, k, case.raw_bytes(k)).clone()
        hip.set_streams(streams)
        many = batch.reduced(hip, fmt, cp, k, case.raw_bytes(k))
        assert batch.torch.equal(one, many)
        for i in range(7):
            assert many[i].cpu().numpy().tobytes() == want[i % 3], (k, i)
    hip.close()


def test_refusals_launch_nothing(oracle):
    """k = 0, k = d, k < 0, Daub97, a component size that 2^k does not divide, misaligned buffers: VC2HIP_EINVAL, the launch
    record and the output buffer untouched"""
    from vc2hip_py import Vc2HipError
    case = pr.Case(oracle, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=7, scalar=2)
    (pay,) = pr.oracle_payloads(oracle, case, _raw(case, 22))
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    batch = Batch([pay], n=2)
    good = batch.reduced(hip, fmt, cp, 1, case.raw_bytes(1)).clone()
    before = hip.dwt_launches()
    daub = pr.Case(oracle, 1024, 64, "422", 10, "Daub97", 3, 1, 2, q=7, scalar=2)
    odd = pr.Case(oracle, 1020, 60, "422", 10, "DD97", 3, 1, 2, q=7, scalar=2)   # chroma 510 wide: not a multiple of 4
    tries = [(case, 0, 0, 0), (case, 3, 0, 0), (case, -1, 0, 0), (case, 4, 0, 0), (daub, 1, 0, 0), (odd, 2, 0, 0), (case, 1, 8, 0), (case, 1, 0, 8)]
    for cs, k, out_off, pay_off in tries:
        f2, c2 = cs.fmt_cp(hip.lib)
        o = batch.out(case.raw_bytes(), fill=0xA5)
        with pytest.raises(Vc2HipError) as e:
            hip.decode_reduced_batch_dev(batch.d_pay.data_ptr() + pay_off, batch.stride, batch.d_len.data_ptr(), 2, f2, c2, k,
                                         o.data_ptr() + out_off)
        assert e.value.code == -1, (cs.kernel, k, e.value.code)   # VC2HIP_EINVAL
        hip.sync()
        assert bool((o == 0xA5).all()), (cs.kernel, k)
        assert hip.dwt_launches() == before, (cs.kernel, k)
    with pytest.raises(Vc2HipError, match="Daub97"):
        f2, c2 = daub.fmt_cp(hip.lib)
        hip.decode_reduced_batch_dev(batch.d_pay.data_ptr(), batch.stride, batch.d_len.data_ptr(), 2, f2, c2, 1, batch.out(64).data_ptr())
    # the context is usable afterwards
    assert batch.torch.equal(batch.reduced(hip, fmt, cp, 1, case.raw_bytes(1)), good)
    hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# full size
# ---------------------------------------------------------------------------------------------------------------------
def test_cfg2_128_pictures_mixed_with_full_calls(oracle):
    """cfg 2 (UHD-1 4:2:2 10-bit DD97 depth 4 q16 S2), 4 distinct pictures cycled to 128 per call (the one-pass index and
    the large-batch plans): k = 1 and 2, twice per context, then the full decoder on the same context -- mixing the calls
    disturbs neither"""
    w, h, n = 3840, 2160, 128
    case = pr.Case(oracle, w, h, "422", 10, "DD97", 4, 1, 2, q=16, scalar=2)
    raws = [synth_fast(w, h, "422", 10, 900 + i) for i in range(4)]
    pays = [pr.oracle_payloads(oracle, case, r)[0] for r in raws]
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    batch = Batch(pays, n=n)
    for rep in range(2):
        for k in (1, 2):
            got = batch.reduced(hip, fmt, cp, k, case.raw_bytes(k))
            _launch_facts(hip, k, "default")
            for i in range(4):
                want = batch.torch.frombuffer(bytearray(pr.reduced_picture(oracle, case, pays[i], k)), dtype=batch.torch.uint8).to("cuda:0")
                for j in range(i, n, 4):
                    assert batch.torch.equal(got[j], want), (rep, k, j)
            del got
    full = batch.full(hip, fmt, cp, case.raw_bytes())
    for i in range(4):
        dec, _ = oracle.decode_stream(case.params(), oracle.encode_stream(case.params(), raws[i], 1), 1)
        want = batch.torch.frombuffer(bytearray(dec), dtype=batch.torch.uint8).to("cuda:0")
        for j in range(i, n, 4):
            assert batch.torch.equal(full[j], want), j
    hip.close()


@pytest.mark.parametrize("cfg", ["cfg1", "cfg5"])
def test_cfg1_and_cfg5_full_size(oracle, cfg):
    if cfg == "cfg1":
        case = pr.Case(oracle, 1920, 1080, "422", 10, "LeGall", 2, 2, 4, q=12, scalar=1)
    else:
        case = pr.Case(oracle, 1920, 1080, "422", 8, "LeGall", 3, 1, 2, mode="LD", s=1036800, word_bytes=1)
    raws = [synth_fast(1920, 1080, "422", case.bits, 700 + i, word_bytes=case.word_bytes) for i in range(2)]
    pays = [pr.oracle_payloads(oracle, case, r)[0] for r in raws]
    hip = _ctx()
    fmt, cp = case.fmt_cp(hip.lib)
    batch = Batch(pays, n=8)
    got = batch.reduced(hip, fmt, cp, 1, case.raw_bytes(1)).cpu().numpy()
    _launch_facts(hip, 1, "default")
    for i in range(2):
        want = pr.reduced_picture(oracle, case, pays[i], 1)
        for j in range(i, 8, 2):
            assert got[j].tobytes() == want, (cfg, j)
    hip.close()
