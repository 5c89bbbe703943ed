"""An independent witness for the oracle's wavelet transform (oracle/vc2_oracle.c, vc2o_dwt_forward / _inverse).

The reference digests (tests/golden/reference_digests.json) pin the oracle's transform for LeGall, DD97 and Fidelity only.
For DD137, Haar0, Haar1 and Daub97 the oracle's own checks are self-consistency (inverse undoes forward, q = 0 is lossless),
which any invertible lifting passes -- and every GPU test of those wavelets compares against this oracle.  So here is a
second, plain statement of the seven filters: numpy int64, written from the lifting definitions of SMPTE ST 2042-1 (the
synthesis steps with their tap offsets, the same-parity clamp at the ends of a line, the per-level accuracy shift),
forward as the synthesis undone step by step.  It is calibrated on the three wavelets the digests pin, then it is the
witness for the other four.  It also tracks every intermediate value (the samples after each step and each step's sum
before its shift): the oracle and the GPU kernels compute in int32, and the model says whether that is exact."""
import numpy as np
import pytest

from vc2lib import KERNELS

# Synthesis lifting steps, in the order the decoder applies them: (target parity, sign, taps, d, shift).  A step updates
# every sample 2n + parity:  x[2n + parity] += sign * ((sum_i taps[i - d] * x[src(n + i)] + round) >> shift), i = d ...
# d + len(taps) - 1, where src(m) = 2m - 1 for an even target (odd sources) and 2m for an odd one (even sources); a
# source outside the line takes the nearest sample of its own parity; round = 1 << (shift - 1), none for shift 0.
_DD4 = (-1, 9, 9, -1)
SYNTHESIS = {
    "DD97":     [(0, -1, (1, 1), 0, 2), (1, +1, _DD4, -1, 4)],
    "LeGall":   [(0, -1, (1, 1), 0, 2), (1, +1, (1, 1), 0, 1)],
    "DD137":    [(0, -1, _DD4, -1, 5), (1, +1, _DD4, -1, 4)],
    "Haar0":    [(0, -1, (1,), 1, 1), (1, +1, (1,), 0, 0)],
    "Haar1":    [(0, -1, (1,), 1, 1), (1, +1, (1,), 0, 0)],
    "Fidelity": [(1, +1, (-2, 10, -25, 81, 81, -25, 10, -2), -3, 8), (0, -1, (-8, 21, -46, 161, 161, -46, 21, -8), -3, 8)],
    "Daub97":   [(0, -1, (1817, 1817), 0, 12), (1, -1, (3616, 3616), 0, 12), (0, +1, (217, 217), 0, 12),
                 (1, +1, (6497, 6497), 0, 12)],
}
ACCURACY = {"DD97": 1, "LeGall": 1, "DD137": 1, "Haar0": 0, "Haar1": 1, "Fidelity": 0, "Daub97": 1}
I32 = (-2 ** 31, 2 ** 31 - 1)


class Model:
    """the 2-D transform of one padded plane in the interleaved in-place layout (level l works on the samples at
    multiples of 2^l); `peak` is the largest magnitude any intermediate value reached"""

    def __init__(self, wavelet, wrap32=False):
        self.steps = SYNTHESIS[wavelet]
        self.acc = ACCURACY[wavelet]
        self.wrap32 = wrap32   # two's complement int32 arithmetic (what C int32 code does beyond the domain)
        self.peak = 0

    def _w(self, a):
        return (a + 2 ** 31) % 2 ** 32 - 2 ** 31 if self.wrap32 else a

    def _see(self, a):
        if a.size:
            self.peak = max(self.peak, int(np.abs(a).max()))

    def _step(self, x, step, undo):
        """one lifting step along axis 0 of x (columns side by side); undo: the analysis form (opposite sign)"""
        parity, sign, taps, d, shift = step
        n = x.shape[0]
        m = np.arange(n // 2)
        acc = np.zeros((len(m),) + x.shape[1:], np.int64)
        for k, t in enumerate(taps):
            i = m + d + k
            if parity == 0:
                src = np.clip(2 * i - 1, 1, n - 1)
            else:
                src = np.clip(2 * i, 0, n - 2)
            acc += t * x[src]
            self._see(acc)
            acc = self._w(acc)
        if shift:
            acc += 1 << (shift - 1)
            self._see(acc)
            acc = self._w(acc)
        upd = acc >> shift
        x[2 * m + parity] = self._w(x[2 * m + parity] + (-sign * upd if undo else sign * upd))
        self._see(x)

    def _analyse(self, x):
        for st in reversed(self.steps):
            self._step(x, st, True)

    def _synthesise(self, x):
        for st in self.steps:
            self._step(x, st, False)

    def forward(self, plane, depth):
        x = np.array(plane, np.int64)
        for level in range(depth):
            s = 1 << level
            v = x[::s, ::s]            # a view: the lifting writes through to x
            v <<= self.acc
            self._see(v)
            t = v.T.copy()             # rows first ...
            self._analyse(t)
            v[...] = t.T
            t = v.copy()               # ... then columns
            self._analyse(t)
            v[...] = t
        return x

    def inverse(self, coef, depth):
        x = np.array(coef, np.int64)
        for level in range(depth - 1, -1, -1):
            s = 1 << level
            v = x[::s, ::s]
            t = v.copy()               # columns first ...
            self._synthesise(t)
            v[...] = t
            t = v.T.copy()             # ... then rows
            self._synthesise(t)
            v[...] = t.T
            if self.acc:
                v += 1 << (self.acc - 1)
                self._see(v)
                v >>= self.acc
        return x


def _pad(plane, depth):
    """edge replication up to a multiple of 2^depth (the encoder's padding)"""
    q = 1 << depth
    h, w = plane.shape
    return np.pad(plane, ((0, -h % q), (0, -w % q)), mode="edge")


def _inputs(bits, h, w, seed):
    """signed samples of `bits` bits: uniform noise, full-scale noise (every sample at one of the two extremes) and a
    full-scale checkerboard -- the largest growth the lifting steps can see"""
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    yield "noise", rng.integers(lo, hi + 1, size=(h, w)).astype(np.int64)
    yield "extremes", np.where(rng.integers(0, 2, size=(h, w)) == 1, hi, lo).astype(np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    yield "checker", np.where((yy + xx) & 1, hi, lo).astype(np.int64)


CALIBRATION = ["LeGall", "DD97", "Fidelity"]
WITNESSED = ["DD137", "Haar0", "Haar1", "Daub97"]
# (height, width) per depth: none a multiple of 2^depth, so every depth pads both ways
SHAPES = {1: (13, 21), 2: (30, 37), 3: (45, 27), 4: (37, 70), 5: (70, 45)}
# The limit of the int32 domain: (wavelet, bits, depth) where some intermediate value of these inputs leaves int32.  Only
# Daub97's 16-bit pictures from depth 2 on (the sum 6497 * (a + b) of its last analysis step passes 2^31 once the
# coefficients pass ~165 000); Fidelity at 16 bits, depth 5 peaks at ~1.6e9, inside.  There the oracle computes what
# two's complement int32 arithmetic gives (as C int32 code, the GPU kernels' included, does), not the exact lifting.
DOMAIN_LIMITS = {("Daub97", 16, d) for d in (2, 3, 4, 5)}


def _compare(oracle, wavelet, depth, bits, seed):
    h, w = SHAPES[depth]
    k = KERNELS[wavelet]
    outside = False
    for name, x in _inputs(bits, h, w, seed):
        what = f"{wavelet} depth {depth} {bits}-bit {name} {h}x{w}"
        m = Model(wavelet)
        want = m.forward(_pad(x, depth), depth)
        assert np.array_equal(m.inverse(want, depth), _pad(x, depth)), f"{what}: the model's inverse does not undo its forward"
        # the inverse of coefficients the forward transform did not make (a decoder's input after quantisation)
        coef = want + np.random.default_rng(seed + 1).integers(-40, 41, size=want.shape)
        back = m.inverse(coef, depth)
        if m.peak > I32[1]:
            assert (wavelet, bits, depth) in DOMAIN_LIMITS, f"{what}: an intermediate value reaches {m.peak}, outside int32"
            outside = True
            m = Model(wavelet, wrap32=True)
            want = m.forward(_pad(x, depth), depth)
            coef = np.clip(coef, *I32)
            back = m.inverse(coef, depth)
        got = oracle.dwt_forward(x.astype(np.int32), k, depth)
        assert np.array_equal(got, want), f"{what}: forward differs at {np.argwhere(got != want)[:4].tolist()}"
        got = oracle.dwt_inverse(coef.astype(np.int32), k, depth)
        assert np.array_equal(got, back), f"{what}: inverse differs at {np.argwhere(got != back)[:4].tolist()}"
    assert outside == ((wavelet, bits, depth) in DOMAIN_LIMITS), f"{wavelet} depth {depth} {bits}-bit: DOMAIN_LIMITS is stale"


@pytest.mark.parametrize("wavelet", CALIBRATION)
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_model_calibrated_on_the_pinned_wavelets(oracle, wavelet, depth):
    """the model equals the oracle where the reference digests pin the oracle: if this fails, the model is wrong"""
    for bits in (8, 10, 12, 16):
        _compare(oracle, wavelet, depth, bits, seed=1000 * depth + bits)


@pytest.mark.parametrize("wavelet", WITNESSED)
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_oracle_matches_the_model(oracle, wavelet, depth):
    """the oracle's DD137 / Haar0 / Haar1 / Daub97 transforms equal the calibrated model, forward and inverse; where an
    intermediate value leaves int32 (DOMAIN_LIMITS, and only there) they equal the model in int32 arithmetic"""
    for bits in (8, 10, 12, 16):
        _compare(oracle, wavelet, depth, bits, seed=2000 * depth + bits)


def test_model_is_not_self_consistency_only(oracle):
    """the witness tells lifting filters apart: a wrong rounding shift is still invertible (it would pass the round-trip
    checks) but differs from the model, and so does a neighbouring wavelet"""
    x = next(_inputs(10, 30, 37, 7))[1]
    good = Model("DD137").forward(_pad(x, 2), 2)
    bad = Model("DD137")
    bad.steps = [(0, -1, _DD4, -1, 5), (1, +1, _DD4, -1, 3)]
    assert not np.array_equal(bad.forward(_pad(x, 2), 2), good)
    assert np.array_equal(bad.inverse(bad.forward(_pad(x, 2), 2), 2), _pad(x, 2))
    assert not np.array_equal(oracle.dwt_forward(x.astype(np.int32), KERNELS["Haar0"], 2), Model("Haar1").forward(_pad(x, 2), 2))
