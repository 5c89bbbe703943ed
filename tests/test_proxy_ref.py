"""CPU checks of the reduced-picture definition (tests/proxy_ref.py) against the oracle, and of the ABI's three places
(header, library, binding) for vc2hip_decode_reduced_batch_dev.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import proxy_ref as pr
from synth import synth
from vc2lib import KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vc2hip_decode_reduced_batch_dev"


def _constant_raw(case, value):
    """a picture whose every sample is `value` (signed, around the mid level) in all three components"""
    word = (value + (1 << (case.bits - 1))) << (8 * case.word_bytes - case.bits)
    n = case.raw_bytes() // case.word_bytes
    return bytes(word.to_bytes(case.word_bytes, "big")) * n


@pytest.mark.parametrize("kernel", list(pr.LOWPASS_GAIN_BITS))
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_constants_come_back_exact(oracle, kernel, depth):
    """a constant picture, coded without loss (q = 0) by the oracle's encoder, is that constant at every reduced size: the
    normalisation takes out exactly the low-pass gain of the dropped levels.  The bit depths' extremes included -- but for
    the one combination the reference itself cannot code: Fidelity's LL is value * 4**depth, and at 12 bits and depth 3 or 4
    the extremes pass the 65534 of the reference's code words, so the oracle's own decoder does not return the picture;
    there is no lossless stream to reduce, and the case is left out by that very condition."""
    for bits, wb in ((8, 1), (10, 2), (12, 2)):
        for value in (-(1 << (bits - 1)), (1 << (bits - 1)) - 1, 37):
            case = pr.Case(oracle, 64, 32, "422", bits, kernel, depth, 1, 2, q=0, scalar=4, word_bytes=wb)
            raw = _constant_raw(case, value)
            (payload,) = pr.oracle_payloads(oracle, case, raw)
            if abs(value) << (pr.LOWPASS_GAIN_BITS[kernel] * depth) > 65534:
                assert oracle.decode_stream(case.params(), oracle.encode_stream(case.params(), raw, 1), 1)[0] != raw
                continue
            assert pr.full_picture(oracle, case, payload) == raw
            for k in range(1, depth):
                want = raw[:case.word_bytes] * (case.raw_bytes(k) // case.word_bytes)
                assert pr.reduced_picture(oracle, case, payload, k) == want, (bits, value, k)


def test_without_the_normalisation_the_values_are_too_large(oracle):
    case = pr.Case(oracle, 64, 32, "422", 10, "Fidelity", 3, 1, 2, q=0, scalar=4)
    (payload,) = pr.oracle_payloads(oracle, case, _constant_raw(case, 100))
    y = pr.dequantised_planes(oracle, case, payload)[0]
    raw2 = oracle.dwt_inverse(np.ascontiguousarray(y[::4, ::4]), KERNELS["Fidelity"], 1, (8, 16))
    assert np.all(raw2 == 100 << 4) and np.all(pr.normalise(raw2, pr.norm_bits("Fidelity", 2)) == 100)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_one_level_at_a_time_is_the_oracles_inverse(oracle, kernel):
    """step 2 against the oracle's own transform: inverting ONE level at a time on plane[::2**l, ::2**l], l = d - 1 ... 0,
    written back in place, reproduces dwt_inverse(plane, K, d); and the state after level k, subsampled, is the subsampled
    plane inverted at depth d - k -- what proxy_ref.reduced_component computes.  All seven wavelets, a padded 136 x 240 plane."""
    d, K = 4, KERNELS[kernel]
    rng = np.random.default_rng(11)
    ph, pw = oracle.padded_size(136, d), oracle.padded_size(240, d)
    plane = rng.integers(-900, 900, size=(ph, pw)).astype(np.int32)
    plane[rng.random((ph, pw)) < 0.4] = 0
    state = plane.copy()
    for l in range(d - 1, -1, -1):
        state[::1 << l, ::1 << l] = oracle.dwt_inverse(np.ascontiguousarray(state[::1 << l, ::1 << l]), K, 1)
        if 1 <= l <= d - 1:
            sub = oracle.dwt_inverse(np.ascontiguousarray(plane[::1 << l, ::1 << l]), K, d - l)
            assert np.array_equal(state[::1 << l, ::1 << l], sub), (kernel, l)
    assert np.array_equal(state, oracle.dwt_inverse(plane, K, d)), kernel


@pytest.mark.parametrize("mode,kw", [("HQ_ConstQ", dict(q=9, scalar=2, prefix=3)), ("HQ_CBR", dict(s=9000, scalar=1)), ("LD", dict(s=6000))])
def test_payloads_and_composition_are_the_oracles(oracle, mode, kw):
    """the helpers the GPU tests stand on: oracle_payloads finds the slice bytes of the oracle's stream, and the
    composition unpack -> dequantise -> inverse -> emit at k = 0 gives oracle.decode_stream's picture (padded in both
    directions: 76 x 44 at depth 3 is 80 x 48)"""
    case = pr.Case(oracle, 76, 44, "422", 10, "LeGall", 3, 1, 2, mode=mode, **kw)
    raw = synth(76, 44, "422", 10, 17, frames=2)
    stream = oracle.encode_stream(case.params(), raw, 2)
    dec, n = oracle.decode_stream(case.params(), stream, 2)
    pays = pr.oracle_payloads(oracle, case, raw, 2)
    assert n == 2 and stream[:-13].endswith(pays[1]) and pays[0] in stream
    rb = case.raw_bytes()
    assert [pr.full_picture(oracle, case, p) for p in pays] == [dec[:rb], dec[rb:]]
    if mode != "HQ_CBR":   # (and packing the planes again gives the payload back)
        assert pr.pack_planes(oracle, case, *pr.quantised_planes(oracle, case, pays[0])) == pays[0]
    for k in case.drops():
        assert len(pr.reduced_picture(oracle, case, pays[0], k)) == case.raw_bytes(k)


def test_reduced_picture_is_close_to_the_subsampled_one(oracle):
    """a plausibility check of the whole definition on a real picture (the exact pins are above): LeGall's low-pass sample
    sits on the even sample it replaces, so the reduced picture is the full one at every 2**k-th sample, smoothed.  The
    pictures differ by the generator's noise (sigma = 1 % of full scale, 10.2 levels: a mean absolute difference of
    8.2 where nothing is smoothed) and the smoothing of a sinusoid of 43 samples' period, a few levels: below 16."""
    case = pr.Case(oracle, 128, 64, "444", 10, "LeGall", 3, 1, 1, q=0, scalar=4)
    raw = synth(128, 64, "444", 10, 23)
    (payload,) = pr.oracle_payloads(oracle, case, raw)
    full = np.frombuffer(raw, ">u2").reshape(3, 64, 128).astype(np.int64) >> 6
    for k in (1, 2):
        got = np.frombuffer(pr.reduced_picture(oracle, case, payload, k), ">u2").reshape(3, 64 >> k, 128 >> k).astype(np.int64) >> 6
        assert np.abs(got - full[:, ::1 << k, ::1 << k]).mean() < 16, k


def test_header_declares_the_call():
    hdr = open(os.path.join(ROOT, "include", "vc2hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", code)
    assert m, NAME + " is not declared in include/vc2hip.h"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["vc2hip_ctx *ctx", "const void *d_payload", "size_t payload_stride", "const uint64_t *d_lens", "int n",
                    "const vc2hip_picture_format *fmt", "const vc2hip_coding_params *cp", "int drop_levels", "void *d_raw_out"]
    # the header says what the call does not validate
    assert "not validated" in hdr[hdr.index("1/2, 1/4, 1/8"):hdr.index("int " + NAME)]


def test_library_and_binding_carry_the_call():
    import vc2hip_py
    assert NAME in vc2hip_py.EXPORTS
    lib = C.CDLL(os.path.join(ROOT, "vc2-reference_amd", "libvc2hip.so"))
    assert hasattr(lib, NAME)
    assert hasattr(vc2hip_py.Vc2Hip, "decode_reduced_batch_dev")
    f = vc2hip_py.reduced_format(vc2hip_py.picture_format(1920, 1080, "422", 10), 3)
    assert (f.width, f.height, f.chroma_format, f.bit_depth, f.word_bytes) == (240, 135, 1, 10, 2)
    exports = open(os.path.join(ROOT, "vc2-reference_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*vc2hip_\*;", exports)   # the map exports every vc2hip_ name the header declares
