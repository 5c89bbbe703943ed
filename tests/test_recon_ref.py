"""CPU checks of the definition of vc2hip_encode_recon_batch_dev (tests/recon_ref.py) against the oracle, of psnr_db, and
of the ABI's three places (header, library, binding).  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import proxy_ref as pr
import recon_ref as rr
from synth import noise_frame, synth, words_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vc2hip_encode_recon_batch_dev"

# (w, h, cf, bits, word_bytes, wavelet, depth, u, a, coding, picture); the LD rows include tight budgets: indices near the top
# of the range, where a slice cut by the bounded write would show as a picture other than the shortcut's
SHORTCUT = [
    (76, 44, "422", 10, 2, "LeGall", 3, 1, 2, dict(q=9, scalar=2, prefix=3), "synth"),
    (128, 64, "444", 12, 2, "DD97", 3, 1, 1, dict(q=0, scalar=8), "noise"),
    (128, 32, "420", 8, 1, "Daub97", 2, 2, 2, dict(q=21, scalar=1), "synth"),
    (64, 32, "422", 16, 3, "Fidelity", 2, 1, 2, dict(q=30, scalar=4), "words"),
    (128, 64, "422", 10, 2, "DD137", 3, 1, 2, dict(q=110, scalar=1), "noise"),
    (76, 44, "422", 10, 2, "Haar0", 3, 1, 2, dict(mode="HQ_CBR", s=9000, scalar=1), "synth"),
    (128, 64, "420", 12, 2, "Haar1", 2, 2, 4, dict(mode="HQ_CBR", s=6000, scalar=2, prefix=1), "noise"),
    (76, 44, "422", 10, 2, "LeGall", 3, 1, 2, dict(mode="LD", s=6000), "synth"),
    (128, 64, "444", 10, 2, "DD97", 3, 1, 1, dict(mode="LD", s=1500), "noise"),
    (128, 64, "422", 12, 2, "Haar1", 2, 2, 2, dict(mode="LD", s=700), "noise"),
    (64, 64, "420", 8, 1, "Daub97", 2, 2, 2, dict(mode="LD", s=300), "noise"),
    (128, 64, "422", 16, 2, "LeGall", 3, 1, 2, dict(mode="LD", s=400), "noise"),
]


def _raw(c, seed, kind):
    if c.word_bytes > 2 or kind == "words":
        return words_frame(c.w, c.h, c.cf, c.bits, seed, c.word_bytes)
    if kind == "noise":
        return noise_frame(c.w, c.h, c.cf, c.bits, seed, word_bytes=c.word_bytes)
    return synth(c.w, c.h, c.cf, c.bits, seed, word_bytes=c.word_bytes)


@pytest.mark.parametrize("row", SHORTCUT, ids=lambda r: "-".join(str(x) for x in r[:9]) + "-" + r[9].get("mode", "HQ_ConstQ"))
def test_the_shortcut_is_the_definition(oracle, row):
    """dwt_inverse(dequantise(quantise(dwt_forward(ingest(raw))))) with the encoder's indices is the decoder's picture of
    the encoder's payload, byte for byte, and the indices are the payload's: entropy coding is lossless.  For LD this also
    says that no slice of a payload the oracle writes is cut by the bounded write (a cut slice would lose coefficients the
    shortcut keeps)."""
    w, h, cf, bits, wb, kernel, depth, u, a, kw, kind = row
    case = pr.Case(oracle, w, h, cf, bits, kernel, depth, u, a, word_bytes=wb, **kw)
    raw = _raw(case, 31 + w + depth, kind)
    (pay, pic, sse, q), = rr.recon(oracle, case, raw)
    got, gq = rr.shortcut(oracle, case, raw)
    assert np.array_equal(gq, q)
    assert got == pic
    if case.mode == "LD":
        print("LD indices", int(q.min()), int(q.max()))
    assert all(s >= 0 for s in sse)


def test_ld_tight_budgets_reach_high_indices(oracle):
    """the tight LD rows above do what they are there for: the search ends near the top of the range"""
    top = 0
    for row in SHORTCUT:
        w, h, cf, bits, wb, kernel, depth, u, a, kw, kind = row
        if kw.get("mode") != "LD":
            continue
        case = pr.Case(oracle, w, h, cf, bits, kernel, depth, u, a, word_bytes=wb, **kw)
        top = max(top, int(rr.recon(oracle, case, _raw(case, 31 + w + depth, kind))[0][3].max()))
    assert top >= 60, top


@pytest.mark.parametrize("mode,kw", [("HQ_ConstQ", dict(q=0, scalar=8)), ("HQ_CBR", dict(s=12000, scalar=4)), ("LD", dict(s=12000))])
def test_lossless_pictures_have_no_error(oracle, mode, kw):
    """index 0 on pictures whose bits below the depth are clear (a budget that admits index 0 for the searches): the
    picture is the input, the sums are 0"""
    case = pr.Case(oracle, 64, 32, "422", 10, "LeGall", 2, 1, 2, mode=mode, **kw)
    raw = synth(64, 32, "422", 10, 5)
    (pay, pic, sse, q), = rr.recon(oracle, case, raw)
    assert int(q.max()) == 0
    assert pic == raw and sse == [0, 0, 0]


def test_sums_ignore_input_bits_below_the_depth(oracle):
    case = pr.Case(oracle, 64, 32, "422", 10, "LeGall", 2, 1, 2, q=0, scalar=8)
    raw = bytearray(synth(64, 32, "422", 10, 5))
    pic = bytes(raw)
    raw[1::2] = bytes((b | 0x3F) for b in raw[1::2])   # the six bits below a 10-bit sample in a 16-bit word
    assert rr.squared_errors(case, bytes(raw), pic) == [0, 0, 0]
    # and one level of difference in every sample is one per sample
    up = (np.frombuffer(pic, ">u2").astype(np.int64) ^ 0x40).astype(">u2").tobytes()
    assert rr.squared_errors(case, up, pic) == [64 * 32, 32 * 32, 32 * 32]


def test_psnr_db_is_the_references_formula():
    import vc2hip_py
    rng = np.random.default_rng(2)
    for bits in (8, 10, 12, 16):
        for samples in (64 * 32, 1920 * 1080, 3840 * 2160):
            for _ in range(20):
                # 30 - 90 dB: mean squared errors from 2^(2 bits) / 10^3 down to 2^(2 bits) / 10^9
                mse = float(1 << (2 * bits)) / 10 ** rng.uniform(3, 9)
                sse = max(1, int(mse * samples))
                got = vc2hip_py.psnr_db(sse, samples, bits)
                assert abs(got - rr.psnr_float32(sse, samples, bits)) < 1e-4, (bits, samples, sse)
    assert vc2hip_py.psnr_db(0, 100, 10) == float("inf")
    assert abs(vc2hip_py.psnr_db(100, 100, 10) - 20 * np.log10(1024)) < 1e-9


def test_header_declares_the_call():
    hdr = open(os.path.join(ROOT, "include", "vc2hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", code)
    assert m, NAME + " is not declared in include/vc2hip.h"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["vc2hip_ctx *ctx", "const void *d_raw", "int n", "const vc2hip_picture_format *fmt", "const vc2hip_coding_params *cp",
                    "void *d_payload", "size_t payload_stride", "uint64_t *d_lens", "void *d_recon", "uint64_t *d_sse", "int32_t *d_qidx"]
    text = hdr[hdr.index("-o Decoded"):hdr.index("int " + NAME)]
    assert "cannot wrap" in text and "DC-predicted" in text and "never decodes its own" in text


def test_library_and_binding_carry_the_call():
    import vc2hip_py
    assert NAME in vc2hip_py.EXPORTS
    so = os.path.join(ROOT, "vc2-reference_amd", "libvc2hip.so")
    names = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if ln.split()}
    assert NAME in names
    assert hasattr(C.CDLL(so), NAME)
    assert hasattr(vc2hip_py.Vc2Hip, "encode_recon_batch_dev") and callable(vc2hip_py.psnr_db)


@pytest.mark.parametrize("i", range(len(rr.MATRIX)))
def test_matrix_rows_are_encodable(oracle, i):
    """every row of the GPU matrix: the oracle encodes both pictures, the encoder's and the decoder's padded chroma planes
    agree, and the rows picked for a property have it"""
    row = rr.MATRIX[i]
    case = rr.matrix_case(oracle, row)
    assert (case.cph, case.cpw) == (oracle.padded_size(case.ch, case.depth), oracle.padded_size(case.cw, case.depth))
    raw = rr.matrix_raw(case, row)
    res = rr.recon(oracle, case, raw, 2)
    assert len(res) == 2
    if i in rr.ESCAPES:
        assert max(int(np.abs(p).max()) for p in rr.transform_planes(oracle, case, raw[:case.raw_bytes()])) > 32767
    if i == rr.NO_COEFFICIENT:
        assert not any(np.any(p) for p in pr.quantised_planes(oracle, case, res[0][0])[:3])
    if i == rr.WHOLE_PLANE:
        assert (case.ys, case.xs) == (1, 1)
