"""The CPU definition of vc2hip_encode_recon_batch_dev, composed of what tests/proxy_ref.py has:

  payload   the oracle encoder's slice bytes (oracle_payloads)
  picture   the full decoder's bytes for that payload (full_picture)
  indices   what the payload's slices carry (quantised_planes(...)[3])
  sums      per component, over the unpadded h x w samples, of (a - b)^2 with a, b = word >> (8 * word_bytes - bits) of
            the input and of the picture: int64 differences, Python-int sums

and the shortcut the GPU path takes instead of coding and decoding: ingest -> forward transform -> indices -> quantise ->
dequantise -> inverse transform -> emit, through the oracle's own functions (tests/test_recon_ref.py shows the two agree)."""
import numpy as np

import proxy_ref as pr
from vc2lib import KERNELS


def sample_values(data, word_bytes, bits):
    """big-endian MSB-justified words -> sample values (int64); bits below the depth are dropped"""
    b = np.frombuffer(data, np.uint8).reshape(-1, word_bytes).astype(np.int64)
    w = np.zeros(b.shape[0], np.int64)
    for k in range(word_bytes):
        w = (w << 8) | b[:, k]
    return w >> (8 * word_bytes - bits)


def component_bytes(case):
    return [case.h * case.w * case.word_bytes] + [case.ch * case.cw * case.word_bytes] * 2


def squared_errors(case, raw, picture):
    """[Y, U, V] as Python ints"""
    out, at = [], 0
    for nb in component_bytes(case):
        d = sample_values(raw[at:at + nb], case.word_bytes, case.bits) - sample_values(picture[at:at + nb], case.word_bytes, case.bits)
        if case.bits > 24:   # (products beyond int64's reach: Python ints)
            d = d.astype(object)
        out.append(int((d * d).sum()))
        at += nb
    return out


def recon(oracle, case, raw, n=1):
    """per picture: (payload, picture, [Y, U, V] sums, indices ys x xs)"""
    rb = case.raw_bytes()
    out = []
    for i, pay in enumerate(pr.oracle_payloads(oracle, case, raw, n)):
        pic = pr.full_picture(oracle, case, pay)
        out.append((pay, pic, squared_errors(case, raw[i * rb:(i + 1) * rb], pic), pr.quantised_planes(oracle, case, pay)[3]))
    return out


def shortcut(oracle, case, raw):
    """(picture, indices) of ONE picture without an entropy coder: what entitles the GPU path to skip it"""
    assert (case.cph, case.cpw) == (oracle.padded_size(case.ch, case.depth), oracle.padded_size(case.cw, case.depth)), \
        "the decoder derives other chroma planes than the encoder pads"
    K, d = KERNELS[case.kernel], case.depth
    qm = oracle.quant_matrix(K, d)
    shapes = [(case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)]
    planes, at = [], 0
    for (h, w) in shapes:
        nb = h * w * case.word_bytes
        planes.append(oracle.dwt_forward(oracle.ingest(raw[at:at + nb], case.word_bytes, case.bits, (h, w)), K, d))
        at += nb
    if case.mode == "HQ_ConstQ":
        q = np.full((case.ys, case.xs), case.q, np.int32)
    elif case.mode == "HQ_CBR":
        q = oracle.cbr_qindices(*planes, d, qm, oracle.slice_bytes(case.ys, case.xs, case.s, case.scalar), case.scalar)
    else:
        q = oracle.ld_qindices(*planes, d, qm, oracle.slice_bytes(case.ys, case.xs, case.s, 1))
    quant, dequant = (oracle.quantise_ld, oracle.dequantise_ld) if case.mode == "LD" else (oracle.quantise_np, oracle.dequantise_np)
    out = []
    for p, shape in zip(planes, shapes):
        x = oracle.dwt_inverse(dequant(quant(p, d, q, qm), d, q, qm), K, d, shape)
        out.append(oracle.clip_emit(x, case.word_bytes, case.bits).tobytes())
    return b"".join(out), q


def psnr_float32(sse, samples, bits):
    """EncodeStream.cpp:716-717 as the reference evaluates it: float variables throughout"""
    rms = np.sqrt(np.float32(sse) / np.float32(samples)) / np.float32(2 ** bits)
    return float(np.float32(-20) * np.log10(np.float32(rms)))


# The GPU matrix (tests/test_gpu_recon.py), chosen here on the CPU so that the oracle encodes every row
# (tests/test_recon_ref.py::test_matrix_rows_are_encodable): (w, h, cf, bits, word_bytes, wavelet, depth, u, a, coding, picture).
# Every wavelet, chroma format, bit depth 8 / 10 / 12 / 16 and word size 1 - 4 at least twice; all three modes; prefix and
# scalar other than 0 / 1; pictures padded in height (270 -> 272), in width (1004 -> 1008) and in both (1004 x 60);
# q = 0, mid indices, an index of 100 or more that leaves no coefficient; 12- and 16-bit noise whose transform
# coefficients leave 16 bits (ESCAPES: the escape store); one slice per picture (WHOLE_PLANE: the whole-plane path).
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
    (1024, 64, "422", 10, 2, "Daub97", 3, 1, 2, dict(q=12, scalar=2), "synth"),
    (512, 64, "444", 16, 2, "Daub97", 2, 2, 4, dict(mode="HQ_CBR", s=60000, scalar=4), "noise"),
    (1004, 60, "422", 10, 2, "Daub97", 3, 1, 2, dict(mode="LD", s=20000), "synth"),
    (256, 64, "422", 16, 4, "LeGall", 2, 2, 4, dict(q=20, scalar=8), "words"),
    (512, 64, "420", 10, 4, "DD97", 2, 2, 4, dict(q=104, scalar=1), "words"),
    (1024, 64, "422", 16, 2, "LeGall", 2, 2, 4, dict(q=16, scalar=8), "noise"),
    (1024, 64, "422", 12, 2, "Fidelity", 3, 1, 2, dict(q=30, scalar=8), "noise"),
    (1024, 512, "444", 10, 2, "DD97", 3, 64, 128, dict(q=24, scalar=4000), "synth"),
]
ESCAPES = (20, 21)     # rows whose transform coefficients pass 32767
NO_COEFFICIENT = 19    # the row whose index leaves no coefficient
WHOLE_PLANE = 22


def matrix_case(oracle, row):
    w, h, cf, bits, wb, kernel, depth, u, a, kw, kind = row
    return pr.Case(oracle, w, h, cf, bits, kernel, depth, u, a, word_bytes=wb, **kw)


def matrix_raw(case, row, frames=2):
    from synth import noise_frame, synth, words_frame
    seed, kind = 40 + case.w + case.depth, row[10]
    if case.word_bytes > 2 or kind == "words":
        return b"".join(words_frame(case.w, case.h, case.cf, case.bits, seed + f, case.word_bytes) for f in range(frames))
    if kind == "noise":
        return b"".join(noise_frame(case.w, case.h, case.cf, case.bits, seed + f, word_bytes=case.word_bytes) for f in range(frames))
    return synth(case.w, case.h, case.cf, case.bits, seed, frames=frames, word_bytes=case.word_bytes)


def transform_planes(oracle, case, raw):
    """the forward transform of one picture's three components"""
    out, at = [], 0
    for (h, w) in [(case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)]:
        nb = h * w * case.word_bytes
        out.append(oracle.dwt_forward(oracle.ingest(raw[at:at + nb], case.word_bytes, case.bits, (h, w)), KERNELS[case.kernel], case.depth))
        at += nb
    return out
