"""Deterministic synthetic frames (SURVEY.md Appendix B generator, reproduced verbatim
as the measurement contract: same seed => same bytes => the SHA-256 digests recorded
there apply)."""
import numpy as np


def synth(w, h, cf, bits, seed, frames=1, word_bytes=2):
    rng = np.random.default_rng(seed)
    cw = w if cf == '444' else w // 2
    ch = h // 2 if cf == '420' else h
    out = []
    for f in range(frames):
        for (pw, ph, c) in [(w, h, 0), (cw, ch, 1), (cw, ch, 2)]:
            y, x = np.mgrid[0:ph, 0:pw]
            base = (0.5 + 0.35 * np.sin(2 * np.pi * (x / pw * 3 + c * 0.3 + f * 0.1))
                    * np.cos(2 * np.pi * (y / ph * 2))) * (2 ** bits - 1)
            v = np.clip(np.rint(base + rng.normal(0, (2 ** bits) * 0.01, size=(ph, pw))),
                        0, 2 ** bits - 1).astype(np.uint16)
            if word_bytes == 2:
                out.append((v << (16 - bits)).astype('>u2').tobytes())
            else:
                out.append((v << (8 - bits)).astype(np.uint8).tobytes())
    return b''.join(out)


def synth_fast(w, h, cf, bits, seed, frames=1, word_bytes=2):
    """The same bytes as synth() (tests/test_synth.py compares them), ~3x sooner: the sin / cos product is formed from
    one row and one column instead of the whole grid (the same float64 operations on every sample), and the rest runs
    in place.  What remains is the generator's normal draws, which set the bytes and cannot be reordered."""
    rng = np.random.default_rng(seed)
    cw = w if cf == '444' else w // 2
    ch = h // 2 if cf == '420' else h
    top = 2 ** bits - 1
    out = []
    for f in range(frames):
        for (pw, ph, c) in [(w, h, 0), (cw, ch, 1), (cw, ch, 2)]:
            sx = 0.35 * np.sin(2 * np.pi * (np.arange(pw) / pw * 3 + c * 0.3 + f * 0.1))
            cy = np.cos(2 * np.pi * (np.arange(ph) / ph * 2))
            v = sx[None, :] * cy[:, None]
            v += 0.5
            v *= top
            v += rng.normal(0, (2 ** bits) * 0.01, size=(ph, pw))
            np.rint(v, out=v)
            np.clip(v, 0, top, out=v)
            if word_bytes == 2:
                out.append((v.astype(np.uint16) << (16 - bits)).astype('>u2').tobytes())
            else:
                out.append((v.astype(np.uint16) << (8 - bits)).astype(np.uint8).tobytes())
    return b''.join(out)


def noise_frame(w, h, cf, bits, seed, word_bytes=2, full_scale=False):
    """Uniform-noise frame (worst case for coefficient growth / code lengths)."""
    rng = np.random.default_rng(seed)
    cw = w if cf == '444' else w // 2
    ch = h // 2 if cf == '420' else h
    out = []
    for (pw, ph) in [(w, h), (cw, ch), (cw, ch)]:
        if full_scale:
            v = (rng.integers(0, 2, size=(ph, pw)) * (2 ** bits - 1)).astype(np.uint16)
        else:
            v = rng.integers(0, 2 ** bits, size=(ph, pw)).astype(np.uint16)
        if word_bytes == 2:
            out.append((v << (16 - bits)).astype('>u2').tobytes())
        else:
            out.append((v << (8 - bits)).astype(np.uint8).tobytes())
    return b''.join(out)


def words_frame(w, h, cf, bits, seed, word_bytes, kind="noise"):
    """A frame in words of 1 to 4 bytes (big-endian, MSB justified: what the ABI reads for any word size).  synth() and
    synth_fast() make 1- and 2-byte words only, and their bytes are a digest contract, so wider words come from here.
    kind: "noise" (uniform), "extremes" (every sample 0 or full scale) or "checker" (a full-scale checkerboard)."""
    assert 1 <= word_bytes <= 4 and 1 <= bits <= 8 * word_bytes
    rng = np.random.default_rng(seed)
    cw = w if cf == '444' else w // 2
    ch = h // 2 if cf == '420' else h
    top = (1 << bits) - 1
    out = []
    for (pw, ph) in [(w, h), (cw, ch), (cw, ch)]:
        if kind == "noise":
            v = rng.integers(0, top + 1, size=(ph, pw), dtype=np.uint64)
        elif kind == "extremes":
            v = rng.integers(0, 2, size=(ph, pw), dtype=np.uint64) * np.uint64(top)
        else:
            yy, xx = np.mgrid[0:ph, 0:pw]
            v = ((yy + xx) & 1).astype(np.uint64) * np.uint64(top)
        v = v << np.uint64(8 * word_bytes - bits)
        b = np.stack([(v >> np.uint64(8 * (word_bytes - 1 - k))) & np.uint64(0xFF) for k in range(word_bytes)], axis=-1)
        out.append(b.astype(np.uint8).tobytes())
    return b''.join(out)
