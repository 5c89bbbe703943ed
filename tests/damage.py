"""Damaged slice payloads by class, and what the CPU oracle makes of them (pure CPU: no GPU import here).

A mutation is a Mut: the bytes of a payload slot and the length the decoder is told (d_lens).  For most classes the two
agree; `short` tells a smaller length over the whole payload's bytes, `long` a larger one over a slot that is zero behind
the payload.  Every generator is seeded and deterministic: same input, same seed, same list.

The rule the tests hold the decoders to ("Damaged payloads"): for every byte string and length the library gives
the oracle's picture or refuses as the oracle does, and the other pictures of the batch are untouched.

References
  HQ   proxy_ref.full_picture / reduced_picture over slot[:length] (hq_unpack, dequantise_np, dwt_inverse, clip_emit)
  LD   oracle.decode_stream over the stream's own head, the mutated payload and the 13-byte end of sequence: the
       reference's reader goes on into what follows a slice whose luma length field exceeds it (Slices.cpp:246-303), so
       ld_unpack, which reads every slice at its own offset, is NOT the reference here."""
import random
from collections import namedtuple

import numpy as np

import index_ref
import proxy_ref as pr
from synth import noise_frame, synth
from vc2lib import OracleError

Mut = namedtuple("Mut", "cls tag data length")
Slice = namedtuple("Slice", "start lenpos end")      # lenpos: the positions of the three length bytes

ESTREAM, EQINDEX = -10, -2                           # VC2O_ESTREAM / VC2O_EQINDEX == VC2HIP_ESTREAM / VC2HIP_EQINDEX


def index_chunk(prefix, scalar):
    """the bytes the slice index takes per chunk: by the longest slice the length bytes can describe (idx_entries and
    idx_chunk of vc2hip_slices.hip, restated in index_ref.plan) -- 8 KiB at scalar 1, 16 KiB from scalar 2 on"""
    return index_ref.plan(prefix, scalar, 0).CH


# the share of a class the oracle must accept, so that "both refuse" cannot carry a comparison (`length`, `hdr0`: no cap)
MIN_ACCEPTED = {"random": 0.9, "boundary": 0.9, "run00": 0.9, "runff": 0.9, "long": 0.9, "hdr1": 0.9, "body00": 0.9, "bodyff": 0.9}


class Base:
    """one valid payload and what the generators and references need of it"""

    def __init__(self, oracle, case, raw, chunk_mutations=False):
        self.case, self.raw = case, raw
        # (chunk > 0: `random` and `length` add a mutation on either side of a chunk boundary of the slice index)
        self.chunk = index_chunk(case.prefix, case.scalar) if chunk_mutations and case.mode != "LD" else 0
        self.ns = case.ys * case.xs
        if case.mode == "LD":
            stream = oracle.encode_stream(case.params(), raw, 1)
            self.head, self.payload, self.tail = stream[:-13 - case.s], stream[-13 - case.s:-13], stream[-13:]
            sb = oracle.slice_bytes(case.ys, case.xs, case.s, 1).ravel()
            off = np.concatenate([[0], np.cumsum(sb)])
            assert int(off[-1]) == len(self.payload)
            self.slices = [Slice(int(off[i]), (), int(off[i + 1])) for i in range(self.ns)]
        else:
            (self.payload,) = pr.oracle_payloads(oracle, case, raw)
            self.head = self.tail = b""
            self.slices = hq_walk(self.payload, self.ns, case.prefix, case.scalar)


def hq_walk(payload, ns, prefix, scalar):
    """per slice: prefix bytes, the index byte, three times a length byte and length * scalar bytes"""
    pos, out = 0, []
    for _ in range(ns):
        start = pos
        pos += prefix + 1
        lenpos = []
        for _ in range(3):
            lenpos.append(pos)
            pos += 1 + payload[pos] * scalar
        out.append(Slice(start, tuple(lenpos), pos))
    assert pos == len(payload), f"the slice walk ends on byte {pos} of {len(payload)}"
    return out


def _picked(ns):
    return sorted({0, 1 % ns, ns // 2, max(ns - 2, 0), ns - 1})


def _mut(cls, tag, data, length=None):
    data = bytes(data)
    return Mut(cls, tag, data, len(data) if length is None else length)


def gen_random(base, seed, count=24):
    """tools/fuzz_decode.py's rule: 1, 1, 2 or 5 bytes overwritten with 0, 0xFF or a random value"""
    rnd = random.Random(seed)
    out = []
    for i in range(count):
        pay = bytearray(base.payload)
        for _ in range(rnd.choice([1, 1, 2, 5])):
            pay[rnd.randrange(len(pay))] = rnd.choice([0, 0xFF, rnd.randrange(256)])
        out.append(_mut("random", f"#{i}", pay))
    if base.chunk and len(base.payload) > base.chunk:   # the byte just before and the byte just after a chunk boundary
        b = (len(base.payload) // base.chunk + 1) // 2 * base.chunk
        for at in (b - 1, b):
            pay = bytearray(base.payload)
            pay[at] = rnd.choice([0, 0xFF]) if pay[at] not in (0, 0xFF) else 0x55
            out.append(_mut("random", f"byte {at} at chunk boundary {b}", pay))
    return out


def gen_boundary(base, seed=0, slices=None, deltas=(1, -1, 3)):
    """inside one slice the border between two components moves by d length units: both length bytes change, the data bytes
    are re-split, the slice keeps its size.  The chain stays whole; two components decode bytes coded as the other's."""
    sc, out = base.case.scalar, []
    for si in (_picked(base.ns) if slices is None else slices):
        s = base.slices[si]
        lens = [base.payload[p] for p in s.lenpos]
        data = b"".join(base.payload[p + 1:p + 1 + l * sc] for p, l in zip(s.lenpos, lens))
        for a, b in ((0, 1), (1, 2), (0, 2)):
            for d in deltas:
                for dd in (d, -d):    # (a length byte that cannot give or take: the other way)
                    if 0 <= lens[a] + dd <= 255 and 0 <= lens[b] - dd <= 255:
                        break
                else:
                    continue
                new = list(lens)
                new[a] += dd
                new[b] -= dd
                body, at = bytearray(), 0
                for l in new:
                    body.append(l)
                    body += data[at:at + l * sc]
                    at += l * sc
                pay = bytearray(base.payload)
                pay[s.lenpos[0]:s.end] = body
                assert len(pay) == len(base.payload)
                out.append(_mut("boundary", f"slice {si} {'YUV'[a]}{'YUV'[b]} {dd:+d}", pay))
    return out


def gen_length(base, seed=0):
    """one length byte set to 0, 1, 255, L - 1 or L + 1: the chain breaks, mostly refused"""
    out = []
    for si in _picked(base.ns):
        for c, p in enumerate(base.slices[si].lenpos):
            L = base.payload[p]
            for v in (0, 1, 255, (L - 1) & 255, (L + 1) & 255):
                pay = bytearray(base.payload)
                pay[p] = v
                out.append(_mut("length", f"slice {si} {'YUV'[c]} {L}->{v}", pay))
    if base.chunk and len(base.payload) > base.chunk:   # the length bytes nearest a chunk boundary, one on either side
        b = (len(base.payload) // base.chunk + 1) // 2 * base.chunk
        allpos = [p for s in base.slices for p in s.lenpos]
        before, after = max(p for p in allpos if p < b), min(p for p in allpos if p >= b)
        for p, d in ((before, 1), (after, -1)):
            pay = bytearray(base.payload)
            pay[p] = (pay[p] + d) & 255
            out.append(_mut("length", f"length byte {p} at chunk boundary {b} {d:+d}", pay))
    return out


QINDEX_VALUES = (0, 63, 100, 116, 119, 120, 127, 128, 255)


def gen_qindex(base, seed=0, slices=None):
    out = []
    for si in (sorted({0, base.ns // 3, base.ns - 1}) if slices is None else slices):
        at = base.slices[si].start + base.case.prefix
        for v in QINDEX_VALUES:
            pay = bytearray(base.payload)
            pay[at] = v
            out.append(_mut("qindex", f"slice {si} index {v}", pay))
    return out


def _largest_luma(base, count=6):
    by = sorted(range(base.ns), key=lambda i: (-base.payload[base.slices[i].lenpos[0]], i))
    return by[:count]


def _gen_runs(base, seed, cls, value, runs, count=6):
    """runs of one byte value in the luma data of the slices with the most of it (0 = the whole component).  Nine or more
    zero bytes are an exp-Golomb code of more than 32 bits.  The first run of the list opens the component, where the
    coarsest bands are (the record heads of the deep levels); the others lie anywhere in it."""
    rnd = random.Random(seed)
    out = []
    for si in _largest_luma(base, count):
        p = base.slices[si].lenpos[0]
        nbytes = base.payload[p] * base.case.scalar
        for run in runs:
            n = nbytes if run == 0 else min(run, nbytes)
            at = p + 1 + (0 if n == nbytes or run == runs[0] else rnd.randrange(nbytes - n + 1))
            pay = bytearray(base.payload)
            pay[at:at + n] = bytes([value]) * n
            out.append(_mut(cls, f"slice {si} {n} x {value:#04x} at {at}", pay))
    return out


def gen_run00(base, seed, count=6):
    return _gen_runs(base, seed, "run00", 0x00, (5, 9, 17, 0), count)


def gen_runff(base, seed, count=6):
    return _gen_runs(base, seed, "runff", 0xFF, (9, 0), count)


def gen_short(base, seed=0):
    """d_lens cut; the slot keeps every byte, so a decoder that reads past the length shows the clean picture"""
    n = len(base.payload)
    last = base.slices[-1].end - base.slices[-1].start
    return [_mut("short", f"length {n} -> {m}", base.payload, m) for m in (n - 1, n - 2, n - last, n // 2, 3, 0)]


def gen_long(base, seed=0):
    """d_lens beyond the payload; the slot is zero there"""
    n = len(base.payload)
    return [_mut("long", f"length {n} -> {n + d}", base.payload, n + d) for d in (1, 16, 300)]


LD_HDR_VALUES = (0x00, 0xFF, 0x7F, 0xF0)


def _ld_picked(ns):
    return sorted({0, 1 % ns, ns // 2, ns - 1})


def _gen_ld_hdr(base, cls, k):
    out = []
    for si in _ld_picked(base.ns):
        for v in LD_HDR_VALUES:
            pay = bytearray(base.payload)
            pay[base.slices[si].start + k] = v
            out.append(_mut(cls, f"slice {si} header byte {k} = {v:#04x}", pay))
    return out


def gen_hdr0(base, seed=0):
    return _gen_ld_hdr(base, "hdr0", 0)


def gen_hdr1(base, seed=0):
    return _gen_ld_hdr(base, "hdr1", 1)


def _gen_ld_body(base, cls, value):
    out = []
    for si in _ld_picked(base.ns):
        s = base.slices[si]
        pay = bytearray(base.payload)
        pay[s.start + 2:s.end] = bytes([value]) * (s.end - s.start - 2)
        out.append(_mut(cls, f"slice {si} body = {value:#04x}", pay))
    return out


def gen_body00(base, seed=0):
    return _gen_ld_body(base, "body00", 0x00)


def gen_bodyff(base, seed=0):
    return _gen_ld_body(base, "bodyff", 0xFF)


HQ_CLASSES = {"random": gen_random, "boundary": gen_boundary, "length": gen_length, "qindex": gen_qindex, "run00": gen_run00,
              "runff": gen_runff, "short": gen_short, "long": gen_long}
LD_CLASSES = {"random": gen_random, "hdr0": gen_hdr0, "hdr1": gen_hdr1, "body00": gen_body00, "bodyff": gen_bodyff}


def classes(base):
    return LD_CLASSES if base.case.mode == "LD" else HQ_CLASSES


def mutations(base, cls, seed):
    out = classes(base)[cls](base, seed)
    assert out and all(m.cls == cls for m in out)
    return out


def visible(base, m):
    """the bytes the decoder is given: slot[:length], the slot being the data and zeros behind it"""
    return (m.data + bytes(max(m.length - len(m.data), 0)))[:m.length]


def reference(oracle, base, m, k=0):
    """("ok", picture bytes) or ("refused", the oracle's error code); k > 0: the reduced picture (HQ)"""
    case = base.case
    try:
        if case.mode == "LD":
            assert k == 0
            out, n = oracle.decode_stream(case.params(), base.head + visible(base, m) + base.tail, 1)
            return ("ok", out) if n == 1 else ("refused", ESTREAM)
        data = visible(base, m)
        return "ok", (pr.reduced_picture(oracle, case, data, k) if k else pr.full_picture(oracle, case, data))
    except OracleError as e:
        return "refused", e.code


def cbr_claim_holds(oracle, base, m):
    """what k_cbr_index_check decides for one slot of an HQ_CBR picture, restated: the length is the sum of the budgets, and
    at every offset the budgets predict the three length bytes add up to that slice's budget"""
    case = base.case
    assert case.mode == "HQ_CBR"
    budgets = oracle.slice_bytes(case.ys, case.xs, case.s, case.scalar).ravel()
    data, pos = visible(base, m), 0
    if m.length != int(budgets.sum()) + base.ns * case.prefix:
        return False
    for b in budgets:
        at = pos + case.prefix + 1
        for _ in range(3):
            if at >= len(data):
                return False
            at += 1 + data[at] * case.scalar
        if at != pos + case.prefix + int(b):
            return False
        pos = at
    return True


def ld_shifted(oracle, base, m):
    """does some LD slice, read at its own offset, carry a luma length beyond the slice?  (the decoder's flag for the
    serial walk and the second pass, Slices.cpp:246-303)"""
    data = visible(base, m)
    for s in base.slices:
        size = s.end - s.start
        split = (8 * size - 7 - 1).bit_length()
        head = int.from_bytes(data[s.start:s.start + 4].ljust(4, b"\xff"), "big")
        ybits = (head << 7 & 0xFFFFFFFF) >> (32 - split) if split else 0
        if ybits > 8 * size - 7 - split:
            return True
    return False


def clean(base):
    return _mut("clean", "clean", base.payload)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs: one per decoder form (tests/test_gpu_damaged.py says which form each reaches and asserts it)
# ---------------------------------------------------------------------------------------------------------------------
def _input_a(o):
    c = pr.Case(o, 128, 64, "420", 8, "LeGall", 2, 2, 4, q=3, prefix=2, word_bytes=1)
    return Base(o, c, synth(128, 64, "420", 8, 403, word_bytes=1))


def _input_b1(o):
    c = pr.Case(o, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=8, scalar=1)
    return Base(o, c, synth(1024, 64, "422", 10, 401), chunk_mutations=True)


def _input_b2(o):
    c = pr.Case(o, 1024, 64, "422", 10, "DD97", 3, 1, 2, q=4, scalar=2)
    return Base(o, c, noise_frame(1024, 64, "422", 10, 402), chunk_mutations=True)


def _input_c(o):
    c = pr.Case(o, 1024, 128, "422", 10, "DD97", 3, 2, 4, q=8, scalar=8)
    return Base(o, c, synth(1024, 128, "422", 10, 404))


def _input_d(o):
    c = pr.Case(o, 2048, 256, "422", 10, "DD97", 4, 1, 2, q=8, scalar=8)
    return Base(o, c, synth(2048, 256, "422", 10, 405))


def _input_e(o):
    c = pr.Case(o, 1024, 64, "422", 10, "DD97", 3, 1, 2, mode="HQ_CBR", s=30000, scalar=1)
    return Base(o, c, synth(1024, 64, "422", 10, 406), chunk_mutations=True)


def _input_f1(o):
    c = pr.Case(o, 256, 32, "422", 10, "Haar1", 1, 2, 4, mode="LD", s=8000)
    return Base(o, c, synth(256, 32, "422", 10, 407))


def _input_f2(o):
    c = pr.Case(o, 512, 64, "422", 8, "LeGall", 3, 1, 2, mode="LD", s=12000, word_bytes=1)
    return Base(o, c, synth(512, 64, "422", 8, 408, word_bytes=1))


INPUTS = {"A": _input_a, "B1": _input_b1, "B2": _input_b2, "C": _input_c, "D": _input_d, "E": _input_e, "F1": _input_f1, "F2": _input_f2}
# geometry D: the oracle needs ~0.2 s per picture there, so three classes and at most 30 mutations (two slices per class)
D_CLASSES = ("boundary", "run00", "qindex")
SEED = 20


def input_classes(name):
    if name == "D":
        return D_CLASSES
    return tuple(LD_CLASSES) if name.startswith("F") else tuple(HQ_CLASSES)


def input_mutations(base, name, cls):
    """the mutations of one class on one input, as both test files use them"""
    if name == "D":
        ns = base.ns
        if cls == "boundary":
            return gen_boundary(base, slices=(0, ns - 1), deltas=(1, -1))     # 12
        if cls == "run00":
            return gen_run00(base, SEED, count=2)                             # 8
        return gen_qindex(base, slices=(ns // 3,))                            # 9
    return mutations(base, cls, SEED)


_CACHE = {}


def load(oracle, name):
    """the input and, per mutation, the full-size reference: computed once per session and shared"""
    if name not in _CACHE:
        _CACHE[name] = (INPUTS[name](oracle), {})
    return _CACHE[name]


def references(oracle, name, cls, k=0):
    """[(mutation, verdict, picture or code)] of one class; cached"""
    base, refs = load(oracle, name)
    key = (cls, k)
    if key not in refs:
        refs[key] = [(m,) + reference(oracle, base, m, k) for m in input_mutations(base, name, cls)]
    return refs[key]


def clean_picture(oracle, name, k=0):
    base, refs = load(oracle, name)
    key = ("clean", k)
    if key not in refs:
        verdict, pic = reference(oracle, base, clean(base), k)
        assert verdict == "ok"
        refs[key] = pic
    return refs[key]
