"""The CPU definition of vc2hip_stream_read_dev (include/vc2hip.h) and the designed streams that pin it.

  U, chain            a unit-chain builder: parse-info units from a list, next / prev offsets re-chained, every field open to an
                      explicit override (prefix bytes, parse code, next_parse_offset, prev, the body; the body builders take
                      the picture number, fragment data length, slice count, x and y offsets and the bytes)
  fragments           a fragmenter for an ARBITRARY cut (a list of slice counts summing to ns), not the greedy rule
  walk                the walk model: the header's contract and the unit rules of the reference's DataUnit.cpp / DecodeStream.cpp
                      in plain Python -- (lens, picture numbers, consumed, payloads, segments) or (reason text, byte offset)
  accepted, refused   seeded generators of accepted streams and the catalogue of refused ones; every case names its edge
  census              which gather forms (source phase, destination phase, segment length, segments per word, payload length
                      mod 16) a set of cases reaches, from the model's segment lists and the device offsets
  MUTATIONS           one-line wrong copies of the walk, each of which some designed stream must tell from the model

The model is written from the contract and the reference, not from the kernel.  Where those leave something open the kernel
was looked at and the choice is recorded in DESIGN.md as "implementation choice, pinned":
  * any unit that is not a fragment, between the fragments of a picture, is refused (the reference keeps its fragments in a map
    by picture number and takes padding, auxiliary data, sequence headers and even other pictures in between);
  * a slice fragment's payload is the fragment_data_length bytes it states (the reference parses the slices themselves);
  * a slice fragment's (x, y) is held against the running slice count as y * x_slices + x, so x >= x_slices may alias a later
    row (the reference and the oracle place the slices the same way);
  * where a unit breaks several rules at once, the order of the checks decides the reason."""
import random

import frag_ref
import qmatrix_ref

SEQ, EOS, AUX, PAD, HQ_PIC, LD_PIC, HQ_FRAG, LD_FRAG = 0x00, 0x10, 0x20, 0x30, 0xE8, 0xC8, 0xEC, 0xCC
KNOWN = (SEQ, EOS, AUX, PAD, HQ_PIC, LD_PIC, HQ_FRAG, LD_FRAG)
WINDOW = 128   # bytes of a unit the reader looks at (the contract: a longer head counts as running past the end)

R_PREFIX = "parse info prefix is not BBCD"
R_CODE = "unknown parse code"
R_PAST = "data unit runs past the end of the stream"
R_ZERO = "next_parse_offset is 0"
R_FEWER = "end of sequence before the pictures asked for"
R_PARAMS = "picture parameters differ from the coding parameters"
R_MATRIX = "quantisation matrix differs from the context's"
R_ASYM = "asymmetric transform"
R_VERSION = "picture before any sequence header and no major version given"
R_FRAGMENT = "fragment out of order"
R_ENTRY = "quantisation matrix entry above 255, the largest the library takes"
WALK_REASONS = (R_PREFIX, R_CODE, R_PAST, R_ZERO, R_FEWER, R_PARAMS, R_MATRIX, R_ASYM, R_VERSION, R_FRAGMENT, R_ENTRY)


# ---- the unit-chain builder ----------------------------------------------------------------------------------------------
class U:
    """one data unit; next / prev None: chained from the bodies' real lengths"""

    def __init__(self, code, body=b"", prefix=b"BBCD", next=None, prev=None):
        self.code, self.body, self.prefix, self.next, self.prev = code, bytes(body), bytes(prefix), next, prev

    def but(self, **kw):
        u = U(self.code, self.body, self.prefix, self.next, self.prev)
        for k, v in kw.items():
            setattr(u, k, bytes(v) if k in ("body", "prefix") else v)
        return u


def chain(units, prev=0):
    """(stream bytes, unit offsets): the units in order; an overridden next changes the field, not where the next unit lies"""
    out, offsets = bytearray(), []
    for u in units:
        real = 13 + len(u.body)
        nxt = u.next if u.next is not None else (0 if u.code == EOS else real)
        offsets.append(len(out))
        out += u.prefix + bytes([u.code]) + nxt.to_bytes(4, "big") + (u.prev if u.prev is not None else prev).to_bytes(4, "big") + u.body
        prev = real
    return bytes(out), offsets


def be(v, n):
    return (v & ((1 << 8 * n) - 1)).to_bytes(n, "big")


def sequence_header(major):
    return U(SEQ, qmatrix_ref.sequence_header_stub(major))


def picture(code, number, tp, payload):
    return U(code, be(number, 4) + tp + payload)


def params_fragment(code, number, tp, flen=None, count=0):
    return U(code, be(number, 4) + be(len(tp) if flen is None else flen, 2) + be(count, 2) + tp)


def slice_fragment(code, number, data, count, x, y, flen=None, slack=b""):
    return U(code, be(number, 4) + be(len(data) if flen is None else flen, 2) + be(count, 2) + be(x, 2) + be(y, 2) + data + slack)


def fragments(code, number, tp, payload, sizes, counts, xs, alias=(), slack=None):
    """the parameters fragment and one slice fragment per entry of counts (slice counts summing to len(sizes)).  alias: the
    indices of slice fragments written as (x + xs, y - 1), the same y * xs + x; slack: {fragment index: bytes behind its data}"""
    assert sum(counts) == len(sizes) and min(counts) > 0 and sum(sizes) == len(payload)
    out, first, at = [params_fragment(code, number, tp)], 0, 0
    for f, c in enumerate(counts):
        size = sum(sizes[first:first + c])
        x, y = first % xs, first // xs
        if f in alias:
            assert y > 0
            x, y = x + xs, y - 1
        out.append(slice_fragment(code, number, payload[at:at + size], c, x, y, slack=(slack or {}).get(f, b"")))
        first, at = first + c, at + size
    return out


def raw_bits(items):
    """("u", value) exp-Golomb fields, ("b", bit) bare bits and ("z", pairs) that many 0 0 bit pairs with no end, to bytes"""
    w = frag_ref.Bits()
    for kind, v in items:
        if kind == "u":
            w.uvlc(v)
        elif kind == "b":
            w.bit(v)
        else:
            for _ in range(2 * v):
                w.bit(0)
    return w.bytes()


# ---- the walk model --------------------------------------------------------------------------------------------------------
class Want:
    """what the caller says the pictures are: cp's fields as the stream states them, the context's effective matrix and the
    default matrix of cp's wavelet and depth (the effective matrix of a picture that carries none)"""

    def __init__(self, cp, default, matrix=None):
        self.ld = cp.mode == qmatrix_ref.LD
        self.kernel, self.depth, self.xs, self.ys = cp.kernel, cp.depth, cp.x_slices, cp.y_slices
        self.a, self.b = qmatrix_ref._ab(cp)
        self.default = [int(v) for v in default]
        self.matrix = self.default if matrix is None else [int(v) for v in matrix]


class _Reader:
    """MSB-first over bytes [pos, end): past the end it notes it and reads ones; a field of more than 32 zero-led pairs counts
    as running past the end too (no 32-bit value needs more)"""

    def __init__(self, data, pos, end):
        self.d, self.pos, self.end, self.nbit, self.over = data, pos, end, 0, False

    def bit(self):
        if self.pos >= self.end:
            self.over = True
            return 1
        b = self.d[self.pos] >> (7 - self.nbit) & 1
        self.nbit += 1
        if self.nbit == 8:
            self.nbit, self.pos = 0, self.pos + 1
        return b

    def uvlc(self):
        v, n = 1, 0
        while not self.bit():
            if n == 32:
                self.over = True
                break
            v = (v << 1) | self.bit()
            n += 1
        return v - 1

    def align(self):
        if self.nbit:
            self.nbit, self.pos = 0, self.pos + 1


def _check_params(r, want, major, ld, m):
    kernel, depth = r.uvlc(), r.uvlc()
    asym = False
    if major >= 3:
        if m == "asym_bare_bits":
            r.bit(), r.bit()
        else:
            if r.bit():
                asym |= r.uvlc() != kernel
            if r.bit():
                asym |= r.uvlc() != 0
    xs, ys, a, b = r.uvlc(), r.uvlc(), r.uvlc(), r.uvlc()
    custom = r.bit()
    if r.over:
        return R_PAST
    if asym:
        return R_ASYM
    if ld != want.ld or (kernel, depth, xs, ys) != (want.kernel, want.depth, want.xs, want.ys):
        return R_PARAMS
    if custom:
        entries = [r.uvlc() for _ in range(3 * depth + 1)]
        if r.over:
            return R_PAST
        if max(entries) > 255:
            return R_ENTRY
        if entries != want.matrix:
            return R_MATRIX
    elif want.matrix != want.default:
        return R_MATRIX
    r.align()
    if not ld or m == "ld_fieldwise":
        return None if (a, b) == (want.a, want.b) else R_PARAMS
    return None if b and a * want.b == b * want.a else R_PARAMS


class Result:
    """ok: n pictures were read.  lens has n entries (0 behind the pictures completed); numbers, payloads and segs one entry per
    picture completed; segs[k] = [(source offset in the stream, destination offset in the slot, bytes)].  consumed: the end of
    the n-th picture; after a refusal, at: the offset of the refused unit"""

    def __init__(self):
        self.ok, self.reason, self.at, self.lens, self.numbers, self.consumed, self.payloads, self.segs = True, None, None, [], [], 0, [], []

    def key(self):
        return (self.ok, self.reason, self.at, tuple(self.lens), tuple(self.numbers), self.consumed if self.ok else None,
                tuple(self.payloads))


def walk(stream, length, n, want, major=0, mutate=None):
    """the first n pictures of stream[:length]; major: the version given with the call (0: none)"""
    m = mutate
    s = bytes(stream[:length])
    ns = want.xs * want.ys
    res = Result()
    pos, why = 0, None
    is_open, fr_number, fr_slices, segs, dst = False, 0, 0, [], 0

    def complete(number):
        res.numbers.append(number)
        res.lens.append(dst)
        res.segs.append(list(segs))
        res.payloads.append(b"".join(s[a:a + l] for a, _, l in segs))

    while len(res.numbers) < n:
        if (pos + 13 >= length) if m == "head_ge" else (pos + 13 > length):
            why = R_PAST
            break
        if s[pos:pos + 4] != b"BBCD":
            why = R_PREFIX
            break
        code, nxt = s[pos + 4], int.from_bytes(s[pos + 5:pos + 9], "big")
        uend = pos + min(nxt, WINDOW)
        pic, frag = code in (HQ_PIC, LD_PIC), code in (HQ_FRAG, LD_FRAG)
        if code not in KNOWN:
            why = R_CODE
        elif code == EOS:
            why = R_FEWER
        elif nxt == 0:
            why = R_ZERO
        elif nxt < (12 if m == "next_lt_12" else 13) or ((pos + nxt >= length) if m == "end_ge" else (pos + nxt > length)):
            why = R_PAST
        elif is_open and not frag and not (m == "padding_between_fragments" and code == PAD):
            why = R_FRAGMENT
        elif (pic or frag) and major == 0:
            why = R_VERSION
        elif code == SEQ:
            r = _Reader(s, pos + 13, uend)
            v = r.uvlc()
            if r.over:
                why = R_PAST
            elif not (m == "sp_version_wins" and major):
                major = v
        elif pic:
            r = _Reader(s, pos + 17, uend)
            why = _check_params(r, want, major, code == LD_PIC, m)
            if not why:
                segs, dst = [(r.pos, 0, pos + nxt - r.pos)], pos + nxt - r.pos
                complete(int.from_bytes(s[pos + 13:pos + 17], "big"))
        elif frag:
            number = int.from_bytes(s[pos + 13:pos + 17], "big")
            flen = int.from_bytes(s[pos + 17:pos + 19], "big")
            count = int.from_bytes(s[pos + 19:pos + 21], "big")
            if nxt < 13 + (7 if m == "frag_header_20" else 8):
                why = R_PAST
            elif count == 0:
                if is_open:
                    why = R_FRAGMENT
                else:
                    why = _check_params(_Reader(s, pos + 21, uend), want, major, code == LD_FRAG, m)
                    is_open, fr_number, fr_slices, segs, dst = not why, number, 0, [], 0
            elif not is_open or (number != fr_number and m != "no_number"):
                why = R_FRAGMENT
            elif nxt < 13 + (11 if m == "slice_header_24" else 12) or 12 + flen > nxt - 13 + (1 if m == "flen_off_by_one" else 0):
                why = R_PAST
            else:
                x, y = int.from_bytes(s[pos + 21:pos + 23], "big"), int.from_bytes(s[pos + 23:pos + 25], "big")
                if (m != "no_xy" and y * want.xs + x != fr_slices) or count > (ns if m == "count_vs_ns" else ns - fr_slices):
                    why = R_FRAGMENT
                else:
                    segs.append((pos + 25, dst, flen))
                    dst += (nxt - 25) if m == "dst_by_body" else flen
                    fr_slices += count
                    if fr_slices >= ns:
                        is_open = False
                        complete(fr_number)
        if why:
            break
        pos += nxt
    res.consumed = pos
    if why:
        res.ok, res.reason, res.at = False, why, pos
    res.lens += [0] * (n - len(res.lens))
    return res


# Wrong copies of the walk, one line each.  tests/test_stream_ref.py shows that every one of MUTATIONS is told from the model
# by a designed stream, and that nothing tells UNCATCHABLE's from it.
MUTATIONS = ("head_ge", "end_ge", "next_lt_12", "count_vs_ns", "no_xy", "no_number", "flen_off_by_one", "sp_version_wins",
             "asym_bare_bits", "ld_fieldwise", "dst_by_body", "padding_between_fragments")
UNCATCHABLE = {"frag_header_20": "a fragment unit with next 20 is refused as running past the end either way: with slice count 0 "
                                 "its parameters start at byte 21, beyond the unit, and with a count it is shorter than the 25 "
                                 "bytes of a slice fragment's head",
               "slice_header_24": "a slice fragment with next 24 fails 12 + fragment_data_length <= next - 13 whatever length it "
                                  "states: that bound alone keeps next at 25 or more"}


# ---- the sources: coded pictures of the test geometries ---------------------------------------------------------------------
# the designed geometry: 96 x 64 4:2:0 8-bit, LeGall depth 2, slices of 16 x 16: xs = 6 (no power of two), ys = 4, ns = 24
MINI = dict(w=96, h=64, cf="420", bits=8, kernel="LeGall", depth=2, u=4, a=4, wb=1)
MINI_KW = {"mini4": dict(q=80, prefix=0, scalar=1),      # every coefficient 0: slices of 4 bytes
           "mini5": dict(q=80, prefix=1, scalar=1),      # ... of 5 bytes
           "mix": dict(q=14, prefix=0, scalar=1),        # slices of many sizes
           "ld1": dict(mode="LD", s=24)}                 # LD slices of 1 byte
# mix: (index, seed) of oracle pictures whose payload lengths are 15, 1 and 0 mod 16 (test_stream_ref asserts the residues),
# and one in which runs of slices have 17, 31 and 33 bytes
MIX_PICKS = ((34, 3), (34, 1), (34, 5), (30, 3))


class Source:
    """coded pictures of one geometry: payloads[k], sizes[k] (the bytes of every slice), cp, the oracle's params"""

    def __init__(self, name, c, cp, p, payloads, sizes, want):
        self.name, self.c, self.cp, self.p, self.payloads, self.sizes, self.want = name, c, cp, p, payloads, sizes, want
        self.xs, self.ns = cp.x_slices, cp.x_slices * cp.y_slices
        self.pic, self.frag = (LD_PIC, LD_FRAG) if cp.mode == qmatrix_ref.LD else (HQ_PIC, HQ_FRAG)

    def tp(self, major, **kw):
        return qmatrix_ref.transform_parameters(self.cp, major, **kw)

    def whole(self, k, major, number=None):
        return picture(self.pic, k if number is None else number, self.tp(major), self.payloads[k])

    def cut(self, k, counts, number=None, **kw):
        return fragments(self.frag, k if number is None else number, self.tp(3), self.payloads[k], self.sizes[k], counts, self.xs, **kw)

    def plain(self, pics, major=3):
        """the plain stream the designed ones derive from: a sequence header, whole pictures, the end of sequence"""
        return chain([sequence_header(major)] + [self.whole(k, major, i) for i, k in enumerate(pics)] + [U(EOS)])[0]


def units_of(stream):
    """[(code, body)] of a well-formed stream, the end of sequence included"""
    out, pos = [], 0
    while True:
        code, nxt = stream[pos + 4], int.from_bytes(stream[pos + 5:pos + 9], "big")
        if code == EOS:
            out.append((code, b""))
            return out
        out.append((code, stream[pos + 13:pos + nxt]))
        pos += nxt


def major_of(stream):
    r = _Reader(stream, 13, len(stream))
    return r.uvlc()


def oracle_stream(oracle, c, n, seed, **over):
    """(cp, oracle params, stream) of n synthetic pictures of case c (the dictionaries of test_gpu_stream_dev.CASES)"""
    import vc2hip_py
    from synth import synth
    from vc2lib import make_params
    kw = dict(c["kw"], **over)
    wb = c.get("wb", 2)
    fmt = vc2hip_py.picture_format(c["w"], c["h"], c["cf"], c["bits"], wb)
    ckw = dict(kw)
    ckw.pop("fragment_length", None)
    cp = vc2hip_py.coding_params(vc2hip_py.load_library(), fmt, c["kernel"], c["depth"], c["u"], c["a"], **ckw)
    p = make_params(c["w"], c["h"], c["cf"], c["bits"], c["kernel"], c["depth"], c["u"], c["a"], word_bytes=wb, **kw)
    raw = synth(c["w"], c["h"], c["cf"], c["bits"], seed, frames=n, word_bytes=wb)
    return cp, p, oracle.encode_stream(p, raw, n)


def want_of(oracle, cp):
    return Want(cp, oracle.quant_matrix(cp.kernel, cp.depth))


def slice_sizes(oracle, cp, payload):
    if cp.mode == qmatrix_ref.LD:
        return [int(v) for v in oracle.slice_bytes(cp.y_slices, cp.x_slices, cp.compressed_bytes, 1).ravel()]
    return frag_ref.slice_sizes_hq(payload, cp.y_slices * cp.x_slices, cp.prefix, cp.scalar)


def oracle_payloads(cp, stream, n):
    major = major_of(stream)
    hl = len(qmatrix_ref.picture_header(cp, major, 0))
    pics = [b[hl:] for code, b in units_of(stream) if code in (HQ_PIC, LD_PIC)]
    assert len(pics) == n
    return pics


_SOURCES = {}


def sources(oracle):
    """the four sources of the designed geometry, coded once.  The all-zero pictures are made tellable: every slice of mini4 and
    mini5 gets an index byte of its own (60 ... 99: a zero coefficient dequantises to zero at any index) and mini5's prefix
    byte, which no decoder reads, the slice's number; ld1's one-byte slices (seven bits of index, one length bit, no
    coefficient) get indices 20 ... 59 -- a segment put in the wrong place then shows"""
    if _SOURCES:
        return _SOURCES
    for name, kw in MINI_KW.items():
        c = dict(MINI, kw=kw)
        if name == "mix":
            pays = []
            for q, seed in MIX_PICKS:
                cp, p, stream = oracle_stream(oracle, c, 1, seed, q=q)
                pays += oracle_payloads(cp, stream, 1)
        else:
            cp, p, stream = oracle_stream(oracle, c, 3, 11)
            pays = oracle_payloads(cp, stream, 3)
        sizes = [slice_sizes(oracle, cp, pay) for pay in pays]
        if name in ("mini4", "mini5"):
            step = 4 + cp.prefix
            assert all(s == [step] * len(s) for s in sizes)
            for k, pay in enumerate(pays):
                b = bytearray(pay)
                for i in range(len(pay) // step):
                    b[i * step + cp.prefix] = 60 + (7 * i + 13 * k) % 40
                    if cp.prefix:
                        b[i * step] = 0x80 + 32 * k + i
                pays[k] = bytes(b)
        if name == "ld1":
            assert all(s == [1] * len(s) for s in sizes)
            pays = [bytes(((20 + (7 * i + 13 * k) % 40) << 1) | (v & 1) for i, v in enumerate(pay)) for k, pay in enumerate(pays)]
        _SOURCES[name] = Source(name, c, cp, p, pays, sizes, want_of(oracle, cp))
    return _SOURCES


# ---- the cases -------------------------------------------------------------------------------------------------------------
class Case:
    """one call: stream[start:length] read for n pictures with `major` given.
    edge: what the case is there for; expect: None (accepted) or the reason text the catalogue means it to be refused with;
    pics: the source pictures an accepted stream carries, in order (None: its payloads are not pictures);
    oracle_no: why the oracle cannot parse the designed stream (None: it can); offs: device offsets from a 16-byte boundary;
    stride: the slot stride to use (None: the geometry's)"""

    def __init__(self, name, edge, src, stream, n, major=0, expect=None, pics=None, length=None, start=0, oracle_no=None,
                 offs=(0,), stride=None):
        self.name, self.edge, self.src, self.n, self.major, self.expect, self.pics = name, edge, src, n, major, expect, pics
        self.stream = bytes(stream)
        self.length = len(self.stream) if length is None else length
        self.start, self.oracle_no, self.offs, self.stride = start, oracle_no, offs, stride

    def bytes(self):
        return self.stream[self.start:]

    def model(self, mutate=None):
        return walk(self.bytes(), self.length - self.start, self.n, self.src.want, self.major, mutate)


def _random_cut(rng, ns):
    counts, left = [], ns
    while left:
        c = min(left, rng.choice((1, 1, 2, 3, 4, 5, 7, 9)))
        counts.append(c)
        left -= c
    return counts


def _cut_with(sizes, target):
    """a cut one of whose fragments has `target` bytes, or None"""
    pre = [0]
    for s in sizes:
        pre.append(pre[-1] + s)
    for i in range(len(sizes)):
        for j in range(i + 1, len(sizes) + 1):
            if pre[j] - pre[i] == target:
                return ([i] if i else []) + [j - i] + ([len(sizes) - j] if j < len(sizes) else [])
    return None


ALL_OFFS = (0, 1, 7, 15)
SEGMENT_LENGTHS = (1, 15, 16, 17, 31, 32, 33)


def accepted(S):
    """the designed accepted streams; S: sources(oracle)"""
    out = []

    def add(name, edge, src, units, pics, n=None, **kw):
        out.append(Case(name, edge, src, chain(units)[0], len(pics) if n is None else n, pics=pics, **kw))

    seq3, eos = sequence_header(3), U(EOS)
    rng = random.Random(2042)
    # cuts
    for src in S.values():
        ns, xs = src.ns, src.xs
        cuts = {"ones": ([1] * ns, "ns fragments of one slice: a 16-byte word from several segments"),
                "all": ([ns], "one fragment of ns slices"),
                "midrow": ([4, 5, 7, 3, ns - 19], "fragments that end mid-row: x offsets 4, 3, 4, 1, wrapping rows"),
                "random_a": (_random_cut(rng, ns), "a random cut"), "random_b": (_random_cut(rng, ns), "a random cut")}
        for cname, (counts, edge) in cuts.items():
            other = _random_cut(rng, ns)
            add("%s_cut_%s" % (src.name, cname), edge, src,
                [seq3] + src.cut(0, counts) + src.cut(1, other) + src.cut(2, counts[::-1]) + [eos], [0, 1, 2], offs=ALL_OFFS)
        add("%s_alias" % src.name, "x >= xs with y * xs + x the running count (x = 2 + xs, y = 0 for slice 8)", src,
            [seq3] + src.cut(0, [xs + 2, 3, ns - xs - 5], alias=(1, 2)) + [eos], [0])
    # segment lengths
    for target in SEGMENT_LENGTHS:
        found = 0
        for src in S.values():
            for k in range(len(src.payloads)):
                counts = _cut_with(src.sizes[k], target)
                if counts and found < 2:
                    found += 1
                    add("%s_seglen_%d_%d" % (src.name, target, k), "a segment of %d bytes" % target, src,
                        [seq3] + src.cut(k, counts) + [eos], [k], offs=ALL_OFFS)
        assert found, target
    # whole pictures at every base offset (the payload-length classes: mix's pictures are 15, 1 and 0 mod 16 long)
    for src in S.values():
        for major in (2, 3):
            add("%s_whole_v%d" % (src.name, major), "a sequence header at major %d before whole pictures" % major, src,
                [sequence_header(major)] + [src.whole(k, major) for k in range(3)] + [eos], [0, 1, 2], offs=ALL_OFFS)
    # units that are skipped
    src = S["mini5"]
    w = [src.whole(k, 3) for k in range(3)]
    add("skip_padding", "padding of body 0, 1 and 115 (115: the unit fills the walk's window exactly)", src,
        [seq3, U(PAD), w[0], U(PAD, b"\x42"), w[1], U(PAD, bytes(range(115))), U(PAD), w[2], eos], [0, 1, 2])
    add("skip_auxiliary", "auxiliary units, one that looks like a parse info", src,
        [seq3, U(AUX, b"BBCD\xe8" + bytes(8)), w[0], U(AUX, b"a" * 300), w[1], U(AUX), w[2], eos], [0, 1, 2])
    add("skip_repeated_headers", "repeated sequence headers", src, [seq3, w[0], seq3, seq3, w[1], seq3, w[2], eos], [0, 1, 2])
    add("version_of_the_stream_wins", "a sequence header whose major version differs from the one given: the stream's wins",
        src, [seq3] + w + [eos], [0, 1, 2], major=2, oracle_no=None)
    add("version_changes_mid_stream", "sequence headers at major 2 and 3 in one stream, each before its pictures", src,
        [sequence_header(2), src.whole(0, 2), seq3, w[1], sequence_header(2), src.whole(2, 2), eos], [0, 1, 2])
    # unit slack
    for src in (S["mini5"], S["mix"]):
        add("%s_slack" % src.name, "slice fragments whose unit is longer than 12 + fragment_data_length: the stated bytes are the payload",
            src, [seq3] + src.cut(0, [5, 7, src.ns - 12], slack={0: b"\xee", 1: b"\xee" * 17, 2: b"\xee" * 40}) + [src.whole(1, 3), eos], [0, 1])
    # parameters written differently but equal
    src = S["ld1"]
    cp = src.cp
    a, b = src.want.a, src.want.b
    for mul in (2, 7):
        tp = raw_bits([("u", cp.kernel), ("u", cp.depth), ("b", 0), ("b", 0), ("u", cp.x_slices), ("u", cp.y_slices),
                       ("u", a * mul), ("u", b * mul), ("b", 0)])
        add("ld_fraction_times_%d" % mul, "an LD fraction not in lowest terms (%d / %d)" % (a * mul, b * mul), src,
            [seq3, picture(LD_PIC, 0, tp, src.payloads[0])] + fragments(LD_FRAG, 1, tp, src.payloads[1], src.sizes[1], [10, 14], src.xs) + [eos], [0, 1])
    for src in (S["mini5"], S["ld1"]):
        cp = src.cp
        tp = raw_bits([("u", cp.kernel), ("u", cp.depth), ("b", 1), ("u", cp.kernel), ("b", 1), ("u", 0), ("u", cp.x_slices),
                       ("u", cp.y_slices), ("u", src.want.a), ("u", src.want.b), ("b", 0)])
        add("%s_identity_asym" % src.name, "major 3, both asymmetric flags set with wavelet_index_ho == wavelet_index, dwt_depth_ho == 0",
            src, [seq3, picture(src.pic, 0, tp, src.payloads[0])] + fragments(src.frag, 1, tp, src.payloads[1], src.sizes[1], [9, 15], src.xs) + [eos],
            [0, 1], oracle_no="the oracle reads the two flags as bare bits and takes the values behind them for the slice counts")
    # resumption: whole and fragmented pictures mixed, every split, the second call at consumed with the version given
    src = S["mix"]
    units = ([seq3, src.whole(0, 3), U(PAD, b"pad")] + src.cut(1, _random_cut(rng, src.ns), number=1) + [src.whole(2, 3, 2), seq3] +
             src.cut(0, [src.ns], number=3) + [eos])
    pics = [0, 1, 2, 0]
    stream = chain(units)[0]
    for k in range(1, len(pics) + 1):
        first = Case("resume_first_%d" % k, "n = %d of 4 pictures" % k, src, stream, k, pics=pics[:k])
        out.append(first)
        if k < len(pics):
            out.append(Case("resume_rest_%d" % k, "the second call at d_stream + consumed for the other %d" % (len(pics) - k), src,
                            stream, len(pics) - k, major=3, pics=pics[k:], start=first.model().consumed, offs=(0, 7),
                            oracle_no="the rest of a stream has no sequence header: the oracle assumes major version 2"))
    # picture numbers
    src = S["mini4"]
    nums = [0xFFFFFFFE, 0xFFFFFFFF, 0]
    add("numbers_wrap", "picture numbers 0xFFFFFFFE, 0xFFFFFFFF, 0 through whole and fragmented pictures", src,
        [seq3] + src.cut(0, [7, 17], number=nums[0]) + src.cut(1, [1, 23], number=nums[1]) + [src.whole(2, 3, nums[2])] + [eos], [0, 1, 2])
    add("numbers_wrap_fragmented", "0xFFFFFFFF on every fragment of a picture, then 0 on the next one's", src,
        [seq3] + src.cut(0, [6, 6, 12], number=nums[1]) + src.cut(1, [12, 12], number=nums[2]) + [eos], [0, 1])
    # no version needed when it is given
    src = S["mini5"]
    add("whole_with_version_given", "a whole picture before any sequence header, major version 3 given", src, [src.whole(0, 3), eos], [0],
        major=3, oracle_no="no sequence header: the oracle assumes major version 2")
    add("fragment_with_version_given", "a parameters fragment before any sequence header, major version 3 given", src,
        src.cut(0, [11, 13]) + [eos], [0], major=3, oracle_no="no sequence header: the oracle assumes major version 2")
    # the accepted sides of the catalogue's boundaries
    w = [src.whole(k, 3) for k in range(3)]
    stream, offs = chain([seq3] + w + [eos])
    out.append(Case("ends_exactly_at_len", "pos + next == len: the stream ends with the n-th picture", src, stream, 3, pics=[0, 1, 2],
                    length=offs[4]))
    f = src.cut(0, [1, src.ns - 1])
    f[1] = slice_fragment(src.frag, 0, b"", 1, 0, 0)
    f[2] = slice_fragment(src.frag, 0, src.payloads[0], src.ns - 1, 1, 0)
    add("slice_fragment_of_25_bytes", "a slice fragment with next 25: no data, the next fragment carries its slice too", src,
        [seq3] + f + [eos], [0], oracle_no="the oracle parses the slices of every fragment and finds none in the first")
    add("empty_payload", "next ends the unit right behind its transform parameters: a picture of 0 bytes", src,
        [seq3, picture(src.pic, 0, src.tp(3), b""), w[1], eos], None, n=2)
    f = src.cut(1, [9, 15])
    add("count_exactly_remaining", "a last fragment of exactly the slices that remain", src, [seq3] + f + [eos], [1])
    return out


def refused(S):
    """the catalogue: every stream is a valid one with exactly one rule broken; expect is the reason it is meant to give"""
    out = []
    src = S["mini5"]
    seq3, eos = sequence_header(3), U(EOS)
    w = [src.whole(k, 3) for k in range(3)]
    W = [seq3] + w + [eos]                                                 # units 1 .. 3 are the pictures
    F = [seq3, w[0]] + src.cut(1, [4, 5, 7, 8]) + src.cut(2, [12, 12]) + [eos]    # units 2 .. 6: picture 1, 7 .. 9: picture 2

    def add(name, edge, expect, units, n, src_=None, **kw):
        out.append(Case(name, edge, src_ or src, chain(units)[0], n, expect=expect, **kw))

    def swap(units, i, u):
        return units[:i] + [u] + units[i + 1:]

    # prefix
    for i in range(4):
        for at in (0, 2):
            bad = bytearray(b"BBCD")
            bad[i] ^= 0x01 << i
            add("prefix_byte%d_unit%d" % (i, at), "prefix byte %d wrong on unit %d" % (i, at), R_PREFIX, swap(W, at, W[at].but(prefix=bad)), 3)
    # parse codes: all 256 in place of the second picture's; the model classifies them
    for code in range(256):
        if code == HQ_PIC:
            continue   # (the stream as it was)
        expect = {SEQ: R_FEWER, EOS: R_FEWER, AUX: R_FEWER, PAD: R_FEWER, LD_PIC: R_PARAMS, HQ_FRAG: R_FRAGMENT, LD_FRAG: R_FRAGMENT}.get(code, R_CODE)
        add("code_%02x" % code, "parse code 0x%02X on the second picture" % code, expect, swap(W, 2, W[2].but(code=code)), 3)
    add("eos_early", "the end of sequence after one picture", R_FEWER, [seq3, w[0], eos, w[1], w[2], eos], 3)
    # past the end
    units = [seq3, w[0], U(PAD), w[1], eos]
    stream, offs = chain(units)
    out.append(Case("len_leaves_12", "len leaves 12 bytes for a unit", src, stream, 2, expect=R_PAST, length=offs[2] + 12))
    out.append(Case("len_leaves_13", "len leaves 13: the padding unit is read, the stream ends behind it", src, stream, 2, expect=R_PAST,
                    length=offs[2] + 13))
    for nxt in range(1, 13):
        add("next_%d" % nxt, "next_parse_offset %d on a padding unit" % nxt, R_PAST, swap(units, 2, U(PAD, next=nxt)), 2)
    stream, offs = chain(W)
    out.append(Case("len_one_short", "pos + next == len + 1", src, stream, 3, expect=R_PAST, length=offs[4] - 1))
    out.append(Case("no_end_no_pictures", "the stream ends at len with neither an end of sequence nor n pictures", src, stream, 4,
                    expect=R_PAST, length=offs[4]))
    hl = 13 + 4 + len(src.tp(3))
    add("next_inside_parameters", "next cuts the unit inside its transform parameters", R_PAST, swap(W, 2, W[2].but(next=hl - 2)), 3)
    cp = src.cp
    for pairs, expect in ((33, R_PAST), (32, R_PARAMS)):
        tp = raw_bits([("z", pairs), ("b", 1), ("u", cp.depth), ("b", 0), ("b", 0), ("u", cp.x_slices), ("u", cp.y_slices),
                       ("u", cp.prefix), ("u", cp.scalar), ("b", 0)])
        add("field_of_%d_zero_pairs" % pairs, "a parameters field led by %d zero bits" % pairs, expect,
            swap(W, 2, picture(src.pic, 1, tp, src.payloads[1])), 3)
    add("fragment_next_20", "a parameters fragment with next 20", R_PAST, swap(F, 2, F[2].but(next=20)), 3)
    add("fragment_next_21", "a parameters fragment with next 21: no room for the parameters", R_PAST, swap(F, 2, F[2].but(next=21)), 3)
    add("slice_fragment_next_24", "a slice fragment with next 24", R_PAST, swap(F, 4, F[4].but(next=24)), 3)
    add("slice_fragment_next_24_no_data", "a slice fragment with next 24 that states no data", R_PAST,
        swap(F, 4, slice_fragment(src.frag, 1, b"", 5, 4, 0).but(next=24)), 3)
    f = F[4]
    flen = int.from_bytes(f.body[4:6], "big")
    add("flen_one_above", "12 + fragment_data_length one above next - 13", R_PAST, swap(F, 4, f.but(body=f.body[:4] + be(flen + 1, 2) + f.body[6:])), 3)
    # next = 0
    for code in (SEQ, AUX, PAD, HQ_PIC, LD_PIC, HQ_FRAG, LD_FRAG):
        add("next_zero_%02x" % code, "next_parse_offset 0 on code 0x%02X" % code, R_ZERO, swap(W, 2, W[2].but(code=code, next=0)), 3)
    # no version
    add("whole_no_version", "a whole picture before any sequence header, no version given", R_VERSION, [w[0], eos], 1)
    add("fragment_no_version", "a parameters fragment before any sequence header, no version given", R_VERSION, src.cut(0, [11, 13]) + [eos], 1)
    # parameters
    import vc2hip_py

    def cp_but(s, **kw):
        v = {k: getattr(s.cp, k) for k, _ in vc2hip_py.CodingParams._fields_}
        v.update(kw)
        return vc2hip_py.CodingParams(*[v[k] for k, _ in vc2hip_py.CodingParams._fields_])

    ld = S["ld1"]
    for s, fields in ((src, ("kernel", "depth", "x_slices", "y_slices", "prefix", "scalar")), (ld, ("kernel", "depth", "x_slices", "y_slices"))):
        for field in fields:
            for d in (1, -1):
                if getattr(s.cp, field) + d < 0:
                    continue
                tp = qmatrix_ref.transform_parameters(cp_but(s, **{field: getattr(s.cp, field) + d}), 3)
                add("%s_%s_%+d" % (s.name, field, d), "%s off by %+d" % (field, d), R_PARAMS,
                    [seq3, s.whole(0, 3), picture(s.pic, 1, tp, s.payloads[1]), eos], 2, src_=s)
    tp = qmatrix_ref.transform_parameters(cp_but(src, x_slices=src.cp.x_slices + 1), 3)
    add("fragment_x_slices", "x_slices off by one in a parameters fragment", R_PARAMS, swap(F, 2, params_fragment(src.frag, 1, tp)), 3)
    add("other_profile_fragment", "fragments of the other profile", R_PARAMS, swap(F, 2, F[2].but(code=LD_FRAG)), 3)
    cpl = ld.cp
    for name, a, b in (("unequal", ld.want.a + 1, ld.want.b), ("unequal_b", ld.want.a, ld.want.b + 1), ("zero_denominator", ld.want.a, 0),
                       ("zero_over_zero", 0, 0)):
        tp = raw_bits([("u", cpl.kernel), ("u", cpl.depth), ("b", 0), ("b", 0), ("u", cpl.x_slices), ("u", cpl.y_slices), ("u", a), ("u", b), ("b", 0)])
        add("ld_fraction_%s" % name, "an LD fraction of %d / %d" % (a, b), R_PARAMS, [seq3, ld.whole(0, 3), picture(LD_PIC, 1, tp, ld.payloads[1]), eos], 2, src_=ld)
    for field in ("x_slices", "scalar"):
        items = [("u", cp.kernel), ("u", cp.depth), ("b", 0), ("b", 0), ("u", cp.x_slices), ("u", cp.y_slices), ("u", cp.prefix), ("u", cp.scalar), ("b", 0)]
        i = 4 if field == "x_slices" else 7
        items[i] = ("u", items[i][1] + (1 << 32))
        add("%s_plus_2_32" % field, "%s written as its value + 2^32: equal only in 32-bit arithmetic" % field, R_PARAMS,
            swap(W, 2, picture(src.pic, 1, raw_bits(items), src.payloads[1])), 3)
    # asymmetric
    for asym in ((1, 0), (0, 1)):
        add("asym_%d%d" % asym, "asymmetric flag %s set with a differing value" % ("wavelet_index_ho", "dwt_depth_ho")[asym[1]], R_ASYM,
            swap(W, 2, picture(src.pic, 1, src.tp(3, asym=asym), src.payloads[1])), 3)
        add("asym_%d%d_fragment" % asym, "the same in a parameters fragment", R_ASYM, swap(F, 2, params_fragment(src.frag, 1, src.tp(3, asym=asym))), 3)
    # matrix, inside a parameters fragment
    tp = bytearray(src.tp(3))
    r = _Reader(bytes(tp), 0, len(tp))
    for _ in range(2):
        r.uvlc()
    r.bit(), r.bit()
    for _ in range(4):
        r.uvlc()
    tp[r.pos] |= 0x80 >> r.nbit
    add("matrix_flag_bare", "custom_quant_matrix set in a parameters fragment, no entries behind it", R_PAST, swap(F, 2, params_fragment(src.frag, 1, bytes(tp))), 3)
    other = [v + 1 for v in src.want.default]
    add("matrix_differs", "a parameters fragment with a matrix that is not the context's", R_MATRIX,
        swap(F, 2, params_fragment(src.frag, 1, src.tp(3, qm=other))), 3)
    add("matrix_entry_256", "a parameters fragment with a matrix entry of 256", R_ENTRY,
        swap(F, 2, params_fragment(src.frag, 1, src.tp(3, qm=[256] + other[1:]))), 3)
    # fragment order
    add("no_parameters_fragment", "a slice fragment with no parameters fragment before it", R_FRAGMENT, F[:2] + F[3:], 3)
    f = F[4]
    add("number_differs", "a picture number that differs within the chain", R_FRAGMENT, swap(F, 4, f.but(body=be(2, 4) + f.body[4:])), 3)
    add("second_parameters_fragment", "a second parameters fragment while a picture is open", R_FRAGMENT, F[:4] + [F[2]] + F[4:], 3)
    for name, u in (("whole_picture", w[2]), ("padding", U(PAD, b"p")), ("auxiliary", U(AUX, b"a")), ("sequence_header", seq3)):
        add("%s_between_fragments" % name, "a %s between the fragments of a picture" % name.replace("_", " "), R_FRAGMENT, F[:4] + [u] + F[4:], 3)
    add("skipped_slices", "a fragment left out", R_FRAGMENT, F[:4] + F[5:], 3)
    add("repeated_slices", "a fragment twice", R_FRAGMENT, F[:5] + [F[4]] + F[5:], 3)
    add("rows_in_the_wrong_order", "two fragments exchanged", R_FRAGMENT, F[:4] + [F[5], F[4]] + F[6:], 3)
    f = F[6]
    count = int.from_bytes(f.body[6:8], "big")
    add("count_remaining_plus_1", "a slice count of the slices that remain + 1", R_FRAGMENT, swap(F, 6, f.but(body=f.body[:6] + be(count + 1, 2) + f.body[8:])), 3)
    return out


def capacity(S):
    """(exact, longer): with a stride of picture 0's bytes, pictures of exactly the stride, and one of stride + 1 between them"""
    src = S["mini4"]
    stride = len(src.payloads[0])
    assert stride % 16 == 0
    seq3, eos = sequence_header(3), U(EOS)
    exact = Case("capacity_exact", "pictures of exactly stride bytes", src, chain([seq3, src.whole(0, 3), src.whole(1, 3), src.whole(2, 3), eos])[0],
                 3, pics=[0, 1, 2], stride=stride)
    long1 = picture(src.pic, 1, src.tp(3), src.payloads[1] + b"\x77")
    longer = Case("capacity_plus_1", "a picture of stride + 1 bytes between two of stride bytes", src,
                  chain([seq3, src.whole(0, 3), long1, src.whole(2, 3), eos])[0], 3, stride=stride)
    f = src.cut(1, [10, 14])
    f[2] = slice_fragment(src.frag, 1, f[2].body[12:] + b"\x77", 14, 10 % src.xs, 10 // src.xs)
    longer_f = Case("capacity_plus_1_fragmented", "a fragmented picture of stride + 1 bytes", src,
                    chain([seq3, src.whole(0, 3)] + f + [src.whole(2, 3), eos])[0], 3, stride=stride)
    return exact, longer, longer_f


# ---- the census ----------------------------------------------------------------------------------------------------------------
def census(cases):
    """what the gather meets on the accepted cases, from the model's segments and the device offsets: the classes of
    (segment source address mod 16), of (segment destination mod 16), the segment lengths, the source phases of 16-byte slot
    words taken whole from one segment (0: no realignment), the most segments one slot word is assembled from, and the
    payload lengths mod 16"""
    src_phase, dst_phase, seg_len, word_phase, plen, most = set(), set(), set(), set(), set(), 0
    for c in cases:
        if c.expect is not None:
            continue
        res = c.model()
        for off in c.offs:
            for segs, total in zip(res.segs, res.lens):
                plen.add(total % 16)
                for a, d, l in segs:
                    if l:
                        src_phase.add((off + a) % 16)
                        dst_phase.add(d % 16)
                    seg_len.add(l)
                for x0 in range(0, total, 16):
                    inside = [(a, d, l) for a, d, l in segs if d <= x0 and x0 + 16 <= d + l]
                    if inside:
                        a, d, _ = inside[0]
                        word_phase.add((off + a + x0 - d) % 16)
                    else:
                        most = max(most, sum(1 for a, d, l in segs if l and d < x0 + 16 and d + l > x0))
    return dict(src_phase=src_phase, dst_phase=dst_phase, seg_len=seg_len, word_phase=word_phase, payload_mod16=plen, segments_per_word=most)
