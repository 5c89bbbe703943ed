"""The three HQ slice readers restated on the CPU, and designed coefficient codes for them (pure CPU: no GPU import).

Three kernels read the exp-Golomb codes of an HQ slice component, each with a bit reader and token logic of its own:
  - decode_round over WordReader (k_hq_unpack<32>, csrc/vc2hip_slices.hip): a 64-bit window, a run of '1' bits (zero
    coefficients) and one code per turn, a second token from the same window where it lies wholly inside it;
  - the turn of k_hq_unpack16 over Reader32 (same file): up to four look-ups of the next 10 bits in a table of "what these
    bits decode to", one long code by arithmetic, codes beyond 32 bits bit by bit; rows of 32 + 8 with a spill;
  - tc_turn / tc_long over TcReader (k_transcode_measure, csrc/vc2hip_transcode.hip): the same table, three look-ups, or a
    run of up to 32 and one code by arithmetic.
component() and payload() build payloads from designed VALUES (codes of any length, cuts, slack); the generators design
them to stand on the readers' edges; model_unpack16 / model_round / model_tc transcribe the token logic over a bit string
with endless ones behind it; trace() says what an input reaches, and by arithmetic alone which fetch form each reader
meets at the end of every component.

MUTANTS names one-line wrong copies of the models; tests/test_reader_ref.py shows that every one of them is caught by a
designed input.  They stand in for wrong kernels, which are never built."""
from collections import Counter, namedtuple

import numpy as np

SEED = 23
LUT_BITS = 10
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------
# codes, components, payloads
# ---------------------------------------------------------------------------------------------------------------------
def code(v):
    """'1' for 0, (0 b)^K 1 s otherwise; any magnitude (a code of more than 32 bits is outside the encoder's domain)"""
    if v == 0:
        return "1"
    return "".join("0" + b for b in bin(abs(v) + 1)[3:]) + "1" + ("1" if v < 0 else "0")


def as_read(v):
    """the value every reader makes of code(v): the magnitude wraps in 32 bits as the oracle's does (VLC.cpp:283-317)"""
    mag = abs(v) & M32
    assert mag, "a magnitude that wraps to 0 has no sign bit on the reader's side"
    r = (-mag if v < 0 else mag) & M32
    return r - (1 << 32) if r >> 31 else r


def plain(bits, n):
    """n coefficients from a bit string with endless ones behind it: the definition (VLC.cpp:182-185, 283-317)"""
    out, p, L = [], 0, len(bits)

    def bit():
        nonlocal p
        b = bits[p] == "1" if p < L else True
        p += 1
        return b

    for _ in range(n):
        value = 1
        while not bit():
            value = ((value << 1) | bit()) & M32
        mag = (value - 1) & M32
        if mag and bit():
            mag = (-mag) & M32
        out.append(mag - (1 << 32) if mag >> 31 else mag)
    return out


# data bits (8 * units * scalar of them), the n designed values, cut or whole, the positions of the values designed on purpose
# (empty: a filler), what the component is there for
Comp = namedtuple("Comp", "bits units want cut named note", defaults=((), ""))


def component(values, n, cut_bits=None, pad="0", scalar=1, units=None, raw="", named=None, note=""):
    """the codes of `values` (then the bit string `raw`, for slack that looks like codes), cut after cut_bits if given,
    padded with the bit pattern `pad` to whole length units -- as many as the bits need, or `units` (more: slack; fewer: a
    cut at that length).  The designed values are what the definition reads of the data: the values themselves, zeros
    behind them, where nothing is cut.  named: the positions designed on purpose (a list, "nonzero": every non-zero value, "last":
    the last non-zero value, or position 0 where there is none, "largest": the value of the largest magnitude, which no
    neighbour hides under the clip)."""
    values = list(values)
    bits = "".join(code(v) for v in values)
    if not raw:
        bits += "1" * max(n - len(values), 0)            # the zero coefficients behind the last value
        if cut_bits is None and units is None:           # as the encoder writes it: whole units through the last non-zero value
            last = max((k for k, v in enumerate(values) if v), default=-1)
            through = sum(len(code(v)) for v in values[:last + 1])
            bits = bits[:8 * scalar * -(-through // (8 * scalar))]
    bits += raw
    if cut_bits is not None:
        bits = bits[:cut_bits]
    if units is None:
        units = -(-len(bits) // (8 * scalar))
    assert 0 <= units <= 255, f"a component of {units} length units"
    total = 8 * scalar * units
    bits = bits[:total] + (pad * (total - len(bits)))[:max(total - len(bits), 0)]
    want = plain(bits, n)
    designed = ([as_read(v) if v else 0 for v in values] + [0] * n)[:n]
    if named == "nonzero":
        named = [k for k in range(n) if want[k]]
    elif named == "last":
        named = [k for k in range(n) if want[k]][-1:] or [0]
    elif named == "largest":
        named = [max(range(n), key=lambda k: (abs(want[k]), k))]
    return Comp(bits, units, want, False if raw else want != designed, tuple(k for k in (named or ()) if k < n), note)


def payload(slices, prefix, scalar, seed=SEED):
    """slices: [(index byte, [Comp, Comp, Comp])] -> (payload bytes, byte offset of every component's data).  Prefix bytes
    are seeded, never zero."""
    rng = np.random.default_rng(seed)
    out, starts = bytearray(), []
    for q, comps in slices:
        out += bytes((rng.integers(0, 256, prefix, dtype=np.uint8) | np.uint8(0x18)).tolist())
        out.append(q)
        for c in comps:
            assert len(c.bits) == 8 * scalar * c.units
            out.append(c.units)
            starts.append(len(out))
            if c.bits:
                out += int(c.bits, 2).to_bytes(len(c.bits) // 8, "big")
    return bytes(out), starts


Geo = namedtuple("Geo", "lshape cshape depth ys xs")


def geo_n(g):
    """coefficients per slice component: (luma, chroma)"""
    return (g.lshape[0] // g.ys) * (g.lshape[1] // g.xs), (g.cshape[0] // g.ys) * (g.cshape[1] // g.xs)


# the int32 reader's geometries (any works for vc2hip_hq_unpack): 256 slices each
GEOS = {
    "n16": Geo((64, 64), (32, 32), 1, 16, 16),         # luma 4 x 4, chroma 2 x 2 per slice: n < 32
    "n128": Geo((128, 256), (64, 128), 2, 16, 16),     # luma 8 x 16 = 128, chroma 4 x 8 = 32: rounds of exactly 32
    "n48": Geo((64, 192), (64, 96), 1, 16, 16),        # luma 4 x 12 = 48 (a last round of 16), chroma 4 x 6 = 24
}


# the decoders' geometries (proxy_ref.Case arguments; 16-bit samples at index 0, so that clipping is rarest): C and D of
# tests/test_gpu_damaged.py, and a depth-1 picture whose chroma components have 16 coefficients
CASES = {
    "C": (1024, 128, "422", 16, "DD97", 3, 2, 4),      # 256 slices of 16 x 32: luma 512, chroma 256 coefficients
    "D": (2048, 256, "422", 16, "DD97", 4, 1, 2),      # 1024 slices of 16 x 32
    "S": (256, 32, "422", 16, "LeGall", 1, 2, 4),      # 256 slices of 4 x 8: luma 32, chroma 16
}


def case_of(oracle, name, **kw):
    import proxy_ref as pr
    return pr.Case(oracle, *CASES[name], q=0, scalar=1, **kw)


def geo_of(case):
    return Geo((case.ph, case.pw), (case.cph, case.cpw), case.depth, case.ys, case.xs)


def order(sh, sw, depth):
    """(y, x) inside a slice tile in coding order: LL, then per level HL, LH, HH (WaveletTransform.cpp:428-450)"""
    out = []
    for band in range(3 * depth + 1):
        if band == 0:
            s, oy, ox = 1 << depth, 0, 0
        else:
            level, kind = (band - 1) // 3 + 1, (band - 1) % 3
            s = 1 << (depth + 1 - level)
            oy, ox = (0 if kind == 0 else s // 2), (0 if kind == 1 else s // 2)
        out += [(y, x) for y in range(oy, sh, s) for x in range(ox, sw, s)]
    return out


Input = namedtuple("Input", "name tag prefix scalar slices domain named")   # named: [(slice, component, position)] designed on purpose
SMALL, SMALL_INDEX = 8, 12


def make_input(name, tag, slices, domain=True, prefix=0, scalar=1, index=None):
    """the slices with their index bytes set and the named positions listed.  Index 0, so that clipping is rarest -- but
    SMALL_INDEX in a slice with a named value below SMALL: at index 0 the inverse transform's rounding swallows a lone -1
    whole, and the decode window of tests/test_gpu_reader.py would not see it; at 12 the dequantiser makes it -5 or more."""
    out, named = [], []
    for i, (_, cs) in enumerate(slices):
        small = any(0 < abs(c.want[k]) < SMALL for c in cs for k in c.named)
        out.append((SMALL_INDEX if small or (index is not None and any(c.named for c in cs)) else 0, cs))
        named += [(i, ci, k) for ci, c in enumerate(cs) for k in c.named]
    return Input(name, tag, prefix, scalar, out, domain, named)


def designed_components(inp):
    """[(slice, component index, Comp)] of the components that hold a named value: the fillers left out"""
    return [(i, ci, c) for i, (_, cs) in enumerate(inp.slices) for ci, c in enumerate(cs) if c.named]


def planes(inp, g):
    """the designed coefficient planes (y, u, v) and indices of an input on geometry g"""
    out = [np.zeros(g.lshape, np.int32), np.zeros(g.cshape, np.int32), np.zeros(g.cshape, np.int32)]
    assert len(inp.slices) == g.ys * g.xs
    for c in range(3):
        sh, sw = out[c].shape[0] // g.ys, out[c].shape[1] // g.xs
        oy, ox = np.array(order(sh, sw, g.depth)).T
        for i, (_, comps) in enumerate(inp.slices):
            y0, x0 = (i // g.xs) * sh, (i % g.xs) * sw
            out[c][y0 + oy, x0 + ox] = comps[c].want
    q = np.array([s[0] for s in inp.slices], np.int32).reshape(g.ys, g.xs)
    return out[0], out[1], out[2], q


def is_cut(inp):
    return any(c.cut for _, comps in inp.slices for c in comps)


def max_abs(inp):
    return max(abs(v) for _, comps in inp.slices for c in comps for v in c.want)


# ---------------------------------------------------------------------------------------------------------------------
# generators: each (nl, nc, ns, seed) -> [Input]; ns slices a picture
# ---------------------------------------------------------------------------------------------------------------------
def _val(rng, K):
    m = int(rng.integers((1 << K) - 1, (2 << K) - 1))
    return -m if rng.integers(2) else m


def _sparse(rng, count, p=0.12, kmax=3):
    """seeded background: mostly zeros, small values (codes the table holds)"""
    return [_val(rng, int(rng.integers(1, kmax + 1))) if rng.random() < p else 0 for _ in range(count)]


def _filler(rng, n, scalar=1):
    return component(_sparse(rng, n), n, scalar=scalar)


def _pictures(name, tag, comps, nl, nc, ns, seed, domain=True, prefix=0, scalar=1, luma_only=False, index=None):
    """components [(Comp maker: n -> Comp, note)] dealt over the slices of as many pictures as they need: luma and chroma in
    turn, or luma alone; seeded fillers elsewhere"""
    rng = np.random.default_rng(seed + 1)
    per = ns * (1 if luma_only else 3)
    out = []
    for p0 in range(0, max(len(comps), 1), per):
        part = comps[p0:p0 + per]
        slices = []
        for i in range(ns):
            cs = []
            for c in range(3):
                k = i if luma_only else 3 * i + c
                n = nc if c else nl
                if (c == 0 or not luma_only) and k < len(part):
                    cs.append(part[k](n))
                    assert cs[-1].named
                else:
                    cs.append(_filler(rng, n, scalar))
            slices.append((0, cs))
        out.append(make_input(name, f"{tag} {p0 // per}" if len(comps) > per else tag, slices, domain, prefix, scalar, index))
    return out


LENGTH_EXTRA = (128, -128, 129, -129, -32768, 32768, 32766, -32766, 126, -126)


def length_values():
    """both magnitude extremes of every length class K = 0 .. 15, both signs, and the neighbours of the stores' bounds"""
    vals = [0]
    for K in range(1, 16):
        for m in ((1 << K) - 1, (2 << K) - 2):
            vals += [m, -m]
    return vals + list(LENGTH_EXTRA)


def gen_lengths(nl, nc, ns, seed=SEED):
    """every value of length_values() in Y, U and V, each at a seeded position among zeros and small values"""
    vals = length_values()
    assert ns >= len(vals)
    rng = np.random.default_rng(seed)
    slices = []
    for i in range(ns):
        cs = []
        for c in range(3):
            n = nc if c else nl
            v = vals[(3 * i + c) % len(vals)]
            at = int(rng.integers(0, n))
            body = _sparse(rng, n, 0.05)
            body[at] = v
            cs.append(component(body, n, named=[at]))
        slices.append((0, cs))
    return [make_input("lengths", f"{len(vals)} values", slices)]


OVER32 = (65535, -65535, 1 << 17, -(200000), 1 << 20, -(1 << 20), (1 << 23) + 5, (1 << 31) - 1, -((1 << 31) - 1), (1 << 32) + 5, -((1 << 32) + 77))


def gen_over32(nl, nc, ns, seed=SEED):
    """codes of 34, 36, 42, 48, 64 and 66 bits (the last: a magnitude that wraps in 32 bits): outside the encoder's domain"""
    rng = np.random.default_rng(seed)
    comps = []
    for k in range(3 * len(OVER32)):
        v = OVER32[k % len(OVER32)]

        def make(n, v=v, s=int(rng.integers(1 << 30))):
            r = np.random.default_rng(s)
            body = _sparse(r, n, 0.1)
            at = [int(r.integers(0, n))]
            body[at[0]] = v
            return component(body, n, named=at)       # (one such value a component: two would hide each other under the clip)
        comps.append(make)
    # (every designed slice at SMALL_INDEX: at index 0 the dequantiser's 32-bit arithmetic wraps +-(2^31 - 1) to +-1)
    return _pictures("over32", "codes of 34 to 66 bits", comps, nl, nc, ns, seed, domain=False, index=SMALL_INDEX)


PHASE_K = (5, 10, 15)
PHASE_V = {5: 45, 10: -1500, 15: -40000}


def phase_specials(n):
    """value lists on decode_round's second-token conditions and the run caps (those that fit n coefficients)"""
    sp = {
        "second taken, n + z2 = 32": [40] + [0] * 20 + [-40000, 1],
        "second refused, n + z2 = 33": [40] + [0] * 21 + [-40000, 1],
        "second taken, n = 31": [0] * 27 + [1, -65534],
        "second refused, n = 32": [0] * 28 + [1, -65534],
        "second refused, cnt + z2 = room": [1] * 5 + [0] * 27 + [-3, 2],
        "second taken, cnt + z2 = room - 1": [1] * 5 + [0] * 26 + [-3, 2],
        "run of 31 then 32 bits": [0] * 31 + [-65534, 1],
        "run of 32 then 32 bits": [0] * 32 + [-65534, 1],
        "run of 33 then 32 bits": [0] * 33 + [-65534, 1],
        "run of 64 then 32 bits": [0] * 64 + [-65534, 1],
        "run of 65 then 32 bits": [0] * 65 + [65534, -1],
    }
    return {k: v for k, v in sp.items() if len(v) <= n}


def gen_phase(nl, nc, ns, seed=SEED):
    """one long code (K = 5, 10, 15) behind r zero coefficients, r = 0 .. 40 (as far as the component holds them), with a
    short code or zeros behind it; then the special value lists of phase_specials.  In luma, which holds the most coefficients."""
    comps = []
    for K in PHASE_K:
        for r in range(41):
            for tail in ([[1, -2]] if r not in (31, 32, 33) else [[1, -2], []]):
                vals = [0] * r + [PHASE_V[K]] + tail

                def make(n, vals=vals):
                    return component(vals[:n] if len(vals) > n else vals, n, named="nonzero" if any(vals[:n]) else [0])
                comps.append(make)
    names = list(phase_specials(1 << 20))
    for nm in names:
        def make(n, nm=nm):
            sp = phase_specials(n)
            return component(sp.get(nm, [0] * (n - 1) + [PHASE_V[5]]), n, named="nonzero", note=nm)
        comps.append(make)
    return _pictures("phase", f"{len(comps)} components", comps, nl, nc, ns, seed, luma_only=True)


def _complete(bits, n, rng, p=0.15):
    """seeded legal codes behind an arbitrary opening: the pending code is finished, then sparse values up to n coefficients"""
    bits, count, i = list(bits), 0, 0
    while count < n and i < len(bits):
        if bits[i] == "1":
            i, count = i + 1, count + 1
            continue
        pairs = 0
        while True:                                     # bits[i] is a follow bit of 0: a data bit, then the next follow bit
            if i + 1 >= len(bits):
                bits.append(str(int(rng.integers(2))))
            i, pairs = i + 2, pairs + 1
            if i >= len(bits):
                bits.append("1" if pairs >= 15 or rng.random() < 0.6 else "0")
            assert pairs <= 15, "the opening alone is a code of more than 32 bits"
            if bits[i] == "1":
                if i + 1 >= len(bits):
                    bits.append(str(int(rng.integers(2))))   # the sign
                i += 2
                break
        count += 1
    return "".join(bits) + "".join(code(v) for v in _sparse(rng, max(n - count, 0), p))


def gen_table(nl, nc, ns, seed=SEED):
    """every one of the 1024 table indices opens a luma component at bit 0; the same patterns behind 1 .. 9 zero
    coefficients in U and V, so that each also occurs at a later look-up"""
    rng = np.random.default_rng(seed)
    out = []
    for p0 in range(0, 1 << LUT_BITS, ns):
        slices = []
        for i in range(ns):
            idx = p0 + i
            pat = format(idx % (1 << LUT_BITS), "010b")
            cs = []
            for c, shift in ((0, 0), (1, 1 + idx % 9), (2, 1 + (idx // 9) % 9)):
                n = nc if c else nl
                shift = min(shift, max(n - 1, 0))
                comp = component([], n, raw=_complete("1" * shift + pat, n, rng))
                # named: what the opening holds -- the non-zero values among its first coefficients (an index of ten '1' bits is
                # ten zeros; the first two of them), or the component's first coefficient where it holds none
                first = [k for k in range(min(shift + LUT_BITS, n)) if comp.want[k]]
                cs.append(comp._replace(named=tuple(first[:2]) or (0,), note=f"index {idx} behind {shift} zeros"))
            slices.append((0, cs))
        out.append(make_input("table", f"indices {p0} .. {p0 + ns - 1}", slices))
    return out


def gen_spill(nl, nc, ns, seed=SEED):
    """a table entry of 7 or 8 coefficients applied at cnt = room - 1 .. room - 7: a long code (K = 5: no table entry) at the
    coefficient before makes the next turn's first look-up start there.  7 coefficients: six zeros and a +-1 at each of the
    seven places, so the value also falls into the carried part; 8: eight zeros, a value right behind.  At every round
    boundary the component has; at its END the carried part is slack that looks like codes, and is discarded."""
    comps = []
    for d in range(1, 8):
        for j in list(range(7)) + [8]:
            for which in ("first", "last"):
                def make(n, d=d, j=j, which=which):
                    R = min(32, n) if which == "first" else n
                    c = R - d
                    if c < 1:
                        return component([0] * (n - 1) + [45], n, named=[n - 1])
                    if j == 8:
                        pat = "1" * 8 + code(-2) + code(3)
                    else:
                        pat = "".join(code((-1) ** (d + j)) if k == j else "1" for k in range(7)) + code(2)
                    head = [0] * (c - 1) + [45 if (d + j) % 2 else -45]
                    comp = component(head, n, raw=pat + code(-1) + "1" * 5 + code(1) + code(0) + code(-5))
                    return comp._replace(named=tuple(k for k in range(c - 1, n) if comp.want[k]), note=f"{which} d={d} j={j}")
                comps.append(make)
    return _pictures("spill", f"{len(comps)} components", comps, nl, nc, ns, seed)


END_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255)


def _sum_codes(total, slots, rng, end_nonzero):
    """values whose codes are `total` bits together, at most `slots` of them, none beyond 32 bits; the last one non-zero
    if asked.  None where the rule below says that it cannot be; a seeded walk, tried again where it runs into a dead end,
    and an error -- never a silently thinner design -- if 200 walks all do."""
    # the rule: what lies beyond it is left out of the design by every caller (an odd total spends one slot on a 1-bit code)
    if total > 30 * (slots - 1) or (end_nonzero and 0 < total < 4):
        return None
    for _ in range(200):
        vals = _sum_codes_once(total, slots, rng, end_nonzero)
        if vals is not None:
            assert sum(len(code(v)) for v in vals) == total and len(vals) <= slots
            return vals
    raise AssertionError(f"no {total} bits in {slots} codes found: the design would be thinner than its rule says")


def _sum_codes_once(total, slots, rng, end_nonzero):
    vals, R = [], total
    while R > 0:
        if slots <= 0:
            return None
        if R <= 32 and R % 2 == 0 and R >= 4 and (slots == 1 or R <= 6 or rng.random() < 0.25):
            vals.append(_val(rng, (R - 2) // 2))
            return vals
        cand = []
        for ell in [1] + list(range(4, 34, 2)):
            rest = R - ell
            if rest < 0 or rest > 32 * (slots - 1):
                continue
            if rest == 0 and (ell == 1 and end_nonzero):
                continue
            if end_nonzero and 0 < rest < 4:
                continue
            if rest and slots - 1 == 1 and (rest % 2 or rest < 4 or rest > 32) and not (rest == 1 and not end_nonzero):
                continue
            cand.append(ell)
        if not cand:
            return None
        avg = R / slots
        near = [e for e in cand if e <= 2 * avg + 3] or [min(cand)]
        need = [e for e in near if e >= avg - 1] if avg > 3 else near
        ell = int(rng.choice(need or near)) if rng.random() < 0.5 or avg > 3 else min(near)
        vals.append(0 if ell == 1 else _val(rng, (ell - 2) // 2))
        R -= ell
        slots -= 1
    return vals


def end_items(n, rng):
    """the designed components of `ends` that n coefficients can hold: [(length, treatment, maker of the Comp)]"""
    items = []
    for L in END_LENGTHS:
        if L == 0:
            items.append((0, "empty", lambda n=n: component([], n, units=0, named=[0], note="empty")))
            continue
        vals = _sum_codes(8 * L, n, rng, True)
        if vals is not None:
            items.append((L, "exact", lambda vals=vals, L=L, n=n: component(vals, n, units=L, named="largest", note="exact")))
        for j in range(1, 15):                     # the K = 6 code (14 bits) cut after j of its bits
            if 8 * L - j < 0:
                continue
            head = _sum_codes(8 * L - j, n - 1, rng, False) if 8 * L - j else []
            if head is not None:
                v = -100 if j % 2 else 77
                items.append((L, f"cut{j}", lambda head=head, v=v, L=L, n=n, j=j: component(head + [v], n, units=L, named="largest", note=f"cut{j}")))
        if n <= 8 * L:
            for pad in "01":
                body = _sparse(rng, n, 0.1)
                while len("".join(code(v) for v in body)) > 8 * L:
                    body[int(np.flatnonzero(body)[0])] = 0
                items.append((L, f"slack{pad}", lambda body=body, pad=pad, L=L, n=n: component(body, n, pad=pad, units=L, named="largest", note=f"slack{pad}")))
    return items


def gen_ends(nl, nc, ns, seed=SEED):
    """component data of every length of END_LENGTHS at scalar 1: codes that end on the data's last bit, a K = 6 code cut
    after each of its 14 bits, all coefficients coded early with slack of 0x00 and of 0xFF behind -- as far as n
    coefficients of at most 32 bits can fill the length.  `exact`, `slack` and `empty` at every byte offset mod 8, `cut`
    at the offsets as they fall: a component is placed where the payload's running offset is one it still wants."""
    rng = np.random.default_rng(seed)
    items = {0: end_items(nl, rng), 1: end_items(nc, rng)}
    out = []

    def place(want, tag):
        slices, pos, guard = [], 0, 0
        while want:
            guard += 1
            assert guard < 200000
            pos += 1                                   # the index byte (prefix 0)
            cs = []
            for c in range(3):
                kind, n = (1 if c else 0), (nc if c else nl)
                pos += 1
                o = pos % 8
                key = next((k for k in want if k[0] == kind and k[2] == o), None) or next((k for k in want if k[0] == kind and k[2] is None), None)
                if key is not None:
                    del want[key]
                    comp = items[kind][key[1]][2]()
                else:
                    comp = component(_sparse(rng, min(n, 8 * int(rng.integers(1, 8)))), n)   # a filler that moves the offset on
                cs.append(comp)
                pos += comp.units
            slices.append((0, cs))
            if len(slices) == ns or not want:
                while len(slices) < ns:
                    slices.append((0, [_filler(rng, nl), _filler(rng, nc), _filler(rng, nc)]))
                out.append(make_input("ends", f"{tag} {len(out)}", slices))
                slices, pos = [], 0

    # (component kind, item index, offset) to place.  A component of 255 bytes that is cut decodes to values whose codes need
    # more than 255 bytes: no slice writer can repack it at scalar 1, so those go into pictures of their own
    for last in (False, True):
        want = {}
        for kind in (0, 1):
            for k, (L, t, _) in enumerate(items[kind]):
                if (L == 255 and t.startswith("cut")) == last:
                    for o in (range(8) if not t.startswith("cut") else [None]):
                        want[(kind, k, o)] = True
        place(want, "cut at 255 bytes, picture" if last else "picture")
    return out


def gen_slot_end(nl, nc, ns, seed=SEED, multiple=256):
    """payloads whose length is a multiple of `multiple` (of 16 and 64 with it), so that a slot of exactly that stride ends
    with the payload: the last slice's components are 1 .. 17 bytes long, three lengths a payload, and end on their last
    bit (as far as n coefficients can fill them); slack in the slices before brings the length up"""
    rng = np.random.default_rng(seed)
    out = []
    for a in range(1, 18, 3):
        lens = [min(a + k, 17) for k in range(3)]
        last = []
        for c, L in enumerate(lens):
            n = nc if c else nl
            vals = _sum_codes(8 * L, n, rng, True)
            if vals is None:                        # n codes of 32 bits cannot fill L bytes: all coefficients early, zeros behind
                vals = [0] * (n - 1) + [-9]
            last.append(component(vals, n, units=L, named="last", note=f"{L} bytes"))
        slices = [(0, [_filler(rng, nl), _filler(rng, nc), _filler(rng, nc)]) for _ in range(ns - 1)] + [(0, last)]
        size = sum(4 + sum(c.units for c in cs) for _, cs in slices)
        short = -size % multiple
        i = 0
        while short:                                # slack of 0xFF in the fillers
            q, cs = slices[i % (ns - 1)]
            c = i % 3
            add = min(short, 255 - cs[c].units, 40)
            if add:
                n = nc if c else nl
                cs[c] = cs[c]._replace(bits=cs[c].bits + "1" * (8 * add), units=cs[c].units + add)
                assert plain(cs[c].bits, n) == cs[c].want
                short -= add
            i += 1
        out.append(make_input("slot_end", f"last components of {lens} bytes", slices))
    return out


def gen_random(nl, nc, ns, seed=SEED, pictures=1):
    """seeded streams: K geometric over 0 .. 15, zero runs geometric up to 64.  The net under the designed inputs."""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(pictures):
        slices = []
        for i in range(ns):
            cs = []
            for c in range(3):
                n = nc if c else nl
                vals = []
                mean_run = float(rng.choice([0.5, 2, 8, 24]))
                budget = 8 * 250
                while len(vals) < n:
                    run = min(int(rng.geometric(1 / (1 + mean_run))) - 1, 64)
                    K = min(int(rng.geometric(0.45)) - 1, 15)
                    v = _val(rng, K) if K else 0
                    if budget - run - len(code(v)) < n - len(vals):
                        break
                    vals += [0] * run + [v]
                    budget -= run + len(code(v))
                cs.append(component(vals[:n], n))
            slices.append((0, cs))
        out.append(make_input("random", f"seed {seed} picture {p}", slices))
    return out


GENERATORS = {"lengths": gen_lengths, "over32": gen_over32, "phase": gen_phase, "table": gen_table, "spill": gen_spill, "ends": gen_ends,
              "slot_end": gen_slot_end, "random": gen_random}
DESIGNED = tuple(k for k in GENERATORS if k != "random")
_INPUTS = {}


def inputs(name, nl, nc, ns=256, seed=SEED):
    key = (name, nl, nc, ns, seed)
    if key not in _INPUTS:
        _INPUTS[key] = GENERATORS[name](nl, nc, ns, seed)
    return _INPUTS[key]


def payload_of(inp):
    return payload(inp.slices, inp.prefix, inp.scalar)[0]


# ---------------------------------------------------------------------------------------------------------------------
# the readers' token logic, transcribed
# ---------------------------------------------------------------------------------------------------------------------
# Three wrong copies that no input can catch, because what they change is dead at the table's 10 bits and rows of 32: the
# cap of two values per entry (a third whole code needs 12 bits); the cap of 8 coefficients per entry (an entry of 9 or 10
# holds zeros only, and zeros are not stored); the run cap of 32 (decode_round's run is bounded by room <= 32 first, and
# tc_turn reaches its arithmetic token only where the first look-up finds no whole code -- a run of 0 -- or fewer than 8
# coefficients are left).  test_reader_ref.py asserts the three facts.
MUTANTS = {
    "lut_whole": "the table's `whole` off by one: a code whose sign bit is the first bit behind the index counts as whole",
    "guard4": "the fourth look-up's `used + 10 <= have` guard dropped",
    "n_z2_33": "decode_round's second token: n + z2 <= 33",
    "cnt_z2_le": "decode_round's second token: cnt + z2 <= room",
    "fill_short": "the ones-fill mask one bit short: the first bit behind the data is read from memory",
    "fill_long": "the ones-fill mask one bit long: the data's last bit reads as 1",
    "lead": "`lead` from the wrong residue: the 8-byte readers take the address mod 4, the 4-byte reader mod 8",
    "spill_drop": "k_hq_unpack16's spill: the count is carried, the values are not",
    "sentinel32768": "the 16-bit store's fit test lets -32768 through: the sentinel without a wide value",
    "byte128": "the byte planes' bound at 128: +128 stored as the byte 0x80, the sentinel without a wide value",
    "sign_k15": "the sign bit's position at K = 15 (a shift count of 0) taken one too high",
    "tc_room": "tc_turn's later look-ups tested against the turn's room, not what the earlier ones left of it",
}


def _clz(x, width):
    return width - x.bit_length()


class _Bits:
    def __init__(self, s):
        self.L, self.v = len(s), int(s, 2) if s else 0

    def peek(self, p, k):
        """k bits from bit p on; ones behind the string"""
        end = p + k
        if end <= self.L:
            return (self.v >> (self.L - end)) & ((1 << k) - 1)
        if p >= self.L:
            return (1 << k) - 1
        extra = end - self.L
        return ((self.v & ((1 << (self.L - p)) - 1)) << extra) | ((1 << extra) - 1)


Ctx = namedtuple("Ctx", "pre data post pos")     # the 64 bits before the data, the data, the 64 bits behind; the data's byte address


def ctx_of(pay, start, nbytes):
    bits = lambda b: "".join(format(x, "08b") for x in b)
    pre = pay[max(start - 8, 0):start]
    return Ctx("0" * (64 - 8 * len(pre)) + bits(pre), bits(pay[start:start + nbytes]), (bits(pay[start + nbytes:start + nbytes + 8]) + "1" * 64)[:64], start)


def _stream(cx, mut, word):
    """the bits a reader sees before the endless ones; word: 4 (Reader32) or 8 (WordReader, TcReader)"""
    d = cx.data
    if not d:
        return ""
    if mut == "fill_short":
        return d + cx.post[0]
    if mut == "fill_long":
        return d[:-1] + "1"
    if mut == "lead" and cx.pos & 4:
        if word == 4:        # lead = 8 * (pos & 7): 32 bits too many are shifted out, the bound moves with them
            return (d + cx.post)[32:32 + len(d)]
        return (cx.pre + d)[32:32 + len(d)]
    return d


def unpack_lut(mut=None):
    """vc2_unpack_lut_host: bits [3:0] consumed, [7:4] coefficients, [11:8] / [15:12] positions, [23:16] / [31:24] values"""
    tab = []
    for idx in range(1 << LUT_BITS):
        bit = lambda i: (idx >> (LUT_BITS - 1 - i)) & 1 if i < LUT_BITS else 0
        pos = nc = nnz = 0
        at, val = [0, 0], [0, 0]
        while nc < 8 and pos < LUT_BITS:
            if bit(pos):
                nc, pos = nc + 1, pos + 1
                continue
            q, mag, whole = pos, 1, False
            while q + 1 < LUT_BITS:
                mag = (mag << 1) | bit(q + 1)
                q += 2
                if q >= LUT_BITS:
                    break
                if bit(q):
                    whole = q + 1 <= LUT_BITS if mut == "lut_whole" else q + 1 < LUT_BITS
                    break
            if not whole or nnz == 2:
                break
            v = -(mag - 1) if bit(q + 1) else mag - 1
            at[nnz], val[nnz] = nc, v
            nnz, nc, pos = nnz + 1, nc + 1, q + 2
        if nnz == 1:
            at[1], val[1] = at[0], val[0]
        tab.append(0 if nc == 0 else pos | nc << 4 | at[0] << 8 | at[1] << 12 | (val[0] & 0xFF) << 16 | (val[1] & 0xFF) << 24)
    return tab


_LUTS = {}


def _lut(mut):
    key = mut if mut == "lut_whole" else None
    if key not in _LUTS:
        _LUTS[key] = unpack_lut(key)
    return _LUTS[key]


def _s8(x):
    x &= 0xFF
    return x - 256 if x & 0x80 else x


def _s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def _compact_even32(x):
    return int("0" + format(x & M32, "032b")[1::2], 2)


def _arith(hi, follow, mut):
    """a code of up to 32 bits at the top of hi by arithmetic -> (value, bits)"""
    K = _clz(follow, 32) >> 1
    body = hi >> ((32 - 2 * K) & 31)
    mag = (((1 << K) | _compact_even32(body)) - 1) & M32
    sh = (30 - 2 * K) & 31
    if mut == "sign_k15":
        sh = max(30 - 2 * K, 1)
    neg = (hi >> sh) & 1
    return _s32(-mag if neg else mag), 2 * K + 2


def _serial(B, p):
    """bit by bit from bit p on -> (value, p behind the code)"""
    value = 1
    while True:
        f = B.peek(p, 1)
        p += 1
        if f:
            break
        value = ((value << 1) | B.peek(p, 1)) & M32
        p += 1
    value = (value - 1) & M32
    v = 0
    if value:
        v = _s32(-value if B.peek(p, 1) else value)
        p += 1
    return v, p


LOST = None    # a coefficient whose store element is a sentinel without a wide value: whatever the wide array held before


def model_unpack16(cx, n, mut=None, st=None, store="s16"):
    """the turn of k_hq_unpack16 over the rounds of one component -> its n values as the store and the wide array give them
    back (store: s16, or b8 for byte planes)"""
    lut, B = _lut(mut), _Bits(_stream(cx, mut, 4))
    st = st if st is not None else Counter()
    p, have = 0, 64 - 8 * (cx.pos & 3)
    row, wide, out, cnt = [0] * 40, {}, [], 0

    def skip(k):
        nonlocal p, have
        p, have = p + k, have - k
        if have <= 32:
            have += 32

    def fits(v):
        return (-32768 if mut == "sentinel32768" else -32767) <= v <= 32767

    for base in range(0, n, 32):
        room = min(32, n - base)
        while cnt < room:
            used = 0
            for look in range(4):
                valid = have - used                                          # real bits in (acc << used): zeros behind them
                w = B.peek(p + used, LUT_BITS)
                if valid < LUT_BITS:
                    w &= ~((1 << (LUT_BITS - valid)) - 1)
                e = lut[w]
                if look:
                    ok4 = look < 3 or mut == "guard4" or used + LUT_BITS <= have
                    if look == 3 and cnt < room:
                        st["u16 look4 taken" if used + LUT_BITS <= have else "u16 look4 refused"] += 1
                    e = e if cnt < room and ok4 else 0
                if e:
                    st["u16 index at look 0" if look == 0 else "u16 index at a later look", w] += 1
                    nc = (e >> 4) & 15
                    two = ((e >> 8) & 15) != ((e >> 12) & 15)
                    st["u16 entry of 8" if nc == 8 else "u16 entry of two values" if two else "u16 entry of one value" if (e >> 16) else "u16 entry of zeros"] += 1
                    if look:
                        st[f"u16 entry at look {look}"] += 1
                    if cnt + nc > room:
                        st[f"u16 spill {cnt + nc - room}" + (" at the end" if base + room == n else "")] += 1
                        if any(_s8(e >> s) and cnt + ((e >> a) & 15) >= room for s, a in ((16, 8), (24, 12))):
                            st["u16 spill carries a value" + (" at the end" if base + room == n else "")] += 1
                row[cnt + ((e >> 8) & 15)] = _s8(e >> 16)
                row[cnt + ((e >> 12) & 15)] = _s8(e >> 24)
                cnt += (e >> 4) & 15
                used += e & 15
            if used == 0 and cnt < room:
                hi = B.peek(p, 32)
                follow = hi & 0xAAAAAAAA
                if follow:
                    v, used = _arith(hi, follow, mut)
                    st[f"u16 long K={used // 2 - 1}"] += 1
                else:
                    st["u16 bit-serial"] += 1
                    v, q = _serial(B, p)
                    for _ in range(q - p):
                        skip(1)
                if not fits(v):
                    wide[base + cnt] = v
                    v = -32768
                    st["u16 escape"] += 1
                row[cnt] = v
                cnt += 1
            skip(used)
        for k in range(room):
            v = row[k]
            if store == "b8":
                if not -127 <= v <= (128 if mut == "byte128" else 127):
                    if v != -32768:
                        wide[base + k] = v
                    v = -128
                    st["u16 byte escape"] += 1
                v = _s8(v)
                out.append(wide.get(base + k, LOST) if v == -128 else v)
            else:
                out.append(wide.get(base + k, LOST) if v == -32768 else v)
        spill = row[32:40]
        row = [0] * 40
        cnt = max(cnt - 32, 0)
        if cnt and mut != "spill_drop":
            row[:8] = spill
    return out


def _vlut():
    """decode_round's own table (vlut_init): codes of up to 10 bits by their leading 10 bits: length << 8 | value"""
    tab = []
    for i in range(1024):
        e = 0
        for K in range(1, 5):
            if e:
                break
            ok = (i >> (9 - 2 * K)) & 1 == 1 and all((i >> (9 - 2 * j)) & 1 == 0 for j in range(K))
            if ok:
                m = 1
                for j in range(K):
                    m = (m << 1) | ((i >> (8 - 2 * j)) & 1)
                m -= 1
                v = -m if (i >> (8 - 2 * K)) & 1 else m
                e = (2 * K + 2) << 8 | (v & 0xFF)
        tab.append(e)
    return tab


_VLUT = _vlut()


def model_round(cx, n, mut=None, st=None):
    """decode_round<32, int> over the rounds of one component (k_hq_unpack<32>)"""
    B = _Bits(_stream(cx, mut, 8))
    st = st if st is not None else Counter()
    p, out = 0, []
    for base in range(0, n, 32):
        room = min(32, n - base)
        row, cnt = [0] * 36, 0
        while cnt < room:
            win = B.peek(p, 64)
            lz = _clz(~win & M64, 64)
            z = min(lz, room - cnt, 32)
            if min(lz, room - cnt) > 32:
                st["rnd run capped at 32"] += 1
            if z == room - cnt and lz > z:
                st["rnd run cut by the round"] += 1
            cnt += z
            nz = cnt < room and z == lz
            hi = ((win << z) & M64) >> 32
            follow = hi & 0xAAAAAAAA
            if nz and follow == 0:
                st["rnd bit-serial"] += 1
                row[cnt], p = _serial(B, p + z)
                cnt += 1
                continue
            e1 = _VLUT[hi >> 22]
            if e1:
                val, ln = _s8(e1), e1 >> 8
            else:
                val, ln = _arith(hi, follow | 1, mut)
                if nz:
                    st[f"rnd long K={ln // 2 - 1}"] += 1
            if nz:
                row[cnt] = val
                cnt += 1
            nb = z + ln if nz else z
            if nb <= 31:
                w2 = (win << nb) & M64
                z2 = min(_clz(~w2 & M64, 64), room - cnt)
                hi2 = ((w2 << z2) & M64) >> 32
                follow2 = hi2 & 0xAAAAAAAA
                c_n = nb + z2 <= (33 if mut == "n_z2_33" else 32)
                c_room = cnt + z2 <= room if mut == "cnt_z2_le" else cnt + z2 < room
                if nz and follow2:
                    st["rnd second taken" if nb + z2 <= 32 and cnt + z2 < room else "rnd second refused: n + z2 > 32" if cnt + z2 < room else
                       "rnd second refused: cnt + z2 = room"] += 1
                    if nb + z2 == 32 and cnt + z2 < room:
                        st["rnd second taken at n + z2 = 32"] += 1
                if nz and c_n and c_room and follow2:
                    e2 = _VLUT[hi2 >> 22]
                    val2, ln2 = (_s8(e2), e2 >> 8) if e2 else _arith(hi2, follow2, mut)
                    if not e2:
                        st[f"rnd long K={ln2 // 2 - 1}"] += 1
                    cnt += z2
                    row[cnt] = val2
                    cnt += 1
                    nb += z2 + ln2
            elif nz:
                st["rnd second refused: n > 31"] += 1
            p += nb
        out += row[:room]
    return out


def model_tc(cx, n, mut=None, st=None):
    """tc_turn / tc_long over one component, as k_transcode_measure's loop drives them -> the values it measures"""
    lut, B = _lut(mut), _Bits(_stream(cx, mut, 8))
    st = st if st is not None else Counter()
    p, j, out = 0, 0, {}
    while j < n:
        room = n - j
        win = B.peek(p, 64)
        t_nc = consume = 0
        longcode = False
        e = lut[win >> (64 - LUT_BITS)]
        if e and ((e >> 4) & 15) <= room:
            go = True
            for k in range(3):
                if k:
                    e = lut[((win << consume) & M64) >> (64 - LUT_BITS)]
                nc = (e >> 4) & 15
                fit = nc <= (room if mut == "tc_room" else room - t_nc)
                if go and e and not nc <= room - t_nc:
                    st["tc look-up refused by the room"] += 1
                go = go and e != 0 and fit
                if go:
                    a0, a1 = (e >> 8) & 15, (e >> 12) & 15
                    if _s8(e >> 16):
                        out[j + t_nc + a0] = _s8(e >> 16)
                    if a1 != a0:
                        out[j + t_nc + a1] = _s8(e >> 24)
                    t_nc += nc
                    consume += e & 15
                    st["tc look-up"] += 1
        else:
            if e:
                st["tc first look-up refused by the room"] += 1
            lz = _clz(~win & M64, 64)
            z = min(lz, room, 32)
            if min(lz, room) > 32:
                st["tc run capped at 32"] += 1
            t_nc = consume = z
            if z < room and z == lz:
                hi = ((win << z) & M64) >> 32
                follow = hi & 0xAAAAAAAA
                if not follow:
                    longcode = True
                else:
                    v, ln = _arith(hi, follow, mut)
                    st[f"tc long K={ln // 2 - 1}"] += 1
                    out[j + z] = v
                    t_nc, consume = z + 1, z + ln
        p += consume
        j += t_nc
        if longcode:
            st["tc_long"] += 1
            out[j], p = _serial(B, p)
            j += 1
    return [out.get(k, 0) for k in range(max([n] + [k + 1 for k in out]))]


# ---------------------------------------------------------------------------------------------------------------------
# what an input reaches
# ---------------------------------------------------------------------------------------------------------------------
def reader32_end(pos, nbytes, safe):
    """Reader32 by arithmetic: the fetch forms from the component's start to its end -> (set of forms, the form that
    holds the last data bit).  Forms: `16` (sixteen bytes of data), `tail16` (the last bytes in one load, inside the slot),
    `words` (word by word: the slot ends inside the piece), `whole` (64 bytes in one request), `none` (no data)."""
    off, left = pos & ~3, (8 * nbytes + 8 * (pos & 3)) if nbytes > 0 else 0
    forms, last, k = set(), "none", 0
    while left > 0:
        if k >= 6 and (k - 6) % 4 == 0 and left >= 512:
            forms.add("whole")
            off, left, k, last = off + 64, left - 512, k + 4, "whole"
            continue
        last = "16" if left >= 128 else "tail16" if off + 16 <= safe else "words"
        forms.add(last)
        off, left, k = off + 16, left - 128, k + 1
    return forms, last


def word_end(pos, nbytes):
    """WordReader / TcReader by arithmetic: data bits in the last 8-byte word (64: it ends on a word), words in TcReader's
    last request (8: a full one)"""
    if nbytes <= 0:
        return 0, 0
    total = 8 * nbytes + 8 * (pos & 7)
    return (total - 1) % 64 + 1, (-(-total // 64) - 1) % 8 + 1


def trace(inp, nl, nc, stride=None, models=("unpack16", "round", "tc"), fillers=False):
    """what the designed components of an input reach on each model (a Counter of events), and the fetch forms at their
    ends; fillers: the seeded fillers around them too"""
    pay, starts = payload(inp.slices, inp.prefix, inp.scalar)
    stride = stride or (len(pay) + 63) & ~63
    st = Counter()
    comps = [c for _, cs in inp.slices for c in cs]
    for k, (c, start) in enumerate(zip(comps, starts)):
        n = nc if k % 3 else nl
        nbytes = c.units * inp.scalar
        if not (c.named or fillers):
            continue
        cx = ctx_of(pay, start, nbytes)
        if "unpack16" in models:
            model_unpack16(cx, n, st=st)
        if "round" in models:
            model_round(cx, n, st=st)
        if "tc" in models:
            model_tc(cx, n, st=st)
        forms, last = reader32_end(start, nbytes, stride)
        st[f"reader32 ends in {last}"] += 1
        if "whole" in forms:
            st["reader32 whole request"] += 1
        bits_last, words_last = word_end(start, nbytes)
        st[f"word reader: {bits_last % 64 // 8} bytes in the last word"] += 1 if nbytes else 0
        st[f"tc request of {words_last} words"] += 1 if nbytes else 0
        st[f"start offset {start % 8}"] += 1
        if c.cut:
            st["cut"] += 1
        if nbytes == 0:
            st["empty"] += 1
    return st


def run_models(inp, nl, nc, mut=None, models=("unpack16", "b8", "round", "tc")):
    """every component of an input through the models -> {model: [values per component]}"""
    pay, starts = payload(inp.slices, inp.prefix, inp.scalar)
    comps = [c for _, cs in inp.slices for c in cs]
    out = {m: [] for m in models}
    for k, (c, start) in enumerate(zip(comps, starts)):
        n = nc if k % 3 else nl
        cx = ctx_of(pay, start, c.units * inp.scalar)
        if "unpack16" in models:
            out["unpack16"].append(model_unpack16(cx, n, mut))
        if "b8" in models:
            out["b8"].append(model_unpack16(cx, n, mut, store="b8"))
        if "round" in models:
            out["round"].append(model_round(cx, n, mut))
        if "tc" in models:
            out["tc"].append(model_tc(cx, n, mut))
    return out


def wants(inp):
    return [c.want for _, cs in inp.slices for c in cs]
