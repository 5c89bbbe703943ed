"""The slice index of the HQ decoders restated on the CPU, and designed length chains for it (pure CPU: no GPU import).

vc2_launch_slice_index (csrc/vc2hip_slices.hip) turns the serial chain through the length bytes of an HQ payload into one
offset per slice.  What it launches follows from (prefix, scalar, payload stride) alone; plan() restates that arithmetic.
The offsets depend on nothing but the length bytes, so build_chain() makes payloads from designed length bytes, the
generators design them to stand on the edges of a plan (a slice that ends exactly on a chunk boundary, a maximal slice that
starts on a chunk's last candidate position, a chunk full of minimal slices, ...), emulate() is a plain transcription of
the kernels with their packed fields (numpy over the entries of a table), and trace() says what an input reaches.

MUTANTS names one-line wrong copies of emulate(); tests/test_index_ref.py shows that every one of them is caught by a
named input.  They stand in for wrong kernels, which are never built."""
import math
from collections import namedtuple

import numpy as np

IDX_MAX_E = 32767          # beyond: k_index_serial
IDX_GROUP = 16
IDX_MAX_GROUPS = 1024      # g_entry of k_index_chain
MERGE_MAX_EU = 4096
DEDUPE_MAX_EU = 8192
LDS_BYTES = 160 * 1024     # per workgroup on gfx950

Plan = namedtuple("Plan", "prefix scalar stride kind cause CH gsh G E EU merge dedupe n_chunks n_groups n_supers threads PER EPT "
                          "lds_tables lds_group")


def entries(prefix, scalar):
    return prefix + 4 + 3 * 255 * scalar


def chunk_of(E):
    return 8192 if E <= 1024 else 16384 if E <= 8191 else 32768


def gshift(prefix, scalar):
    gsh = 0
    while gsh < 2 and scalar % (2 << gsh) == 0 and (prefix + 4) % (2 << gsh) == 0:
        gsh += 1
    return gsh


def plan(prefix, scalar, stride):
    """what vc2_launch_slice_index does for a slot of `stride` bytes"""
    E = entries(prefix, scalar)
    CH, gsh = chunk_of(E), gshift(prefix, scalar)
    n_chunks = (stride + CH - 1) // CH + 1
    too_many = E <= IDX_MAX_E and n_chunks > IDX_MAX_GROUPS * IDX_GROUP
    cause = "long" if E > IDX_MAX_E else "too_many" if too_many else ""
    EU, NP = E >> gsh, CH >> gsh
    merge = EU <= MERGE_MAX_EU and 2 * E <= CH
    dedupe = EU <= DEDUPE_MAX_EU
    threads = 512 if NP <= 8192 else 1024
    n_groups = (n_chunks + IDX_GROUP - 1) // IDX_GROUP
    n_supers = (n_groups + IDX_GROUP - 1) // IDX_GROUP if n_groups > 128 else 0
    stage = (CH + E + 16 + 15) & ~15
    lds_tables = stage + NP * 2 + (EU * 6 + (EU + 31) // 32 * 4 + 16 if merge else 0)
    lds_group = ((EU + 1) & ~1) * 4 + EU * 8 + EU * 2 + 16 if dedupe else 0
    return Plan(prefix, scalar, stride, "serial" if cause else "tables", cause, CH, gsh, 1 << gsh, E, EU, merge, dedupe, n_chunks,
                n_groups, n_supers, threads, NP // threads, 4096 // threads, lds_tables, lds_group)


# (prefix, scalar): the rows every generator runs on
ROWS = [(0, 1), (255, 1),
        (256, 1), (0, 2), (1, 2), (0, 4), (0, 7), (0, 8), (537, 10),
        (538, 10), (0, 11), (0, 20), (0, 24), (0, 42), (633, 42),
        (634, 42), (0, 43)]

# slices -> (y_slices, x_slices); depth 1, luma 4 x 4 and chroma 2 x 2 coefficients per slice.  The odd counts are there for
# `end`: with prefix + 4 = 4 and scalar 8, say, an even number of slices is a multiple of 8 bytes long and an odd number is not
GEOMS = {1: (1, 1), 2: (1, 2), 4: (2, 2), 9: (3, 3), 16: (4, 4), 25: (5, 5), 64: (8, 8), 81: (9, 9), 225: (15, 15), 256: (16, 16),
         1024: (32, 32), 4096: (64, 64), 16384: (128, 128)}
THIRD_LEVEL_STRIDE = 2048 * 8192     # scalar 1: 2049 chunks, 129 groups -- the third chain level
FULL_CHAIN_STRIDE = 16383 * 8192     # scalar 1: 16384 chunks, 1024 groups, 64 super-groups -- all that k_index_chain holds
TOO_MANY_STRIDE = 16383 * 8192 + 256  # scalar 1: 16385 chunks, the first count k_index_chain holds no groups for -- the serial walk
COEF_BOUND = 14            # build_chain's data bytes: see there
MAX_PAYLOAD = 12 << 20


def shapes(ns):
    """(luma shape, chroma shape, y_slices, x_slices) of the smallest picture of ns slices"""
    ys, xs = GEOMS[ns]
    return (4 * ys, 4 * xs), (2 * ys, 2 * xs), ys, xs


def _ns_for(n):
    return min(k for k in GEOMS if k >= n)


# ---------------------------------------------------------------------------------------------------------------------
# payloads from length bytes
# ---------------------------------------------------------------------------------------------------------------------
def build_chain(ns, prefix, scalar, lens, seed):
    """payload bytes of ns slices: prefix bytes, an index byte in 0..31, three length bytes each followed by length * scalar
    data bytes.  Every byte that is neither index nor length is seeded random with bits 3 and 4 set: it is never zero (a
    read at a wrong place shows), and with two adjacent ones in every byte an exp-Golomb code meets a one in a follow
    position after at most three data bits -- |coefficient| <= 14, no code near 32 bits, no escape on any decoder form."""
    lens = np.asarray(lens, np.int64).reshape(ns, 3)
    assert lens.min() >= 0 and lens.max() <= 255
    size = prefix + 4 + scalar * lens.sum(axis=1)
    start = np.concatenate([[0], np.cumsum(size)])
    rng = np.random.default_rng(seed)
    pay = rng.integers(0, 256, int(start[-1]), dtype=np.uint8) | np.uint8(0x18)
    s = start[:-1]
    pay[s + prefix] = rng.integers(0, 32, ns, dtype=np.uint8)
    p0 = s + prefix + 1
    p1 = p0 + 1 + lens[:, 0] * scalar
    p2 = p1 + 1 + lens[:, 1] * scalar
    for p, c in ((p0, 0), (p1, 1), (p2, 2)):
        pay[p] = lens[:, c].astype(np.uint8)
    return pay.tobytes()


def walk(payload, length, ns, prefix, scalar):
    """the plain walk, as k_index_serial does it: the offset of every slice and the end of the last one (designed payloads
    hold every slice whole, so the walk never leaves them)"""
    pos, out = 0, np.empty(ns, np.int64)
    for k in range(ns):
        out[k] = pos
        q = pos + prefix + 1
        for _ in range(3):
            q += 1 + (payload[q] * scalar if q < length else 0)
        pos = q
    return out, pos


# ---------------------------------------------------------------------------------------------------------------------
# chain generators
# ---------------------------------------------------------------------------------------------------------------------
Input = namedtuple("Input", "name tag prefix scalar ns lens seed info")    # info: what the design aimed at (positions)
MIXED = (0, 0, 1, 3, 17, 254, 255)


def _split(units, rng):
    """total length units per slice (0..765) -> three length bytes, seeded"""
    u = np.asarray(units, np.int64)
    a = rng.integers(np.maximum(0, u - 510), np.minimum(255, u) + 1)
    r = u - a
    b = rng.integers(np.maximum(0, r - 255), np.minimum(255, r) + 1)
    return np.stack([a, b, r - b], axis=1)


def _fit(dist, n, P, s):
    """length units that make n slices exactly dist bytes long, or None"""
    r = dist - n * P
    if n <= 0 or r < 0 or r % s or r // s > 765 * n:
        return None
    return r // s


def _spread(units, n):
    return [units // n + 1] * (units % n) + [units // n] * (n - units % n)


def _fill(dist, P, s):
    """units per slice of the fewest slices that are exactly dist bytes long together, or None (distance not reachable)"""
    if dist == 0:
        return []
    n0 = max(1, -(-dist // (P + 765 * s)))
    for n in range(n0, min(n0 + s + 1, dist // P + 1)):
        u = _fit(dist, n, P, s)
        if u is not None:
            return _spread(u, n)
    return None


def _finish(pl, name, tag, units, seed, ns, info):
    """the designed slices first, seeded `mixed` slices behind them up to a picture's slice count"""
    rng = np.random.default_rng(seed)
    ns = ns or _ns_for(len(units) + 4)
    assert len(units) <= ns, f"{name} {tag}: {len(units)} designed slices, {ns} in the picture"
    lens = np.concatenate([_split(units, rng).reshape(-1, 3), rng.choice(MIXED, (ns - len(units), 3))])
    return Input(name, tag, pl.prefix, pl.scalar, ns, lens, seed, info)


def gen_min(pl, seed, ns=None):
    """all lengths 0: at least two chunks full of minimal slices (the count field of a table entry)"""
    P = pl.prefix + 4
    ns = ns or _ns_for(-(-2 * pl.CH // P))
    return [Input("min", "all 0", pl.prefix, pl.scalar, ns, np.zeros((ns, 3), np.int64), seed, {})]


def gen_max(pl, seed, ns=None):
    ns = ns or 64
    return [Input("max", "all 255", pl.prefix, pl.scalar, ns, np.full((ns, 3), 255, np.int64), seed, {})]


def gen_mixed(pl, seed, ns=None):
    ns = ns or (1024 if pl.E <= 8191 else 256)
    rng = np.random.default_rng(seed)
    return [Input("mixed", "seeded", pl.prefix, pl.scalar, ns, rng.choice(MIXED, (ns, 3)), seed, {})]


def _target(pl, pos, kmin, d, mult=1):
    """a slice start at k * CH + d for the first k >= kmin (a multiple of mult) that the chain can reach from pos exactly;
    where gcd(prefix + 4, scalar) forbids every such start, the nearest reachable one below or above (the tag says so).
    -> (k, target, units of the slices from pos to it, note)"""
    P, s = pl.prefix + 4, pl.scalar
    g = math.gcd(P, s)
    k0 = -(-kmin // mult) * mult
    for kk in range(k0, k0 + (4 * g + 4) * mult, mult):
        t = kk * pl.CH + d
        if t % g == 0:
            f = _fill(t - pos, P, s)
            if f is not None:
                return kk, t, f, ""
    want = k0 * pl.CH + d
    for t in sorted((want // g * g, want // g * g + g), key=lambda t: (abs(t - want), t)):
        f = _fill(t - pos, P, s)
        if f is not None:
            return k0, t, f, f" nearest {t - want:+d}"
    raise AssertionError(f"no reachable start near {want} for prefix {pl.prefix} scalar {s}")


LANDINGS = ("end_b", "end_bG", "max_bG", "min_bG")


def _land_units(pl, k0, mult=1, which=LANDINGS):
    """the landings on successive boundaries k * CH, k a multiple of mult, from k0 on -> (units, info, notes)"""
    P, s, G = pl.prefix + 4, pl.scalar, pl.G
    units, pos, kmin, info, notes = [], 0, k0, {}, ""
    for what, d, extra in (("end_b", 0, None), ("end_bG", G, None), ("max_bG", -G, 765), ("min_bG", -G, 0)):
        if what not in which:
            continue
        k, t, f, note = _target(pl, pos, kmin, d, mult)
        units += f
        pos = t
        if extra is not None:
            units.append(extra)
            pos += P + s * extra
        info[what] = (k * pl.CH, t)
        notes += f" {what}{note}" if note else ""
        kmin = k + max(2, mult)
    return units, info, notes


def gen_land(pl, seed, ns=None):
    """on successive chunk boundaries b: a slice ending exactly at b; one ending at b + G; a maximal slice starting at b - G;
    a minimal slice starting at b - G"""
    units, info, notes = _land_units(pl, 1)
    return [_finish(pl, "land", "four landings" + notes, units, seed, ns, info)]


def _end_at(pl, seed, ns, tail, deltas):
    """ns slices, seeded `mixed` ones and then a run that ends on a chunk boundary + d for the first d of deltas that can be
    reached, then `tail` minimal slices -> (lens, boundary, d) or None"""
    P, s = pl.prefix + 4, pl.scalar
    rng = np.random.default_rng(seed)
    body = rng.choice(MIXED, (ns, 3))
    for d in deltas:
        for nfill in range(4, ns - tail):
            nb = ns - tail - nfill
            pos = int((P + s * body[:nb].sum(axis=1)).sum())
            for k in range(max(1, -(-(pos + nfill * P) // pl.CH)), (pos + nfill * (P + 765 * s)) // pl.CH + 1):
                u = _fit(k * pl.CH + d - pos, nfill, P, s)
                if u is not None:
                    lens = np.concatenate([body[:nb], _split(_spread(u, nfill), rng), np.zeros((tail, 3), np.int64)])
                    return lens, k * pl.CH, d
    return None


def gen_end(pl, seed, ns=None):
    """one payload ending exactly on a chunk boundary, one ending one minimal slice behind a boundary.  The slice count
    fixes (prefix + 4) * ns, and with it which lengths the chain can reach: each payload takes the first count of 256 (64
    from E = 8192 on), 225, 81, 25, 9 that lets it end where it should.  With a given count, or where no count does, the
    nearest reachable end, and the tag says so."""
    s = pl.scalar
    base = 256 if pl.E <= 8191 else 64
    counts = [ns] if ns else [base] + [k for k in (225, 81, 25, 9) if k < base]
    out = []
    for tag, tail in (("ends on a boundary", 0), ("ends one minimal slice behind a boundary", 1)):
        found = None
        for n in counts:
            found = _end_at(pl, seed, n, tail, (0,))
            if found:
                break
        if not found:
            n = counts[0]
            found = _end_at(pl, seed, n, tail, sorted(range(-s, s + 1), key=lambda d: (abs(d), d)))
        assert found, f"end: no boundary reachable for prefix {pl.prefix} scalar {s}"
        lens, b, d = found
        tag += f" nearest {d:+d}" if d else ""
        out.append(Input("end", tag, pl.prefix, s, n, lens, seed, {"boundary": b, "tail": tail, "delta": d}))
    return out


def gen_short(pl, seed, ns=None):
    """a whole payload shorter than E: one chunk, every entry walk leaves it at once or never"""
    P, s = pl.prefix + 4, pl.scalar
    ns = ns or max(k for k in GEOMS if k * P < pl.E and k <= 64)
    assert ns * P < pl.E, f"short: {ns} slices of {P} bytes are not shorter than E = {pl.E}"
    u = min((pl.E - 1 - ns * P) // s, 765 * ns)
    rng = np.random.default_rng(seed)
    return [Input("short", f"{ns * P + s * u} bytes", pl.prefix, s, ns, _split(_spread(u, ns), rng), seed, {})]


def gen_groups(pl, seed, ns=None):
    """a payload over group boundaries (16 chunks each) with the four landings of `land` on successive ones.  Where
    gcd(prefix + 4, scalar) lets the chain reach only every seventh of them -- (633, 42) -- four landings would make 17 MB:
    there a slice ending exactly on one and a maximal slice that starts G before a later one, and the tag says so."""
    units, info, notes = _land_units(pl, IDX_GROUP, IDX_GROUP)
    tag = "four landings on group boundaries"
    if max(t for _, t in info.values()) + pl.E > MAX_PAYLOAD * 3 // 4:
        units, info, notes = _land_units(pl, IDX_GROUP, IDX_GROUP, ("end_b", "max_bG"))
        tag = "two landings on group boundaries"
    return [_finish(pl, "groups", tag + notes, units, seed, ns, info)]


GENERATORS = {"min": gen_min, "max": gen_max, "mixed": gen_mixed, "land": gen_land, "end": gen_end, "short": gen_short,
              "groups": gen_groups}
SEED = 36


def inputs(prefix, scalar, name, ns=None, seed=SEED):
    """the designed inputs of one generator on one row (the plan of the chunk geometry: the stride plays no part in it)"""
    return GENERATORS[name](plan(prefix, scalar, 0), seed, ns)


def payload_of(inp):
    return build_chain(inp.ns, inp.prefix, inp.scalar, inp.lens, inp.seed)


def slot_stride(length):
    """the slot vc2hip_hq_unpack gives a payload"""
    return (length + 63) & ~63


# ---------------------------------------------------------------------------------------------------------------------
# the kernels, transcribed
# ---------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "nx15": "nx kept in 15 bits",
    "exit14": "exit offset masked to 14 bits",
    "cnt4095": "count field saturating at 4095",
    "lim_gt": "the boundary test n > lim for n >= lim",
    "drop_last_entry": "the entry at EU - 1 dropped",
    "ept": "EPT one too small",
    "group15": "group composition stopping at 15 chunks",
    "super_skip_last": "super-group expansion skipping the last group",
    "gsh_exits": "gsh applied to exits",
}


class Stuck(Exception):
    """a walk that does not advance: the kernel would never end"""


def _hops(nx, pos, cnt, stop, gsh):
    """every walk of pos[] goes on through nx[] until it stands at `stop` or beyond"""
    idx = np.nonzero(pos < stop)[0]
    while idx.size:
        new = nx[pos[idx] >> gsh]
        if (new <= pos[idx]).any():       # (a right nx[] leads forward: a slice is at least four bytes long)
            raise Stuck
        pos[idx] = new
        cnt[idx] += 1
        idx = idx[new < stop]


def _pack(exit_, cnt, mut):
    if mut == "exit14":
        exit_ = exit_ & 0x3FFF
    if mut == "cnt4095":
        cnt = np.minimum(cnt, 4095)
    return ((exit_.astype(np.int64) << 16 | cnt) & 0xFFFFFFFF).astype(np.uint32)


def _tables(pay, plen, pl, c, mut, st):
    """k_index_tables_nx for chunk c: the table words of its EU entries"""
    CH, E, EU, gsh, prefix, scalar = pl.CH, pl.E, pl.EU, pl.gsh, pl.prefix, pl.scalar
    nbytes, NP, c0 = (CH + E + 16 + 15) & ~15, CH >> gsh, c * CH
    buf = np.zeros(nbytes, np.uint8)
    seg = pay[c0:min(plen, c0 + nbytes)]
    buf[:seg.size] = seg
    lim = min(CH, plen - c0)
    q = (np.arange(NP, dtype=np.int64) << gsh) + prefix + 1
    for _ in range(3):
        q = q + 1 + buf[np.minimum(q, nbytes - 1)].astype(np.int64) * scalar
    out = q > lim if mut == "lim_gt" else q >= lim
    n = np.where(out, np.where(q >= CH, q, CH), q)
    nx = n & (0x7FFF if mut == "nx15" else 0xFFFF)                      # unsigned short nx[]
    st["max_nx"] = max(st["max_nx"], int(n[:(lim + pl.G - 1) >> gsh].max()))
    e = np.arange(EU, dtype=np.int64)
    tab = np.zeros(EU, np.uint32)                                        # (what an unwritten word holds is anyone's guess)
    if not pl.merge:
        pos, cnt = e << gsh, np.zeros(EU, np.int64)
        pos[pos >= lim] = CH
        _hops(nx, pos, cnt, CH, gsh)
        tab[:] = _pack(pos - CH, cnt, mut)
        if mut == "drop_last_entry":
            tab[EU - 1] = 0
        return tab
    ept = pl.EPT - (1 if mut == "ept" else 0)
    mine = e < pl.threads * ept                                          # the entries some thread holds
    if mut == "drop_last_entry":
        mine &= e < EU - 1
    la, ca = np.full(EU, CH, np.int64), np.zeros(EU, np.int64)
    live = mine & ((e << gsh) < lim)
    pos, cnt = (e << gsh)[live], np.zeros(int(live.sum()), np.int64)
    _hops(nx, pos, cnt, E, gsh)
    la[live], ca[live] = pos, cnt
    inside = la < CH
    t = np.unique((la[inside] - E) >> gsh)                               # need[] / list[]
    assert t.size == 0 or t.max() < EU
    st["landings"] = max(st["landings"], int(t.size))
    W = np.zeros(EU, np.uint32)
    pos, cnt = E + (t << gsh), np.zeros(t.size, np.int64)
    _hops(nx, pos, cnt, CH, gsh)
    W[t] = _pack(pos - CH, cnt, mut)
    word = np.where(inside, (W[np.where(inside, (la - E) >> gsh, 0)].astype(np.int64) + ca) & 0xFFFFFFFF,
                    _pack(la - CH, ca, mut).astype(np.int64)).astype(np.uint32)
    if mut == "cnt4095":
        word = (word & 0xFFFF0000) | np.minimum(word & 0xFFFF, 4095)
    tab[mine] = word[mine]
    return tab


def _compose(X, Y, n_in, n_out, span, plen, pl, mut, st):
    """k_index_group: out[g] = in[16 g + 15] o ... o in[16 g]; X exits (bytes), Y slices, one row per input function"""
    EU, gsh = pl.EU, pl.gsh
    members = IDX_GROUP - 1 if mut == "group15" else IDX_GROUP
    OX, OY = np.zeros((n_out, EU), np.int64), np.zeros((n_out, EU), np.int64)
    for g in range(n_out):
        if g * IDX_GROUP * span >= plen:
            continue
        c0 = g * IDX_GROUP
        if not pl.dedupe:
            x, cnt = np.arange(EU, dtype=np.int64) << gsh, np.zeros(EU, np.int64)
            for k in range(members):
                c = c0 + k
                if c >= n_in or c * span >= plen:
                    break
                i = x >> gsh
                x, cnt = X[c][i], cnt + Y[c][i]
            OX[g], OY[g] = x, cnt
            continue
        x1 = X[c0] >> gsh
        uniq = np.unique(x1)
        st["exits"] = max(st["exits"], int(uniq.size))
        x, cnt = uniq.copy(), np.zeros(uniq.size, np.int64)
        for k in range(1, members):
            c = c0 + k
            if c >= n_in or c * span >= plen:
                break
            x, cnt = X[c][x] >> gsh, cnt + Y[c][x]
        rx, ry = np.zeros(EU, np.int64), np.zeros(EU, np.int64)
        rx[uniq], ry[uniq] = x << gsh, cnt
        OX[g], OY[g] = rx[x1], Y[c0] + ry[x1]
    return OX, OY


def emulate(payload, length, pl, ns, mut=None, stats=None):
    """the offsets vc2_launch_slice_index writes for one picture slot (0xFFFFFFFF where it writes none), and per live chunk
    the table word (exit, slices) the chain took.  stats, if given, receives what trace() reports of the tables."""
    assert mut is None or mut in MUTANTS
    st = stats if stats is not None else {}
    st.update(max_nx=0, landings=0, exits=0)
    pay = np.frombuffer(payload, np.uint8)
    plen = min(length, pl.stride)
    offs = np.full(ns, 0xFFFFFFFF, np.int64)
    if pl.kind == "serial":
        w, _ = walk(payload, plen, ns, pl.prefix, pl.scalar)
        return w, []
    CH, EU, gsh = pl.CH, pl.EU, pl.gsh
    live = min(-(-plen // CH), pl.n_chunks)
    tabs = np.zeros((live, EU), np.uint32)
    for c in range(live):
        tabs[c] = _tables(pay, plen, pl, c, mut, st)
    TX, TY = (tabs >> 16).astype(np.int64), (tabs & 0xFFFF).astype(np.int64)
    lg = min(-(-live // IDX_GROUP), pl.n_groups)
    GX, GY = _compose(TX, TY, live, lg, CH, plen, pl, mut, st)
    if pl.n_supers:
        SX, SY = _compose(GX, GY, lg, -(-lg // IDX_GROUP), CH * IDX_GROUP, plen, pl, mut, st)
    # k_index_chain
    gspan = IDX_GROUP * CH
    sspan = gspan * IDX_GROUP
    g_entry = np.zeros((pl.n_groups, 2), np.int64)
    if pl.n_supers == 0:
        entry = base = 0
        for g in range(pl.n_groups):
            g_entry[g] = entry, base
            if g * gspan >= plen:
                continue
            entry, base = GX[g][entry >> gsh], base + GY[g][entry >> gsh]
    else:
        s_entry = np.zeros((pl.n_supers, 2), np.int64)
        entry = base = 0
        for sg in range(pl.n_supers):
            s_entry[sg] = entry, base
            if sg * sspan >= plen:
                continue
            entry, base = SX[sg][entry >> gsh], base + SY[sg][entry >> gsh]
        for sg in range(pl.n_supers):
            entry, base = s_entry[sg]
            for k in range(IDX_GROUP - 1 if mut == "super_skip_last" else IDX_GROUP):
                g = sg * IDX_GROUP + k
                if g >= pl.n_groups:
                    break
                g_entry[g] = entry, base
                if g * gspan >= plen:
                    continue
                entry, base = GX[g][entry >> gsh], base + GY[g][entry >> gsh]
    taken = []
    for g in range(lg):
        entry, base = g_entry[g]
        for k in range(IDX_GROUP):
            c = g * IDX_GROUP + k
            if c >= live:
                break
            t = int(tabs[c][(entry >> gsh) % EU]) if entry >> gsh < EU else 0
            taken.append((t >> 16, t & 0xFFFF))
            # k_index_emit for chunk c
            if base < ns and entry < CH:
                pos, k2, end = c * CH + int(entry), int(base), (c + 1) * CH
                while pos < end and k2 < ns:
                    offs[k2] = pos
                    if pos >= plen:
                        break
                    q = pos + pl.prefix + 1
                    for _ in range(3):
                        q += 1 + (int(pay[q]) * pl.scalar if q < plen else 0)
                    pos, k2 = q, k2 + 1
            entry, base = t >> 16, base + (t & 0xFFFF)
            if mut == "gsh_exits":
                entry >>= gsh
    return offs, taken


def chunk_functions(starts, end, pl):
    """per live chunk of a whole chain (slice starts, end of the last slice): (exit offset, slices started in it), the word
    the chain must take from that chunk's table"""
    out = []
    for c in range(-(-end // pl.CH)):
        lo, hi = c * pl.CH, (c + 1) * pl.CH
        inside = starts[(starts >= lo) & (starts < hi)]
        nxt = starts[starts >= hi]
        first_after = int(nxt[0]) if nxt.size else end
        out.append((max(first_after - hi, 0), int(inside.size)))
    return out


def trace(payload, length, pl, ns):
    """what an input reaches: the exits the chain takes, the largest nx, the fullest chunk, the groups and super-groups it
    crosses, the distinct landing positions of the merged walks and the distinct exits of the deduped composition"""
    starts, end = walk(payload, length, ns, pl.prefix, pl.scalar)
    fn = chunk_functions(starts, end, pl)
    sizes = np.diff(np.concatenate([starts, [end]]))
    reach = starts % pl.CH + sizes                       # chunk-relative position a slice reaches: nx where it leaves
    leaving = reach[reach >= pl.CH]
    bounds = np.arange(1, -(-end // pl.CH)) * pl.CH
    st = {}
    if pl.kind == "tables":
        emulate(payload, length, pl, ns, stats=st)
    return dict(exits=sorted({x for x, _ in fn[:-1]}), exit0=bool(np.isin(bounds, starts).any()),
                exit_max=bool(any(x == pl.E - pl.G for x, _ in fn)), max_nx_chain=int(leaving.max()) if leaving.size else 0,
                max_nx=st.get("max_nx", 0), max_count=max(n for _, n in fn), chunks=len(fn),
                groups=-(-len(fn) // IDX_GROUP), supers=-(-len(fn) // (IDX_GROUP * IDX_GROUP)),
                end_on_boundary=end % pl.CH == 0, landings=st.get("landings", 0), distinct_exits=st.get("exits", 0),
                length=end)
