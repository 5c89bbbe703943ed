"""A CPU model of what the HQ_CBR quantiser search kernels decide (vc2_launch_cbr, csrc/vc2hip_slices.hip), in numpy and
the oracle only: which of the five kernels takes a geometry, and, per slice, the facts of the search -- the threshold T,
the trials the reference's bisection visits, the index after the refinement by the luma error, the class of slice the
register kernels hand back, and where the last non-zero quantised coefficient of every component lies at T.

tests/test_cbr_ref.py asserts, without a GPU, that every input of tests/test_gpu_cbr_search.py reaches what its row
claims; the GPU file compares the library with the oracle on those inputs, byte for byte.

Quantised values come from oracle.quantise_np / dequantise_np with ONE index for the whole plane, code lengths from the
closed form of the signed exp-Golomb code (VLC.cpp:78-85); nothing here is taken from the kernels' arithmetic.  What IS
restated from the library is its control flow: the `reg` condition and the LDS limit of vc2_launch_cbr, cbr16_plan, the
16-bit store's rule (use_store16, csrc/vc2hip_api.hip) and the walk of k_cbr_search_reg over CBR_SPW consecutive slices
(bisection for the first, gallop from the predecessor's threshold for the others), so that a row can say which slices
the register pass marks."""
from dataclasses import dataclass, field, replace

import numpy as np

from synth import noise_frame, synth
from vc2lib import KERNELS, make_params

CBR_SPW = 8            # consecutive slices per wavefront of the register kernels
REG_MAX_INDEX = 79     # adjusted indices beyond it leave the float domain of the register kernels
LDS_BYTES = 160 * 1024
CLASSES = ("escape", "index", "length", "none")
POSITIONS = ("none", "head", "first", "last", "mid")


# ------------------------------------------------------------------------------------------
# geometry: which kernel
# ------------------------------------------------------------------------------------------
@dataclass
class Geometry:
    """planes of lh x lw (luma) and ch x cw (both chroma components), padded; ys x xs slices"""
    lh: int
    lw: int
    ch: int
    cw: int
    depth: int
    ys: int
    xs: int

    @property
    def n_slices(self):
        return self.ys * self.xs

    @property
    def n_bands(self):
        return 3 * self.depth + 1

    def slice_dims(self, c):
        h, w = (self.lh, self.lw) if c == 0 else (self.ch, self.cw)
        return h // self.ys, w // self.xs

    @property
    def comp_n(self):
        return [self.slice_dims(c)[0] * self.slice_dims(c)[1] for c in range(3)]

    @property
    def comp_n0(self):
        return [(self.slice_dims(c)[0] >> self.depth) * (self.slice_dims(c)[1] >> self.depth) for c in range(3)]

    @property
    def comp_off(self):
        n = self.comp_n
        return [0, n[0], n[0] + n[1]]

    @property
    def slice_coefs(self):
        return sum(self.comp_n)

    def band_sizes(self, c):
        n0 = self.comp_n0[c]
        return [n0 if b == 0 else n0 << (2 * ((b - 1) // 3)) for b in range(self.n_bands)]


def picture_geometry(oracle, w, h, cf, depth, u, a):
    """the geometry of a w x h picture coded with the reference's -u / -a slice sizes"""
    ch = h // 2 if cf == "420" else h
    cw = w if cf == "444" else w // 2
    lh, lw = oracle.padded_size(h, depth), oracle.padded_size(w, depth)
    pch, pcw = oracle.padded_size(ch, depth), oracle.padded_size(cw, depth)
    ys = oracle.lib.vc2o_slice_size_is_valid(depth, h, ch, u)
    xs = oracle.lib.vc2o_slice_size_is_valid(depth, w, cw, a)
    assert ys and xs, (w, h, cf, depth, u, a)
    return Geometry(lh, lw, pch, pcw, depth, ys, xs)


def store16(g):
    """use_store16: every level of every component runs through the fast level kernels (tiles of 32 x 128 samples: slice
    footprints that are powers of two from 2 up to the tile, planes of at least one tile and a multiple of 8 samples
    wide at every level) and every component record moves eight coefficients at a time"""
    off = g.comp_off
    for c in range(3):
        sh, sw = g.slice_dims(c)
        if (sh * sw) % 8 or off[c] % 8:
            return False
    if g.slice_coefs % 8:
        return False
    for level in range(g.depth):
        for c in range(3):
            sh, sw = g.slice_dims(c)
            ph, pw = (g.lh, g.lw) if c == 0 else (g.ch, g.cw)
            fh, fw, ih, iw = sh >> level, sw >> level, ph >> level, pw >> level
            if fh & (fh - 1) or fw & (fw - 1) or fh > 32 or fw > 128 or fh < 2 or fw < 2:
                return False
            if ih < 32 or iw < 128 or iw & 7:
                return False
    return True


def cbr16_plan(g, qm, is16):
    """cbr16_plan (csrc/vc2hip_cbr16.h), whole: (headY, headC, runsY, runsC) or None where it refuses"""
    n, n0, off = g.comp_n, g.comp_n0, g.comp_off
    if not is16 or n[1] != n[2] or n0[1] != n0[2]:
        return None
    if g.slice_coefs & 7 or (g.n_slices * g.slice_coefs) & 7:
        return None
    heads, runs = [], []
    for c in range(3):
        if n[c] <= 0 or n0[c] <= 0 or off[c] & 7:
            return None
        start, head = 0, -1
        for b, size in enumerate(g.band_sizes(c)):
            if qm[b] < 0 or qm[b] > 255:
                return None
            if head < 0 and size & 7 == 0 and start & 7 == 0:
                head = start
            if head < 0:
                if start + size > (32 if c == 0 else 16):
                    return None
            else:
                for j in range(start, start + size, 8):
                    run = (j - head) // 8
                    if c == 0:
                        if run >= 64:
                            return None
                    elif 2 * ((n[c] - head) // 8) > 64:
                        return None
            start += size
        if start != n[c]:
            return None
        if head < 0:
            head = n[c]
        if head & 7:
            return None
        heads.append(head)
        runs.append((n[c] - head) // 8)
    if heads[1] != heads[2] or runs[1] != runs[2]:
        return None
    if runs[0] < 40 or runs[1] < 20:      # small slices: the lanes would idle
        return None
    return heads[0], heads[1], runs[0], runs[1]


def kernel_for(g, qm, is16, general_only=False):
    """(name, (headY, headC, runsY, runsC) or None): the kernel of vc2_launch_cbr's FIRST launch.  The register kernels
    are followed by the general one (LDS or global, by the same limit) over the slices they marked."""
    n, off = g.comp_n, g.comp_off
    reg = (not general_only and n[0] <= 512 and n[1] <= 256 and n[1] == n[2] and g.n_bands <= 32 and n[0] % 8 == 0
           and n[1] % 8 == 0 and (g.n_slices * g.slice_coefs) % 8 == 0 and g.slice_coefs % 8 == 0
           and off[1] % 8 == 0 and off[2] % 8 == 0)
    if reg:
        plan = cbr16_plan(g, qm, is16)
        if plan:
            return "search16", plan
        return ("reg16" if is16 else "reg32"), None
    per_wave = g.slice_coefs * 4 + 32 * 16
    return ("global" if per_wave + 768 > LDS_BYTES else "general"), None


def heads(g):
    """(head, runs) of every component in cbr16_plan's sense -- the leading subbands whose blocks are not whole runs of
    eight -- without the plan's lane limits: the last-non-zero positions are named by it on every kernel"""
    out = []
    for c in range(3):
        start, head = 0, -1
        for size in g.band_sizes(c):
            if head < 0 and size & 7 == 0 and start & 7 == 0:
                head = start
            start += size
        if head < 0:
            head = g.comp_n[c]
        out.append((head, (g.comp_n[c] - head) // 8))
    return out


# ------------------------------------------------------------------------------------------
# slices in coding order
# ------------------------------------------------------------------------------------------
def coding_order(sh, sw, depth):
    """flat positions (y * sw + x) of a slice's coefficients in coding order, and the subband of each
    (WaveletTransform.cpp:428-450: LL, then HL, LH, HH per level, coarsest first)"""
    pos, band = [], []
    for b in range(3 * depth + 1):
        if b == 0:
            s, oy, ox = 1 << depth, 0, 0
        else:
            level, kind = (b - 1) // 3 + 1, (b - 1) % 3
            s = 1 << (depth + 1 - level)
            o = s // 2
            oy, ox = (0 if kind == 0 else o), (0 if kind == 1 else o)
        yy, xx = np.mgrid[oy:sh:s, ox:sw:s]
        p = (yy * sw + xx).ravel()
        pos.append(p)
        band.append(np.full(p.size, b, np.int32))
    return np.concatenate(pos), np.concatenate(band)


def slice_records(plane, ys, xs, depth):
    """(ys * xs, sh * sw): every slice's coefficients in coding order"""
    ph, pw = plane.shape
    sh, sw = ph // ys, pw // xs
    pos, _ = coding_order(sh, sw, depth)
    t = plane.reshape(ys, sh, xs, sw).transpose(0, 2, 1, 3).reshape(ys * xs, sh * sw)
    return t[:, pos]


def planes_from_records(g, recs):
    """the inverse of slice_records for the three components: coefficient planes that hold the given records"""
    out = []
    for c in range(3):
        sh, sw = g.slice_dims(c)
        pos, _ = coding_order(sh, sw, g.depth)
        t = np.zeros((g.n_slices, sh * sw), np.int32)
        t[:, pos] = recs[c]
        out.append(np.ascontiguousarray(t.reshape(g.ys, g.xs, sh, sw).transpose(0, 2, 1, 3).reshape(g.ys * sh, g.xs * sw)))
    return out


def _svlc_bits_exact(mag):
    e = np.frexp((mag.astype(np.int64) + 1).astype(np.float64))[1] - 1   # exact below 2^53
    return np.where(mag == 0, 1, 2 * e + 2).astype(np.int32)


_BITS16 = _svlc_bits_exact(np.arange(1 << 16))


def _svlc_bits(mag):
    """SignedVLC bits of |v| (VLC.cpp:78-85): 1 for 0, else 2 floor(log2(|v| + 1)) + 2"""
    return _BITS16[mag] if int(mag.max(initial=0)) < 1 << 16 else _svlc_bits_exact(mag)


# ------------------------------------------------------------------------------------------
# the search's facts
# ------------------------------------------------------------------------------------------
@dataclass
class Model:
    g: Geometry
    qm: np.ndarray
    scalar: int
    avail: np.ndarray            # per slice: its bytes less the four of the header
    units: np.ndarray            # [128, slices, 3] length units (bytes / scalar) of every component at every index; -1: no such index
    last: np.ndarray             # [128, slices, 3] coding-order position of the last non-zero quantised coefficient, -1: none
    escape: np.ndarray           # per slice: some |coefficient| above 32767
    yss_of: object               # index -> per-slice luma error (None where the oracle refuses the index)
    T: np.ndarray = None
    trials: list = None          # per slice: the reference's trials, in order
    error: list = None           # per slice: None, "index" or "scalar": what the reference raises on its walk
    final: np.ndarray = None     # per slice: the index after the refinement (-1 where the reference raises)
    refine_trials: list = None
    cls: list = None
    marked: np.ndarray = None    # per slice: the register pass hands it back
    why: list = None             # ... and why: escape / index / length / None
    guess: np.ndarray = None     # per slice: the threshold the register walk started from (-1: bisection)
    pos: list = field(default_factory=list)   # per slice: (Y, U, V) position names at T

    @property
    def qm_min(self):
        return int(self.qm.min())

    def need(self, q, s):
        return int(self.units[q, s].sum()) * self.scalar

    def valid(self, q):
        return q - self.qm_min <= 119


def build_tables(oracle, g, planes, qm, scalar, slice_bytes):
    qm = np.ascontiguousarray(qm, np.int32)
    ns = g.n_slices
    recs = [slice_records(p, g.ys, g.xs, g.depth) for p in planes]
    escape = np.zeros(ns, bool)
    for r in recs:
        escape |= (np.abs(r.astype(np.int64)) > 32767).any(axis=1)
    units = np.zeros((128, ns, 3), np.int32)
    last = np.full((128, ns, 3), -1, np.int32)
    qmin = int(qm.min())
    all_zero = False
    for q in range(128):
        if q - qmin > 119:
            units[q] = -1
            continue
        if all_zero:
            continue               # a zero stays a zero under a larger factor
        qi = np.full((g.ys, g.xs), q, np.int32)
        all_zero = True
        for c in range(3):
            quant = oracle.quantise_np(planes[c], g.depth, qi, qm)
            mag = np.abs(slice_records(quant, g.ys, g.xs, g.depth))
            nz = mag != 0
            if not nz.any():
                continue
            all_zero = False
            ends = np.cumsum(_svlc_bits(mag), axis=1, dtype=np.int32)
            n = mag.shape[1]
            lastpos = np.where(nz.any(axis=1), n - 1 - np.argmax(nz[:, ::-1], axis=1), -1)
            count = np.where(lastpos >= 0, ends[np.arange(ns), np.maximum(lastpos, 0)], 0)
            units[q, :, c] = ((count + 7) // 8 + scalar - 1) // scalar
            last[q, :, c] = lastpos
    cache = {}

    def yss_of(q):
        if q not in cache:
            if q - qmin > 119:
                cache[q] = None
            else:
                qi = np.full((g.ys, g.xs), q, np.int32)
                rec = oracle.dequantise_np(oracle.quantise_np(planes[0], g.depth, qi, qm), g.depth, qi, qm)
                d = (planes[0].astype(np.int64) - rec.astype(np.int64)).astype(np.int32).astype(np.int64)
                sq = (d * d).astype(np.int32).astype(np.int64)   # the reference squares in int and sums in long long
                sh, sw = g.slice_dims(0)
                cache[q] = sq.reshape(g.ys, sh, g.xs, sw).sum(axis=(1, 3)).ravel()
        return cache[q]

    avail = np.ascontiguousarray(slice_bytes, np.int32).ravel().astype(np.int64) - 4
    return Model(g, qm, scalar, avail, units, last, escape, yss_of)


def reference_walk(m, s):
    """the bisection of quantIndicesCBR (EncodeStream.cpp:88-104) on slice s: (trials, q, error)"""
    trial, q, delta, trials = 63, 127, 64, []
    while delta > 0:
        delta >>= 1
        trials.append(trial)
        if not m.valid(trial):
            return trials, q, "index"
        if (m.units[trial, s] > 255).any():
            return trials, q, "scalar"
        if m.need(trial, s) <= m.avail[s]:
            q = min(q, trial)
            trial -= delta
        else:
            trial += delta
    return trials, q, None


def refine(m, s, q, limit=None):
    """the refinement by the luma error (EncodeStream.cpp:106-121): (final index or -1, trials, error).  limit: the
    register kernels' domain -- a trial beyond it ends the walk with error "domain" """
    trial, trials = q, [q]
    if limit is not None and trial - m.qm_min > limit:
        return -1, trials, "domain"
    prev = m.yss_of(trial)
    if prev is None:
        return -1, trials, "index"
    prev = prev[s]
    while True:
        trial += 1
        trials.append(trial)
        if limit is not None and trial - m.qm_min > limit:
            return -1, trials, "domain"
        cur = m.yss_of(trial)
        if cur is None:
            return -1, trials, "index"
        d, prev = cur[s] - prev, cur[s]
        if d >= 0:
            return trial - 1, trials, None


def register_walk(m):
    """k_cbr_search_reg's walk (k_cbr_search16 keeps it) over every group of CBR_SPW consecutive slices, on the tables:
    which slices it marks for the general kernel, why, and the guess each started from"""
    ns = m.g.n_slices
    marked, why, guesses = np.zeros(ns, bool), [None] * ns, np.full(ns, -1, np.int32)
    lim = REG_MAX_INDEX

    def measure(t, s):   # need_bytes: the reason it turns bad, or None
        if t - m.qm_min > lim:
            return "index"
        if (m.units[t, s] > 255).any():
            return "length"
        return None

    for s0 in range(0, ns, CBR_SPW):
        guess = -1
        for s in range(s0, min(s0 + CBR_SPW, ns)):
            guesses[s] = guess
            bad = "escape" if m.escape[s] else None
            q = 127
            if bad is None and guess < 0:
                trial, delta = 63, 64
                while delta > 0 and bad is None:
                    delta >>= 1
                    bad = measure(trial, s)
                    if m.need(trial, s) <= m.avail[s]:
                        q = min(q, trial)
                        trial -= delta
                    else:
                        trial += delta
            elif bad is None:
                lo, hi, step, lowest = -1, 127, 1, 127
                t = min(guess, 126)
                while True:
                    bad = measure(t, s)
                    if bad:
                        break
                    lowest = min(lowest, t)
                    if m.need(t, s) <= m.avail[s]:
                        hi = t
                    else:
                        lo = t
                    if hi - lo <= 1:
                        break
                    if hi == 127:
                        if lo >= 126:
                            break
                        t = min(126, lo + step)
                        step *= 2
                    elif lo < 0:
                        if hi <= 0:
                            break
                        t = max(0, hi - step)
                        step *= 2
                    else:
                        t = (lo + hi) >> 1
                q = hi
                if bad is None:
                    rt, rd, rmin, rmax = 63, 64, 127, 0
                    while rd > 0:
                        rd >>= 1
                        rmin, rmax = min(rmin, rt), max(rmax, rt)
                        rt = rt - rd if rt >= q else rt + rd
                    if rmax - m.qm_min > lim:
                        bad = "index"
                    elif rmin < lowest:
                        bad = measure(rmin, s)
            if bad is None:
                _, _, err = refine(m, s, q, limit=lim)
                if err:
                    bad = "index"
            marked[s], why[s] = bad is not None, bad
            guess = -1 if bad else q
    return marked, why, guesses


def position_name(p, head, n):
    if p < 0:
        return "none"
    if p < head:
        return "head"
    if p < head + 8:
        return "first"
    if p >= n - 8:
        return "last"
    return "mid"


def analyse(oracle, g, planes, qm, scalar, slice_bytes):
    """the whole model of one call: tables, the reference's walk and refinement per slice, classes, the register walk"""
    m = build_tables(oracle, g, planes, qm, scalar, slice_bytes)
    ns = g.n_slices
    m.T = np.full(ns, 127, np.int32)
    m.trials, m.error, m.refine_trials, m.cls = [], [], [], []
    m.final = np.full(ns, -1, np.int32)
    hd = heads(g)
    for s in range(ns):
        fits = [q for q in range(127) if m.valid(q) and m.need(q, s) <= m.avail[s]]
        m.T[s] = fits[0] if fits else 127
        trials, q, err = reference_walk(m, s)
        rtr = []
        if err is None:
            m.final[s], rtr, err = refine(m, s, q)
        m.trials.append(trials)
        m.refine_trials.append(rtr)
        m.error.append(err)
        visited = trials + rtr
        if m.escape[s]:
            cls = "escape"
        elif max(visited) - m.qm_min > REG_MAX_INDEX:
            cls = "index"
        elif any(m.valid(t) and (m.units[t, s] > 255).any() for t in trials):
            cls = "length"
        else:
            cls = "none"
        m.cls.append(cls)
        t = min(int(m.T[s]), 126)
        m.pos.append(tuple(position_name(int(m.last[t, s, c]), hd[c][0], g.comp_n[c]) if m.valid(t) else "none" for c in range(3)))
    m.marked, m.why, m.guess = register_walk(m)
    return m


def first_error(m):
    """what the reference raises for the call: the first slice's error in slice order (None: it returns indices)"""
    for e in m.error:
        if e:
            return e
    return None


ERROR_TEXT = {"scalar": "Slice scalar is too small", "index": "quantization index exceeds maximum implemented value"}


def conditions(m):
    """counts of the search conditions of tests/test_cbr_ref.py over one call's slices"""
    c = {}

    def add(k, n=1):
        c[k] = c.get(k, 0) + n

    for s in range(m.g.n_slices):
        add("class:" + m.cls[s])
        if m.marked[s]:
            add("marked")
            add("marked:" + m.why[s])
        if m.error[s]:
            add("error:" + m.error[s])
        if m.T[s] == 0:
            add("T=0")
        if m.T[s] == 127 or (m.error[s] == "index" and m.T[s] > 119):
            add("T=127")
        if s % CBR_SPW and not m.marked[s]:
            if m.marked[s - 1]:
                add("after-hand-back")
            else:
                d = int(m.T[s]) - int(m.guess[s])
                a = abs(d)
                if a:
                    size = "1" if a == 1 else "2-7" if a <= 7 else "8-31" if a < 32 else "32+"
                    add(("up:" if d > 0 else "down:") + size)
                else:
                    add("same")
        tight = m.error[s] is None and 0 < m.T[s] < 127     # the bytes at T - 1 do not fit: a miscounted component moves T
        for k, name in enumerate("YUV"):
            add(f"{name}:{m.pos[s][k]}")
            if tight:
                add(f"tight:{name}:{m.pos[s][k]}")
        if m.pos[s] == ("none", "none", "head"):
            add("only-V-head")
            if tight:
                add("tight:only-V-head")
        if m.error[s] is None:
            t = int(m.T[s])
            y0, y1 = m.yss_of(t), m.yss_of(t + 1)
            if y0 is not None and y1 is not None and y0[s] == y1[s]:
                add("equal-error")
                if y0[s] != 0:
                    add("equal-error-nonzero")
            if m.final[s] - t >= 3:
                add("refined-3+")
    return c


# ------------------------------------------------------------------------------------------
# inputs: coefficient planes for the fine-grained call (exact placement)
# ------------------------------------------------------------------------------------------
FINE_GEOM = (64, 512, 64, 256, 3, 8, 16)     # 128 slices of 8 x 16 luma, 8 x 8 chroma (4:2:2), depth 3: head 8 / 16


@dataclass
class FineRow:
    name: str
    scalar: int
    kernel: str          # the kernel the default context takes
    claims: dict         # condition -> the least count this row must supply (tests/test_cbr_ref.py)
    raises: str = None   # the error the reference raises: "scalar" / "index"
    geom: tuple = FINE_GEOM
    note: str = ""


def _place(rng, n, head, where, big):
    """a component record whose last non-zero coefficient lies `where`; small values in front of it, `big` on it"""
    r = np.zeros(n, np.int32)
    if where == "none":
        return r
    at = {"head": int(rng.integers(0, head)), "first": head + int(rng.integers(0, 8)), "last": n - 1 - int(rng.integers(0, 8))}[where]
    k = int(rng.integers(0, min(at, 6) + 1))
    if k:
        r[rng.choice(at, k, replace=False)] = rng.integers(-9, 10, k)
    r[at] = big * (1 if rng.random() < 0.5 else -1)
    return r


def _position_records(g, seed, big, small_scale=1):
    """of every 128 slices, the first 64 take every combination of (none, head, first, last) over Y, U, V; the others are
    slices where only V's head, only U's head, only the luma's and only V's last run are non-zero"""
    rng = np.random.default_rng(seed)
    hd = heads(g)
    combos = [(a, b, c) for a in POSITIONS[:4] for b in POSITIONS[:4] for c in POSITIONS[:4]]
    extra = [("none", "none", "head"), ("none", "head", "none"), ("last", "none", "none"), ("none", "none", "last")]
    recs = [np.zeros((g.n_slices, g.comp_n[c]), np.int32) for c in range(3)]
    for s in range(g.n_slices):
        combo = combos[s % 128] if s % 128 < 64 else extra[s % 4]
        for c in range(3):
            where = combo[c] if hd[c][0] or combo[c] != "head" else "first"
            recs[c][s] = _place(rng, g.comp_n[c], hd[c][0], where, int(rng.integers(big, 2 * big)))
            if small_scale != 1:
                small = np.abs(recs[c][s]) < 10
                recs[c][s] = np.where(small, recs[c][s] * small_scale, recs[c][s])
    return recs


def _laplace_records(g, rng, amp, zero=0.5):
    recs = []
    for c in range(3):
        p = rng.laplace(0, amp / 3.0, size=(g.n_slices, g.comp_n[c]))
        p[rng.random(p.shape) < zero] = 0
        recs.append(np.clip(np.rint(p), -2 ** 30, 2 ** 30).astype(np.int32))
    return recs


def _scaled_records(g, seed, targets, amp0=6.0):
    """one Laplace record per component, scaled per slice by 2^(target / 4): thresholds that follow the targets"""
    rng = np.random.default_rng(seed)
    base = [rng.laplace(0, amp0, size=g.comp_n[c]) * (rng.random(g.comp_n[c]) < 0.6) for c in range(3)]
    recs = []
    for c in range(3):
        r = np.stack([base[c] * 2.0 ** (targets[s] / 4.0) + rng.normal(0, 0.3, g.comp_n[c]) * (base[c] != 0) for s in range(g.n_slices)])
        recs.append(np.clip(np.rint(r), -32767, 32767).astype(np.int32))
    return recs


GALLOP_TARGETS = [[40, 41, 40, 44, 39, 4, 40, 38], [30, 29, 30, 27, 33, 0, 36, 37], [8, 44, 43, 8, 9, 42, 47, 46], [44, 6, 7, 5, 41, 40, 2, 38]]


def _refine_luma(oracle, aq_max=60):
    """per adjusted index aq: a value c whose reconstruction error falls strictly from aq to aq + 3 (None if there is none)"""
    out = {}
    for aq in range(aq_max):
        out[aq] = None
        for c in range(3, 4000):
            e = [abs(c - oracle.scale(oracle.quant(c, a), a)) for a in range(aq, aq + 5)]
            if e[0] > e[1] > e[2] > e[3]:
                out[aq] = c
                break
    return out


def fine_input(oracle, row):
    """(geometry, [Y, U, V] coefficient planes, matrix, scalar, slice byte table) of a fine-grained row"""
    g = Geometry(*row.geom)
    qm = oracle.quant_matrix(KERNELS["DD97"], g.depth)
    ns, name, scalar = g.n_slices, row.name, row.scalar
    per = 4 + 60            # bytes per slice unless the row says otherwise
    if name == "positions":           # generous: T = 0, the positions are those of the coefficients themselves
        recs, per = _position_records(g, 11, 3), 4 + 400
    elif name == "positions-tight":   # every slice gets exactly the bytes it needs at an index of 4, 8 .. 32: one byte less moves T
        recs = _position_records(g, 12, 3000, small_scale=2)
        planes = planes_from_records(g, recs)
        t = build_tables(oracle, g, planes, qm, scalar, np.zeros((g.ys, g.xs), np.int32))
        sb = np.array([4 + t.need(4 + 4 * (s % 8), s) for s in range(ns)], np.int32).reshape(g.ys, g.xs)
        return g, planes, qm, scalar, sb
    elif name == "gallop":
        targets = [GALLOP_TARGETS[(s // 8) % 4][s % 8] + (s // 32) for s in range(ns)]
        recs, per = _scaled_records(g, 13, targets), 4 + 48
    elif name == "reset":             # slices 2 and 5 of every group of eight escape: their successors bisect again
        targets = [24 + (s * 5) % 13 for s in range(ns)]
        recs, per = _scaled_records(g, 14, targets), 4 + 70
        for s in range(ns):
            if s % 8 in (2, 5):
                recs[s % 3][s, (s * 7) % g.comp_n[s % 3]] = 40000 if s % 2 else -32768
    elif name == "big-scalar":        # coefficients near the store's limit, a scalar that holds them at index 0
        recs, per = _laplace_records(g, np.random.default_rng(15), 20000, zero=0.2), 4 + 3 * 64 * 8
        recs = [np.clip(r, -32767, 32767) for r in recs]
    elif name == "marked-many":       # 4 full words of the marked pass's ballot, then a sparse one
        recs, per = _laplace_records(g, np.random.default_rng(16), 300), 4 + 80
        for s in list(range(256)) + list(range(256, ns, 37)):
            recs[s % 3][s, (s * 11) % g.comp_n[s % 3]] = 70000 + s
    elif name == "marked-one":
        recs, per = _laplace_records(g, np.random.default_rng(17), 300), 4 + 80
        recs[2][77, 63] = -32768
    elif name == "odd-count":
        recs, per = _laplace_records(g, np.random.default_rng(18), 900), 4 + 50
    elif name == "index":             # starved: thresholds beyond 63, the walk visits 95 -- outside the float domain
        recs, per = _laplace_records(g, np.random.default_rng(19), 30000, zero=0.3), 4 + 3
        recs = [np.clip(r, -32767, 32767) for r in recs]
    elif name == "length-error":      # scalar 1 and large coefficients: a length byte overflows at a trial the reference visits
        recs, per = _laplace_records(g, np.random.default_rng(20), 20000, zero=0.0), 4 + 90
        recs = [np.clip(r, -32767, 32767) for r in recs]
        for s in range(0, ns, 2):     # every other slice is quiet: slices that stay beside slices that overflow
            for c in range(3):
                recs[c][s] = recs[c][s] // 4000
    elif name == "nothing-fits":      # a byte table below the four header bytes: no index fits
        recs, per = _laplace_records(g, np.random.default_rng(21), 100), 0
    elif name == "refine":            # luma: one LL value whose error falls over three steps; chroma sets the threshold
        rng = np.random.default_rng(22)
        recs = _laplace_records(g, rng, 400)
        recs[0][:] = 0
        per = 4 + 30
        planes = planes_from_records(g, recs)
        sb = oracle.slice_bytes(g.ys, g.xs, ns * per * scalar, scalar)
        t0 = analyse(oracle, g, planes, qm, scalar, sb).T
        table = _refine_luma(oracle)
        for s in range(ns):
            c = table.get(max(int(t0[s]) - int(qm[0]), 0))
            if c:
                recs[0][s, 0] = c
    else:
        raise KeyError(name)
    planes = planes_from_records(g, recs)
    sb = oracle.slice_bytes(g.ys, g.xs, ns * per * scalar + (7 if name in ("gallop", "odd-count") else 0), scalar)
    return g, planes, qm, scalar, sb


BIG = (128, 512, 128, 256, 3, 16, 32)        # 512 slices
ODD = (72, 528, 72, 264, 3, 9, 33)           # 297 slices: the last wavefront holds one
FINE_ROWS = [
    FineRow("positions", 2, "reg32", {"T=0": 128, "only-V-head": 8, "equal-error": 8}),
    FineRow("positions-tight", 1, "reg32", {f"tight:{c}:{p}": 8 for c in "YUV" for p in POSITIONS[:4]} | {"tight:only-V-head": 8}, geom=(128, 512, 128, 256, 3, 16, 32)),
    FineRow("gallop", 3, "reg32", {"up:1": 8, "down:1": 8, "up:2-7": 8, "down:2-7": 8, "up:32+": 8, "down:32+": 8}),
    FineRow("reset", 7, "reg32", {"after-hand-back": 8, "class:escape": 8}),
    FineRow("big-scalar", 64, "reg32", {"T=0": 128}),
    FineRow("marked-many", 2, "reg32", {"marked": 200}, geom=BIG),
    FineRow("marked-one", 2, "reg32", {"marked": 1}),
    FineRow("odd-count", 1, "reg32", {}, geom=ODD),
    FineRow("index", 1, "reg32", {"class:index": 8}),
    FineRow("length-error", 1, "reg32", {"class:length": 8}, raises="scalar"),
    FineRow("nothing-fits", 1, "reg32", {"T=127": 8, "class:index": 8}, raises="index"),
    FineRow("refine", 1, "reg32", {"refined-3+": 8}),
]


# ------------------------------------------------------------------------------------------
# inputs: pictures for the whole-picture calls (steered, then classified from the forward transform's own output)
# ------------------------------------------------------------------------------------------
@dataclass
class PictureRow:
    name: str
    w: int
    h: int
    cf: str
    bits: int
    wavelet: str
    depth: int
    u: int
    a: int
    s: int               # the picture's compressed bytes
    scalar: int
    picture: str         # half / smooth / noise / stripes / half16 / ramp16 / designed / designed-tight
    kernel: str          # the kernel the default context takes
    plan: tuple = None   # (headY, headC, runsY, runsC) where the kernel is search16
    prefix: int = 0
    claims: dict = field(default_factory=dict)
    raises: str = None
    seed: int = 1
    note: str = ""

    def params(self):
        return make_params(self.w, self.h, self.cf, self.bits, self.wavelet, self.depth, self.u, self.a, mode="HQ_CBR", s=self.s,
                           scalar=self.scalar, prefix=self.prefix)

    def coding(self):
        return dict(mode="HQ_CBR", s=self.s, scalar=self.scalar, prefix=self.prefix)


def half_noise(w, h, cf, bits, seed):
    """left half the smooth generator picture, right half uniform noise: slices of both kinds in one picture"""
    a = np.frombuffer(synth(w, h, cf, bits, seed), ">u2").copy()
    b = np.frombuffer(noise_frame(w, h, cf, bits, seed + 1), ">u2")
    cw = w if cf == "444" else w // 2
    ch = h // 2 if cf == "420" else h
    pos = 0
    for pw, ph in ((w, h), (cw, ch), (cw, ch)):
        pa = a[pos:pos + pw * ph].reshape(ph, pw)
        pa[:, pw // 2:] = b[pos:pos + pw * ph].reshape(ph, pw)[:, pw // 2:]
        pos += pw * ph
    return a.astype(">u2").tobytes()


def designed_picture(oracle, row, tight):
    """oracle.dwt_inverse of a coefficient field that holds the position records, as samples clipped to their range.
    (Exact for the wavelets without a level shift while nothing clips; the rows classify what dwt_forward gives.)"""
    g = picture_geometry(oracle, row.w, row.h, row.cf, row.depth, row.u, row.a)
    recs = _position_records(g, row.seed, 60 if tight else 3, small_scale=1)
    half = 1 << (row.bits - 1)
    out = []
    for c, coef in enumerate(planes_from_records(g, recs)):
        ph, pw = coef.shape
        pic = oracle.dwt_inverse(coef, KERNELS[row.wavelet], row.depth)
        hh, ww = (row.h, row.w) if c == 0 else (row.h // 2 if row.cf == "420" else row.h, row.w if row.cf == "444" else row.w // 2)
        v = np.clip(pic[:hh, :ww] + half, 0, 2 * half - 1).astype(np.uint16)
        out.append((v << (16 - row.bits)).astype(">u2").tobytes())
    return b"".join(out)


def _words(planes, bits):
    half = 1 << (bits - 1)
    return b"".join((np.clip(p + half, 0, 2 * half - 1).astype(np.uint16) << (16 - bits)).astype(">u2").tobytes() for p in planes)


def ramp16(oracle, row):
    """16-bit samples that rise across the picture over an eighth of their range, with a little noise: LL coefficients up
    to the 16-bit store's limit and small ones everywhere else -- under a starved budget the threshold
    of a slice is the index at which its LL vanishes, beyond 63 where |LL| is large"""
    rng = np.random.default_rng(row.seed)
    out = []
    for c in range(3):
        hh = row.h // 2 if c and row.cf == "420" else row.h
        ww = row.w if c == 0 or row.cf == "444" else row.w // 2
        x = np.linspace(-1.0, 1.0, ww)[None, :] * np.ones((hh, 1))
        amp = (32720 >> row.depth) // (2 if c else 1)   # DD97's LL gain is 2 per level
        out.append(np.rint(x * amp + rng.normal(0, 1.0, (hh, ww))).astype(np.int64))
    return _words(out, 16)


def half16(row):
    """16-bit samples: the left half the smooth generator picture at 1 / 16 of the range (coefficients that stay in the
    16-bit store), the right half noise over the whole range (coefficients that escape it)"""
    a = np.frombuffer(synth(row.w, row.h, row.cf, 10, row.seed), ">u2").astype(np.int64) >> 6
    b = np.frombuffer(noise_frame(row.w, row.h, row.cf, 16, seed=row.seed + 1), ">u2").astype(np.int64) - 32768
    a = (a - 512) * 4
    cw = row.w if row.cf == "444" else row.w // 2
    ch = row.h // 2 if row.cf == "420" else row.h
    out, pos = [], 0
    for pw, ph in ((row.w, row.h), (cw, ch), (cw, ch)):
        pa = a[pos:pos + pw * ph].reshape(ph, pw).copy()
        pa[:, pw // 2:] = b[pos:pos + pw * ph].reshape(ph, pw)[:, pw // 2:]
        out.append(pa)
        pos += pw * ph
    return _words(out, 16)


def stripes(row):
    """noise, with every other column of slices (32 luma samples wide) mid-grey: quiet and noisy slices alternate along
    a row of slices, so that neighbouring thresholds lie 32 and more apart"""
    a = np.frombuffer(noise_frame(row.w, row.h, row.cf, row.bits, seed=row.seed), ">u2").copy()
    cw = row.w if row.cf == "444" else row.w // 2
    ch = row.h // 2 if row.cf == "420" else row.h
    pos = 0
    for pw, ph in ((row.w, row.h), (cw, ch), (cw, ch)):
        pa = a[pos:pos + pw * ph].reshape(ph, pw)
        sw = 32 * pw // row.w
        quiet = (np.arange(pw) // sw) % 2 == 0
        pa[:, quiet] = 1 << 15
        pos += pw * ph
    return a.astype(">u2").tobytes()


_raw_cache = {}


def picture_raw(oracle, row):
    key = (row.picture, row.w, row.h, row.cf, row.bits, row.seed, row.wavelet if row.picture.startswith("designed") else "")
    if key not in _raw_cache:
        if row.picture == "half":
            raw = half_noise(row.w, row.h, row.cf, row.bits, row.seed)
        elif row.picture == "smooth":
            raw = synth(row.w, row.h, row.cf, row.bits, row.seed)
        elif row.picture == "noise":
            raw = noise_frame(row.w, row.h, row.cf, row.bits, seed=row.seed)
        elif row.picture == "stripes":
            raw = stripes(row)
        elif row.picture == "ramp16":
            raw = ramp16(oracle, row)
        elif row.picture == "half16":
            raw = half16(row)
        else:
            raw = designed_picture(oracle, row, row.picture == "designed-tight")
        _raw_cache[key] = raw
    return _raw_cache[key]


def picture_input(oracle, row, raw=None):
    """(geometry, the coefficient planes oracle.dwt_forward yields, matrix, scalar, slice byte table) of a picture row"""
    raw = picture_raw(oracle, row) if raw is None else raw
    g = picture_geometry(oracle, row.w, row.h, row.cf, row.depth, row.u, row.a)
    ch = row.h // 2 if row.cf == "420" else row.h
    cw = row.w if row.cf == "444" else row.w // 2
    planes, pos = [], 0
    for hh, ww in ((row.h, row.w), (ch, cw), (ch, cw)):
        p = oracle.ingest(raw[pos:pos + 2 * hh * ww], 2, row.bits, (hh, ww))
        pos += 2 * hh * ww
        planes.append(oracle.dwt_forward(p, KERNELS[row.wavelet], row.depth))
    qm = oracle.quant_matrix(KERNELS[row.wavelet], row.depth)
    sb = oracle.slice_bytes(g.ys, g.xs, row.s, row.scalar)
    return g, planes, qm, row.scalar, sb


def payload_indices(payload, sb, prefix):
    """the index byte of every slice header of an HQ_CBR payload (every slice fills its bytes: Slices.cpp:352-368)"""
    sizes = np.ascontiguousarray(sb, np.int64).ravel() + prefix
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1])) + prefix
    return np.frombuffer(payload, np.uint8)[starts].astype(np.int32)


def _P(name, w, h, wavelet, depth, u, a, s, scalar, picture, kernel, plan=None, cf="422", bits=10, **kw):
    return PictureRow(name, w, h, cf, bits, wavelet, depth, u, a, s, scalar, picture, kernel, plan, **kw)


D4 = (8, 16, 63, 30)     # 32 x 16 slices at depth 4
D3 = (0, 16, 64, 30)
D12 = (0, 0, 64, 32)
# s: bytes per picture; "+ 333" and the like: not a multiple of the slice count, so neighbouring slices' bytes differ by one
PICTURE_ROWS = [
    # 32 x 16 slices at depth 4, every wavelet: 2048 x 256 is the smallest 4:2:2 picture that gets the 16-bit store (the
    # deepest level of every component must fill a 32 x 128 tile of the fast level kernels: chroma 1024 >> 3 = 128 columns,
    # 256 >> 3 = 32 rows).  Fidelity's gains put 10-bit noise beyond 16 bits: escapes beside slices that stay.
    *[_P("d4-" + k, 2048, 256, k, 4, 1, 2, 2048 * 256 // 2 + 333, 16 if k == "Fidelity" else 2, "half", "search16", D4, seed=30 + i,
         claims={"class:escape": 8, "class:none": 8} if k == "Fidelity" else {})
      for i, k in enumerate(KERNELS)],
    # DD97 at depths 1 .. 3, each at the smallest picture with the 16-bit store
    _P("d1", 256, 32, "DD97", 1, 8, 16, 256 * 32 // 2 + 5, 4, "half", "search16", D12, seed=41),
    _P("d2", 512, 64, "DD97", 2, 4, 8, 512 * 64 // 2 + 21, 4, "half", "search16", D12, seed=42),
    _P("d3", 1024, 128, "DD97", 3, 2, 4, 1024 * 128 // 2 + 77, 2, "half", "search16", D3, seed=43),
    _P("d3-64x8", 1024, 128, "DD97", 3, 1, 8, 1024 * 128 // 2 + 77, 2, "half", "search16", D3, seed=44),
    _P("d3-16x32", 1024, 128, "DD97", 3, 4, 2, 1024 * 128 // 2 + 77, 2, "half", "search16", D3, seed=45),
    # 36 x 9 = 324 slices: the last wavefront of the picture holds four
    _P("d3-odd", 1152, 144, "DD97", 3, 2, 4, 1152 * 144 // 2 + 100, 2, "half", "search16", D3, seed=46),
    # quiet and noisy slices in turn: the gallop of k_cbr_search16's own loop at its far end, both ways
    _P("d3-stripes", 1024, 128, "Haar1", 3, 2, 4, 256 * (4 + 16 * 16) + 77, 16, "stripes", "search16", D3, seed=59,
       claims={"up:32+": 8, "down:32+": 8}),
    _P("d3-prefix", 1024, 128, "LeGall", 3, 2, 4, 1024 * 128 // 2, 3, "half", "search16", D3, prefix=2, seed=47),
    # starved: six bytes per slice; thresholds beyond 63 where |LL| is large -- the walk visits 95, outside the float domain
    _P("d3-starved", 1024, 128, "DD97", 3, 2, 4, 256 * 6 + 100, 1, "ramp16", "search16", D3, bits=16, seed=48,
       claims={"class:index": 8, "class:none": 8}),
    _P("d3-generous", 1024, 128, "DD97", 3, 2, 4, 256 * 1400, 8, "smooth", "search16", D3, seed=49, claims={"T=0": 8}),
    _P("d3-16bit", 1024, 128, "DD97", 3, 2, 4, 1024 * 128, 8, "half16", "search16", D3, bits=16, seed=50,
       claims={"class:escape": 8, "class:none": 8}),
    _P("d3-length-error", 1024, 128, "DD97", 3, 2, 4, 1024 * 128, 1, "half", "search16", D3, seed=51, raises="scalar",
       claims={"class:length": 8}),
    # Haar0 has no level shift: the forward transform gives the designed coefficients back
    _P("d4-designed", 2048, 256, "Haar0", 4, 1, 2, 1024 * 124, 1, "designed", "search16", D4, seed=52,
       claims={"T=0": 8, "only-V-head": 8, "Y:head": 8, "U:head": 8, "V:head": 8, "Y:first": 8, "U:first": 8, "V:first": 8,
               "Y:last": 8, "U:last": 8, "V:last": 8, "Y:none": 8, "U:none": 8, "V:none": 8}),
    _P("d4-designed-tight", 2048, 256, "Haar0", 4, 1, 2, 1024 * 14, 1, "designed-tight", "search16", D4, seed=53,
       claims={"tight:only-V-head": 8, "tight:Y:head": 8, "tight:U:head": 8, "tight:V:head": 8, "tight:Y:first": 8,
               "tight:U:first": 8, "tight:V:first": 8, "tight:Y:none": 8, "tight:U:none": 8, "tight:V:none": 8}),
    # where cbr16_plan refuses: chroma of 16 runs (4:2:0), luma of 30 (4:4:4, 16 x 16 slices)
    _P("420", 512, 128, "DD97", 2, 4, 8, 512 * 128 // 2 + 50, 2, "half", "reg16", cf="420", seed=54),
    _P("444", 512, 128, "DD97", 3, 2, 2, 512 * 128 + 50, 2, "half", "reg16", cf="444", seed=55),
    _P("420-starved", 512, 128, "DD97", 2, 4, 8, 128 * 6 + 30, 1, "ramp16", "reg16", cf="420", bits=16, seed=56,
       claims={"class:index": 8, "class:none": 8}),
    _P("444-16bit", 512, 128, "DD97", 3, 2, 2, 512 * 128 * 2, 8, "half16", "reg16", cf="444", bits=16, seed=57,
       claims={"class:escape": 8, "class:none": 8}),
    _P("420-length-error", 512, 128, "DD97", 2, 4, 8, 512 * 128, 1, "half", "reg16", cf="420", seed=58, raises="scalar",
       claims={"class:length": 8}),
]
# geometries the register kernels do not take (fine-grained call): chroma records beyond 256 coefficients; one slice that no
# LDS holds
GENERAL_GEOM = ("general", (64, 512, 64, 512, 3, 2, 8))      # 4:4:4, 32 x 64 slices: 2048 coefficients per component
GLOBAL_GEOM = ("global", (128, 512, 128, 256, 2, 1, 1))      # one slice of 131072 coefficients: 512 KiB
ROWS = {r.name: r for r in FINE_ROWS + PICTURE_ROWS}
# one encode_batch_dev call: three different pictures under d3's coding (the second and third are rows of their own here, so
# that tests/test_cbr_ref.py classifies them like every other input)
BATCH_ROWS = [ROWS["d3"], replace(ROWS["d3"], name="d3-batch-smooth", picture="smooth", seed=60),
              replace(ROWS["d3"], name="d3-batch-half", picture="half", seed=61)]
# one encode_recon_batch_dev call: two pictures, 324 slices each
RECON_ROWS = [ROWS["d3-odd"], replace(ROWS["d3-odd"], name="d3-odd-recon", seed=62)]


_model_cache = {}


def model_of(oracle, row):
    """the analysed model of a row (FineRow or PictureRow), computed once per process"""
    if row.name not in _model_cache:
        inp = fine_input(oracle, row) if isinstance(row, FineRow) else picture_input(oracle, row)
        _model_cache[row.name] = (inp, analyse(oracle, *inp))
    return _model_cache[row.name]
