"""k_hq_unpack16<true>'s byte rounds (csrc/vc2hip_slices.hip) against the CPU oracle on designed payloads; every comparison exact.

With byte band planes the slice reader decodes the record part of a component in 16-bit rounds of 32 coefficients and, from
the first round that starts in the planes, in BYTE rounds of 64: a table entry's value bytes go to the staging row as they
are, the long-code path alone tests the range (a value beyond -127 .. 127 goes to the wide array, the byte becomes -128 and
the batch statistic counts its piece of eight once), the flush moves pieces of eight bytes.  Every case is decoded through
vc2hip_decode_batch_dev on a context with VC2HIP_FLAG_PLANES8_ALWAYS and on one with _NEVER (the 16-bit rounds, unchanged)
and compared byte for byte with the oracle's decode of the same payload (proxy_ref.full_picture).

Geometries (4:2:2, 16-bit samples, DD97; the launch record must show byte planes at exactly the levels the design assumes):
  A  1600 x 128, depth 3, slices of 16 x 32: 400 slices (two workgroups; the second has two whole wavefronts, one of 16
     lanes and an idle one).  Luma 512 coefficients, planes from 32; chroma 256, planes from 16: a 16-bit round straddles
     the planes' start, and 480 = 7.5 and 224 = 3.5 byte rounds: the last one is short.  Block rows of 16, 8 | 8, 4.
  B  3072 x 256, depth 4, slices of 16 x 64: 768 slices.  Luma 1024 from 16, chroma 512 from 8 (both straddle).  Block
     rows of 32, 16, 8 | 16, 8, 4: every branch of the flush with rows of up to 32.
  W  3072 x 256, depth 4, slices of 16 x 128: 384 slices.  Luma 2048 from 32: block rows of 64 that start in the middle of
     a byte round (the rounds start at 32 + 64 k), so they leave piece by piece; chroma rows of 32 leave whole.

Pictures of a geometry, all in one call (so that the wavefronts of one launch need different numbers of turns):
  values   126, -126, 127, -127, 128, -128, -129, 32767, -32768, 32768, 70000, -70000 as the first, a middle and the last
           coefficient of a piece of a byte round, in luma and in chroma; then two such values in one piece.
  carry    a table entry of 8 zeros, or of six zeros and a +-1 in the carried part, applied so that 1 .. 7 of its coefficients
           spill over the end of the round: the last 16-bit round (the switch) and the first two byte rounds.  Every second
           one has an escape (300) as the first coefficient behind the carried ones, in the piece that holds them -- a
           carried coefficient itself is always a table value (|v| <= 30) and cannot be one.
  streams  components of length 0, a component cut inside a code (the bits behind the data read as 1), codes of 36, 42 and
           66 bits in a byte round.
  dense    (A only) a seeded dense picture beside the sparse ones.

The batch statistic is read through what it decides (test_gpu_wide.py::test_band_plane_form_follows_the_batches_...): on a
default-flags context a batch in byte planes keeps them while fewer than 0.5 % of its pieces carry an escape and drops them
above.  One picture has 0.35 % of its pieces with TWO escapes each (counted per escape: 0.7 %, planes dropped), the next
0.6 % with one each (not counted: planes kept).

The host-only test runs tools/sim_unpack_turns.py on a 256 x 128 picture."""
import importlib.util
import os

import numpy as np
import pytest

import proxy_ref as pr
import reader_ref as rr
from test_gpu_reader import decode_call

GEOS = {
    "A": ((1600, 128, "422", 16, "DD97", 3, 2, 4), 2, 1),   # Case arguments, levels kept as band planes, scalar
    "B": ((3072, 256, "422", 16, "DD97", 4, 1, 4), 3, 1),
    "W": ((3072, 256, "422", 16, "DD97", 4, 1, 8), 3, 2),   # (a luma component of 2048 sparse coefficients needs more than 255 bytes)
}
ESCAPES = (126, -126, 127, -127, 128, -128, -129, 32767, -32768, 32768, 70000, -70000)
PAIRS = ((128, -129), (70000, -32768), (-128, 32768), (32767, 127), (-70000, 70000))
ROW16, ROW8 = 32, 64


@pytest.fixture(scope="module")
def ctxs():
    from vc2hip_py import FLAGS, Vc2Hip
    made = {}

    def get(*flags):
        if flags not in made:
            made[flags] = Vc2Hip(flags=sum(FLAGS[f] for f in flags))
        return made[flags]

    yield get
    for hip in made.values():
        hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# the geometry as the reader sees it
# ---------------------------------------------------------------------------------------------------------------------
class Layout:
    """one component kind (0 luma, 1 chroma) of a geometry: n, where the planes start, the rounds, the block rows"""

    def __init__(self, case, kind, levels):
        self.scalar = case.scalar
        sh, sw = ((case.cph, case.cpw) if kind else (case.ph, case.pw))
        sh, sw = sh // case.ys, sw // case.xs
        self.n = sh * sw
        self.rows = [(sw >> l) // 2 for l in range(levels)]                 # coefficients of a block row, finest level first
        self.frm = self.n - sum(3 * ((sh >> l) // 2) * ((sw >> l) // 2) for l in range(levels))
        assert self.frm > 0 and self.frm % 8 == 0 and self.n % ROW16 == 0
        self.base0 = -(-self.frm // ROW16) * ROW16                          # the first byte round
        self.ends = [min(b + ROW8, self.n) for b in range(self.base0, self.n, ROW8)]   # the byte rounds' ends


_CASES, _LAYOUTS = {}, {}


def case(oracle, gname):
    if gname not in _CASES:
        _CASES[gname] = pr.Case(oracle, *GEOS[gname][0], q=0, scalar=GEOS[gname][2])
        _LAYOUTS[gname] = [Layout(_CASES[gname], k, GEOS[gname][1]) for k in (0, 1)]
    return _CASES[gname]


def layouts(oracle, gname):
    case(oracle, gname)
    return _LAYOUTS[gname]


def test_the_geometries_are_what_the_cases_are_designed_for(oracle):
    la, lb, lw = (layouts(oracle, g) for g in "ABW")
    ns = {g: case(oracle, g).ys * case(oracle, g).xs for g in "ABW"}
    assert ns == {"A": 400, "B": 768, "W": 384} and ns["A"] % 64 and ns["A"] > 256
    assert [(l.n, l.frm, l.base0) for l in la] == [(512, 32, 32), (256, 16, 32)]          # chroma: a straddling round
    assert all((l.n - l.base0) % ROW8 == ROW16 for l in la)                                # a short last byte round
    assert [l.rows for l in la] == [[16, 8], [8, 4]]
    assert [(l.n, l.frm, l.base0) for l in lb] == [(1024, 16, 32), (512, 8, 32)]
    assert [l.rows for l in lb] == [[32, 16, 8], [16, 8, 4]]                               # lw 5 .. 2
    assert [(l.n, l.frm, l.base0) for l in lw] == [(2048, 32, 32), (1024, 16, 32)]
    assert lw[0].rows[0] == 64 and (lw[0].n - 3 * (lw[0].n // 4)) % 64 == 0 and lw[0].base0 % 64 == 32   # rows of 64 start mid-round


# ---------------------------------------------------------------------------------------------------------------------
# designed pictures
# ---------------------------------------------------------------------------------------------------------------------
_FILL = {}


def _filler(n, k, scalar):
    """one of 24 seeded sparse components of n coefficients (shared: generating one per slice would take the time)"""
    if (n, k % 24, scalar) not in _FILL:
        _FILL[(n, k % 24, scalar)] = rr._filler(np.random.default_rng(1000 * n + k % 24), n, scalar)
    return _FILL[(n, k % 24, scalar)]


def _picture(name, tag, lay, ns, makers, index=None):
    """makers: [(kind, Layout -> Comp)] dealt over the slices' components of their kind in order; fillers elsewhere"""
    todo = {0: [m for k, m in makers if k == 0], 1: [m for k, m in makers if k == 1]}
    slices = []
    for i in range(ns):
        cs = []
        for c in range(3):
            kind = 1 if c else 0
            cs.append(todo[kind].pop(0)(lay[kind]) if todo[kind] else _filler(lay[kind].n, 3 * i + c, lay[kind].scalar))
        slices.append((0, cs))
    assert not todo[0] and not todo[1], f"{name}: {ns} slices do not hold the design"
    return rr.make_input(name, tag, slices, scalar=lay[0].scalar, index=index)


def _placed(L, placed, seed):
    n = L.n
    body = rr._sparse(np.random.default_rng(seed), n, 0.05)
    for j, v in placed.items():
        body[j] = v
    comp = rr.component(body, n, scalar=L.scalar, named=sorted(placed))
    assert all(comp.want[j] == rr.as_read(v) for j, v in placed.items())
    return comp


def values_picture(lay, ns):
    makers, k = [], 0
    for kind in (0, 1):
        L = lay[kind]
        for v in ESCAPES:
            for pos in (0, 3, 7):
                # a piece of the second byte round, the piece moving through the round; every level's block rows come up
                j0 = L.ends[0] + 8 * (k % 8)
                k += 1
                makers.append((kind, lambda L, j=j0 + pos, v=v, s=k: _placed(L, {j: v}, s)))
        for a, b in PAIRS:
            for pa, pb in ((0, 7), (3, 4)):
                j0 = L.ends[1] + 8 * (k % 8) if pa == 0 else L.ends[-2] + 8 * (k % 4)   # the third byte round; the last one
                k += 1
                makers.append((kind, lambda L, j0=j0, a=a, b=b, pa=pa, pb=pb, s=k: _placed(L, {j0 + pa: a, j0 + pb: b}, s)))
    return _picture("values", "escapes in byte rounds", lay, ns, makers)


def carry_comp(L, R, spill, nonzero, escape):
    """a table entry applied so that `spill` of its coefficients fall behind coefficient R - 1 (the end of a round): a long
    code (45: no table entry) right before makes the next turn's first look-up start at the entry"""
    n, nc = L.n, 7 if nonzero else 8
    c = R - nc + spill
    assert 1 <= spill < nc and c >= 1
    if nonzero:
        at = nc - spill + (spill - 1) // 2                       # a place in the carried part
        pat = "".join(rr.code(-1 if spill % 2 else 1) if k == at else "1" for k in range(nc))
    else:
        pat = "1" * 8
    behind = (rr.code(300) if escape else rr.code(3)) + rr.code(-2)
    comp = rr.component([0] * (c - 1) + [45 if spill % 2 else -45], n, scalar=L.scalar, raw=pat + behind + "1" * n)
    want = [0] * n
    want[c - 1] = 45 if spill % 2 else -45
    if nonzero:
        want[c + at] = -1 if spill % 2 else 1
    if c + nc < n:
        want[c + nc] = 300 if escape else 3
    if c + nc + 1 < n:
        want[c + nc + 1] = -2
    assert comp.want == want, (R, spill, nonzero, escape)
    return comp._replace(named=tuple(k for k in range(n) if want[k]), note=f"R={R} spill={spill}")


def carry_picture(lay, ns):
    makers = []
    for kind in (0, 1):
        L = lay[kind]
        rounds = [L.base0, L.ends[0], L.ends[1]]                  # the switch, then between byte rounds
        assert L.base0 == ROW16 or L.base0 - ROW16 < L.frm        # (the round before base0 is a 16-bit one)
        k = 0
        for R in rounds:
            for spill in range(1, 8):
                for nonzero in (False, True):
                    if nonzero and spill == 7:
                        continue                                  # (an entry of 8 coefficients holds zeros only)
                    k += 1
                    makers.append((kind, lambda L, R=R, s=spill, nz=nonzero, e=k % 2 == 0: carry_comp(L, R, s, nz, e)))
    return _picture("carry", "spills at the switch and between byte rounds", lay, ns, makers)


def streams_picture(lay, ns):
    makers = []
    for kind in (0, 1):
        L = lay[kind]
        makers.append((kind, lambda L: rr.component([], L.n, units=0, named=[0], note="empty")))
        for nbytes in (10, 24, 40):            # zeros up to the middle of the first byte round, then dense codes cut inside one
            def cut(L, nbytes=nbytes):
                rng = np.random.default_rng(nbytes)
                lead = L.base0 + 32
                for _ in range(50):
                    body = [0] * lead + [rr._val(rng, int(rng.integers(3, 9))) for _ in range(L.n - lead)]
                    comp = rr.component(body, L.n, scalar=L.scalar, units=(lead // 8 + nbytes) // L.scalar, named="largest")
                    if comp.cut and any(w and w != b for w, b in zip(comp.want, body)):   # the last code read differs: it was cut
                        return comp
                raise AssertionError("no cut inside a code found")
            makers.append((kind, cut))
        for v in (1 << 17, -(1 << 20), (1 << 32) + 5):
            j = L.ends[0] + 13
            makers.append((kind, lambda L, j=j, v=v: _placed(L, {j: v}, abs(v) % 977)))
    return _picture("streams", "empty, cut, beyond 32 bits", lay, ns, makers, index=rr.SMALL_INDEX)


_PICS = {}


def designed(oracle, gname):
    """[(tag, payload, the oracle's picture)] of a geometry; shared"""
    if gname not in _PICS:
        c, lay = case(oracle, gname), layouts(oracle, gname)
        ns = c.ys * c.xs
        inputs = [values_picture(lay, ns), carry_picture(lay, ns), streams_picture(lay, ns)]
        if gname == "A":
            inputs += rr.gen_random(lay[0].n, lay[1].n, ns, seed=71)
        out = []
        for inp in inputs:
            pay = rr.payload_of(inp)
            out.append((inp.name, pay, pr.full_picture(oracle, c, pay)))
        _PICS[gname] = out
    return _PICS[gname]


def plane_levels(hip, bits):
    rec = hip.dwt_launches()
    assert rec and all(r["inverse"] for r in rec), rec
    return sorted({r["level"] for r in rec if r["band_planes"] == bits})


@pytest.mark.gpu
@pytest.mark.parametrize("gname", list(GEOS))
def test_byte_rounds_against_the_oracle(ctxs, oracle, gname):
    c = case(oracle, gname)
    pics = designed(oracle, gname)
    step = c.raw_bytes()
    for variant, bits in (("PLANES8_ALWAYS", 8), ("PLANES8_NEVER", 16)):
        hip = ctxs(variant)
        got, guards = decode_call(hip, c, [p for _, p, _ in pics])
        assert hip.band_plane_bits() == bits and plane_levels(hip, bits) == list(range(GEOS[gname][1])), \
            f"{gname} [{variant}]: band planes of {hip.band_plane_bits()} bits at levels {plane_levels(hip, bits)}: {hip.dwt_launches()}"
        bad = []
        for i, (tag, _, want) in enumerate(pics):
            g = np.frombuffer(got[i * step:(i + 1) * step], np.uint16)
            w = np.frombuffer(want, np.uint16)
            if not np.array_equal(g, w):
                at = np.flatnonzero(g != w)
                bad.append(f"{tag}: {at.size} samples differ, the first at {int(at[0])}: {int(g[at[0]])}, the oracle {int(w[at[0]])}")
        assert not bad, f"{gname} [{variant}]: " + "; ".join(bad)
        assert guards, f"{gname} [{variant}]: bytes outside the output were written"


# ---------------------------------------------------------------------------------------------------------------------
# the batch statistic: pieces with an escape, each counted once
# ---------------------------------------------------------------------------------------------------------------------
def escape_picture(lay, ns, pieces, per_piece, tag):
    """`pieces` pieces of byte rounds with per_piece escapes (+-300) each, one piece a component, over the slices in order"""
    makers = []
    for k in range(pieces):
        kind = 1 if k % 3 else 0
        L = lay[kind]
        j0 = L.ends[k % 2] + 8 * (k % 4)
        placed = {j0 + 2: 300} if per_piece == 1 else {j0 + 2: 300, j0 + 5: -300}
        makers.append((kind, lambda L, placed=placed, s=k % 24: _placed(L, placed, 5000 + s)))
    # (luma makers fill the slices' Y components in order, chroma makers their U and V: k % 3 deals them one a component)
    return _picture("escapes", tag, lay, ns, makers)


@pytest.mark.gpu
def test_the_batch_statistic_counts_a_piece_with_two_escapes_once(oracle):
    from vc2hip_py import Vc2Hip
    c, lay = case(oracle, "A"), layouts(oracle, "A")
    ns = c.ys * c.xs
    total = (c.w * c.h + 2 * c.cw * c.ch) // 8                  # pieces of a picture
    once, over = int(0.0035 * total), int(0.006 * total)
    assert 2 * once > 0.0055 * total and 0.0025 * total < once < 0.0045 * total and over > 0.0055 * total and over <= 3 * ns
    clean = rr.payload_of(_picture("clean", "fillers", lay, ns, []))
    two = rr.payload_of(escape_picture(lay, ns, once, 2, "0.35 % of the pieces, two escapes each"))
    one = rr.payload_of(escape_picture(lay, ns, over, 1, "0.6 % of the pieces, one escape each"))
    want = {id(p): pr.full_picture(oracle, c, p) for p in (clean, two, one)}
    hip = Vc2Hip()
    try:
        seen = []
        for pay in (clean, two, one, clean):
            got, guards = decode_call(hip, c, [pay])
            assert got == want[id(pay)] and guards, f"call {len(seen)}"
            seen.append(hip.band_plane_bits())
        # fresh: 16-bit planes; few payload bits per sample: bytes; 0.35 % of the pieces escaped: still bytes; 0.6 %: back to 16 bits
        assert seen == [16, 8, 8, 16], seen
    finally:
        hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# tools/sim_unpack_turns.py (host only)
# ---------------------------------------------------------------------------------------------------------------------
def test_sim_unpack_turns_decodes_every_coefficient(oracle):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "sim_unpack_turns.py")
    spec = importlib.util.spec_from_file_location("sim_unpack_turns", path)
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    pay, ns, n_comp, scalar = sim.synthetic_payload(256, 128, 2, seed=3)
    assert (ns, n_comp) == (64, (512, 256, 256))
    comps = sim.components(pay, ns, 0, scalar)
    want = [rr.plain("".join(format(x, "08b") for x in data), n_comp[c]) for _, c, _, data in comps]
    assert any(any(w) for w in want)
    for row in (16, 32, 64):
        r = sim.simulate(pay, ns, n_comp, row, scalar=scalar, values=True)
        assert r["coefficients"] == [ns * n for n in n_comp], (row, r["coefficients"])
        assert r["wavefronts"] == [1, 1, 1] and 0 < r["ideal"] <= r["wavefront_turns"] and 0 < r["efficiency"] <= 1
        for s, c, _, _ in comps:
            assert r["values"][c][s] == want[3 * s + c], (row, s, c)
