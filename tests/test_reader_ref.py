"""tests/reader_ref.py without a GPU: the builder and the oracle witness each other, the three models of the readers'
token logic equal the oracle on every designed input, every generator reaches what it is named for, and every wrong copy
of a model is caught by a designed input (`random` left out).

The decode window of tests/test_gpu_reader.py (whole pictures through the inverse transform and the clip) is there for
placement, escapes and sentinels: test_zeroing_a_named_coefficient_changes_the_picture shows that it sees every named
coefficient.  An error of +-1 under a clipped sample is NOT its business: the exact windows -- vc2hip_hq_unpack's planes and
the transcoder's bytes -- carry that."""
from collections import Counter

import numpy as np
import pytest

import proxy_ref as pr
import reader_ref as rr

NS = 256
GEO_N = {k: rr.geo_n(g) for k, g in rr.GEOS.items()}
GEO_N.update(C=(512, 256), S=(32, 16))     # the decoders' geometries of reader_ref.CASES: where k_hq_unpack16 and tc_turn run


def _all(gname, names=rr.GENERATORS):
    nl, nc = GEO_N[gname]
    return [inp for name in names for inp in rr.inputs(name, nl, nc, NS)]


# ---------------------------------------------------------------------------------------------------------------------
# builder and oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_code_lengths():
    assert rr.code(0) == "1" and rr.code(1) == "0010" and rr.code(-1) == "0011" and rr.code(2) == "0110" and rr.code(-6) == "010111"
    for K in range(1, 16):
        assert len(rr.code((1 << K) - 1)) == len(rr.code(-((2 << K) - 2))) == 2 * K + 2
    assert [len(rr.code(v)) for v in (30, 31, 65534, 65535, 1 << 20, (1 << 31) - 1, (1 << 32) + 5)] == [10, 12, 32, 34, 42, 64, 66]
    assert rr.as_read((1 << 32) + 5) == 5 and rr.as_read(-((1 << 32) + 77)) == -77 and rr.as_read(-((1 << 31) - 1)) == -(2 ** 31 - 1)


SLOW_GEOS = [pytest.param(g, marks=pytest.mark.slow) if g != "n16" else g for g in rr.GEOS]


@pytest.mark.parametrize("gname", SLOW_GEOS)
def test_oracle_accepts_and_returns_the_designed_planes(oracle, gname):
    """none refused; exactly the designed planes, indices and length (cut components: what the definition reads of the data)"""
    g = rr.GEOS[gname]
    for inp in _all(gname):
        pay = np.frombuffer(rr.payload_of(inp), np.uint8)
        ref = oracle.hq_unpack(pay, g.lshape, g.cshape, g.depth, g.ys, g.xs, inp.prefix, inp.scalar)
        des = rr.planes(inp, g)
        assert ref[4] == pay.size, (gname, inp.name, inp.tag)
        for c in range(4):
            assert np.array_equal(ref[c], des[c]), (gname, inp.name, inp.tag, c)
        assert inp.domain == (rr.max_abs(inp) <= 65534), (gname, inp.name, inp.tag)


@pytest.mark.parametrize("gname", SLOW_GEOS)
def test_models_equal_the_oracle(gname):
    """(the designed values ARE the oracle's: the test above) the 16-bit reader's turn with the 16-bit and the byte store,
    decode_round and tc_turn / tc_long, component by component, `random` included"""
    nl, nc = GEO_N[gname]
    for inp in _all(gname):
        want = rr.wants(inp)
        for model, got in rr.run_models(inp, nl, nc).items():
            bad = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
            assert not bad, f"{gname} {inp.name} [{inp.tag}] {model}: {len(bad)} components differ, the first {bad[0]}"


def test_table_is_the_kernels():
    """a few entries by hand, from the entry format above vc2_unpack_lut_host"""
    lut = rr.unpack_lut()
    assert lut[0b1111111111] == 8 | 8 << 4                                   # eight zeros: 8 bits, the cap of 8 coefficients
    assert lut[0b0010111111] == 10 | 7 << 4 | 1 << 16 | 1 << 24              # +1 then six zeros
    assert lut[0b0011001011] == 10 | 4 << 4 | 0 << 8 | 1 << 12 | 0xFF << 16 | 1 << 24  # -1, +1, two zeros
    assert lut[0b0101010111] == 10 | 1 << 4 | (-30 & 0xFF) << 16 | (-30 & 0xFF) << 24  # -30: the sign is the index's last bit
    assert lut[0b0001000110] == 10 | 1 << 4 | 20 << 16 | 20 << 24
    assert lut[0b0001000100] == 0 and lut[0] == 0                            # 31 and beyond: no entry
    assert lut[0b1110001000] == 3 | 3 << 4                                   # three zeros, then a code that is not whole


# ---------------------------------------------------------------------------------------------------------------------
# reach
# ---------------------------------------------------------------------------------------------------------------------
_TRACE = {}


def reach(gname, name):
    if (gname, name) not in _TRACE:
        nl, nc = GEO_N[gname]
        st = Counter()
        for inp in rr.inputs(name, nl, nc, NS):
            st += rr.trace(inp, nl, nc, stride=len(rr.payload_of(inp)) if name == "slot_end" else None)
        _TRACE[(gname, name)] = st
    return _TRACE[(gname, name)]


# (geometry, generator): event -> the least count the design gives, worked out by hand.  Events are counted on the DESIGNED
# components alone (the seeded fillers around them are left out), and on the geometries where the reader in question runs:
# C (luma 512, chroma 256 coefficients) and S (32 / 16) for k_hq_unpack16 and tc_turn, n48 besides for the ends.
#   lengths   71 values dealt over 768 components: each at least 10 times.  Every K = 5 .. 15 has its 4 extremes (40 long
#             codes or more on each reader); beyond 16 bits: +-65534, +32768, -32768 -- exactly 40 escapes
#   over32    33 designed components with one code of 34 bits or more each: a bit-serial step on every reader; nine of the eleven
#             values escape (2^32 + 5 and -(2^32 + 77) wrap to 5 and -77): 27
#   phase     r = 0 .. 40 and the two extra tails at r = 31, 32, 33: 44 long codes per K; the named second-token lists once each
#   table     1024 indices open a luma component: every index with an entry is seen by the first look-up (how many have one
#             is counted from the table itself); the chroma copies put them at later look-ups
#   spill     7 places x 8 patterns x (first, last boundary) = 112 components.  An entry of 7 at room - d spills 7 - d, an entry
#             of 8 spills 8 - d: per boundary 8 spills of every size 1 .. 6 and one of size 7, and the +-1 lies in the carried
#             part for 21 of the 49 (d, place) pairs.  On C both boundaries differ in luma and chroma: 8 / 1 / 21 mid-component
#             and again at the end.  Where a component is one round (S; n48's chroma) `first` is the end too: up to twice that
#   ends      all eight residues of the 8-byte readers' last word, TcReader's requests of 1 .. 5 and 8 words (the lengths asked for
#             give no 6 or 7: 41 .. 56 bytes mod 64), a 64-byte request,
#             both forms of Reader32's last piece inside the slot, cut and empty components
#   slot_end  the last piece word by word in every one of the six payloads
_SPILL_END = dict({f"u16 spill {s} at the end": 8 for s in range(1, 7)}, **{"u16 spill 7 at the end": 1, "u16 spill carries a value at the end": 21})
REACH = {
    ("C", "lengths"): dict({f"u16 long K={K}": 40 for K in range(5, 16)}, **{f"tc long K={K}": 40 for K in range(5, 16)},
                           **{f"rnd long K={K}": 40 for K in range(5, 16)}, **{"u16 escape": 40}),
    ("C", "over32"): {"u16 bit-serial": 33, "rnd bit-serial": 33, "tc_long": 33, "u16 escape": 27},
    ("C", "phase"): {"u16 long K=5": 44, "u16 long K=10": 44, "u16 long K=15": 44, "tc long K=15": 44, "rnd second refused: cnt + z2 = room": 1,
                     "rnd second refused: n + z2 > 32": 1, "rnd second refused: n > 31": 1, "rnd second taken at n + z2 = 32": 1,
                     "rnd run cut by the round": 1},
    ("C", "table"): {"u16 entry of 8": 4, "u16 entry of two values": 1, "u16 look4 refused": 1, "u16 look4 taken": 1, "u16 entry at look 3": 1},
    ("C", "spill"): dict({f"u16 spill {s}": 8 for s in range(1, 7)}, **{"u16 spill 7": 1, "u16 spill carries a value": 21}, **_SPILL_END),
    ("S", "spill"): {k: 2 * v for k, v in _SPILL_END.items()},
    ("n48", "spill"): _SPILL_END,
    ("C", "ends"): dict({f"word reader: {k} bytes in the last word": 1 for k in range(8)}, **{f"tc request of {k} words": 1 for k in (1, 2, 3, 4, 5, 8)},
                        **{f"start offset {k}": 1 for k in range(8)},
                        **{"reader32 whole request": 1, "reader32 ends in 16": 1, "reader32 ends in tail16": 1, "cut": 100, "empty": 16}),
    ("C", "slot_end"): {"reader32 ends in words": 6},
    ("S", "slot_end"): {"reader32 ends in words": 6},
}


SLOW_REACH = {("C", "table"), ("C", "ends"), ("C", "slot_end")}     # seconds of model work each


@pytest.mark.parametrize("key", [pytest.param(k, marks=pytest.mark.slow) if k in SLOW_REACH else k for k in REACH], ids=lambda k: f"{k[0]}-{k[1]}")
def test_generator_reaches_what_it_is_named_for(key):
    st = reach(*key)
    short = {ev: (st[ev], least) for ev, least in REACH[key].items() if st[ev] < least}
    assert not short, f"{key}: (reached, designed at least) {short}"
    if key[1] == "lengths":
        assert st["u16 escape"] == 40


@pytest.mark.slow
def test_table_reaches_every_index():
    lut = rr.unpack_lut()
    st = reach("C", "table")
    with_entry = [w for w in range(1024) if lut[w]]
    assert len(with_entry) == 1024 - 32       # no entry: 0 b 0 b 0 b 0 b 0 b, a code of 12 bits or more
    first = {w for (ev, w), n in ((k, v) for k, v in st.items() if isinstance(k, tuple)) if ev == "u16 index at look 0"}
    later = {w for (ev, w), n in ((k, v) for k, v in st.items() if isinstance(k, tuple)) if ev == "u16 index at a later look"}
    assert first >= set(with_entry), sorted(set(with_entry) - first)[:8]
    assert len(later) >= 900, len(later)
    kinds = Counter("8" if (lut[w] >> 4) & 15 == 8 else "two" if (lut[w] >> 8) & 15 != (lut[w] >> 12) & 15 else "other" for w in with_entry)
    assert kinds["8"] == 4 and kinds["two"] > 100, kinds


@pytest.mark.parametrize("gname", ["n128", pytest.param("C", marks=pytest.mark.slow), "S"])
def test_ends_covers_every_length_at_every_offset(gname):
    """`exact`, `slack` and `empty` at all eight byte offsets, `cut` after each of the code's 14 bits (at the offsets as they
    fall), per length as far as reader_ref._sum_codes' rule says that the component's coefficients can fill it: the rule is
    restated here, so a change of seed cannot thin the design unseen"""
    nl, nc = GEO_N[gname]
    seen = Counter()
    for inp in rr.inputs("ends", nl, nc, NS):
        pay, starts = rr.payload(inp.slices, inp.prefix, inp.scalar)
        for i, c, comp in rr.designed_components(inp):
            seen[(c > 0, comp.units, comp.note if comp.note.startswith("cut") else f"{comp.note}@{starts[3 * i + c] % 8}")] += 1
    for chroma, n in ((False, nl), (True, nc)):
        assert all(seen[(chroma, 0, f"empty@{o}")] for o in range(8))
        for L in rr.END_LENGTHS[1:]:
            if 8 * L <= 30 * (n - 1):
                assert all(seen[(chroma, L, f"exact@{o}")] for o in range(8)), (gname, n, L)
            for j in range(1, min(14, 8 * L) + 1):
                if 8 * L - j <= 30 * (n - 2):
                    assert seen[(chroma, L, f"cut{j}")], (gname, n, L, j)
            if 8 * L >= n:
                assert all(seen[(chroma, L, f"slack{p}@{o}")] for o in range(8) for p in "01"), (gname, n, L)


def test_slot_end_lengths():
    nl, nc = GEO_N["n128"]
    got = set()
    for inp in rr.inputs("slot_end", nl, nc, NS):
        assert len(rr.payload_of(inp)) % 256 == 0
        got |= {c.units for c in inp.slices[-1][1]}
    assert got == set(range(1, 18))


def test_what_no_input_can_reach():
    """the two table caps that are dead at 10 table bits (reader_ref.MUTANTS' comment; that the run cap of 32 binds nowhere
    follows from the kernels' own bounds, stated there: no input is needed to show it)"""
    lut = rr.unpack_lut()
    for w in range(1024):                      # a third whole code in 10 bits: never, so the cap of two values never binds
        bits, p, codes = format(w, "010b"), 0, 0
        while p < 10:
            if bits[p] == "1":
                p += 1
                continue
            q = p
            while q < 10 and bits[q] == "0":
                q += 2
            if q + 1 >= 10:
                break
            codes, p = codes + 1, q + 2
        assert codes <= 2
        if (lut[w] >> 4) & 15 == 8:            # an entry at the cap of 8 coefficients: zeros only
            assert lut[w] >> 16 == 0


# ---------------------------------------------------------------------------------------------------------------------
# wrong copies
# ---------------------------------------------------------------------------------------------------------------------
# mutant -> (geometry, the designed generator that catches it, the models that must show it)
CAUGHT_BY = {
    "lut_whole": ("n128", "table", ("unpack16", "tc")),
    "guard4": ("n128", "table", ("unpack16",)),
    "n_z2_33": ("n128", "phase", ("round",)),
    "cnt_z2_le": ("n128", "phase", ("round",)),
    "fill_short": ("n128", "ends", ("unpack16", "round", "tc")),
    "fill_long": ("n128", "ends", ("unpack16", "round", "tc")),
    "lead": ("n128", "ends", ("unpack16", "round", "tc")),
    "spill_drop": ("n128", "spill", ("unpack16",)),
    "sentinel32768": ("n128", "lengths", ("unpack16",)),
    "byte128": ("n128", "lengths", ("b8",)),
    "sign_k15": ("n128", "lengths", ("unpack16", "round", "tc")),
    "tc_room": ("n128", "spill", ("tc",)),
}


def test_every_mutant_is_listed():
    assert set(CAUGHT_BY) == set(rr.MUTANTS) and len(rr.MUTANTS) >= 12
    assert all(name in rr.DESIGNED for _, name, _ in CAUGHT_BY.values())


@pytest.mark.parametrize("mut", list(CAUGHT_BY))
def test_mutant_is_caught_by_a_designed_input(mut):
    gname, name, models = CAUGHT_BY[mut]
    nl, nc = GEO_N[gname]
    differs = Counter()
    for inp in rr.inputs(name, nl, nc, NS):
        want = rr.wants(inp)
        for model, got in rr.run_models(inp, nl, nc, mut, models).items():
            differs[model] += sum(a != b for a, b in zip(got, want))
    assert all(differs[m] for m in models), f"{mut} ({rr.MUTANTS[mut]}): components that differ on `{name}`: {dict(differs)}"


# ---------------------------------------------------------------------------------------------------------------------
# the decode window
# ---------------------------------------------------------------------------------------------------------------------
SPACING = {"C": 4, "S": 4, "D": 8}     # slices between two coefficients zeroed in one transform: beyond any synthesis filter's reach
# the generators that tests/test_gpu_reader.py sends through the decoder on each geometry
WINDOW = {"C": tuple(rr.GENERATORS), "S": tuple(n for n in rr.GENERATORS if n != "slot_end"), "D": ("table", "lengths")}


def unseen(oracle, case, inp, spacing):
    """the named coefficients of an input whose zeroing leaves the oracle's picture as it is: [(slice, component, position, value)].
    One coefficient in every spacing-th slice each way is zeroed per transform; a coefficient counts as seen where the picture
    changes inside its OWN slice (the others zeroed with it lie spacing - 1 slices away or more)."""
    g = rr.geo_of(case)
    des = rr.planes(inp, g)
    qm = oracle.quant_matrix(pr.KERNELS[case.kernel], case.depth)
    shapes = [(case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)]

    def pic(c, plane):
        x = oracle.dwt_inverse(oracle.dequantise_np(plane, case.depth, des[3], qm), pr.KERNELS[case.kernel], case.depth, shapes[c])
        return np.frombuffer(oracle.clip_emit(x, case.word_bytes, case.bits).tobytes(), ">u2").reshape(shapes[c])

    out = []
    for c in range(3):
        sh, sw = des[c].shape[0] // g.ys, des[c].shape[1] // g.xs
        oy, ox = np.array(rr.order(sh, sw, g.depth)).T
        full = pic(c, des[c])
        todo = {}
        for i, ci, k in inp.named:
            if ci == c and des[c][(i // g.xs) * sh + oy[k], (i % g.xs) * sw + ox[k]] != 0:
                todo.setdefault(((i // g.xs) % spacing, (i % g.xs) % spacing), {}).setdefault(i, []).append(k)
        for cls in todo.values():
            while any(cls.values()):
                p, batch = des[c].copy(), []
                for i, ks in cls.items():
                    if ks:
                        k = ks.pop()
                        y, x = (i // g.xs) * sh + oy[k], (i % g.xs) * sw + ox[k]
                        batch.append((i, k, int(p[y, x])))
                        p[y, x] = 0
                got = pic(c, p)
                for i, k, v in batch:
                    y0, x0 = (i // g.xs) * sh, (i % g.xs) * sw
                    if np.array_equal(got[y0:y0 + sh, x0:x0 + sw], full[y0:y0 + sh, x0:x0 + sw]):
                        out.append((i, c, k, v))
    return out


@pytest.mark.slow
@pytest.mark.parametrize("cname,name", [(c, n) for c in WINDOW for n in WINDOW[c] if n != "random"], ids=lambda x: x)
def test_zeroing_a_named_coefficient_changes_the_picture(oracle, cname, name):
    """for every generator that goes through the decode window, on each of its geometries: the oracle's picture of the
    designed planes with any one named coefficient set to 0 differs from the picture of the designed planes"""
    case = rr.case_of(oracle, cname)
    nl, nc = rr.geo_n(rr.geo_of(case))
    named = 0
    for inp in rr.inputs(name, nl, nc, case.ys * case.xs):
        assert rr.payload_of(inp) and len(inp.named) > 0
        named += len(inp.named)
        missed = unseen(oracle, case, inp, SPACING[cname])
        assert not missed, f"{cname} {name} [{inp.tag}]: {len(missed)} named coefficients the decode window does not see: {missed[:8]}"
    assert named >= 18
