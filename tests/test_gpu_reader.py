"""The three HQ slice readers against the CPU oracle on designed codes (tests/reader_ref.py); every comparison exact.

What each generator reaches is asserted without a GPU in tests/test_reader_ref.py.  Three observation windows, chosen so that
no clip can hide a value:

  - the int32 reader (k_hq_unpack<32>, decode_round over WordReader): every input through vc2hip_hq_unpack against the
    oracle's hq_unpack -- the three planes, the indices, the bytes consumed -- on three geometries: n < 32, rounds of exactly
    32, a last round of 16.
  - the 16-bit reader's values (k_hq_unpack16 over Reader32): vc2hip_transcode_batch_dev at target 0 and at one coarser target
    on geometry C, byte for byte against transcode_ref.Coded, with d_lens_out and d_qidx; inputs inside the encoder's domain.
    At target 0 every slice is kept: the output is the oracle's repack of the oracle's unpack.  The transcode call records no
    transform launch: that it takes the 16-bit reader here follows from the same use_store16 call in vc2hip_api.hip that the
    decoder makes, whose launches on this geometry the decode tests below do record -- not from an observation.
  - the 16-bit reader on every store form: every input, codes beyond 32 bits included, through vc2hip_decode_batch_dev against
    proxy_ref.full_picture -- slots 0xA5 behind their lengths, the output between guards, several inputs a call, the form
    confirmed from the launch record as tests/test_gpu_damaged.py does.  16-bit samples, and index 0 so that clipping is rarest
    (index 12 in a slice with a named value below 8 or a code beyond 32 bits: reader_ref.make_input says why); the window is
    there for placement, escapes and sentinels: tests/test_reader_ref.py shows, for every generator on C, D and S, that it
    sees every named value.
  - k_transcode_measure (tc_turn over TcReader): the capped form on six designed pictures at scalar 1, caps len(T(t)) and
    len(T(t)) - 1 for five targets: index, payload and lengths by Coded's capped definition."""
import numpy as np
import pytest

import proxy_ref as pr
import reader_ref as rr
import transcode_ref as tr
from test_gpu_damaged import check_form
from test_gpu_transcode import Slots, _tp, check_capped, check_fixed

pytestmark = pytest.mark.gpu

GUARD = 4096
TAIL = 4096


@pytest.fixture(scope="module")
def ctxs():
    """contexts by flags, made on first use and shared by the cases of this file"""
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
# the int32 reader through vc2hip_hq_unpack
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}


def unpacked(oracle, gname, name):
    """[(input, payload as an array, the oracle's (y, u, v, indices, consumed))] of one generator on one geometry; shared"""
    if (gname, name) not in _REF:
        g = rr.GEOS[gname]
        out = []
        for inp in rr.inputs(name, *rr.geo_n(g), g.ys * g.xs):
            data = np.frombuffer(rr.payload_of(inp), np.uint8)
            ref = oracle.hq_unpack(data, g.lshape, g.cshape, g.depth, g.ys, g.xs, inp.prefix, inp.scalar)
            assert ref[4] == data.size, (gname, name, inp.tag)
            out.append((inp, data, ref))
        _REF[(gname, name)] = out
    return _REF[(gname, name)]


@pytest.mark.parametrize("name", list(rr.GENERATORS))
@pytest.mark.parametrize("gname", list(rr.GEOS))
def test_int32_reader(ctxs, oracle, gname, name):
    g = rr.GEOS[gname]
    hip = ctxs()
    for inp, data, ref in unpacked(oracle, gname, name):
        got = hip.hq_unpack(data, g.lshape, g.cshape, g.depth, g.ys, g.xs, inp.prefix, inp.scalar)
        what = f"{gname} {name} [{inp.tag}] {data.size} bytes"
        assert got[4] == ref[4], f"{what}: consumed {got[4]}, the oracle {ref[4]}"
        assert np.array_equal(got[3], ref[3]), f"{what}: {int((got[3] != ref[3]).sum())} quantiser indices differ"
        for c in range(3):
            bad = np.argwhere(got[c] != ref[c])
            assert not bad.size, (f"{what}: component {c}: {len(bad)} coefficients differ, the first at {bad[0].tolist()}: "
                                  f"{int(got[c][tuple(bad[0])])}, the oracle {int(ref[c][tuple(bad[0])])}")


# ---------------------------------------------------------------------------------------------------------------------
# the designed pictures of a decoder geometry
# ---------------------------------------------------------------------------------------------------------------------
_CASES, _DESIGNED, _PICS, _CODED = {}, {}, {}, {}


def case(oracle, cname):
    if cname not in _CASES:
        _CASES[cname] = rr.case_of(oracle, cname)
    return _CASES[cname]


def designed(oracle, cname, names=rr.GENERATORS):
    """[(key, input, payload bytes)] of the generators on a decoder geometry; shared"""
    c = case(oracle, cname)
    nl, nc = rr.geo_n(rr.geo_of(c))
    out = []
    for name in names:
        if (cname, name) not in _DESIGNED:
            _DESIGNED[(cname, name)] = [((cname, name, inp.tag), inp, rr.payload_of(inp)) for inp in rr.inputs(name, nl, nc, c.ys * c.xs)]
        out += _DESIGNED[(cname, name)]
    return out


def picture(oracle, cname, key, payload):
    if key not in _PICS:
        _PICS[key] = pr.full_picture(oracle, case(oracle, cname), payload)
    return _PICS[key]


def coded(oracle, cname, key, payload):
    if key not in _CODED:
        _CODED[key] = tr.Coded(oracle, case(oracle, cname), payload)
    return _CODED[key]


# ---------------------------------------------------------------------------------------------------------------------
# the 16-bit reader on every store form, through vc2hip_decode_batch_dev
# ---------------------------------------------------------------------------------------------------------------------
def decode_call(hip, c, payloads, stride=None):
    """one vc2hip_decode_batch_dev call: every payload in a slot that is 0xA5 behind its length, the slots inside a larger
    allocation (0xA5 too), the output between two guards -> (the pictures' bytes, guards intact)"""
    import torch
    fmt, cp = c.fmt_cp(hip.lib)
    n = len(payloads)
    stride = stride or (max(len(p) for p in payloads) + 64 + 255) // 256 * 256
    assert stride % 16 == 0 and all(len(p) <= stride for p in payloads)
    d_pay = torch.full((n * stride + TAIL,), 0xA5, dtype=torch.uint8, device="cuda:0")
    for i, p in enumerate(payloads):
        d_pay[i * stride:i * stride + len(p)] = torch.from_numpy(np.frombuffer(p, np.uint8).copy()).to("cuda:0")
    d_len = torch.tensor([len(p) for p in payloads], dtype=torch.int64, device="cuda:0")
    total = n * c.raw_bytes()
    buf = torch.full((GUARD + total + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()   # (torch fills on its stream, the library works on its own)
    hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n, fmt, cp, buf.data_ptr() + GUARD)
    hip.sync()
    host = buf.cpu().numpy()
    guards = bool((host[:GUARD] == 0x5A).all() and (host[GUARD + total:] == 0x5A).all())
    return host[GUARD:GUARD + total].tobytes(), guards


def check_decode(hip, oracle, cname, items, what, stride=None):
    c = case(oracle, cname)
    got, guards = decode_call(hip, c, [p for _, _, p in items], stride)
    step = c.raw_bytes()
    bad = [key for i, (key, _, p) in enumerate(items) if got[i * step:(i + 1) * step] != picture(oracle, cname, key, p)]
    assert not bad, f"{what}: {len(bad)} of {len(items)} pictures differ from the oracle's: {bad}"
    assert guards, f"{what}: bytes outside the output were written"


C_VARIANTS = ("default", "PLANES8_ALWAYS", "PLANES8_NEVER", "NO_BANDPLANES", "STORE32")


@pytest.mark.parametrize("variant", C_VARIANTS)
def test_decode_every_store_form(ctxs, oracle, variant):
    """geometry C (1024 x 128 4:2:2 DD97 depth 3, 256 slices, luma 512 and chroma 256 coefficients a slice) with 16-bit samples:
    every designed picture but `slot_end` in one call, then every `slot_end` payload as the LAST picture of a call whose slot
    stride equals its length.  16-bit band planes, byte planes (+-127 / +-128 and the wide array), no band planes (records),
    the int32 store: confirmed from the launch record."""
    hip = ctxs() if variant == "default" else ctxs(variant)
    items = designed(oracle, "C", [n for n in rr.GENERATORS if n != "slot_end"])
    assert any(not inp.domain for _, inp, _ in items) and any(rr.is_cut(inp) for _, inp, _ in items)
    check_decode(hip, oracle, "C", items, f"C [{variant}]")
    bits, fams = check_form(hip, "C", variant)
    print(f"C [{variant}]: band planes of {bits} bits, launches (family, level, levels, store bits, band plane bits) {fams}")
    ends = designed(oracle, "C", ["slot_end"])
    for item in ends:
        assert len(item[2]) % 256 == 0
        check_decode(hip, oracle, "C", [ends[0], item] if len(ends[0][2]) <= len(item[2]) else [item, item], f"C [{variant}] {item[0]}", stride=len(item[2]))
    check_form(hip, "C", variant)


@pytest.mark.parametrize("variant", ["default", "NO_HEADS"])
def test_decode_record_heads(oracle, variant):
    """geometry D (2048 x 256, depth 4, 1024 slices): `table` (all 1024 indices in one picture) and `lengths` only -- the
    oracle needs ~0.2 s a picture here.  On a fresh context: one that has seen a batch of few payload bits per sample turns
    to byte planes (decode_batch_common), and the form asked for here is 16-bit planes above the heads.  The record confirms
    the 16-bit store, streaming levels 0 and 1 and the two-level launch below them; that the heads are in use follows from
    the planner's conditions (tests/test_gpu_damaged.py)."""
    from vc2hip_py import FLAGS, Vc2Hip
    items = designed(oracle, "D", ["table", "lengths"])
    assert len(items) == 2
    hip = Vc2Hip(flags=0 if variant == "default" else FLAGS[variant])
    try:
        check_decode(hip, oracle, "D", items, f"D [{variant}]")
        bits, fams = check_form(hip, "D", variant)
        print(f"D [{variant}]: band planes of {bits} bits, launches {fams}")
    finally:
        hip.close()


def test_decode_components_of_16(ctxs, oracle):
    """256 x 32 4:2:2 LeGall depth 1, slices of 4 x 8: chroma components of 16 coefficients, room < 32 in k_hq_unpack16 from
    the first round on -- if the decoder takes the 16-bit store here, which the launch record must show"""
    hip = ctxs()
    items = designed(oracle, "S", ["lengths", "over32", "phase", "table", "spill", "ends", "random"])
    check_decode(hip, oracle, "S", items, "S [default]")
    store = {r["store_bits"] for r in hip.dwt_launches()}
    print(f"S [default]: band planes of {hip.band_plane_bits()} bits, launches {hip.dwt_launches()}")
    assert store == {16}, f"S [16-bit store] not reached: {hip.dwt_launches()}"


# ---------------------------------------------------------------------------------------------------------------------
# the 16-bit reader's values, through vc2hip_transcode_batch_dev
# ---------------------------------------------------------------------------------------------------------------------
COARSER = 6


@pytest.mark.parametrize("variant", ["default", "STORE32"])
def test_transcode_values(ctxs, oracle, variant):
    """every designed picture inside the encoder's domain (all but `over32`) at target 0 and at target 6: those the
    definition can repack in one call, byte for byte; the one it cannot at target 0 (`ends`: components of 255 bytes cut
    inside a code decode to values that need more than 255 bytes at scalar 1) in a call of its own, refused as the oracle's
    slice writer refuses it.  Then every `slot_end` payload last in a call whose input stride equals its length."""
    import vc2hip_py
    hip = ctxs() if variant == "default" else ctxs(variant)
    c = case(oracle, "C")
    items = [it for it in designed(oracle, "C") if it[1].domain]
    assert {it[1].name for it in items} == set(rr.GENERATORS) - {"over32"}
    pics = [coded(oracle, "C", key, p) for key, _, p in items]
    assert all(p.in_domain for p in pics)
    for t in (0, COARSER):
        ok = [i for i, p in enumerate(pics) if p.transcode(t) is not tr.NOT_CODABLE]
        refused = [i for i in range(len(pics)) if i not in ok]
        assert [items[i][0][2].startswith("cut at 255 bytes") for i in refused] == ([True] if t == 0 else []), (t, refused)
        slots = Slots(hip, c, [items[i][2] for i in ok])
        check_fixed(slots.run(_tp(t)), [pics[i] for i in ok], t, ("C", variant, "designed"))
        for i in refused:
            with pytest.raises(vc2hip_py.Vc2HipError) as e:
                Slots(hip, c, [items[ok[0]][2], items[i][2]]).run(_tp(t))
            assert e.value.code == tr.ESCALAR, (items[i][0], e.value.code)
    for key, inp, p in items:
        if inp.name == "slot_end":
            pair = [coded(oracle, "C", key, p)] * 2
            s2 = Slots(hip, c, [p, p], stride_in=len(p))
            for t in (0, COARSER):
                check_fixed(s2.fresh().run(_tp(t)), pair, t, ("C", variant, key))


# ---------------------------------------------------------------------------------------------------------------------
# k_transcode_measure: the capped form
# ---------------------------------------------------------------------------------------------------------------------
MEASURED = ("lengths", "phase", "table", "ends", "spill", "random")
TARGETS = (0, 3, 8, 14, 25)


@pytest.mark.parametrize("k", range(len(MEASURED)), ids=MEASURED)
def test_transcode_measure_on_designed_codes(ctxs, oracle, k):
    """six designed pictures in one call at scalar 1 (one mis-measured byte moves the pick); the caps come from picture k's
    own table of transcoded lengths: len(T(t)) and len(T(t)) - 1 for five targets t.  Every picture's index, payload and
    length by Coded's capped definition."""
    hip = ctxs()
    c = case(oracle, "C")
    items = [designed(oracle, "C", [name])[0] for name in MEASURED]
    pics = [coded(oracle, "C", key, p) for key, _, p in items]
    floor = tr.floor_of(pics)
    assert floor == 0 and c.scalar == 1
    table = pics[k].table()
    slots = Slots(hip, c, [p for _, _, p in items])
    for t in TARGETS:
        assert table[t] is not tr.NOT_CODABLE
        for cap in (table[t], table[t] - 1):
            chosen = check_capped(slots.fresh().run(_tp(floor, cap)), pics, floor, cap, (MEASURED[k], t, cap))
            assert chosen[k] <= t if cap == table[t] else chosen[k] != t, (MEASURED[k], t, cap, chosen)
