"""Damaged slice payloads through every device batch decode path and decoder form, against the CPU oracle.

The rule ("Damaged payloads"): whatever the bytes and the length, the library gives the oracle's picture or
refuses as the oracle does, the other pictures of the batch are untouched and nothing outside the output is written.
tests/damage.py makes the mutations and the references; tests/test_damage_ref.py shows, without a GPU, that the oracle
accepts enough of every class for the comparison to carry weight.

One batch per class and geometry, device-resident:
  - slot i holds mutation i; the first, the middle and the last slot hold the clean payload;
  - the slot bytes behind d_lens[i] are 0xA5 (zero in the `long` class): a read past the length changes the result;
  - the output lies between two guards of 4096 bytes of 0x5A, which must come back unchanged.
Payloads the oracle accepts go together in one call: vc2hip_sync returns OK, every picture is the oracle's.  Payloads it
refuses go one per call between two clean ones (at most 12 per geometry and variant, by class: QUOTA): vc2hip_sync raises
-- VC2HIP_ESTREAM for `short`, VC2HIP_EQINDEX for a quantiser index of 120 or more, either of the two elsewhere, where a
broken chain can produce both -- the clean neighbours are the clean picture, and a clean call on the same context is
right afterwards.  The reduced decode does not validate what it does not read (include/vc2hip.h): for refused payloads
only the neighbours and the guards are asserted there."""
import numpy as np
import pytest

import damage as dm

pytestmark = pytest.mark.gpu

GUARD = 4096
# refused payloads that get a call of their own, per class; per geometry and variant they sum to 12
QUOTA = {"short": 4, "qindex": 4, "length": 3, "random": 1,
         "hdr0": 6, "hdr1": 2, "body00": 1, "bodyff": 1}
LD_QUOTA_RANDOM = 2


# ---------------------------------------------------------------------------------------------------------------------
# contexts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctxs():
    """contexts by (flags, lanes, on a caller's stream), made on first use and shared by the cases of this file"""
    import torch
    from vc2hip_py import FLAGS, Vc2Hip
    made = {}

    def get(flags=(), lanes=1, caller_stream=False):
        key = (tuple(flags), lanes, caller_stream)
        if key not in made:
            stream = torch.cuda.Stream() if caller_stream else None
            hip = Vc2Hip(flags=sum(FLAGS[f] for f in flags), stream=stream.cuda_stream if stream else None)
            if lanes > 1:
                hip.set_streams(lanes)
            hip.torch_stream = stream
            made[key] = hip
        return made[key]

    yield get
    for hip in made.values():
        hip.close()


# ---------------------------------------------------------------------------------------------------------------------
# slots, calls, comparison
# ---------------------------------------------------------------------------------------------------------------------
class Slots:
    """mutations in device slots"""

    def __init__(self, base, muts):
        import torch
        tail = base.tail   # LD: the reader sees the end of sequence behind the unit, and the length counts it in
        self.n = len(muts)
        need = max(max(len(m.data), m.length) for m in muts) + len(tail)
        self.stride = (need + 64 + 255) // 256 * 256
        slots = np.full((self.n, self.stride), 0xA5, np.uint8)
        lens = np.zeros(self.n, np.int64)
        for i, m in enumerate(muts):
            d = m.data + tail
            if m.cls == "long":
                slots[i] = 0
            slots[i, :len(d)] = np.frombuffer(d, np.uint8)
            lens[i] = m.length + len(tail)
        self.d_pay = torch.from_numpy(slots.reshape(-1)).to("cuda:0", non_blocking=False)
        self.d_len = torch.from_numpy(lens).to("cuda:0", non_blocking=False)


def _interleave(case, top, bottom):
    """two field pictures -> the frame of twice the height, top field first"""
    out, at = [], 0
    for h, w in ((case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)):
        nb = h * w * case.word_bytes
        fr = np.empty((2 * h, w * case.word_bytes), np.uint8)
        fr[0::2] = np.frombuffer(top[at:at + nb], np.uint8).reshape(h, -1)
        fr[1::2] = np.frombuffer(bottom[at:at + nb], np.uint8).reshape(h, -1)
        out.append(fr.tobytes())
        at += nb
    return b"".join(out)


def _call(hip, entry, base, muts):
    """one library call over the mutations; (the error vc2hip_sync raised or None, the output bytes, guards intact)"""
    import torch
    import vc2hip_py
    case = base.case
    kind, k = entry
    fmt, cp = case.fmt_cp(hip.lib)
    stream = getattr(hip, "torch_stream", None)
    with torch.cuda.stream(stream) if stream else _Null():
        slots = Slots(base, muts)
        total = slots.n * case.raw_bytes(k if kind == "reduced" else 0)
        buf = torch.full((GUARD + total + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
        if not stream:
            torch.cuda.synchronize()   # (torch fills on its stream, the library works on its own)
        args = (slots.d_pay.data_ptr(), slots.stride, slots.d_len.data_ptr())
        out = buf.data_ptr() + GUARD
        if kind == "reduced":
            hip.decode_reduced_batch_dev(*args, slots.n, fmt, cp, k, out)
        elif kind == "fields":
            assert slots.n % 2 == 0
            frame_fmt = vc2hip_py.picture_format(case.w, 2 * case.h, case.cf, case.bits, case.word_bytes)
            hip.decode_fields_batch_dev(*args, slots.n // 2, frame_fmt, 1, cp, out)
        else:
            hip.decode_batch_dev(*args, slots.n, fmt, cp, out)
        err = None
        if stream:   # the copy back is enqueued behind the call on the caller's stream: no host wait in between
            host = buf.cpu().numpy()
        try:
            hip.sync()
        except vc2hip_py.Vc2HipError as e:
            err = e
        if not stream:
            host = buf.cpu().numpy()
    guards = bool((host[:GUARD] == 0x5A).all() and (host[GUARD + total:] == 0x5A).all())
    return err, host[GUARD:GUARD + total].tobytes(), guards


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _expected(case, entry, pictures):
    """the call's output for the slots' reference pictures"""
    if entry[0] != "fields":
        return b"".join(pictures)
    return b"".join(_interleave(case, pictures[i], pictures[i + 1]) for i in range(0, len(pictures), 2))


def _differing(case, entry, got, pictures):
    """indices of the slots (fields: frames) whose bytes differ"""
    want = _expected(case, entry, pictures)
    assert len(got) == len(want)
    n = len(pictures) // (2 if entry[0] == "fields" else 1)
    step = len(want) // n
    return [i for i in range(n) if got[i * step:(i + 1) * step] != want[i * step:(i + 1) * step]]


def _pick(items, count):
    """count of the items, evenly spread, always the first and the last"""
    if len(items) <= count:
        return list(items)
    if count == 1:
        return [items[0]]
    return [items[round(i * (len(items) - 1) / (count - 1))] for i in range(count)]


def _quota(base, cls):
    if base.case.mode == "LD" and cls == "random":
        return LD_QUOTA_RANDOM
    return QUOTA.get(cls, 0)


def run_class(oracle, hip, name, cls, entry=("full", 0), variant="default"):
    """the comparison rules of this file's docstring for one class on one context"""
    base, _ = dm.load(oracle, name)
    case = base.case
    k = entry[1] if entry[0] == "reduced" else 0
    refs = dm.references(oracle, name, cls, k)
    clean_m, clean_pic = dm.clean(base), dm.clean_picture(oracle, name, k)
    what = f"{name} {cls} [{variant}] {entry[0]}{entry[1] or ''}"

    # accepted payloads: one call, clean slots first, in the middle and last
    acc = [(m, pic) for m, verdict, pic in refs if verdict == "ok"]
    half = len(acc) // 2
    row = [(clean_m, clean_pic)] + acc[:half] + [(clean_m, clean_pic)] + acc[half:] + [(clean_m, clean_pic)]
    if entry[0] == "fields" and len(row) % 2:
        row.append((clean_m, clean_pic))
    err, got, guards = _call(hip, entry, base, [m for m, _ in row])
    assert err is None, f"{what}: {len(acc)} payloads the oracle accepts, vc2hip_sync: {err} ({err.code})"
    bad = _differing(case, entry, got, [p for _, p in row])
    tags = [row[i][0].tag for i in bad] if entry[0] != "fields" else [f"frame {i}: {row[2 * i][0].tag} / {row[2 * i + 1][0].tag}" for i in bad]
    assert not bad, f"{what}: {len(bad)} of {len(row)} pictures differ from the oracle's: {tags[:8]}"
    assert guards, f"{what}: bytes outside the output were written"

    # refused payloads: one per call between clean ones
    refused = [(m, code) for m, verdict, code in refs if verdict == "refused"]
    chosen = _pick(refused, _quota(base, cls))
    if cls == "qindex" and len(refused) == 12:   # three slices x the four values of 120 and more: every value once, every slice
        chosen = [refused[i] for i in (0, 5, 10, 3)]
    for m, code in chosen:
        trio = [clean_m, m, clean_m] + ([clean_m] if entry[0] == "fields" else [])
        err, got, guards = _call(hip, entry, base, trio)
        assert guards, f"{what} {m.tag}: bytes outside the output were written"
        if entry[0] != "reduced":
            assert err is not None, f"{what} {m.tag}: the oracle refuses ({code}), vc2hip_sync returned OK"
            want_codes = (dm.ESTREAM,) if cls == "short" else (dm.EQINDEX,) if cls == "qindex" else (dm.ESTREAM, dm.EQINDEX)
            assert err.code in want_codes, f"{what} {m.tag}: the oracle refuses with {code}, the library with {err.code}: {err}"
        step = len(clean_pic)
        if entry[0] == "fields":   # frame 0: the clean field's rows; frame 1: both fields clean
            frame = _interleave(case, clean_pic, clean_pic)
            rows0 = _field_rows(case, got[:2 * step], 0)
            assert rows0 == _field_rows(case, frame, 0) and got[2 * step:] == frame, f"{what} {m.tag}: a clean neighbour changed"
        else:
            assert got[:step] == clean_pic and got[2 * step:] == clean_pic, f"{what} {m.tag}: a clean neighbour changed"
        # the context is usable afterwards
        pair = [clean_m, clean_m]
        err, got, guards = _call(hip, entry, base, pair)
        assert err is None and guards and not _differing(case, entry, got, [clean_pic, clean_pic]), f"{what}: clean call after {m.tag}: {err}"
    print(f"{what}: accepted {len(acc)} compared, refused {len(refused)} of which {len(chosen)} compared")
    return len(acc), len(chosen)


def _field_rows(case, frame, parity):
    out, at = [], 0
    for h, w in ((case.h, case.w), (case.ch, case.cw), (case.ch, case.cw)):
        nb = 2 * h * w * case.word_bytes
        out.append(np.frombuffer(frame[at:at + nb], np.uint8).reshape(2 * h, -1)[parity::2].tobytes())
        at += nb
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------------
# decoder forms: what the launch record and vc2hip_band_plane_bits say of the context's most recent call
# ---------------------------------------------------------------------------------------------------------------------
def _form(hip):
    rec = hip.dwt_launches()
    assert rec and all(r["inverse"] for r in rec), rec
    return hip.band_plane_bits(), rec


def _families(rec):
    return sorted({(r["family"], r["level"], r["levels"], r["store_bits"], r["band_planes"]) for r in rec})


def check_form(hip, name, variant):
    """fails by name if the geometry does not reach the decoder form it is here for"""
    bits, rec = _form(hip)
    fams = _families(rec)
    store = {r["store_bits"] for r in rec}
    if name == "A":       # slice records only, int32 store
        assert bits == 0 and store == {32}, f"A [records, int32 store] not reached: band planes {bits}, launches {fams}"
    # (B1, B2, E, F: here for the slice index and the LD walk, which the launch record does not hold: the index kernels are
    # confirmed by name in test_index_kernels_by_name, the chunk counts, the claim and the shifted slices on the CPU in
    # tests/test_damage_ref.py)
    elif name == "C":
        want = {"default": (16, 8), "PLANES8_ALWAYS": (8,), "PLANES8_NEVER": (16,), "NO_BANDPLANES": (0,), "NO_PAIR": (16, 8),
                "STORE32": (0,), "NO_STREAM": (0,)}[variant]
        assert bits in want, f"C [{variant}]: band planes of {bits} bits, expected one of {want}; launches {fams}"
        if variant == "STORE32":
            assert store == {32}, f"C [STORE32]: {fams}"
        else:
            assert 16 in store, f"C [{variant}] [16-bit store] not reached: {fams}"
        if variant == "NO_PAIR":
            assert not any(r["family"] == "pair" for r in rec), f"C [NO_PAIR]: a two-level launch: {fams}"
        if variant == "NO_STREAM":
            assert not any(r["family"] in ("stream", "pair") for r in rec), f"C [NO_STREAM]: {fams}"
        if variant in ("default", "PLANES8_NEVER") and bits == 16:
            assert any(r["band_planes"] == 16 for r in rec), f"C [{variant}] [16-bit band planes] read by no launch: {fams}"
        if bits == 8:
            assert any(r["band_planes"] == 8 for r in rec), f"C [{variant}] [byte band planes] read by no launch: {fams}"
    elif name == "D":
        # What plan_decoder_layout wants for record heads, as far as the record shows it: the 16-bit store; band planes at the
        # streaming levels 0 and 1 only (bp.levels = 2 <= the heads' first level); levels 2 and 3 on kernels that read heads --
        # one two-level launch, or with NO_PAIR the tile kernels.  Whether the heads were used is not in the record.
        assert store == {16}, f"D [{variant}] [16-bit store] not reached: {fams}"
        fine = [r for r in rec if r["level"] < 2]
        assert {r["level"] for r in fine} == {0, 1} and all(r["family"] == "stream" and r["band_planes"] == 16 for r in fine), \
            f"D [{variant}] [levels 0, 1 streaming from 16-bit band planes] not reached: {fams}"
        deep = {(r["family"], r["level"], r["levels"]) for r in rec if r["level"] >= 2}
        if "NO_PAIR" in variant:
            assert {d[1:] for d in deep} == {(2, 1), (3, 1)} and {d[0] for d in deep} <= {"fast", "tile"}, \
                f"D [{variant}] [levels 2, 3 on the tile kernels] not reached: {fams}"
        else:
            assert deep == {("pair", 2, 2)}, f"D [{variant}] [levels 2 + 3 in one two-level launch] not reached: {fams}"
    return bits, fams


# ---------------------------------------------------------------------------------------------------------------------
# the geometries
# ---------------------------------------------------------------------------------------------------------------------
def _cases(name, variants):
    return [(v, c) for v in variants for c in dm.input_classes(name)]


@pytest.mark.parametrize("cls", dm.input_classes("A"))
def test_a_records_int32_store(ctxs, oracle, cls):
    """A: 128 x 64 4:2:0 8-bit in 1-byte words, LeGall depth 2, slices of 8 x 16, prefix 2, ~10 KiB of payload with one 8 KiB
    index chunk boundary inside it.  Form confirmed by the record: no band planes (vc2hip_band_plane_bits 0), every inverse
    launch on the int32 store."""
    hip = ctxs()
    run_class(oracle, hip, "A", cls)
    check_form(hip, "A", "default")


@pytest.mark.parametrize("cls", dm.input_classes("B1"))
@pytest.mark.parametrize("name", ["B1", "B2"])
def test_b_index_groups(ctxs, oracle, name, cls):
    """B: 1024 x 64 4:2:2 10-bit DD97 depth 3, 512 slices; scalar 1 (124 KB: 16 index chunks of 8 KiB, one full group) and
    scalar 2 on noise (300 KB: 19 chunks of 16 KiB, the size the index takes from scalar 2 on: two groups of 16; slice
    starts are even: the tables per two bytes).  `random` and `length` carry a mutation on either side of a boundary of
    the input's own chunks.  The launch record holds transforms only; that these payloads go through the chunk tables, the
    group chain and the emit kernel, not the serial walk, is test_index_kernels_by_name's."""
    hip = ctxs()
    run_class(oracle, hip, name, cls)
    check_form(hip, name, "default")


C_VARIANTS = ("default", "PLANES8_ALWAYS", "PLANES8_NEVER", "NO_BANDPLANES", "NO_PAIR", "STORE32", "NO_STREAM")


@pytest.mark.parametrize("variant,cls", _cases("C", C_VARIANTS), ids=lambda x: x)
def test_c_store16_band_planes(ctxs, oracle, variant, cls):
    """C: 1024 x 128 4:2:2 10-bit DD97 depth 3, slices of 16 x 32, scalar 8 -- the "wide" geometry of test_gpu_dwt_paths.py
    at half its height, the smallest that still reports band planes: at 1024 x 64, 768 x 128, 512 x 256 and 512 x 128 the
    decoder keeps the int32 store and vc2hip_band_plane_bits is 0.  Forms confirmed by the record: 16-bit band planes by
    default and with PLANES8_NEVER, byte planes with PLANES8_ALWAYS (and by default once a batch has shown small
    coefficients), none with NO_BANDPLANES, STORE32 (int32 store) and NO_STREAM (tile kernels), no two-level launch with
    NO_PAIR."""
    hip = ctxs(() if variant == "default" else (variant,))
    run_class(oracle, hip, "C", cls, variant=variant)
    check_form(hip, "C", variant)


D_VARIANTS = {"default": (), "NO_HEADS": ("NO_HEADS",), "NO_PAIR": ("NO_PAIR",), "NO_PAIR+NO_HEADS": ("NO_PAIR", "NO_HEADS")}


@pytest.mark.parametrize("variant,cls", _cases("D", tuple(D_VARIANTS)), ids=lambda x: x)
def test_d_record_heads_depth_4(ctxs, oracle, variant, cls):
    """D: 2048 x 256 4:2:2 10-bit DD97 depth 4, slices of 16 x 32, scalar 8 (test_deep_level_shapes_with_escapes' geometry).
    `boundary`, `run00` and `qindex` only, 29 mutations: the oracle needs ~0.2 s per picture here.  The first run of every
    `run00` slice opens the luma component, so the wide escape falls into the coarsest bands: the record heads' gather.
    The decoder plans record heads from a dry run of the inverse that leaves the two-level kernels out
    (plan_decoder_layout): here levels 2 and 3 qualify, with or without NO_PAIR, and both the two-level kernel and the
    fast tile kernels read them.  So the four contexts are the two gathers with and without heads: default = heads read by
    the two-level kernel over levels 2 + 3, NO_HEADS = that kernel on the slice records, NO_PAIR = heads through the fast
    tile kernels' gather at levels 2 and 3, NO_PAIR + NO_HEADS = those kernels on the records.  Confirmed by the record:
    the 16-bit store, streaming kernels with 16-bit band planes at levels 0 and 1, one two-level launch (or two fast
    launches) below them.  The heads themselves leave no trace in the record: that they are in use follows from the
    planner's conditions, which these launches meet, not from an observation."""
    hip = ctxs(D_VARIANTS[variant])
    run_class(oracle, hip, "D", cls, variant=variant)
    check_form(hip, "D", variant)


@pytest.mark.parametrize("variant,cls", _cases("E", ("default", "NO_CBR_INDEX", "CBR_GENERAL")), ids=lambda x: x)
def test_e_hq_cbr_claim_and_fallback(ctxs, oracle, variant, cls):
    """E: geometry B coded as HQ_CBR (s = 30000, scalar 1): the decoder claims the slice offsets from the byte budgets.
    `boundary` keeps every slice on its budget (the claim holds), `length` breaks it (the general index runs): both give
    the oracle's picture or refusal, as does the context that never claims (NO_CBR_INDEX).  Whether the claim held is a
    word in device memory that no call reports, and the general index kernels are launched either way (they return at
    once when it held), so this test cannot see the split: tests/test_damage_ref.py restates the check on the CPU and
    shows that it must hold for the clean and `boundary` batches and fail for the `length` batch;
    test_index_kernels_by_name shows that the claim's kernels run here and not with NO_CBR_INDEX."""
    hip = ctxs(() if variant == "default" else (variant,))
    run_class(oracle, hip, "E", cls, variant=variant)
    check_form(hip, "E", variant)


@pytest.mark.parametrize("cls", dm.input_classes("F1"))
@pytest.mark.parametrize("name", ["F1", "F2"])
def test_f_ld(ctxs, oracle, name, cls):
    """F: LD pictures, 256 x 32 4:2:2 10-bit Haar1 depth 1 (s = 8000) and 512 x 64 4:2:2 8-bit LeGall depth 3 (s = 12000).
    The slot holds the payload and the 13 bytes that follow the unit in the stream, as the reference's reader sees them;
    a luma length beyond its slice moves every later slice (flag, serial walk, second pass).  The walk and the second
    pass are launched for every picture and return at once without the flag, so no record shows them at work:
    tests/test_damage_ref.py shows which accepted mutations raise the flag (F2 `hdr0` on the last slice; none on F1)."""
    run_class(oracle, ctxs(), name, cls)


# ---------------------------------------------------------------------------------------------------------------------
# the other entry points, on B and C
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = {"reduced1": ("reduced", 1), "reduced2": ("reduced", 2), "fields": ("fields", 0), "lanes2": ("full", 0), "lanes3": ("full", 0),
           "caller-stream": ("full", 0)}
ENTRY_CASES = [(n, e, c) for n in ("B1", "B2", "C") for e in ENTRIES for c in dm.input_classes(n)]


@pytest.mark.parametrize("name,entry,cls", ENTRY_CASES, ids=[f"{n}-{e}-{c}" for n, e, c in ENTRY_CASES])
def test_entry_points(ctxs, oracle, name, entry, cls):
    """vc2hip_decode_reduced_batch_dev (k = 1, 2: only what the oracle accepts is compared), vc2hip_decode_fields_batch_dev
    (the same payloads as field slots of a frame of twice the height, against the two field pictures interleaved),
    vc2hip_set_streams(2) and (3) (damaged slots on both sides of every lane border), and a context on a caller's stream
    (slots, call and copy back enqueued on that stream, no host wait in between)."""
    lanes = {"lanes2": 2, "lanes3": 3}.get(entry, 1)
    hip = ctxs((), lanes, entry == "caller-stream")
    run_class(oracle, hip, name, cls, ENTRIES[entry], variant=entry)


def test_index_kernels_by_name(oracle):
    """What the launch record cannot say of B and E, from the per-kernel profile of one clean call on a fresh context: B1
    and B2 go through the chunk tables, the group chain and the emit kernel of the slice index and not through the serial
    walk; E launches the budget claim's kernels by default and not with NO_CBR_INDEX."""
    from vc2hip_py import FLAGS, Vc2Hip
    general = {"slice_index_tables", "slice_index_chain", "slice_index_emit"}
    for name, flags, want, never in (("B1", (), general, {"slice_index_serial", "slice_index_cbr"}),
                                     ("B2", (), general, {"slice_index_serial", "slice_index_cbr"}),
                                     ("E", (), {"slice_index_cbr"}, {"slice_index_serial"}),
                                     ("E", ("NO_CBR_INDEX",), general, {"slice_index_cbr"})):
        base, _ = dm.load(oracle, name)
        pic = dm.clean_picture(oracle, name)
        hip = Vc2Hip(flags=sum(FLAGS[f] for f in flags))
        try:
            hip.profile_reset()
            hip.profile_enable(True)
            err, got, guards = _call(hip, ("full", 0), base, [dm.clean(base)] * 2)
            hip.profile_enable(False)
            seen = {k for k, v in hip.profile().items() if v[0] > 0}
        finally:
            hip.close()
        assert err is None and guards and got == pic * 2, (name, flags, err)
        assert want <= seen and not (never & seen), f"{name} {flags}: kernels launched: {sorted(seen)}"


def test_adaptive_form_never_changes_a_result(oracle):
    """A fresh default context on geometry C: two clean coarse batches (the same picture at q = 16), a `run00` batch
    (escapes by the thousand: every code of more than 32 bits is one, and the coefficients behind it are garbage), the
    coarse batch twice again.  The decoder turns to byte planes below 6.0 payload bits per sample of the batch before
    (decode_batch_common); the coarse payload has 4.4, and the test wants it below 5.0, a bit clear of that threshold.  A
    context's second decode call waits for its first look, so the second coarse batch and the `run00` batch behind it
    run on byte planes.  Every picture is the oracle's whatever form the planes had in each call."""
    import proxy_ref as pr
    from vc2hip_py import Vc2Hip
    base, _ = dm.load(oracle, "C")
    c = base.case
    coarse = dm.Base(oracle, pr.Case(oracle, c.w, c.h, c.cf, c.bits, c.kernel, c.depth, c.u, c.a, q=16, scalar=c.scalar), base.raw)
    bits_per_sample = 8 * len(coarse.payload) / (c.raw_bytes() // c.word_bytes)
    assert bits_per_sample < 5.0, bits_per_sample
    verdict, coarse_pic = dm.reference(oracle, coarse, dm.clean(coarse))
    assert verdict == "ok"
    calm = [(dm.clean(coarse), coarse_pic)] * 4
    runs = [(m, pic) for m, verdict, pic in dm.references(oracle, "C", "run00") if verdict == "ok"]
    assert len(runs) >= 20
    seen = []
    hip = Vc2Hip()
    try:
        for row in (calm, calm, runs, calm, calm):
            err, got, guards = _call(hip, ("full", 0), base, [m for m, _ in row])
            seen.append(hip.band_plane_bits())
            bad = _differing(base.case, ("full", 0), got, [p for _, p in row])
            assert err is None and guards and not bad, f"band planes per call {seen}: {err}, pictures {bad} differ"
    finally:
        hip.close()
    print(f"band planes per call (coarse, coarse, run00, coarse, coarse): {seen}")
    assert all(b in (8, 16) for b in seen), f"band planes per call {seen}"
    assert seen[:3] == [16, 8, 8], f"the adaptive choice did not put the run00 batch on byte planes: band planes per call {seen}"
