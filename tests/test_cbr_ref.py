"""The conditions that keep tests/test_gpu_cbr_search.py from being empty, checked against the oracle alone (no GPU): every
input of that file takes the kernel its row names, reaches the search edges its row claims -- counted -- and raises, or
does not raise, what its row says; over all rows every hand-back class (per register kernel), every threshold and gallop
condition and every last-non-zero position is there at least eight times.  The model itself (tests/cbr_ref.py) is held
to the oracle: its final indices are oracle.cbr_qindices' (the index bytes of oracle.encode_stream's payload for pictures);
where the refinement moves nothing that index IS the threshold, so there T from the per-index lengths is compared with the
oracle directly (most slices of most rows; the test counts them), elsewhere through the model's own refinement; and the
bytes a slice needs never grow with the index (three pictures).

Positions are counted twice: over all slices, and over the TIGHT ones (0 < T: the bytes at T - 1 do not fit, so a
miscounted component moves the index).  A generous row (T = 0 everywhere) pins only the refinement; the minimums that
matter are the tight ones, asserted on the tight rows and, per kernel, over all rows.

(kernel, class) pairs left out: none.  Class `length` -- a length byte overflows at a trial the REFERENCE visits -- is an
error of the reference ("Slice scalar is too small"), so it is reached on rows that raise; a length hand-back without an
error (a gallop trial below the reference's smallest overflows) is counted as marked:length."""
from dataclasses import replace

import numpy as np
import pytest

import cbr_ref as cr
from vc2lib import KERNELS, OracleError

ALL_ROWS = cr.FINE_ROWS + cr.PICTURE_ROWS + cr.BATCH_ROWS[1:] + cr.RECON_ROWS[1:]
MIN = 8
CONDITIONS = (["T=0", "T=127", "after-hand-back", "only-V-head", "equal-error", "refined-3+"]
              + [f"{d}:{k}" for d in ("up", "down") for k in ("1", "2-7", "32+")]
              + [f"{c}:{p}" for c in "YUV" for p in ("none", "head", "first", "last")])


def _geom(oracle, row):
    if isinstance(row, cr.FineRow):
        return cr.Geometry(*row.geom), oracle.quant_matrix(KERNELS["DD97"], row.geom[4]), False
    g = cr.picture_geometry(oracle, row.w, row.h, row.cf, row.depth, row.u, row.a)
    return g, oracle.quant_matrix(KERNELS[row.wavelet], row.depth), cr.store16(g)


@pytest.mark.parametrize("row", ALL_ROWS, ids=lambda r: r.name)
def test_every_row_takes_the_kernel_it_names(oracle, row):
    g, qm, is16 = _geom(oracle, row)
    assert is16 == isinstance(row, cr.PictureRow), "every picture row gets the 16-bit store, the fine-grained call never does"
    assert cr.kernel_for(g, qm, is16) == (row.kernel, getattr(row, "plan", None))
    assert cr.kernel_for(g, qm, False) == ("reg32", None)                      # VC2HIP_FLAG_STORE32
    assert cr.kernel_for(g, qm, is16, general_only=True) == ("general", None)  # VC2HIP_FLAG_CBR_GENERAL


def test_depth_rows_give_the_run_counts_and_are_the_smallest_pictures(oracle):
    want = {"d1": (0, 0, 64, 32), "d2": (0, 0, 64, 32), "d3": (0, 16, 64, 30), "d4-DD97": (8, 16, 63, 30)}
    for name, plan in want.items():
        row = cr.ROWS[name]
        g, qm, is16 = _geom(oracle, row)
        assert is16 and cr.kernel_for(g, qm, True) == ("search16", plan), name
        for smaller in (replace(row, w=row.w // 2), replace(row, h=row.h // 2)):   # the deepest level no longer fills a tile
            gs = cr.picture_geometry(oracle, smaller.w, smaller.h, smaller.cf, smaller.depth, smaller.u, smaller.a)
            assert not cr.store16(gs), (name, smaller.w, smaller.h)
    # 1024 x 128, the smallest at depth 3, keeps the int32 store at depth 4: no 16-bit kernel runs there
    assert not cr.store16(cr.picture_geometry(oracle, 1024, 128, "422", 4, 1, 2))
    # slice counts that are no multiple of eight
    assert cr.Geometry(*cr.ODD).n_slices % 8 == 1 and _geom(oracle, cr.ROWS["d3-odd"])[0].n_slices % 8 == 4


def test_geometries_the_register_kernels_refuse(oracle):
    for name, geom in (cr.GENERAL_GEOM, cr.GLOBAL_GEOM):
        g = cr.Geometry(*geom)
        assert cr.kernel_for(g, oracle.quant_matrix(KERNELS["DD97"], g.depth), False) == (name, None)
    # cbr16_plan's borders: 64 luma runs are taken, 65 are not (run >= 64); 32 chroma runs are, 33 are not (2 * per > 64)
    qm1 = oracle.quant_matrix(KERNELS["DD97"], 1)
    assert cr.cbr16_plan(cr.Geometry(32, 256, 32, 128, 1, 2, 8), qm1, True) == (0, 0, 64, 32)
    assert cr.cbr16_plan(cr.Geometry(32, 256, 32, 256, 1, 2, 8), qm1, True) is None     # 4:4:4: 64 chroma runs
    assert cr.cbr16_plan(cr.Geometry(32, 256, 32, 128, 1, 2, 8), qm1, False) is None    # the int32 store


def _oracle_outcome(oracle, row, inp):
    g, planes, qm, scalar, sb = inp
    try:
        if isinstance(row, cr.FineRow):
            return oracle.cbr_qindices(*planes, g.depth, qm, sb, scalar).ravel(), None
        stream = oracle.encode_stream(row.params(), cr.picture_raw(oracle, row), 1)
        n = int(sb.sum()) + row.prefix * g.n_slices
        return cr.payload_indices(stream[-13 - n:-13], sb, row.prefix), None
    except OracleError as e:
        return None, str(e)


@pytest.mark.parametrize("row", ALL_ROWS, ids=lambda r: r.name)
def test_every_row_reaches_what_it_claims(oracle, row):
    inp, m = cr.model_of(oracle, row)
    got = cr.conditions(m)
    print(row.name, row.kernel, dict(sorted(got.items())))
    for key, least in row.claims.items():
        assert got.get(key, 0) >= least, (row.name, key, got.get(key, 0))
    # the model against the oracle: the same indices, or the same error -- and an error row holds one kind of error only,
    # since the reference raises the first in slice order and the library reports a fixed one of those it met
    want, err = _oracle_outcome(oracle, row, inp)
    assert cr.first_error(m) == row.raises
    if row.raises:
        assert err is not None and cr.ERROR_TEXT[row.raises] in err, (row.name, err)
        assert {e for e in m.error if e} == {row.raises}
    else:
        assert err is None and np.array_equal(want, m.final), row.name
    # the threshold -- the smallest index whose bytes fit -- against the oracle's index itself wherever the refinement
    # moves nothing (the oracle's index is then its bisection's result), and against the model's bisection everywhere
    direct = 0
    for s in range(m.g.n_slices):
        trials, q, e = cr.reference_walk(m, s)
        if e is None:
            assert q == m.T[s], (row.name, s, q, m.T[s])
        if want is not None and len(m.refine_trials[s]) == 2:      # T and T + 1 measured, T kept
            assert want[s] == m.T[s], (row.name, s, want[s], m.T[s])
            direct += 1
    if want is not None and row.name != "refine":
        assert direct >= m.g.n_slices // 2, (row.name, direct)
    if isinstance(row, cr.PictureRow):
        assert max(int(np.abs(p).max()) for p in inp[1]) < 1 << 29    # the model's quantiser domain


def test_marked_rows(oracle):
    many = cr.model_of(oracle, cr.ROWS["marked-many"])[1]
    assert many.g.n_slices == 512 and many.marked[:256].all() and 200 <= many.marked.sum() < 512   # four full ballot words and a sparse tail
    assert 0 < many.marked[256:].sum() < 64
    one = cr.model_of(oracle, cr.ROWS["marked-one"])[1]
    assert one.marked.sum() == 1 and one.marked[77] and one.why[77] == "escape"
    reset = cr.model_of(oracle, cr.ROWS["reset"])[1]
    assert all(reset.guess[s] == -1 for s in range(reset.g.n_slices) if s % 8 in (0, 3, 6))   # bisected again behind a hand-back
    assert all(reset.guess[s] >= 0 for s in range(reset.g.n_slices) if s % 8 in (1, 2, 4, 5, 7))


def test_coverage_over_all_rows(oracle):
    total, per_kernel = {}, {}
    for row in ALL_ROWS:
        c = cr.conditions(cr.model_of(oracle, row)[1])
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
            if k.startswith("class:"):
                per_kernel[(row.kernel, k[6:])] = per_kernel.get((row.kernel, k[6:]), 0) + v
    print("conditions:", dict(sorted(total.items())))
    print("classes per kernel:", dict(sorted(per_kernel.items())))
    for kernel in ("search16", "reg16", "reg32"):
        for cls in cr.CLASSES:
            assert per_kernel.get((kernel, cls), 0) >= MIN, (kernel, cls)
    for key in CONDITIONS:
        assert total.get(key, 0) >= MIN, key
    # tight positions per kernel (reg16's rows have no head at depth 2, and no exact placement: heads on search16 and reg32)
    tight = {}
    for row in ALL_ROWS:
        for k, v in cr.conditions(cr.model_of(oracle, row)[1]).items():
            if k.startswith("tight:"):
                tight[(row.kernel, k[6:])] = tight.get((row.kernel, k[6:]), 0) + v
    print("tight positions per kernel:", dict(sorted(tight.items())))
    for kernel in ("search16", "reg32"):
        for key in [f"{c}:{p}" for c in "YUV" for p in ("none", "head", "first", "last")] + ["only-V-head"]:
            assert tight.get((kernel, key), 0) >= MIN, (kernel, key)
    for key in [f"{c}:last" for c in "YUV"]:
        assert tight.get(("reg16", key), 0) >= MIN, key
    # gallops of 32 and more on k_cbr_search16's own copy of the loop as well as on k_cbr_search_reg's
    for kernel in ("search16", "reg32"):
        for key in ("up:32+", "down:32+"):
            assert sum(cr.conditions(cr.model_of(oracle, r)[1]).get(key, 0) for r in ALL_ROWS if r.kernel == kernel) >= MIN, (kernel, key)
    # the scalars of the fine-grained rows
    assert {1, 2, 3, 7} <= {r.scalar for r in cr.FINE_ROWS} and max(r.scalar for r in cr.FINE_ROWS) >= 64


@pytest.mark.parametrize("name", ["d4-DD97", "d3-16bit", "444"])
def test_bytes_never_grow_with_the_index(oracle, name):
    """the monotonicity the predecessor search rests on, asserted on the tables themselves"""
    m = cr.model_of(oracle, cr.ROWS[name])[1]
    top = 119 + m.qm_min
    need = m.units[:top + 1].astype(np.int64).sum(axis=2)
    assert (need >= 0).all() and (np.diff(need, axis=0) <= 0).all()
    assert (np.diff(m.units[:top + 1].astype(np.int64), axis=0) <= 0).all()      # and no component's do


def test_generators_are_deterministic(oracle):
    for name in ("positions", "gallop", "refine"):
        a, b = cr.fine_input(oracle, cr.ROWS[name]), cr.fine_input(oracle, cr.ROWS[name])
        assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and np.array_equal(a[4], b[4])
    for name in ("d3", "d3-starved", "d3-16bit", "d4-designed"):
        row = cr.ROWS[name]
        first = cr.picture_raw(oracle, row)
        cr._raw_cache.clear()
        assert cr.picture_raw(oracle, row) == first
    # the designed pictures come back from the forward transform as designed (Haar0: no level shift, nothing clips)
    row = cr.ROWS["d4-designed"]
    g = cr.picture_geometry(oracle, row.w, row.h, row.cf, row.depth, row.u, row.a)
    want = cr.planes_from_records(g, cr._position_records(g, row.seed, 3))
    assert all(np.array_equal(x, y) for x, y in zip(cr.picture_input(oracle, row)[1], want))
