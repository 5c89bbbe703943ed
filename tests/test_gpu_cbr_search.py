"""GPU tests of the HQ_CBR quantiser search kernels (vc2_launch_cbr, csrc/vc2hip_slices.hip and csrc/vc2hip_cbr16.h) at their
edges, against the oracle, exactly: quantiser indices against oracle.cbr_qindices, payload bytes against oracle.encode_stream
(every slice header's index byte lies in the payload), and where the oracle raises, a Vc2HipError with the oracle's text.

The inputs are the rows of tests/cbr_ref.py; tests/test_cbr_ref.py shows without a GPU that each reaches the kernel and the
search edges its row names (last non-zero coefficient in every head and run, thresholds 0 and "none fits", gallops by 1,
2 - 7 and 32 or more in both directions, the guess reset behind a hand-back, every hand-back class, one and 263 marked
slices, the refinement's strict `<` and a refinement by three).  Every input runs on three contexts -- the default, the
general kernel alone (CBR_GENERAL) and the int32 store (STORE32) -- which must agree with the oracle and so with each
other; the library's own records say which path ran: hip.dwt_launches() the store, hip.profile() the number of search
launches (two on a register path: the register kernel and the pass over what it marked; one on the general path)."""
import numpy as np
import pytest

import cbr_ref as cr
from vc2lib import KERNELS, OracleError

pytestmark = pytest.mark.gpu

CONTEXTS = {"default": (), "general": ("CBR_GENERAL",), "store32": ("STORE32",)}
REGISTER = ("search16", "reg16", "reg32")


@pytest.fixture(scope="module")
def ctxs():
    from vc2hip_py import FLAGS, Vc2Hip
    out = {name: Vc2Hip(flags=sum(FLAGS[f] for f in flags)) for name, flags in CONTEXTS.items()}
    yield out
    for h in out.values():
        h.close()


def _searches(hip, call):
    """(call()'s result, the library's error if it raised one, the number of cbr_search launches it made)"""
    from vc2hip_py import Vc2HipError
    hip.profile_reset()
    hip.profile_enable(True)
    res = err = None
    try:
        res = call()
    except Vc2HipError as e:      # handed to the caller, who says what it must be
        err = e
    finally:
        hip.profile_enable(False)
    return res, err, hip.profile().get("cbr_search", (0, 0.0))[0]


def _launches_for(ctx, kernel):
    """the launches vc2_launch_cbr makes on a context for a geometry whose default kernel is `kernel`"""
    if ctx == "general":
        return 1
    return 2 if kernel in REGISTER else 1     # STORE32 keeps the register path (reg32)


def _expect(row, res, err, name):
    if row.raises:
        assert err is not None, (row.name, name)
        assert cr.ERROR_TEXT[row.raises] in str(err), (row.name, name, str(err))
        return False
    if err is not None:
        raise err
    return True


# ---- the fine-grained call: k_cbr_search_reg<int32_t> and the general kernels on exact coefficient planes
@pytest.mark.parametrize("row", cr.FINE_ROWS, ids=lambda r: r.name)
def test_fine_grained_rows(ctxs, oracle, row):
    g, planes, qm, scalar, sb = cr.fine_input(oracle, row)
    assert cr.kernel_for(g, qm, False)[0] == row.kernel == "reg32"
    try:
        want = oracle.cbr_qindices(*planes, g.depth, qm, sb, scalar)
    except OracleError as e:
        assert row.raises and cr.ERROR_TEXT[row.raises] in str(e)
        want = None
    for name, hip in ctxs.items():
        got, err, n = _searches(hip, lambda: hip.cbr_qindices(*planes, g.depth, qm, sb, scalar))
        assert n == _launches_for(name, row.kernel), (row.name, name, n)
        if _expect(row, got, err, name):
            bad = np.flatnonzero((got != want).ravel())
            assert bad.size == 0, (row.name, name, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


@pytest.mark.parametrize("kernel,geom", [cr.GENERAL_GEOM, cr.GLOBAL_GEOM], ids=["general", "global"])
def test_geometries_the_register_kernels_refuse(ctxs, oracle, kernel, geom):
    """one launch on every context: the LDS kernel for chroma records beyond 256 coefficients, the global-memory kernel for a
    slice no LDS holds"""
    g = cr.Geometry(*geom)
    qm = oracle.quant_matrix(KERNELS["DD97"], g.depth)
    assert cr.kernel_for(g, qm, False)[0] == kernel
    planes = cr.planes_from_records(g, cr._laplace_records(g, np.random.default_rng(70), 500))
    scalar = 40 if kernel == "general" else 1000      # (the one slice's components take ~30 KB each: a length byte of ~30)
    sb = oracle.slice_bytes(g.ys, g.xs, g.n_slices * g.slice_coefs // 6 + 5 if kernel == "general" else 100000, scalar)
    want = oracle.cbr_qindices(*planes, g.depth, qm, sb, scalar)
    for name, hip in ctxs.items():
        got, err, n = _searches(hip, lambda: hip.cbr_qindices(*planes, g.depth, qm, sb, scalar))
        assert err is None and n == 1 and np.array_equal(got, want), (kernel, name, err, n)


# ---- whole pictures: k_cbr_search16 and k_cbr_search_reg<int16_t>
def _fmt_cp(hip, row):
    import vc2hip_py
    fmt = vc2hip_py.picture_format(row.w, row.h, row.cf, row.bits, 2)
    return fmt, vc2hip_py.coding_params(hip.lib, fmt, row.wavelet, row.depth, row.u, row.a, **row.coding())


def _oracle_payload(oracle, row, raw):
    g = cr.picture_geometry(oracle, row.w, row.h, row.cf, row.depth, row.u, row.a)
    sb = oracle.slice_bytes(g.ys, g.xs, row.s, row.scalar)
    try:
        stream = oracle.encode_stream(row.params(), raw, 1)
    except OracleError as e:
        assert row.raises and cr.ERROR_TEXT[row.raises] in str(e)
        return None, sb
    n = int(sb.sum()) + row.prefix * g.n_slices
    return stream[-13 - n:-13], sb


def _store_bits(hip):
    return {r["store_bits"] for r in hip.dwt_launches() if not r["inverse"]}


@pytest.mark.parametrize("row", cr.PICTURE_ROWS, ids=lambda r: r.name)
def test_picture_rows(ctxs, oracle, row):
    raw = cr.picture_raw(oracle, row)
    want, sb = _oracle_payload(oracle, row, raw)
    for name, hip in ctxs.items():
        fmt, cp = _fmt_cp(hip, row)
        got, err, n = _searches(hip, lambda: hip.encode_picture_hq(raw, fmt, cp))
        assert _store_bits(hip) == ({32} if name == "store32" else {16}), (row.name, name)
        assert n == _launches_for(name, row.kernel), (row.name, name, n)
        if _expect(row, got, err, name):
            payload, qidx = got
            idx, widx = cr.payload_indices(payload, sb, row.prefix), cr.payload_indices(want, sb, row.prefix)
            bad = np.flatnonzero(idx != widx) if len(payload) == len(want) else np.arange(1)
            assert bad.size == 0, (row.name, name, len(payload), len(want), bad[:8], idx[bad[:8]], widx[bad[:8]])
            assert payload == want, (row.name, name)
            assert np.array_equal(qidx.ravel(), widx), (row.name, name)


def test_a_batch_of_three_different_pictures(ctxs, oracle):
    import torch
    rows = cr.BATCH_ROWS
    raws = [cr.picture_raw(oracle, r) for r in rows]
    wants = [_oracle_payload(oracle, r, raw)[0] for r, raw in zip(rows, raws)]
    assert len(set(wants)) == 3
    dev = torch.device("cuda:0")
    for name, hip in ctxs.items():
        fmt, cp = _fmt_cp(hip, rows[0])
        stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
        d_raw = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(dev)
        d_pay = torch.zeros(3 * stride, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(3, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        _, err, n = _searches(hip, lambda: (hip.encode_batch_dev(d_raw.data_ptr(), 3, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr()), hip.sync()))
        assert err is None and n == _launches_for(name, "search16"), (name, err, n)
        assert _store_bits(hip) == ({32} if name == "store32" else {16}), name
        lens, pay = d_len.cpu().tolist(), d_pay.cpu().numpy()
        for k in range(3):
            assert lens[k] == len(wants[k]) and pay[k * stride:k * stride + lens[k]].tobytes() == wants[k], (name, k)


def test_the_indices_of_the_recon_call(ctxs, oracle):
    """vc2hip_encode_recon_batch_dev's d_qidx, element by element, against oracle.cbr_qindices on the coefficient planes
    oracle.dwt_forward yields: 324 slices per picture, the last wavefront of each holds four"""
    import torch
    rows = cr.RECON_ROWS
    raws = [cr.picture_raw(oracle, r) for r in rows]
    wants = []
    for r, raw in zip(rows, raws):
        g, planes, qm, scalar, sb = cr.picture_input(oracle, r, raw)
        wants.append(oracle.cbr_qindices(*planes, g.depth, qm, sb, scalar).ravel())
    ns = wants[0].size
    assert ns % 8 == 4 and not np.array_equal(wants[0], wants[1])
    dev = torch.device("cuda:0")
    for name, hip in ctxs.items():
        fmt, cp = _fmt_cp(hip, rows[0])
        d_raw = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(dev)
        d_q = torch.full((2 * ns,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        _, err, n = _searches(hip, lambda: (hip.encode_recon_batch_dev(d_raw.data_ptr(), 2, fmt, cp, d_qidx=d_q.data_ptr()), hip.sync()))
        assert err is None and n == _launches_for(name, "search16"), (name, err, n)
        got = d_q.cpu().numpy()
        for k in range(2):
            assert np.array_equal(got[k * ns:(k + 1) * ns], wants[k]), (name, k)
