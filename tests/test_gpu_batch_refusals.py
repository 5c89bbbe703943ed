"""GPU test of what the six device batch calls refuse in their arguments (vc2hip_encode_batch_dev, _encode_recon_, _encode_fields_,
vc2hip_decode_batch_dev, _decode_reduced_, _decode_fields_): one fault at a time, on a context with one stream and on one with
vc2hip_set_streams(3).  Every call but the last is refused before anything is launched; a refused call must leave the
context usable -- vc2hip_sync returns OK after each, and at the end both contexts code three pictures to the oracle's bytes.

The return code and the vc2hip_last_error text of every (entry, case, lanes) are pinned by tests/golden/batch_refusals.json.
The table was recorded from the library as it was BEFORE the calls' front ends were folded into one lane split and one
argument check (`VC2HIP_LIB=<that build> python tests/test_gpu_batch_refusals.py > tests/golden/batch_refusals.json`):
it is what a change to those front ends has to keep.

Geometry: the smallest on which all six calls are valid.  64 x 32, 4:2:2, 10 bits in 2-byte words, LeGall, depth 2, 16 x 16
luma slices; 3 items per call -- for the field calls 3 frames of 64 x 32, so 6 slots.  Every buffer is really allocated,
with 64 bytes of slack; a misaligned pointer is base + 8 (+ 4 under the 8-byte rule of lengths and squared errors, + 2 under
the 4-byte rule of the indices), so it still lies inside its allocation."""
import ctypes as C
import json
import os

import pytest

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_refusals.json")
W, H, CFMT, BITS, KERNEL, DEPTH, U, A, N, DROP = 64, 32, "422", 10, "LeGall", 2, 4, 4, 3, 1
Q, SCALAR = 9, 2
LANES = (1, 3)

# entry -> (C function, its arguments after the context, in order).  "fmt" is the frame's format for the field calls and
# "cp" one field's coding parameters there; "raw" is the input pictures, "out" the decoded ones.
ENTRIES = {
    "encode": ("vc2hip_encode_batch_dev", ("raw", "n", "fmt", "cp", "payload", "stride", "lens")),
    "encode_recon": ("vc2hip_encode_recon_batch_dev", ("raw", "n", "fmt", "cp", "payload", "stride", "lens", "recon", "sse", "qidx")),
    "encode_fields": ("vc2hip_encode_fields_batch_dev", ("raw", "n", "fmt", "tff", "cp", "payload", "stride", "lens")),
    "decode": ("vc2hip_decode_batch_dev", ("payload", "stride", "lens", "n", "fmt", "cp", "out")),
    "decode_reduced": ("vc2hip_decode_reduced_batch_dev", ("payload", "stride", "lens", "n", "fmt", "cp", "drop", "out")),
    "decode_fields": ("vc2hip_decode_fields_batch_dev", ("payload", "stride", "lens", "n", "fmt", "tff", "cp", "out")),
}
BUFFERS = {"raw": 8, "payload": 8, "out": 8, "recon": 8, "lens": 4, "sse": 4, "qidx": 2}   # buffer -> its misaligning offset
REQUIRED = {   # the pointers a call cannot do without (the lengths: of an HQ picture)
    "encode": ("raw", "fmt", "cp", "payload", "lens"), "encode_recon": ("raw", "fmt", "cp"),
    "encode_fields": ("raw", "fmt", "cp", "payload", "lens"),
    "decode": ("payload", "lens", "fmt", "cp", "out"), "decode_reduced": ("payload", "lens", "fmt", "cp", "out"),
    "decode_fields": ("payload", "lens", "fmt", "cp", "out"),
}


def cases(entry):
    """[(case, {argument: what replaces it})]: None a null pointer, ("+", k) the argument plus k, ("=", name) another argument's
    value, a dict the fields of fmt / cp to change; "layout" / "packed": the context's sample layout / packed format"""
    args = ENTRIES[entry][1]
    out = [(f"null_{p}", {p: None}) for p in REQUIRED[entry]]
    out.append(("n_0", {"n": 0}))
    out += [(f"misaligned_{p}", {p: ("+", BUFFERS[p])}) for p in args if p in BUFFERS]
    out.append(("stride_plus_8", {"stride": ("+", 8)}))
    out.append(("kernel_7", {"cp": dict(kernel=7)}))
    out.append(("layout_pitch_below_row", {"layout": dict(pitch=(16, 0, 0))}))
    out.append(("v210_on_12_bits", {"packed": "v210", "fmt": dict(bit_depth=12)}))
    if entry == "decode_reduced":
        out += [("drop_0", {"drop": 0}), ("drop_depth", {"drop": DEPTH}), ("daub97", {"cp": dict(kernel=6)}),
                ("width_not_multiple", {"fmt": dict(width=W - 2)})]
    if entry in ("encode_fields", "decode_fields"):
        out.append(("odd_frame_height", {"fmt": dict(height=H - 1)}))
    if entry == "encode_recon":
        out += [("no_output", {"payload": None, "stride": 0, "lens": None, "recon": None, "sse": None, "qidx": None}),
                ("sse_without_recon", {"recon": None}), ("payload_without_lens", {"lens": None}),
                ("recon_overlaps_raw", {"recon": ("=", "raw")}), ("chroma_depth_with_recon", {"fmt": dict(chroma_bit_depth=8)})]
    if entry.startswith("encode"):
        out.append(("capped_0_bytes", {"cp": dict(mode=3, compressed_bytes=0)}))
    return out


ALL = [(e, name) for e in ENTRIES for name, _ in cases(e)]


class Bench:
    """the two contexts, the formats and the device buffers all cases share"""

    def __init__(self):
        import torch
        import vc2hip_py
        self.py = vc2hip_py
        self.ctx = {1: vc2hip_py.Vc2Hip(0), 3: vc2hip_py.Vc2Hip(0)}
        self.ctx[3].set_streams(3)
        hip = self.ctx[1]
        self.fmt = vc2hip_py.picture_format(W, H, CFMT, BITS)
        self.field = vc2hip_py.picture_format(W, H // 2, CFMT, BITS)
        self.cp = vc2hip_py.coding_params(hip.lib, self.fmt, KERNEL, DEPTH, U, A, q=Q, scalar=SCALAR)
        self.cp_field = vc2hip_py.coding_params(hip.lib, self.field, KERNEL, DEPTH, U, A, q=Q, scalar=SCALAR)
        self.rb = hip.raw_picture_bytes(self.fmt)
        self.stride = (hip.max_payload_bytes(self.fmt, self.cp) + 255) // 256 * 256
        ns = self.cp.y_slices * self.cp.x_slices
        sizes = {"raw": N * self.rb, "out": N * self.rb, "recon": N * self.rb, "payload": 2 * N * self.stride, "lens": 2 * N * 8,
                 "sse": N * 24, "qidx": N * ns * 4}
        self.buf = {k: torch.zeros(v + 64, dtype=torch.uint8, device="cuda:0") for k, v in sizes.items()}
        torch.cuda.synchronize()

    def values(self, entry):
        fields = entry.endswith("fields")
        v = {k: t.data_ptr() for k, t in self.buf.items()}
        v.update(n=N, stride=self.stride, tff=1, drop=DROP, fmt=self.fmt, cp=self.cp_field if fields else self.cp)
        return v

    def call(self, entry, change, lanes):
        """the entry's call with one thing changed -> (return code, vc2hip_last_error); the context's layout state is put back"""
        py, hip = self.py, self.ctx[lanes]
        v = self.values(entry)
        for k, how in change.items():
            if k in ("layout", "packed"):
                continue
            if isinstance(how, dict):
                s = type(v[k]).from_buffer_copy(v[k])
                for f, x in how.items():
                    setattr(s, f, x)
                v[k] = s
            elif isinstance(how, tuple):
                v[k] = v[k] + how[1] if how[0] == "+" else v[how[1]]
            else:
                v[k] = how
        if "layout" in change:
            hip.set_sample_layout(py.sample_layout(**change["layout"]))
        if "packed" in change:
            hip.set_packed_format(py.packed_format(change["packed"]))
        fn, names = ENTRIES[entry]
        args = [C.byref(v[k]) if isinstance(v[k], C.Structure) else v[k] for k in names]
        try:
            rc = getattr(hip.lib, fn)(hip.h, *args)
            text = hip.lib.vc2hip_last_error(hip.h).decode()
        finally:
            hip.set_sample_layout(None)
            hip.set_packed_format(None)
        return rc, text

    def close(self):
        for hip in self.ctx.values():
            hip.close()


@pytest.fixture(scope="module")
def bench():
    pytest.importorskip("torch")
    b = Bench()
    yield b
    b.close()


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return {(r["entry"], r["case"], r["lanes"]): (r["code"], r["text"]) for r in json.load(f)}


def test_table_covers_every_case(table):
    assert set(table) == {(e, name, lanes) for e, name in ALL for lanes in LANES}
    assert all(code != 0 for code, _ in table.values())          # (every recorded call was a refusal)


@pytest.mark.parametrize("entry,case", ALL, ids=[f"{e}-{name}" for e, name in ALL])
def test_refusal(bench, table, entry, case):
    change = dict(cases(entry))[case]
    for lanes in LANES:
        got = bench.call(entry, change, lanes)
        print(f"{entry} {case} lanes {lanes}: {got}")
        assert got == table[(entry, case, lanes)], (entry, case, lanes)
        bench.ctx[lanes].sync()                                   # (raises unless vc2hip_sync returns VC2HIP_OK)


def test_contexts_still_code_to_the_oracles_bytes(bench, oracle):
    """after all the refusals above: one valid encode_batch_dev + decode_batch_dev of the 3 pictures on each context"""
    import torch
    from synth import synth
    from vc2lib import make_params
    raw = synth(W, H, CFMT, BITS, 23, frames=N)
    p = make_params(W, H, CFMT, BITS, KERNEL, DEPTH, U, A, q=Q, scalar=SCALAR)
    stream = oracle.encode_stream(p, raw, N)
    want = oracle.decode_stream(p, stream, N)[0]
    bodies, pos = [], 0                                           # the picture data units of the oracle's stream
    while stream[pos + 4] != 0x10:
        nxt = int.from_bytes(stream[pos + 5:pos + 9], "big")
        if stream[pos + 4] == 0xE8:
            bodies.append(stream[pos + 13:pos + nxt])
        pos += nxt
    assert len(bodies) == N
    d_raw = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda:0")
    rb, stride = bench.rb, bench.stride
    for lanes in LANES:
        hip, b = bench.ctx[lanes], bench.buf
        for t in (b["payload"], b["lens"], b["out"]):
            t.zero_()
        torch.cuda.synchronize()
        hip.encode_batch_dev(d_raw.data_ptr(), N, bench.fmt, bench.cp, b["payload"].data_ptr(), stride, b["lens"].data_ptr())
        hip.decode_batch_dev(b["payload"].data_ptr(), stride, b["lens"].data_ptr(), N, bench.fmt, bench.cp, b["out"].data_ptr())
        hip.sync()
        lens = b["lens"][:N * 8].cpu().numpy().view("<u8").tolist()
        pay = b["payload"].cpu().numpy()
        for k in range(N):
            assert 0 < lens[k] <= stride and pay[k * stride:k * stride + lens[k]].tobytes() == bodies[k][-lens[k]:], (lanes, k)
        assert b["out"][:N * rb].cpu().numpy().tobytes() == want, lanes


if __name__ == "__main__":   # record the table from the library VC2HIP_LIB names (module docstring)
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(os.path.dirname(here), "vc2-reference_amd")]
    bench_ = Bench()
    rows = []
    for e_, name_ in ALL:
        for lanes_ in LANES:
            code_, text_ = bench_.call(e_, dict(cases(e_))[name_], lanes_)
            if code_ == 0:                                        # accepted: not a case for this table, and nothing more is run
                raise SystemExit(f"{e_} {name_} lanes {lanes_}: the call was accepted")
            bench_.ctx[lanes_].sync()
            rows.append(dict(entry=e_, case=name_, lanes=lanes_, code=code_, text=text_))
    bench_.close()
    sys.stdout.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")   # (one row per line)
