"""Timing of the batch calls under a packed format on cfg 2 (UHD-1 3840x2160 4:2:2 10-bit HQ_ConstQ DD97 depth 4, -u 1 -a 2
-q 16 -S 2), 128 pictures per call, encode and decode.  Device events around each form, the forms alternated and the median
(min - max) of the repeats taken (not the bench metric):
  (a) v210     vc2hip_set_packed_format(V210, rows pitched to 128 bytes), the batch call on the v210 buffer itself
  (b) p210     vc2hip_set_packed_format(SEMIPLANAR, little-endian, MSB-justified), the batch call on the P210 buffer
  (c) planar   the planar little-endian LSB-justified call (vc2hip_set_sample_layout) -- of the library given with
               --planar-lib (the parent commit's build, for the cost of the feature to callers who do not use it and as
               the yardstick of (a) and (b)), else of this tree's
  (d) torch    an eager torch v210 conversion (shifts, masks and strided copies) in front of / behind (c): what a caller
               with v210 in HBM had before
Then the new kernels' own times from vc2hip_profile_* and their bytes per second (bytes read + written over the kernel's
time), beside --copy-gbps: what tools/probe/stream_bw.hip reached for a plain copy on the same box, read + write, from its
best time and the bytes its kernel moves (2 x 4096 x 256 x 1 KiB per launch; the probe's own printout counts the whole
7680-byte row span of which a wavefront touches 1 KiB).
Writes one JSON line; --out FILE also stores it."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, vc2hip_py
import layout_ref, packed_ref
from synth import synth_fast

ap = argparse.ArgumentParser()
ap.add_argument("--planar-lib", help="libvc2hip.so of the parent commit for form (c)")
ap.add_argument("--copy-gbps", type=float, help="tools/probe/stream_bw.hip on this box, GB/s read + write")
ap.add_argument("--pictures", type=int, default=128)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--out")
args = ap.parse_args()

W, H, BITS = 3840, 2160, 10
CW = W // 2
N, REPS = args.pictures, args.repeats
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
hip = vc2hip_py.Vc2Hip(0, stream=stream)          # (one stream: the torch passes and the calls in order)
if args.planar_lib:                               # a second library in the same process: its own context on the same stream
    import ctypes as C

    def load_planar():                            # (an older build: only the calls form (c) makes)
        lib = C.CDLL(os.path.abspath(args.planar_lib))
        ours = hip.lib
        for name in ("vc2hip_create_on_stream", "vc2hip_destroy", "vc2hip_last_error", "vc2hip_sync", "vc2hip_set_sample_layout",
                     "vc2hip_encode_batch_dev", "vc2hip_decode_batch_dev"):
            getattr(lib, name).argtypes = getattr(ours, name).argtypes
            getattr(lib, name).restype = getattr(ours, name).restype
        return lib

    keep, vc2hip_py.load_library = vc2hip_py.load_library, load_planar
    hip_c = vc2hip_py.Vc2Hip(0, stream=stream)
    vc2hip_py.load_library = keep
else:
    hip_c = vc2hip_py.Vc2Hip(0, stream=stream)
fmt = vc2hip_py.picture_format(W, H, "422", BITS)
cp = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, q=16, scalar=2)
LE_LSB = vc2hip_py.sample_layout(True, True)
PITCH = vc2hip_py.v210_pitch(W)
V210 = vc2hip_py.packed_format("v210", pitch=(PITCH, 0))
P210 = vc2hip_py.packed_format("semiplanar", little_endian=True)
GROUPS = (W + 5) // 6

# four pictures, repeated: the file format -> planar LE / LSB, v210 and P210 through the tests' model (host, once)
raws = b"".join(synth_fast(W, H, "422", BITS, 900 + i) for i in range(4))


def tile(a):
    t = torch.from_numpy(a).to(dev).view(4, -1)
    return t[torch.arange(N, device=dev) % 4].reshape(-1).contiguous()


d_planar = tile(layout_ref.to_layout(raws, fmt, 4, LE_LSB))
d_v210 = tile(packed_ref.to_packed(raws, fmt, 4, V210))
d_p210 = tile(packed_ref.to_packed(raws, fmt, 4, P210))
rb = d_planar.numel() // N


def v210_to_planar(src, dst):
    """eager torch: v210 rows -> Y, U, V int16 planes (little-endian, LSB-justified), picture by picture layout of `dst`"""
    w = src.view(torch.int32).view(N, H, PITCH // 4)[:, :, :GROUPS * 4].view(N, H, GROUPS, 4)
    f = lambda k, s: (w[..., k] >> s) & 1023   # noqa: E731
    out = dst.view(torch.int16).view(N, rb // 2)
    y = out[:, :H * W].view(N, H, GROUPS, 6)
    u = out[:, H * W:H * W + H * CW].view(N, H, GROUPS, 3)
    v = out[:, H * W + H * CW:].view(N, H, GROUPS, 3)
    for k, (word, shift) in enumerate(((0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20))):
        y[..., k] = f(word, shift)
    for k, (word, shift) in enumerate(((0, 0), (1, 10), (2, 20))):
        u[..., k] = f(word, shift)
    for k, (word, shift) in enumerate(((0, 20), (2, 0), (3, 10))):
        v[..., k] = f(word, shift)


def planar_to_v210(src, dst):
    s = src.view(torch.int16).view(N, rb // 2)
    y = s[:, :H * W].view(N, H, GROUPS, 6).to(torch.int32)
    u = s[:, H * W:H * W + H * CW].view(N, H, GROUPS, 3).to(torch.int32)
    v = s[:, H * W + H * CW:].view(N, H, GROUPS, 3).to(torch.int32)
    w = dst.view(torch.int32).view(N, H, PITCH // 4)[:, :, :GROUPS * 4].view(N, H, GROUPS, 4)
    w[..., 0] = u[..., 0] | y[..., 0] << 10 | v[..., 0] << 20
    w[..., 1] = y[..., 1] | u[..., 1] << 10 | y[..., 2] << 20
    w[..., 2] = v[..., 1] | y[..., 3] << 10 | u[..., 2] << 20
    w[..., 3] = y[..., 4] | v[..., 2] << 10 | y[..., 5] << 20


assert W % 6 == 0, "the torch conversion above views a row as whole groups"
stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
d_pay = {k: torch.zeros(N * stride, dtype=torch.uint8, device=dev) for k in "abcd"}
d_len = {k: torch.zeros(N, dtype=torch.int64, device=dev) for k in "abcd"}
d_out = {"a": torch.zeros_like(d_v210), "b": torch.zeros_like(d_p210), "c": torch.zeros_like(d_planar), "d": torch.zeros_like(d_v210)}
d_tmp = torch.zeros_like(d_planar)


def packed_call(pf, fn):
    hip.set_packed_format(pf)       # (pure host state: nothing launched, nothing waited for)
    fn()
    hip.set_packed_format(None)


def planar_call(fn):
    hip_c.set_sample_layout(LE_LSB)
    fn()
    hip_c.set_sample_layout(None)


def E(h, src, k):
    return lambda: h.encode_batch_dev(src.data_ptr(), N, fmt, cp, d_pay[k].data_ptr(), stride, d_len[k].data_ptr())


def D(h, dst):
    return lambda: h.decode_batch_dev(d_pay["c"].data_ptr(), stride, d_len["c"].data_ptr(), N, fmt, cp, dst.data_ptr())


enc = {
    "a_v210": lambda: packed_call(V210, E(hip, d_v210, "a")),
    "b_p210": lambda: packed_call(P210, E(hip, d_p210, "b")),
    "c_planar": lambda: planar_call(E(hip_c, d_planar, "c")),
    "d_torch": lambda: (v210_to_planar(d_v210, d_tmp), planar_call(E(hip_c, d_tmp, "d"))),
}
dec = {
    "a_v210": lambda: packed_call(V210, D(hip, d_out["a"])),
    "b_p210": lambda: packed_call(P210, D(hip, d_out["b"])),
    "c_planar": lambda: planar_call(D(hip_c, d_out["c"])),
    "d_torch": lambda: (planar_call(D(hip_c, d_tmp)), planar_to_v210(d_tmp, d_out["d"])),
}
result = {"pictures": N, "repeats": REPS, "planar_lib": "parent" if args.planar_lib else "this tree", "median_ms": {}, "min_max_ms": {}}
for direction, calls in (("encode", enc), ("decode", dec)):
    for fn in calls.values():
        fn(); hip.sync(); hip_c.sync()          # warm-up (sizes the workspaces)
    times = {k: [] for k in calls}
    for _ in range(REPS):                       # the forms alternated
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hip.sync(); hip_c.sync()
            a.record(torch.cuda.current_stream()); fn(); b.record(torch.cuda.current_stream()); b.synchronize()
            hip.sync(); hip_c.sync()            # (errors of the call)
            times[k].append(a.elapsed_time(b))
    result["median_ms"][direction] = {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()}
    result["min_max_ms"][direction] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
# the four forms computed the same thing
for k in "abd":
    assert torch.equal(d_len[k], d_len["c"]) and torch.equal(d_pay[k], d_pay["c"]), f"the payload of form {k} differs from the planar call's"
assert torch.equal(d_out["a"], d_out["d"]), "the v210 pictures decoded by the library differ from the torch conversion's"
v210_to_planar(d_out["a"], d_tmp)
assert torch.equal(d_tmp, d_out["c"]), "the pictures decoded under v210 differ from the planar call's"

# the new kernels' own times (events on every launch of the four, nothing else)
plane_bytes = 2 * (H * W + 2 * H * CW)
moved = {"v210_unpack": H * GROUPS * 16 + plane_bytes, "v210_pack": H * GROUPS * 16 + plane_bytes,
         "uv_deinterleave": 2 * (2 * H * CW * 2), "uv_interleave": 2 * (2 * H * CW * 2)}   # bytes read + written per picture
kern = {}
for name, (pf, calls) in {"v210_unpack": (V210, enc), "v210_pack": (V210, dec), "uv_deinterleave": (P210, enc), "uv_interleave": (P210, dec)}.items():
    form = "a_v210" if pf is V210 else "b_p210"
    hip.profile_reset(); hip.profile_enable(True); hip.profile_only(name)
    for _ in range(REPS):
        calls[form]()
    hip.sync()
    launches, ms = hip.profile().get(name, (0, 0.0))
    hip.profile_enable(False); hip.profile_only(None)
    per = ms / max(launches, 1)
    kern[name] = {"ms_per_launch": round(per, 4), "gb_per_s": round(N * moved[name] / per / 1e6, 1) if per else None}
if args.copy_gbps:
    for v in kern.values():
        v["fraction_of_copy_probe"] = round(v["gb_per_s"] / args.copy_gbps, 2) if v["gb_per_s"] else None
result["kernels"] = kern
result["copy_probe_gb_per_s"] = args.copy_gbps
line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
