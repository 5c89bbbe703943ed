"""Timing of vc2hip_encode_recon_batch_dev on cfg 2 (UHD-1 3840x2160 4:2:2 10-bit HQ_ConstQ DD97 depth 4, -u 1 -a 2 -q 16
-S 2), 128 pictures per call.  Device events around each form, the forms alternated and the median of the repeats taken
(not the bench metric):
  (a) parent_enc_dec   encode_batch_dev + decode_batch_dev through ANOTHER build of the library (argv[1]: the parent
                       commit's libvc2hip.so; left out when no path is given), in the same process on the same box
  (b) enc_dec          the same two calls through this tree's library
  (c) recon_all        encode_recon_batch_dev: payload, lengths, picture, sums, indices
  (d) recon_only       encode_recon_batch_dev: picture and sums, no payload
  (e) enc_dec_torch    (b), then a torch expression that turns the two raw buffers into the three sums: what a caller did
                       before the call existed
then the per-kernel table of (c) and (d) from vc2hip_profile_* (TIME_RECON_PROFILE=0: without it)."""
import ctypes as C
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, vc2hip_py
from synth import synth_fast

W, H, N, REPS = 3840, 2160, int(os.environ.get("TIME_RECON_PICTURES", "128")), int(os.environ.get("TIME_RECON_REPS", "7"))
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
hip = vc2hip_py.Vc2Hip(0, stream=stream)  # (one stream: the torch pass and the calls in order)
fmt = vc2hip_py.picture_format(W, H, "422", 10)
cp = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, q=16, scalar=2)
rb = hip.raw_picture_bytes(fmt)
raws = [synth_fast(W, H, "422", 10, 900 + i) for i in range(4)]
d_raw = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(dev).view(4, rb)[torch.arange(N, device=dev) % 4].reshape(-1).contiguous()
stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
d_pay = torch.zeros(N * stride, dtype=torch.uint8, device=dev)
d_len = torch.zeros(N, dtype=torch.int64, device=dev)
d_out = torch.empty(N * rb, dtype=torch.uint8, device=dev)
d_sse = torch.zeros(N * 3, dtype=torch.int64, device=dev)
d_q = torch.zeros(N * cp.y_slices * cp.x_slices, dtype=torch.int32, device=dev)
PLANES = [H * W, H * W // 2, H * W // 2]


class Other:
    """the two batch calls of another build of the library (no binding of its own: it may lack newer entry points)"""

    def __init__(self, path):
        vp = C.c_void_p
        self.lib = C.CDLL(path)
        self.lib.vc2hip_create_on_stream.argtypes = [C.c_int, vp, C.POINTER(vp)]
        self.lib.vc2hip_sync.argtypes = [vp]
        self.lib.vc2hip_encode_batch_dev.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_size_t, vp]
        self.lib.vc2hip_decode_batch_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, vp, vp, vp]
        self.h = vp()
        assert self.lib.vc2hip_create_on_stream(0, vp(stream), C.byref(self.h)) == 0

    def enc_dec(self):
        assert self.lib.vc2hip_encode_batch_dev(self.h, d_raw.data_ptr(), N, C.byref(fmt), C.byref(cp), d_pay.data_ptr(), stride, d_len.data_ptr()) == 0
        assert self.lib.vc2hip_decode_batch_dev(self.h, d_pay.data_ptr(), stride, d_len.data_ptr(), N, C.byref(fmt), C.byref(cp), d_out.data_ptr()) == 0

    def sync(self):
        assert self.lib.vc2hip_sync(self.h) == 0


def enc_dec():
    hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, d_out.data_ptr())


def torch_sums():
    """per picture and component, the sum of squared differences of the 10-bit samples of two buffers of big-endian words"""
    def values(buf):
        b = buf.view(N, rb // 2, 2)
        return ((b[..., 0].to(torch.int32) << 8) | b[..., 1].to(torch.int32)) >> 6
    d = (values(d_raw) - values(d_out)).to(torch.int64)
    return torch.stack([(x * x).sum(dim=1) for x in torch.split(d, PLANES, dim=1)], dim=1)


def recon_all():
    hip.encode_recon_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr(), d_out.data_ptr(), d_sse.data_ptr(), d_q.data_ptr())


def recon_only():
    hip.encode_recon_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_recon=d_out.data_ptr(), d_sse=d_sse.data_ptr())


calls, syncs = {}, [hip.sync]
if len(sys.argv) > 1:
    other = Other(sys.argv[1])
    calls["a_parent_enc_dec"] = other.enc_dec
    syncs.append(other.sync)
calls.update({"b_enc_dec": enc_dec, "c_recon_all": recon_all, "d_recon_only": recon_only, "e_enc_dec_torch": lambda: (enc_dec(), torch_sums())})


def sync_all():
    for s in syncs:
        s()


for fn in calls.values():
    fn(); sync_all()                    # warm-up (sizes the workspaces)
# the forms agree before they are timed: the call's picture and sums are the two calls' and the torch expression's
enc_dec(); sync_all(); want_pic, want_sums = d_out.clone(), torch_sums()
recon_only(); sync_all()
assert torch.equal(d_out, want_pic) and torch.equal(d_sse.view(N, 3), want_sums), "encode_recon_batch_dev differs from encode + decode"
del want_pic
times = {k: [] for k in calls}
for _ in range(REPS):                   # the forms alternated
    for k, fn in calls.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync_all()
        a.record(torch.cuda.current_stream()); fn(); b.record(torch.cuda.current_stream()); b.synchronize()
        sync_all()                      # (errors of the call)
        times[k].append(a.elapsed_time(b))
result = {"pictures": N, "repeats": REPS,
          "median_ms": {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()},
          "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}}
if os.environ.get("TIME_RECON_PROFILE", "1") != "0":
    result["kernels_ms"] = {}
    for name in ("b_enc_dec", "c_recon_all", "d_recon_only"):
        hip.profile_enable(True); hip.profile_reset()
        for _ in range(3):
            calls[name]()
        hip.sync()
        result["kernels_ms"][name] = {kn: round(ms / 3, 3) for kn, (n, ms) in sorted(hip.profile().items())}
        hip.profile_enable(False)
print(json.dumps(result))
