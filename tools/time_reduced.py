"""Timing of the reduced decoder on cfg 2 (UHD-1 3840x2160 4:2:2 10-bit HQ_ConstQ DD97 depth 4, -u 1 -a 2 -q 16 -S 2), 128
pictures per call.  Device events around each call, the forms alternated and the median of the repeats taken (not the
bench metric):
  (a) full        decode_batch_dev
  (b) reduced_k   decode_reduced_batch_dev at k = 1, 2, 3
  (c) full_pool_k decode_batch_dev, then torch avg_pool2d of the three planes by 2^k: what a caller did before the call
                  existed (its samples differ from (b)'s -- a box filter, not the wavelet's low-pass; here for its time only)
then the per-kernel table of (a) and (b) from vc2hip_profile_* (TIME_REDUCED_PROFILE=0: without it)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, vc2hip_py
from synth import synth_fast

W, H, N, REPS = 3840, 2160, 128, int(os.environ.get("TIME_REDUCED_REPS", "7"))
KS = (1, 2, 3)
dev = torch.device("cuda:0")
hip = vc2hip_py.Vc2Hip(0, stream=torch.cuda.current_stream().cuda_stream)  # (one stream: the torch pass and the calls in order)
fmt = vc2hip_py.picture_format(W, H, "422", 10)
cp = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, q=16, scalar=2)
rb = hip.raw_picture_bytes(fmt)
raws = [synth_fast(W, H, "422", 10, 900 + i) for i in range(4)]
d_raw = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(dev).view(4, rb)[torch.arange(N, device=dev) % 4].reshape(-1).contiguous()
stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
d_pay = torch.zeros(N * stride, dtype=torch.uint8, device=dev)
d_len = torch.zeros(N, dtype=torch.int64, device=dev)
hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr()); hip.sync()
del d_raw
d_out = torch.empty(N * rb, dtype=torch.uint8, device=dev)
d_red = torch.empty(N * rb // 4, dtype=torch.uint8, device=dev)
PLANES = [(H, W), (H, W // 2), (H, W // 2)]


def pool(k):
    """the decoded pictures' planes (big-endian 16-bit words) averaged over 2^k x 2^k blocks, as words again"""
    pics = d_out.view(N, rb)
    at, outs = 0, []
    for h, w in PLANES:
        b = pics[:, at:at + 2 * h * w].reshape(N, h, w, 2)
        v = (b[..., 0].to(torch.int32) << 8 | b[..., 1].to(torch.int32)).to(torch.float32)
        p = torch.nn.functional.avg_pool2d(v.unsqueeze(1), 1 << k).squeeze(1).round().to(torch.int32)
        outs.append(torch.stack((p >> 8, p & 255), dim=-1).to(torch.uint8).reshape(N, -1))
        at += 2 * h * w
    return torch.cat(outs, dim=1)


def full():
    hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, d_out.data_ptr())


def reduced(k):
    hip.decode_reduced_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, k, d_red.data_ptr())


calls = {"a_full": full}
for k in KS:
    calls[f"b_reduced_{k}"] = lambda k=k: reduced(k)
for k in KS:
    calls[f"c_full_pool_{k}"] = lambda k=k: (full(), pool(k))
for fn in calls.values():
    fn(); hip.sync()                    # warm-up (sizes the workspace)
times = {k: [] for k in calls}
for _ in range(REPS):                   # the forms alternated
    for k, fn in calls.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        a.record(torch.cuda.current_stream()); fn(); b.record(torch.cuda.current_stream()); b.synchronize()
        hip.sync()                      # (errors of the call)
        times[k].append(a.elapsed_time(b))
result = {"pictures": N, "repeats": REPS,
          "median_ms": {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()},
          "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}}
if os.environ.get("TIME_REDUCED_PROFILE", "1") != "0":
    result["kernels_ms"] = {}
    for name in ["a_full"] + [f"b_reduced_{k}" for k in KS]:
        hip.profile_enable(True); hip.profile_reset()
        for _ in range(3):
            calls[name]()
        hip.sync()
        result["kernels_ms"][name] = {kn: round(ms / 3, 3) for kn, (n, ms) in sorted(hip.profile().items())}
        hip.profile_enable(False)
print(json.dumps(result))
