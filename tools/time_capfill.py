"""Timing of VC2HIP_HQ_CAPPED_FILL against VC2HIP_HQ_CAPPED, and what the mode buys, on the set-up of
tools/time_cap.py: cfg 2 (UHD-1 3840x2160 4:2:2 10-bit DD97 depth 4, -u 1 -a 2 -S 2; the bench's generator, its first
TIME_CAP_DISTINCT frames cycled to 128 pictures per call), floor = the bench's index 16, cap = the median of the pictures'
ConstQ lengths at the floor.  Device events around each form, the two forms alternated in one session, median and min - max of
the repeats (not the bench metric):
  (a) capped   encode_batch_dev, mode HQ_Capped
  (b) filled   encode_batch_dev, mode HQ_CappedFill
then the per-kernel tables of both from vc2hip_profile_* (cap_measure3 and cap_fill: the third round and the fill of (b)), and
from one vc2hip_encode_recon_batch_dev call per mode, over the pictures that left the floor: mean d_lens / cap and the mean luma
PSNR from d_sse.  Before anything is timed: every filled length is at most the cap wherever the capped one is, and at least the
capped one."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch, vc2hip_py
from synth import synth_fast

W, H = 3840, 2160
N, REPS = int(os.environ.get("TIME_CAP_PICTURES", "128")), int(os.environ.get("TIME_CAP_REPS", "9"))
DISTINCT, FLOOR = int(os.environ.get("TIME_CAP_DISTINCT", "8")), 16
FLAGS = sum(vc2hip_py.FLAGS[f] for f in os.environ.get("TIME_CAP_FLAGS", "").split(",") if f)
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
hip = vc2hip_py.Vc2Hip(0, stream=stream, flags=FLAGS)
fmt = vc2hip_py.picture_format(W, H, "422", 10)
rb = hip.raw_picture_bytes(fmt)


def params(mode, q=0, s=0):
    return vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, mode=mode, q=q, s=s, scalar=2)


cp_q = params("HQ_ConstQ", q=FLOOR)
frames = synth_fast(W, H, "422", 10, 1234, frames=DISTINCT)
d_raw = torch.frombuffer(bytearray(frames), dtype=torch.uint8).to(dev).view(DISTINCT, rb)[torch.arange(N, device=dev) % DISTINCT].contiguous()
stride = (hip.max_payload_bytes(fmt, cp_q) + 255) // 256 * 256
d_pay = torch.zeros(N, stride, dtype=torch.uint8, device=dev)
d_len = torch.zeros(N, dtype=torch.int64, device=dev)
ns = cp_q.y_slices * cp_q.x_slices


def encode(cp):
    hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())


encode(cp_q); hip.sync()
floor_lens = d_len.cpu().numpy().copy()
CAP = int(np.median(floor_lens))
cps = {"a_capped": params("HQ_Capped", q=FLOOR, s=CAP), "b_filled": params("HQ_CappedFill", q=FLOOR, s=CAP)}

# what each mode gives: lengths, indices, squared errors (also the warm-up of the recon path; not timed)
d_rec = torch.empty(N * rb, dtype=torch.uint8, device=dev)
d_sse = torch.zeros(N, 3, dtype=torch.int64, device=dev)
d_q = torch.zeros(N, ns, dtype=torch.int32, device=dev)
got = {}
for name, cp in cps.items():
    hip.encode_recon_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr(), d_rec.data_ptr(), d_sse.data_ptr(), d_q.data_ptr())
    hip.sync()
    got[name] = (d_len.cpu().numpy().copy(), d_q.cpu().numpy().copy(), d_sse.cpu().numpy().copy())
del d_rec
len_a, q_a, sse_a = got["a_capped"]
len_b, q_b, sse_b = got["b_filled"]
assert (q_a == q_a[:, :1]).all(), "HQ_Capped: one index per picture"
assert ((len_b <= CAP) | (len_a > CAP)).all(), "a filled length passes the cap where the capped one does not"
assert (len_b >= len_a).all(), "a filled length below the capped one"
assert ((q_b == q_a) | (q_b == q_a - 1)).all(), "HQ_CappedFill: q_i or q_i - 1 in every slice"
left = q_a[:, 0] > FLOOR
assert (q_b[~left] == FLOOR).all() and (len_b[~left] == len_a[~left]).all(), "a picture at the floor changed"


def psnr_y(sse):
    return float(np.mean(10 * np.log10(1023.0 ** 2 * W * H / np.maximum(sse[left, 0].astype(np.float64), 1.0))))


bought = {"pictures_that_left_the_floor": int(left.sum()),
          "mean_len_over_cap": {"a_capped": round(float(np.mean(len_a[left] / CAP)), 7), "b_filled": round(float(np.mean(len_b[left] / CAP)), 7)},
          "mean_luma_psnr_db": {"a_capped": round(psnr_y(sse_a), 4), "b_filled": round(psnr_y(sse_b), 4)},
          "mean_promoted_slices": round(float(np.mean((q_b[left] == q_a[left] - 1).sum(axis=1))), 1), "slices": ns}

calls = {k: (lambda cp=cp: encode(cp)) for k, cp in cps.items()}
for fn in calls.values():
    fn(); hip.sync()                    # warm-up (sizes the workspaces)
times = {k: [] for k in calls}
for _ in range(REPS):                   # the forms alternated
    for k, fn in calls.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        a.record(torch.cuda.current_stream()); fn(); b.record(torch.cuda.current_stream()); b.synchronize()
        hip.sync()
        times[k].append(a.elapsed_time(b))
med = {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()}
result = {"pictures": N, "distinct": DISTINCT, "repeats": REPS, "floor": FLOOR, "cap": CAP, "flags": FLAGS,
          "indices": {str(int(t)): int((q_a[:, 0] == t).sum()) for t in np.unique(q_a[:, 0])},
          "median_ms": med, "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
          "filled_minus_capped_ms": round(med["b_filled"] - med["a_capped"], 3), "bought": bought, "kernels_ms": {}}
for name in calls:
    hip.profile_enable(True); hip.profile_reset()
    for _ in range(3):
        calls[name]()
    hip.sync()
    result["kernels_ms"][name] = {kn: round(ms / 3, 3) for kn, (n, ms) in sorted(hip.profile().items())}
    hip.profile_enable(False)
print(json.dumps(result))
