"""Timing of vc2hip_transcode_batch_dev on cfg 2 (UHD-1 3840x2160 4:2:2 10-bit DD97 depth 4, -u 1 -a 2 -S 2; the bench's
generator, its first TIME_TRANSCODE_DISTINCT frames cycled to 128 pictures per call).  The input is the batch encoded at
HQ_ConstQ 16.  Device events around each form, the forms alternated, median and min - max of the repeats (not the bench
metric):
  (a) transcode          to index 24
  (b) transcode_capped   floor 16, cap = the median of the lengths a transcode to index 20 gives
  (c) decode_encode      the route a caller had before: decode_batch_dev, then encode_batch_dev at HQ_ConstQ 24
  (d) decode             decode_batch_dev alone
then the per-kernel tables of (a) and (b) from vc2hip_profile_* (the slice index, hq_unpack, transcode_scale, hq_pack; capped:
also transcode_measure and transcode_pick).  Before timing: (a)'s output decodes without error, and no output length exceeds its input's.
The gate of DESIGN.md section 22: (a)'s slowest repeat below (c)'s fastest (the line's gate_a_max_below_c_min).
b_measure_passes is what the profile shows: the launches of transcode_measure per capped call."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch, vc2hip_py
from synth import synth_fast

W, H = 3840, 2160
N, REPS = int(os.environ.get("TIME_TRANSCODE_PICTURES", "128")), int(os.environ.get("TIME_TRANSCODE_REPS", "9"))
DISTINCT, Q_IN, Q_OUT, Q_CAP = int(os.environ.get("TIME_TRANSCODE_DISTINCT", "8")), 16, 24, 20
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
hip = vc2hip_py.Vc2Hip(0, stream=stream)
fmt = vc2hip_py.picture_format(W, H, "422", 10)
rb = hip.raw_picture_bytes(fmt)


def params(q):
    return vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, mode="HQ_ConstQ", q=q, scalar=2)


cp_in, cp_out = params(Q_IN), params(Q_OUT)
frames = synth_fast(W, H, "422", 10, 1234, frames=DISTINCT)
d_raw = torch.frombuffer(bytearray(frames), dtype=torch.uint8).to(dev).view(DISTINCT, rb)[torch.arange(N, device=dev) % DISTINCT].contiguous()
stride = (hip.max_payload_bytes(fmt, cp_in) + 255) // 256 * 256
d_in, d_out = torch.zeros(N, stride, dtype=torch.uint8, device=dev), torch.zeros(N, stride, dtype=torch.uint8, device=dev)
d_len_in, d_len_out = torch.zeros(N, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
d_dec = torch.empty_like(d_raw)

hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp_in, d_in.data_ptr(), stride, d_len_in.data_ptr()); hip.sync()
in_lens = d_len_in.cpu().numpy().copy()


def transcode(tp):
    hip.transcode_batch_dev(d_in.data_ptr(), stride, d_len_in.data_ptr(), N, fmt, cp_in, tp, d_out.data_ptr(), stride, d_len_out.data_ptr())


def decode(pay=d_in, lens=d_len_in):
    hip.decode_batch_dev(pay.data_ptr(), stride, lens.data_ptr(), N, fmt, cp_in, d_dec.data_ptr())


def decode_encode():
    decode()
    hip.encode_batch_dev(d_dec.data_ptr(), N, fmt, cp_out, d_out.data_ptr(), stride, d_len_out.data_ptr())


transcode(vc2hip_py.transcode_params(Q_CAP)); hip.sync()
CAP = int(np.median(d_len_out.cpu().numpy()))
tp_a, tp_b = vc2hip_py.transcode_params(Q_OUT), vc2hip_py.transcode_params(Q_IN, CAP)
calls = {"a_transcode": lambda: transcode(tp_a), "b_transcode_capped": lambda: transcode(tp_b), "c_decode_encode": decode_encode,
         "d_decode": decode}
for fn in calls.values():
    fn(); hip.sync()                    # warm-up (sizes the workspaces)
# (b): every picture at or under the cap unless nothing fits, never longer than its input
transcode(tp_b); hip.sync()
b_lens = d_len_out.cpu().numpy().copy()
assert (b_lens <= in_lens).all(), "a capped output is longer than its input"
# (a) decodes without error, and no output length exceeds its input's
transcode(tp_a); hip.sync()
a_lens = d_len_out.cpu().numpy().copy()
assert (a_lens <= in_lens).all() and (a_lens > 0).all(), "an output is longer than its input"
decode(d_out, d_len_out); hip.sync()    # (vc2hip_sync raises on any device-side error)
times = {k: [] for k in calls}
for _ in range(REPS):                   # the forms alternated
    for k, fn in calls.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        a.record(torch.cuda.current_stream()); fn(); b.record(torch.cuda.current_stream()); b.synchronize()
        hip.sync()
        times[k].append(a.elapsed_time(b))
med = {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()}
result = {"pictures": N, "distinct": DISTINCT, "repeats": REPS, "index_in": Q_IN, "index_out": Q_OUT, "cap": CAP,
          "input_lengths_min_max": [int(in_lens.min()), int(in_lens.max())],
          "a_lengths_min_max": [int(a_lens.min()), int(a_lens.max())], "b_lengths_min_max": [int(b_lens.min()), int(b_lens.max())],
          "b_over_cap": int((b_lens > CAP).sum()), "b_measure_passes": None,
          "median_ms": med, "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
          "gate_a_max_below_c_min": bool(max(times["a_transcode"]) < min(times["c_decode_encode"])), "kernels_ms": {}}
for name in ("a_transcode", "b_transcode_capped"):
    hip.profile_enable(True); hip.profile_reset()
    for _ in range(3):
        calls[name]()
    hip.sync()
    prof = hip.profile()
    result["kernels_ms"][name] = {kn: round(ms / 3, 3) for kn, (n, ms) in sorted(prof.items())}
    if name == "b_transcode_capped":
        result["b_measure_passes"] = prof["transcode_measure"][0] // 3
    hip.profile_enable(False)
line = json.dumps(result)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "r12_time_transcode.json"), "w") as f:
    f.write(line + "\n")
