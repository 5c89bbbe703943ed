"""Timing of vc2hip_transcode_batch_dev on cfg 2 (UHD-1 3840x2160 4:2:2 10-bit DD97 depth 4, -u 1 -a 2 -S 2; the bench's
generator, its first TIME_TRANSCODE_DISTINCT frames cycled to 128 pictures per call).  The input is the batch encoded at
HQ_ConstQ 16.  Device events around each form, the forms alternated, median and min - max of the repeats (not the bench
metric):
  (a) transcode          to index 24
  (b) transcode_capped   floor 16, cap = the median of the lengths a transcode to index 20 gives
  (c) decode_encode      the route a caller had before: decode_batch_dev, then encode_batch_dev at HQ_ConstQ 24
  (d) decode             decode_batch_dev alone
  (e) transcode_cbr      vc2hip_transcode_cbr_batch_dev to cfg 3's budget (-s 8294400 -S 2: HQ_CBR, same prefix and scalar)
  (f) decode_encode_cbr  decode_batch_dev, then encode_batch_dev at HQ_CBR with the same budget
then the per-kernel tables of (a), (b) and (e) from vc2hip_profile_* (the slice index, hq_unpack, transcode_scale, hq_pack; capped:
also transcode_measure and transcode_pick; (e): transcode_fit, cbr_search, transcode_settle), and the share of (e)'s slices that
are kept: the input is a VBR payload at the output's scalar, so a slice is kept iff its coded bytes are at most its budget.  Before timing: (a)'s output decodes without error, and no output length exceeds its input's.
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
CBR_BYTES = 8294400
cp_cbr = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, mode="HQ_CBR", s=CBR_BYTES, scalar=2)
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


def decode_encode(cp=cp_out):
    decode()
    hip.encode_batch_dev(d_dec.data_ptr(), N, fmt, cp, d_out.data_ptr(), stride, d_len_out.data_ptr())


def transcode_cbr():
    hip.transcode_cbr_batch_dev(d_in.data_ptr(), stride, d_len_in.data_ptr(), N, fmt, cp_in, cp_cbr, d_out.data_ptr(), stride, d_len_out.data_ptr())


def kept_share():
    """of the distinct input pictures' slices: coded bytes (index byte and three length bytes included) at most the budget"""
    ns = cp_in.y_slices * cp_in.x_slices
    budgets = np.zeros(ns, np.int32)
    assert hip.lib.vc2hip_slice_bytes(cp_in.y_slices, cp_in.x_slices, CBR_BYTES, 2, budgets) == 0
    kept = 0
    for i in range(min(DISTINCT, N)):
        pay = d_in[i, :int(in_lens[i])].cpu().numpy()
        pos = 0
        for s in range(ns):
            start = pos
            pos += 1
            for _ in range(3):
                pos += 1 + int(pay[pos]) * 2
            kept += pos - start <= budgets[s]
        assert pos == len(pay)
    return kept / (ns * min(DISTINCT, N))


transcode(vc2hip_py.transcode_params(Q_CAP)); hip.sync()
CAP = int(np.median(d_len_out.cpu().numpy()))
tp_a, tp_b = vc2hip_py.transcode_params(Q_OUT), vc2hip_py.transcode_params(Q_IN, CAP)
calls = {"a_transcode": lambda: transcode(tp_a), "b_transcode_capped": lambda: transcode(tp_b), "c_decode_encode": decode_encode,
         "d_decode": decode, "e_transcode_cbr": transcode_cbr, "f_decode_encode_cbr": lambda: decode_encode(cp_cbr)}
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
# (e): every picture is the budgets' sum and decodes without error
transcode_cbr(); hip.sync()
e_lens = d_len_out.cpu().numpy().copy()
assert len(set(e_lens.tolist())) == 1 and 0 < e_lens[0] <= CBR_BYTES, "an HQ_CBR output is not the budgets' sum"
hip.decode_batch_dev(d_out.data_ptr(), stride, d_len_out.data_ptr(), N, fmt, cp_cbr, d_dec.data_ptr()); hip.sync()
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
          "gate_a_max_below_c_min": bool(max(times["a_transcode"]) < min(times["c_decode_encode"])),
          "cbr_bytes": CBR_BYTES, "e_length": int(e_lens[0]), "e_kept_share": round(kept_share(), 4),
          "e_median_at_or_below_f": bool(med["e_transcode_cbr"] <= med["f_decode_encode_cbr"]), "kernels_ms": {}}
for name in ("a_transcode", "b_transcode_capped", "e_transcode_cbr"):
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
with open(os.path.join(ROOT, "profiles", "r13_time_transcode.json"), "w") as f:
    f.write(line + "\n")
