"""Timing of the three HQ VBR modes with and without per-slice index offsets (vc2hip_set_index_offsets),
on the set-up of tools/time_cap.py: cfg 2 (UHD-1 3840x2160 4:2:2 10-bit DD97 depth 4, -u 1 -a 2 -S 2; the bench's generator,
its first TIME_CAP_DISTINCT frames cycled to 128 pictures per call), floor = the bench's index 16, cap = the median of the
pictures' ConstQ lengths at the floor.  Device events around each form, the seven forms alternated in one session, median and
min - max of the repeats (not the bench metric):
  constq, constq_zero, constq_roi, capped, capped_roi, filled, filled_roi
`zero`: a map of zeros (the same bytes as without a map -- the only forms comparable with the plain ones); `roi`: -6 in the
central third of the slice rows and columns, +4 elsewhere, one map for every picture (these code other payloads).  Before
anything is timed the tool asserts the definition's invariants on its own outputs."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch, vc2hip_py
from synth import synth_fast

W, H = 3840, 2160
N, REPS = int(os.environ.get("TIME_CAP_PICTURES", "128")), int(os.environ.get("TIME_CAP_REPS", "9"))
DISTINCT, FLOOR, TOP = int(os.environ.get("TIME_CAP_DISTINCT", "8")), 16, 115
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
hip = vc2hip_py.Vc2Hip(0, stream=stream)
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
ys, xs = cp_q.y_slices, cp_q.x_slices
ns = ys * xs
v, h = np.divmod(np.arange(ns), xs)
roi = np.where((v >= ys // 3) & (v < (2 * ys + 2) // 3) & (h >= xs // 3) & (h < (2 * xs + 2) // 3), -6, 4).astype(np.int8)
maps = {"zero": torch.zeros(ns, dtype=torch.int8, device=dev), "roi": torch.from_numpy(roi).to(dev)}
torch.cuda.synchronize()


def encode(cp, offs=None):
    hip.set_index_offsets(maps[offs].data_ptr() if offs else None, 0)
    hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
    hip.set_index_offsets(None)


encode(cp_q); hip.sync()
CAP = int(np.median(d_len.cpu().numpy()))
cps = {"constq": cp_q, "capped": params("HQ_Capped", q=FLOOR, s=CAP), "filled": params("HQ_CappedFill", q=FLOOR, s=CAP)}
forms = {"constq": ("constq", None), "constq_zero": ("constq", "zero"), "constq_roi": ("constq", "roi"), "capped": ("capped", None),
         "capped_roi": ("capped", "roi"), "filled": ("filled", None), "filled_roi": ("filled", "roi")}

# the invariants, from one vc2hip_encode_recon_batch_dev call per form (also the warm-up of every path; not timed)
d_q = torch.zeros(N, ns, dtype=torch.int32, device=dev)
got = {}
for name, (mode, offs) in list(forms.items()) + [("capped_zero", ("capped", "zero")), ("filled_zero", ("filled", "zero"))]:
    d_pay.zero_()
    hip.set_index_offsets(maps[offs].data_ptr() if offs else None, 0)
    hip.encode_recon_batch_dev(d_raw.data_ptr(), N, fmt, cps[mode], d_pay.data_ptr(), stride, d_len.data_ptr(), None, None, d_q.data_ptr())
    hip.set_index_offsets(None)
    hip.sync()
    got[name] = (d_len.cpu().numpy().copy(), d_q.cpu().numpy().copy(), d_pay.clone() if offs != "roi" else None)
for mode in cps:
    a, z = got[mode], got[mode + "_zero"]
    assert (a[0] == z[0]).all() and (a[1] == z[1]).all() and torch.equal(a[2], z[2]), mode + ": a map of zeros changed a byte"
o = roi.astype(np.int64)[None, :]
e = lambda b: np.clip(b + o, 0, TOP)
assert (got["constq_roi"][1] == e(FLOOR)).all(), "HQ_CONSTQ: slice s is not at e_s(q_index)"
len_c, q_c, _ = got["capped_roi"]
c0 = int(np.argmax(roi == -6))
base = q_c[:, c0:c0 + 1] + 6                       # (from a slice of the region: no clamp acts there, 16 - 6 >= 0)
assert (q_c == e(base)).all() and (base >= FLOOR).all() and (base <= TOP).all(), "HQ_CAPPED: the map is not e_s(b_i)"
assert ((len_c <= CAP) | (base[:, 0] == TOP)).all(), "HQ_CAPPED: a picture above the cap below base 115"
len_f, q_f, _ = got["filled_roi"]
assert ((q_f == e(base)) | (q_f == e(base - 1))).all(), "HQ_CAPPED_FILL: a slice at neither e_s(b_i) nor e_s(b_i - 1)"
assert (len_f >= len_c).all() and ((len_f <= CAP) | (len_c > CAP)).all(), "HQ_CAPPED_FILL: outside [L(b_i), cap]"
stay = base[:, 0] == FLOOR
assert (q_f[stay] == q_c[stay]).all() and (len_f[stay] == len_c[stay]).all(), "a picture at the floor changed"
del got

calls = {k: (lambda m=m, offs=offs: encode(cps[m], offs)) for k, (m, offs) in forms.items()}
for fn in calls.values():
    fn(); hip.sync()
times = {k: [] for k in calls}
for _ in range(REPS):                   # the forms alternated
    for k, fn in calls.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        a.record(torch.cuda.current_stream()); fn(); b.record(torch.cuda.current_stream()); b.synchronize()
        hip.sync()
        times[k].append(a.elapsed_time(b))
med = {k: round(sorted(t)[len(t) // 2], 3) for k, t in times.items()}
result = {"pictures": N, "distinct": DISTINCT, "repeats": REPS, "floor": FLOOR, "cap": CAP, "slices": ns,
          "roi_slices_at_minus_6": int((roi == -6).sum()),
          "bases_capped_roi": {str(int(t)): int((base[:, 0] == t).sum()) for t in np.unique(base[:, 0])},
          "mean_len_over_cap": {"capped_roi": round(float(np.mean(len_c / CAP)), 7), "filled_roi": round(float(np.mean(len_f / CAP)), 7)},
          "median_ms": med, "min_max_ms": {k: [round(min(t), 3), round(max(t), 3)] for k, t in times.items()}, "kernels_ms": {}}
for name in calls:
    hip.profile_enable(True); hip.profile_reset()
    for _ in range(3):
        calls[name]()
    hip.sync()
    result["kernels_ms"][name] = {kn: round(ms / 3, 3) for kn, (n, ms) in sorted(hip.profile().items())}
    hip.profile_enable(False)
print(json.dumps(result))
