"""Timing of VC2HIP_HQ_CAPPED on cfg 2 (UHD-1 3840x2160 4:2:2 10-bit DD97 depth 4, -u 1 -a 2 -S 2; the bench's generator,
its first TIME_CAP_DISTINCT frames cycled to 128 pictures per call), floor = the bench's index 16, cap = the median of the
pictures' ConstQ lengths at the floor (about half the pictures move off the floor).  Device events around each form, the
forms alternated, median and min - max of the repeats (not the bench metric):
  (a) capped        encode_batch_dev, mode HQ_Capped
  (b) constq        encode_batch_dev, mode HQ_ConstQ at the floor, same pictures
  (c) host_bisect   what a caller did before the mode existed: ConstQ at the floor, d_lens read back; the pictures over the
                    cap are bisected on the host over floor + 1 .. 115, one ConstQ call per distinct trial index and step on
                    the gathered pictures, d_lens read back after each; a last call per distinct result writes the payloads
  (d) cbr           for scale: encode_batch_dev, mode HQ_CBR of cfg 3 on the same pictures (its cbr_search measures slices
                    as the capped mode's rounds do)
then the per-kernel tables of (a), (b) and (d) from vc2hip_profile_* (cap_measure1, cap_measure2, cap_pick: the rounds and
the picks of (a))."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch, vc2hip_py
from synth import synth_fast

W, H = 3840, 2160
N, REPS = int(os.environ.get("TIME_CAP_PICTURES", "128")), int(os.environ.get("TIME_CAP_REPS", "9"))
DISTINCT, FLOOR, TOP = int(os.environ.get("TIME_CAP_DISTINCT", "8")), 16, 115
FLAGS = sum(vc2hip_py.FLAGS[f] for f in os.environ.get("TIME_CAP_FLAGS", "").split(",") if f)
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
hip = vc2hip_py.Vc2Hip(0, stream=stream, flags=FLAGS)
fmt = vc2hip_py.picture_format(W, H, "422", 10)
rb = hip.raw_picture_bytes(fmt)


def params(mode, q=0, s=0):
    return vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, mode=mode, q=q, s=s, scalar=2)


cp_q = params("HQ_ConstQ", q=FLOOR)
cp_cbr = params("HQ_CBR", s=8294400)
frames = synth_fast(W, H, "422", 10, 1234, frames=DISTINCT)
d_raw = torch.frombuffer(bytearray(frames), dtype=torch.uint8).to(dev).view(DISTINCT, rb)[torch.arange(N, device=dev) % DISTINCT].contiguous()
stride = (hip.max_payload_bytes(fmt, cp_q) + 255) // 256 * 256
d_pay = torch.zeros(N, stride, dtype=torch.uint8, device=dev)
d_len = torch.zeros(N, dtype=torch.int64, device=dev)
g_raw, g_pay, g_len = torch.empty_like(d_raw), torch.empty_like(d_pay), torch.zeros_like(d_len)   # (c): the gathered pictures


def encode(cp, raw=d_raw, pay=d_pay, lens=d_len, n=N):
    hip.encode_batch_dev(raw.data_ptr(), n, fmt, cp, pay.data_ptr(), stride, lens.data_ptr())


encode(cp_q); hip.sync()
floor_lens = d_len.cpu().numpy().copy()
CAP = int(np.median(floor_lens))
cp_cap = params("HQ_Capped", q=FLOOR, s=CAP)


def host_bisect():
    """returns the per-picture indices; d_pay / d_len hold their payloads"""
    encode(cp_q); hip.sync()
    lens = d_len.cpu().numpy()
    q = np.full(N, FLOOR)
    over = np.nonzero(lens > CAP)[0]
    lo, hi = np.full(N, FLOOR), np.full(N, TOP + 1)      # lo does not fit; hi fits, or is past the top
    while True:
        todo = over[hi[over] - lo[over] > 1]
        if not len(todo):
            break
        trial = (lo + hi) // 2
        for t in np.unique(trial[todo]):
            idx = todo[trial[todo] == t]
            k = len(idx)
            torch.index_select(d_raw, 0, torch.from_numpy(idx).to(dev), out=g_raw[:k])
            encode(params("HQ_ConstQ", q=int(t)), g_raw, g_pay, g_len, k); hip.sync()
            fits = g_len[:k].cpu().numpy() <= CAP
            hi[idx[fits]], lo[idx[~fits]] = t, t
    q[over] = np.minimum(hi[over], TOP)
    for t in np.unique(q[over]):                          # the payloads at the indices found
        idx = over[q[over] == t]
        k, ix = len(idx), torch.from_numpy(idx).to(dev)
        torch.index_select(d_raw, 0, ix, out=g_raw[:k])
        encode(params("HQ_ConstQ", q=int(t)), g_raw, g_pay, g_len, k)
        d_pay.index_copy_(0, ix, g_pay[:k]); d_len.index_copy_(0, ix, g_len[:k])
    hip.sync()
    return q


calls = {"a_capped": lambda: encode(cp_cap), "b_constq": lambda: encode(cp_q), "c_host_bisect": host_bisect, "d_cbr": lambda: encode(cp_cbr)}
for fn in calls.values():
    fn(); hip.sync()                    # warm-up (sizes the workspaces)
# the forms agree before they are timed: the capped call's payloads are the host bisection's
want_q = host_bisect(); want_pay, want_len = d_pay.clone(), d_len.clone()
d_pay.zero_(); torch.cuda.synchronize()
encode(cp_cap); hip.sync()
assert torch.equal(d_len, want_len), "HQ_Capped lengths differ from the host bisection's"
same = all(torch.equal(d_pay[i, :int(want_len[i])], want_pay[i, :int(want_len[i])]) for i in range(N))
assert same, "HQ_Capped payloads differ from the host bisection's"
del want_pay
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
          "floor_lengths_min_max": [int(floor_lens.min()), int(floor_lens.max())],
          "indices": {str(int(t)): int((want_q == t).sum()) for t in np.unique(want_q)},
          "median_ms": med, "min_max_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
          "capped_minus_constq_ms": round(med["a_capped"] - med["b_constq"], 3), "kernels_ms": {}}
for name in ("a_capped", "b_constq", "d_cbr"):
    hip.profile_enable(True); hip.profile_reset()
    for _ in range(3):
        calls[name]()
    hip.sync()
    result["kernels_ms"][name] = {kn: round(ms / 3, 3) for kn, (n, ms) in sorted(hip.profile().items())}
    hip.profile_enable(False)
print(json.dumps(result))
