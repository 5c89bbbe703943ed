"""Timing of the field-picture batch calls at 1080i (1920x1080 4:2:2 10-bit, 128 frames = 256 field pictures): HQ_ConstQ
LeGall depth 2 -u 1 -a 4 q12, and LD LeGall depth 3 -u 1 -a 4.  Device events around each call, the forms alternated and the
median of the repeats taken (not the bench metric):
  (a) fields     encode_fields_batch_dev / decode_fields_batch_dev on the interleaved frames
  (b) split      a torch split pass + encode_batch_dev on 256 field pictures / decode_batch_dev + a torch merge pass
  (c) progressive  encode_batch_dev / decode_batch_dev alone on the pre-split fields
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_fields.py`, once per form with
TIME_FIELDS_ONLY=a_fields / c_progressive (the two forms launch the same kernels, so one run cannot tell them apart)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, vc2hip_py
from synth import synth_fast

W, H, N, REPS = 1920, 1080, 128, int(os.environ.get("TIME_FIELDS_REPS", "7"))
ONLY = os.environ.get("TIME_FIELDS_ONLY")           # one form only (a_fields, b_split or c_progressive)
CFGS = {
    "constq_legall_d2": dict(kernel="LeGall", depth=2, kw=dict(q=12, scalar=1)),
    "ld_legall_d3": dict(kernel="LeGall", depth=3, kw=dict(mode="LD", s=1036800 // 2)),
}
dev = torch.device("cuda:0")
hip = vc2hip_py.Vc2Hip(0, stream=torch.cuda.current_stream().cuda_stream)  # (one stream: the torch passes and the calls in order)
ffmt = vc2hip_py.picture_format(W, H, "422", 10)
fmt = vc2hip_py.picture_format(W, H // 2, "422", 10)
fb, pb = hip.raw_picture_bytes(ffmt), hip.raw_picture_bytes(fmt)
ROWS = [(H, W * 2), (H, W), (H, W)]                       # (rows, bytes per row) of the frame's planes (4:2:2)
raws = [synth_fast(W, H, "422", 10, 700 + i) for i in range(3)]
d_frames = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(dev).view(3, fb)[torch.arange(N, device=dev) % 3]
d_frames = d_frames.reshape(-1).contiguous()


def split(frames, out):
    """interleaved frames -> field pictures in stream order (top field first): one pass over every plane"""
    f = frames.view(N, fb)
    o = out.view(N, 2, pb)
    at = ato = 0
    for r, rw in ROWS:
        src = f[:, at:at + r * rw].view(N, r // 2, 2, rw)
        for k in (0, 1):
            o[:, k, ato:ato + (r // 2) * rw].view(N, r // 2, rw).copy_(src[:, :, k])
        at += r * rw
        ato += (r // 2) * rw


def merge(fields, out):
    f = fields.view(N, 2, pb)
    o = out.view(N, fb)
    at = ato = 0
    for r, rw in ROWS:
        dst = o[:, at:at + r * rw].view(N, r // 2, 2, rw)
        for k in (0, 1):
            dst[:, :, k].copy_(f[:, k, ato:ato + (r // 2) * rw].view(N, r // 2, rw))
        at += r * rw
        ato += (r // 2) * rw


d_fields = torch.empty(2 * N * pb, dtype=torch.uint8, device=dev)
split(d_frames, d_fields)
d_tmp = torch.empty_like(d_fields)
d_out = torch.empty(N * fb, dtype=torch.uint8, device=dev)
d_out_f = torch.empty_like(d_out)
result = {"frames": N, "field_pictures": 2 * N, "median_ms": {}}
for name, c in CFGS.items():
    cp = vc2hip_py.coding_params(hip.lib, fmt, c["kernel"], c["depth"], 1, 4, **c["kw"])
    stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
    d_pay = torch.zeros(2 * N * stride, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(2 * N, dtype=torch.int64, device=dev)
    enc = {
        "a_fields": lambda: hip.encode_fields_batch_dev(d_frames.data_ptr(), N, ffmt, 1, cp, d_pay.data_ptr(), stride, d_len.data_ptr()),
        "b_split": lambda: (split(d_frames, d_tmp),
                            hip.encode_batch_dev(d_tmp.data_ptr(), 2 * N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())),
        "c_progressive": lambda: hip.encode_batch_dev(d_fields.data_ptr(), 2 * N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr()),
    }
    dec = {
        "a_fields": lambda: hip.decode_fields_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, ffmt, 1, cp, d_out_f.data_ptr()),
        "b_split": lambda: (hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), 2 * N, fmt, cp, d_tmp.data_ptr()),
                            merge(d_tmp, d_out)),
        "c_progressive": lambda: hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), 2 * N, fmt, cp, d_tmp.data_ptr()),
    }
    if ONLY:
        enc, dec = {ONLY: enc[ONLY]}, {ONLY: dec[ONLY]}
    for direction, calls in (("encode", enc), ("decode", dec)):
        for fn in calls.values():
            fn(); hip.sync()                    # warm-up (sizes the workspace)
        times = {k: [] for k in calls}
        for _ in range(REPS):                   # the three forms alternated
            for k, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                hip.sync()
                a.record(torch.cuda.current_stream()); fn(); b.record(torch.cuda.current_stream()); b.synchronize()
                hip.sync()                      # (errors of the call)
                times[k].append(a.elapsed_time(b))
        result["median_ms"][f"{name} {direction}"] = {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()}
    if not ONLY:
        assert torch.equal(d_out, d_out_f), name  # (b)'s merged frames == (a)'s frames
print(json.dumps(result))
