"""Timing of the device stream calls at cfg 2 (UHD-1 4:2:2 10-bit DD97 d4 q16 S2), 128 pictures per call: vc2hip_stream_write_dev
and vc2hip_stream_read_dev next to vc2hip_encode_batch_dev / vc2hip_decode_batch_dev, device events around each call (not the
bench metric).  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_stream.py`."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, vc2hip_py
from synth import synth_fast

W, H, N, REPS = 3840, 2160, 128, 5
dev = torch.device("cuda:0")
hip = vc2hip_py.Vc2Hip(0)
fmt = vc2hip_py.picture_format(W, H, "422", 10)
cp = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, q=16, scalar=2)
rb = hip.raw_picture_bytes(fmt)
stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
raws = [synth_fast(W, H, "422", 10, 900 + i) for i in range(3)]
d_raw = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(dev).view(3, rb)[torch.arange(N, device=dev) % 3].reshape(-1)
d_pay = torch.zeros(N * stride, dtype=torch.uint8, device=dev)
d_pay2 = torch.zeros_like(d_pay)
d_len = torch.zeros(N, dtype=torch.int64, device=dev)
d_len2 = torch.zeros_like(d_len)
cap = N * (stride + 64)
d_stream = torch.zeros(cap, dtype=torch.uint8, device=dev)
d_slen = torch.zeros(1, dtype=torch.int64, device=dev)
d_out = torch.zeros(N * rb, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
sp = vc2hip_py.stream_params(2, 0, 0, True)
calls = {
    "encode_batch_dev": lambda: hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr()),
    "stream_write_dev": lambda: hip.stream_write_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, cp, sp, d_stream.data_ptr(), cap,
                                                     d_slen.data_ptr()),
    "stream_read_dev": lambda: hip.stream_read_dev(d_stream.data_ptr(), int(d_slen.item()), N, cp, vc2hip_py.stream_params(2),
                                                   d_pay2.data_ptr(), stride, d_len2.data_ptr()),
    "decode_batch_dev": lambda: hip.decode_batch_dev(d_pay2.data_ptr(), stride, d_len2.data_ptr(), N, fmt, cp, d_out.data_ptr()),
}
ms = {}
for name, fn in calls.items():
    fn(); hip.sync()                            # warm-up (sizes the workspace)
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        a.record(torch.cuda.current_stream()); fn(); hip.sync(); b.record(torch.cuda.current_stream()); b.synchronize()
        times.append(a.elapsed_time(b))
    ms[name] = sorted(times)[len(times) // 2]
payload = int(d_len.sum().item())
assert torch.equal(d_len, d_len2)
print(json.dumps({"pictures": N, "payload_bytes": payload, "stream_bytes": int(d_slen.item()),
                  "median_ms": {k: round(v, 3) for k, v in ms.items()},
                  "copy_GBps_on_payload": {k: round(2 * payload / (ms[k] * 1e6), 1) for k in ("stream_write_dev", "stream_read_dev")}}))
