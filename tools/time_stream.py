"""Timing of the device stream calls at cfg 2 (UHD-1 4:2:2 10-bit DD97 d4 q16 S2), 128 pictures per call: vc2hip_stream_write_dev,
vc2hip_stream_write_fragments_dev (fragment_length 1400) and vc2hip_stream_read_dev next to vc2hip_encode_batch_dev /
vc2hip_decode_batch_dev, device events around each call (not the bench metric); then the two writers again on cfg 3 (HQ_CBR)
slots.  The fragmented writer's kernels are timed one by one through the library's own launch events.
Per-kernel times of everything: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_stream.py`."""
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
FLEN = 1400
ns = cp.y_slices * cp.x_slices
fcap = N * (stride + 64 + 25 * ns) + 64          # the header's worst case
ucap = N * (ns + 1) + 1
d_fstream = torch.zeros(fcap, dtype=torch.uint8, device=dev)
d_flen = torch.zeros(1, dtype=torch.int64, device=dev)
d_units = torch.zeros(ucap, dtype=torch.int64, device=dev)
d_count = torch.zeros(1, dtype=torch.int64, device=dev)
sp3 = vc2hip_py.stream_params(3, 0, 0, True)


def write_fragments(cpx):
    hip.stream_write_fragments_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, cpx, sp3, FLEN, d_fstream.data_ptr(), fcap,
                                   d_flen.data_ptr(), d_units.data_ptr(), ucap, d_count.data_ptr())


def median_ms(fn):
    fn(); hip.sync()                            # warm-up (sizes the workspace)
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hip.sync()
        a.record(torch.cuda.current_stream()); fn(); hip.sync(); b.record(torch.cuda.current_stream()); b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def kernel_split(fn):
    """ms per launch name of one call (the library's event pairs around every launch)"""
    hip.sync(); hip.profile_reset(); hip.profile_enable(True)
    fn(); hip.sync()
    out = {k: round(v[1], 4) for k, v in hip.profile().items()}
    hip.profile_enable(False); hip.profile_reset()
    return out


calls = {
    "encode_batch_dev": lambda: hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr()),
    "stream_write_dev": lambda: hip.stream_write_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, cp, sp, d_stream.data_ptr(), cap,
                                                     d_slen.data_ptr()),
    "stream_write_fragments_dev": lambda: write_fragments(cp),
    "stream_read_dev": lambda: hip.stream_read_dev(d_stream.data_ptr(), int(d_slen.item()), N, cp, vc2hip_py.stream_params(2),
                                                   d_pay2.data_ptr(), stride, d_len2.data_ptr()),
    "decode_batch_dev": lambda: hip.decode_batch_dev(d_pay2.data_ptr(), stride, d_len2.data_ptr(), N, fmt, cp, d_out.data_ptr()),
}
ms = {name: median_ms(fn) for name, fn in calls.items()}
payload = int(d_len.sum().item())
assert torch.equal(d_len, d_len2)
writers = ("stream_write_dev", "stream_write_fragments_dev")
print(json.dumps({"cfg": 2, "pictures": N, "payload_bytes": payload, "stream_bytes": int(d_slen.item()),
                  "fragment_length": FLEN, "fragmented_stream_bytes": int(d_flen.item()), "units": int(d_count.item()),
                  "median_ms": {k: round(v, 3) for k, v in ms.items()},
                  "copy_GBps_on_payload": {k: round(2 * payload / (ms[k] * 1e6), 1) for k in writers + ("stream_read_dev",)},
                  "fragments_kernel_ms": kernel_split(lambda: write_fragments(cp))}))

# cfg 3: the same pictures as HQ_CBR slots (8,294,400 bytes each), the two writers
cp3 = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, mode="HQ_CBR", s=8294400, scalar=2)
assert hip.max_payload_bytes(fmt, cp3) <= stride
hip.encode_batch_dev(d_raw.data_ptr(), N, fmt, cp3, d_pay.data_ptr(), stride, d_len.data_ptr()); hip.sync()
calls3 = {"stream_write_dev": lambda: hip.stream_write_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, cp3, sp, d_stream.data_ptr(),
                                                           cap, d_slen.data_ptr()),
          "stream_write_fragments_dev": lambda: write_fragments(cp3)}
ms3 = {name: median_ms(fn) for name, fn in calls3.items()}
payload3 = int(d_len.sum().item())
print(json.dumps({"cfg": 3, "pictures": N, "payload_bytes": payload3, "stream_bytes": int(d_slen.item()),
                  "fragment_length": FLEN, "fragmented_stream_bytes": int(d_flen.item()), "units": int(d_count.item()),
                  "median_ms": {k: round(v, 3) for k, v in ms3.items()},
                  "copy_GBps_on_payload": {k: round(2 * payload3 / (ms3[k] * 1e6), 1) for k in writers},
                  "fragments_kernel_ms": kernel_split(lambda: write_fragments(cp3))}))
