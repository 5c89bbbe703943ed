"""Timing of the batch calls under a caller's sample layout on cfg 2 (UHD-1 3840x2160 4:2:2 10-bit HQ_ConstQ DD97 depth 4,
-u 1 -a 2 -q 16 -S 2), 128 pictures per call, encode and decode.  The pictures live on the GPU as a torch user holds them:
int16 planes, little-endian, the sample in the low bits.  Device events around each form, the forms alternated and the
median of the repeats taken (not the bench metric):
  (a) layout     vc2hip_set_sample_layout(little-endian, LSB-justified), then the batch call on the int16 buffer itself
  (b) convert    a torch conversion pass around the file-format call (eager ops: a shift, and two strided byte copies for
                 the byte order) into a second buffer before the encode, and back after the decode -- what a caller did
                 before the layout
  (c) file       the file-format call alone on pre-converted pictures (what the call itself costs)
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_layout.py`, once per form with
TIME_LAYOUT_ONLY=a_layout / c_file (the two forms launch the same kernels, so one run cannot tell them apart)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, vc2hip_py
from synth import synth_fast

W, H, BITS = 3840, 2160, 10
N, REPS = int(os.environ.get("TIME_LAYOUT_PICTURES", "128")), int(os.environ.get("TIME_LAYOUT_REPS", "9"))
ONLY = os.environ.get("TIME_LAYOUT_ONLY")             # one form only (a_layout, b_convert or c_file)
dev = torch.device("cuda:0")
hip = vc2hip_py.Vc2Hip(0, stream=torch.cuda.current_stream().cuda_stream)  # (one stream: the torch passes and the calls in order)
fmt = vc2hip_py.picture_format(W, H, "422", BITS)
cp = vc2hip_py.coding_params(hip.lib, fmt, "DD97", 4, 1, 2, q=16, scalar=2)
rb = hip.raw_picture_bytes(fmt)
LE_LSB = vc2hip_py.sample_layout(True, True)
raws = [synth_fast(W, H, "422", BITS, 900 + i) for i in range(4)]
d_file = torch.frombuffer(bytearray(b"".join(raws)), dtype=torch.uint8).to(dev).view(4, rb)[torch.arange(N, device=dev) % 4].reshape(-1).contiguous()


def swap_bytes(src, dst):
    """the two bytes of every 16-bit word exchanged: two strided byte copies (eager torch has no byte swap)"""
    s2, d2 = src.view(-1, 2), dst.view(-1, 2)
    d2[:, 0] = s2[:, 1]
    d2[:, 1] = s2[:, 0]


def to_file(words, out):
    """int16 little-endian LSB-justified words -> the file format's big-endian MSB-justified words"""
    torch.bitwise_left_shift(words.view(torch.int16), 16 - BITS, out=d_scratch.view(torch.int16))   # justify
    swap_bytes(d_scratch, out)                                                                     # byte order


def from_file(words, out):
    swap_bytes(words, d_scratch)
    o = out.view(torch.int16)
    torch.bitwise_right_shift(d_scratch.view(torch.int16), 16 - BITS, out=o)
    o.bitwise_and_((1 << BITS) - 1)                # (the shift of an int16 is arithmetic: a word with its top bit set)


d_scratch = torch.empty_like(d_file)
d_words = torch.empty_like(d_file)                    # the caller's pictures: int16, little-endian, LSB-justified
from_file(d_file, d_words)
d_tmp = torch.empty_like(d_file)
d_out_a, d_out_b, d_out_c = (torch.empty_like(d_file) for _ in range(3))
stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
d_pay = torch.zeros(N * stride, dtype=torch.uint8, device=dev)
d_len = torch.zeros(N, dtype=torch.int64, device=dev)
d_pay_a, d_len_a = torch.zeros_like(d_pay), torch.zeros_like(d_len)


def with_layout(lay, fn):
    hip.set_sample_layout(lay)      # (pure host state: nothing launched, nothing waited for)
    fn()
    hip.set_sample_layout(None)


enc = {
    "a_layout": lambda: with_layout(LE_LSB, lambda: hip.encode_batch_dev(d_words.data_ptr(), N, fmt, cp, d_pay_a.data_ptr(), stride, d_len_a.data_ptr())),
    "b_convert": lambda: (to_file(d_words, d_tmp), hip.encode_batch_dev(d_tmp.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())),
    "c_file": lambda: hip.encode_batch_dev(d_file.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr()),
}
dec = {
    "a_layout": lambda: with_layout(LE_LSB, lambda: hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, d_out_a.data_ptr())),
    "b_convert": lambda: (hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, d_tmp.data_ptr()), from_file(d_tmp, d_out_b)),
    "c_file": lambda: hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), N, fmt, cp, d_out_c.data_ptr()),
}
if ONLY:
    enc, dec = {ONLY: enc[ONLY]}, {ONLY: dec[ONLY]}
result = {"pictures": N, "repeats": REPS, "median_ms": {}, "min_max_ms": {}}
for direction, calls in (("encode", enc), ("decode", dec)):
    if direction == "decode" and "c_file" not in calls:
        enc_file = lambda: hip.encode_batch_dev(d_file.data_ptr(), N, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())   # noqa: E731
        enc_file(); hip.sync()                  # (the payload the decode forms read)
    for fn in calls.values():
        fn(); hip.sync()                        # warm-up (sizes the workspace)
    times = {k: [] for k in calls}
    for _ in range(REPS):                       # the forms alternated
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            hip.sync()
            a.record(torch.cuda.current_stream()); fn(); b.record(torch.cuda.current_stream()); b.synchronize()
            hip.sync()                          # (errors of the call)
            times[k].append(a.elapsed_time(b))
    result["median_ms"][direction] = {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()}
    result["min_max_ms"][direction] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()}
if not ONLY:   # the three forms computed the same thing
    assert torch.equal(d_len_a, d_len) and torch.equal(d_pay_a, d_pay), "the payload under the layout differs from the file format's"
    assert torch.equal(d_out_a, d_out_b), "the pictures decoded under the layout differ from the converted ones"
    to_file(d_out_a, d_tmp)
    assert torch.equal(d_tmp, d_out_c), "the pictures decoded under the layout differ from the file format's"
print(json.dumps(result))
