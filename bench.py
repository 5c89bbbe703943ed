#!/usr/bin/env python3
"""bench.py -- VC-2 HQ encode+decode throughput of the HIP hot path on MI355X.

A "step" = one pass of the hot path (encode_batch_dev then decode_batch_dev) over one batch of
synthetic pictures that are already resident in HBM.  Workload at every N: BASELINE.json config 2
(UHD-1 3840x2160 4:2:2 10-bit, HQ_ConstQ, DD97, 4 levels, slices -u 1 -a 2, q 16, scalar 2);
each rank/GPU owns its own batch of 128 distinct pictures (frames are independent: weak scaling, no collective on the data
path; --streams 2 cuts the batch over two HIP streams: +1.4 % on one MI355X, per-kernel durations then overlap).  Prints ONE JSON line on rank 0.

A plain run does what its headline needs and nothing else: it makes the pictures, warms up W steps, times exactly K steps,
writes what the last step computed (--dump-outputs DIR) and prints the line:

  value            encode+decode, device resident, K timed steps (barrier + synchronize on both sides); ms_per_step = their mean

--full adds everything else, as the line carried it before the option existed (then `value` / `ms_per_step` are the median
of three timed regions of K steps each, and every slot of the batch is checked before the line is printed):

  encode_only / decode_only   the two halves timed the same way, outside the timed region of `value`
  roofline         the dominant kernel (HIP events on each of its launches inside the timed region; every kernel in the warm-up steps) and the whole path
  e2e              pictures that start and end in pinned host memory, copies overlapped with kernels (PCIe bound)
  cpu_baseline     the oracle (a port of the reference algorithm) on the host cores: 1 thread, and one process per core;
                   the run that also supplies the expected bytes of EVERY slot of the batch

  other_configs    the other BASELINE configurations (cfg 1, 3, 4, 5-decode), 5 device-resident steps each, digest-checked
                   against tests/golden/reference_digests.json (cfg 5: against the oracle) -- beside `value`, never part of it

  python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--dump-outputs DIR]
                  [--full [--no-cpu-baseline] [--no-e2e] [--no-other-configs] [--no-batch32]]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
N > 1: one process per GPU over RCCL (backend nccl); every rank checks its own slots and the verdicts are AND-reduced
before rank 0 prints.  --dist-backend gloo with VC2_BENCH_DEVICE_MAP=0,0 runs two ranks on ONE GPU (tests/test_multi_rank_gpu.py:
the real HIP path under torch.distributed.run on the one-GPU box; a correctness exercise, not a scaling measurement).
"""
import argparse
import glob
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "vc2-reference_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable)
W, H, CFMT, BITS = 3840, 2160, "422", 10
KERNEL, DEPTH, U, A, Q, SCALAR = "DD97", 4, 1, 2, 16, 2
# oracle : reference speed on the same machine, measured in the build container (8 cores, g++ -O3 reference built with
# the survey's header shim): reference 2.9 + 1.86 s per UHD cfg-2 frame, oracle 2.2 + 1.5 s
PORT_VS_REFERENCE = 1.29


class ClockSampler:
    """The GPU's own clocks and socket power, read from the amdgpu hwmon files of the HIP device while a region runs
    (freq1_input = sclk, freq2_input = mclk in Hz, power1_input in microwatts; no root, no subprocess).  VERDICT r4
    item 2: the level-0 transforms run in one of two modes from box to box (DESIGN.md "Where the spread between runs comes
    from"); this puts a clock / power reading next to every line so that the attribution is evidence."""

    def __init__(self, pci_bus_id):
        self.dir, self.samples, self._stop, self._thread = None, [], False, None
        want = (pci_bus_id or "").lower()
        for d in sorted(glob.glob("/sys/class/drm/card*/device")):
            try:
                addr = os.path.basename(os.path.realpath(d)).lower()
            except OSError:
                continue
            hw = sorted(glob.glob(os.path.join(d, "hwmon", "hwmon*")))
            if hw and (addr == want or (not want and self.dir is None)):
                self.dir = hw[0]
                self.card = d
                if addr == want:
                    break

    def _read(self, name):
        try:
            with open(os.path.join(self.dir, name)) as f:
                return int(f.read().strip())
        except (OSError, ValueError, TypeError):
            return None

    def read(self):
        if self.dir is None:
            return None
        return (self._read("freq1_input"), self._read("freq2_input"), self._read("power1_input"))

    def start(self):
        import threading
        self.samples, self._stop = [], False

        def run():
            while not self._stop:
                r = self.read()
                if r is not None:
                    self.samples.append(r)
                time.sleep(0.01)   # 100 Hz (a 2 kHz poll contends with the launch loop for the GIL and queries the SMU)
        if self.dir is not None:
            self._thread = threading.Thread(target=run, daemon=True)
            self._thread.start()

    def stop(self):
        self._stop = True
        if self._thread is not None:
            self._thread.join()
            self._thread = None
        return self.summary(self.samples)

    @staticmethod
    def summary(samples):
        def col(i, scale):
            v = [s[i] / scale for s in samples if s[i] is not None]
            return {"min": round(min(v), 1), "mean": round(sum(v) / len(v), 1), "max": round(max(v), 1)} if v else None
        return {"samples": len(samples), "sclk_MHz": col(0, 1e6), "mclk_MHz": col(1, 1e6), "socket_power_W": col(2, 1e6)}


def picture_shard(n_pictures, rank, world):
    """Pictures are independent: picture k belongs to rank k mod world."""
    return list(range(rank, n_pictures, world))


DUMP_SAMPLES = 1 << 22   # bytes of the coded slices and samples of the decoded pictures in the dumped samples: 16 MB each


def dump_outputs(out_dir, torch, d_pay, stride, d_len, d_out, B, rb):
    """--dump-outputs: what a caller of the timed path holds after its last step -- every picture's coded slices (its
    length and payload bytes) and every decoded picture -- as float arrays in DIR/<name>.npy, 32 MB in all.  In full: the
    lengths and per-picture sums of the payload bytes and of the decoded samples (float64, exact); sampled: the bytes
    and samples at DUMP_SAMPLES positions drawn by a fixed seed (float32; a payload position beyond its picture's length
    reads -1).  Decoded samples are the raw pictures' 16-bit big-endian words."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    lens = d_len.cpu().numpy().astype(np.int64)
    pay = d_pay.view(B, stride)
    words = d_out.view(B, rb // 2, 2)
    pay_sum = [int(pay[k, :int(lens[k])].sum(dtype=torch.int64)) for k in range(B)]
    dec_sum = [256 * int(words[k, :, 0].sum(dtype=torch.int64)) + int(words[k, :, 1].sum(dtype=torch.int64)) for k in range(B)]
    rng = np.random.default_rng(20260)
    pos = np.sort(rng.integers(0, B * stride, size=DUMP_SAMPLES))
    got = d_pay[torch.from_numpy(pos).to(d_pay.device)].cpu().numpy().astype(np.float32)
    got[(pos % stride) >= lens[pos // stride]] = -1.0
    wpos = np.sort(rng.integers(0, B * rb // 2, size=DUMP_SAMPLES))
    hl = d_out.view(-1, 2)[torch.from_numpy(wpos).to(d_out.device)].cpu().numpy().astype(np.float32)
    arrays = {"payload_lengths": lens.astype(np.float64), "payload_byte_sums": np.array(pay_sum, np.float64),
              "payload_bytes_sampled": got, "decoded_sample_sums": np.array(dec_sum, np.float64),
              "decoded_samples_sampled": hl[:, 0] * 256 + hl[:, 1]}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def csrc_digest():
    """identifies the kernel sources a committed PMC profile belongs to"""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "vc2-reference_amd", "csrc", "*.h*"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


# ---- CPU side (oracle): runs BEFORE anything touches the GPU (worker processes are forked) -------------------------
def _cpu_frame(args):
    """encode + decode ONE picture through the oracle; returns timings and digests of what it produced"""
    k, raw = args
    from vc2lib import load_oracle, make_params
    oracle = load_oracle()
    p = make_params(W, H, CFMT, BITS, KERNEL, DEPTH, U, A, q=Q, scalar=SCALAR)
    t0 = time.perf_counter()
    stream = oracle.encode_stream(p, raw, 1)
    t1 = time.perf_counter()
    dec, n = oracle.decode_stream(p, stream, 1)
    t2 = time.perf_counter()
    assert n == 1
    return k, t1 - t0, t2 - t1, stream, hashlib.sha256(dec).hexdigest()


def cpu_reference(frames, rb, procs):
    """the oracle over every distinct picture: one alone (1 thread), then all of them, one process per core"""
    import multiprocessing as mp
    n = len(frames) // rb
    one = [_cpu_frame((k, bytes(frames[k * rb:(k + 1) * rb]))) for k in range(min(n, 8))]   # 1 thread: ~10 - 30 s of CPU work
    ctx = mp.get_context("fork")
    t0 = time.perf_counter()
    with ctx.Pool(processes=procs) as pool:
        res = pool.map(_cpu_frame, [(k, bytes(frames[k * rb:(k + 1) * rb])) for k in range(n)], chunksize=1)
    wall = time.perf_counter() - t0
    return one, sorted(res), wall


def dry_run(args, rank, world):
    """CPU-only exercise of the multi-rank control flow (tests/test_multi_rank.py): rendezvous, barrier, picture sharding,
    MAX-over-ranks of the step time and the rank-0 JSON line, with the ORACLE coding each rank's pictures (small ones) in
    place of the HIP library.  The line is marked dry_run: it is not a measurement."""
    import torch
    import torch.distributed as dist
    from synth import synth
    from vc2lib import load_oracle, make_params
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    w, h = 256, 128
    n_pictures = args.batch * world
    frames = synth(w, h, "422", 10, 1234, frames=n_pictures)
    rb = len(frames) // n_pictures
    mine = picture_shard(n_pictures, rank, world)
    oracle = load_oracle()
    p = make_params(w, h, "422", 10, "DD97", 3, 1, 2, q=8, scalar=1)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    check = 0
    for k in mine:   # this rank's pictures: encode and decode; what comes out must not depend on which rank did it
        raw = frames[k * rb:(k + 1) * rb]
        stream = oracle.encode_stream(p, raw, 1)
        dec, n = oracle.decode_stream(p, stream, 1)
        assert n == 1 and len(dec) == rb
        check += int.from_bytes(hashlib.sha256(stream + dec).digest()[:6], "big")   # summed over pictures: order-free
    time.sleep(0.01 * (rank + 1))       # ranks finish at different times: MAX must pick the slowest
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    counts = torch.tensor([len(mine)], dtype=torch.int64)
    mixed = torch.tensor([check], dtype=torch.int64)
    if world > 1:
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
        dist.all_reduce(mixed, op=dist.ReduceOp.SUM)
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "pictures": int(counts.item()),
                          "ms_per_step": dt.item() * 1e3, "scaling": "weak",
                          "check": int(mixed.item())}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128,
                    help="pictures per GPU per step (all distinct).  128 since round 5's two-level kernels: measured on one box, "
                         "alternating, on the round's last sources 32 / 64 / 96 / 128 / 160 / 192 / 256 pictures per step give 110.3 / "
                         "115.9 / 117.5 / 121.7 / 117.2 / 118.4 / 119.9 Gpixel/s (the launch gaps, the ramps and the tails of sixteen "
                         "kernels per step are paid once per step, and every wavefront of the streaming kernels fills and drains its "
                         "ring once per launch; between the peaks the segment plan does not fill whole rounds of wavefront slots)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: the per-kernel table and roofline, three timed regions, the halves, the "
                         "32-picture step, the parity check of every slot, the CPU baseline, end to end, the other configurations "
                         "(the options below thin it out)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (float, 32 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--cpu-procs", type=int, default=0, help="processes of the per-core CPU run (0: one per core)")
    ap.add_argument("--no-other-configs", action="store_true")
    ap.add_argument("--no-batch32", action="store_true",
                    help="skip `value_at_32_pictures_per_step` (the rocprofv3 passes: every launch of a kernel is then of the full batch, "
                         "and the per-kernel averages in profiles/ are those of the timed step)")
    ap.add_argument("--no-rank-oracle", action="store_true",
                    help="N > 1: skip the oracle's coding of every rank's slots 2..5 (profiling runs)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend of the barrier and the MAX-over-ranks (nccl = RCCL; gloo: CPU tensors, for ranks that share a GPU)")
    ap.add_argument("--streams", type=int, default=1,
                    help="HIP streams the library cuts each batch over (vc2hip_set_streams): every kernel is launched once per "
                         "stream on batch / streams pictures, and the launches of one stream fill the ramps and tails of the other's")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} != WORLD_SIZE {world}")
    if args.gpus > 1 and world == 1:
        raise SystemExit("launch with: python -m torch.distributed.run --nnodes=1 --nproc-per-node N bench.py --gpus N")
    if os.environ.get("VC2_BENCH_DRYRUN") == "1":
        return dry_run(args, rank, world)

    import numpy as np
    from synth import synth_fast

    t_start = time.perf_counter()
    B = args.batch
    # synthetic pictures: SURVEY Appendix-B generator.  Rank 0: seed 1234, B distinct frames (frames 0-1 are the pair whose
    # reference digests tests/golden holds).  Every other rank keeps that pair in its slots 0-1 (its own golden check) and
    # fills the rest with frames of its own seed 1234 + rank: the ranks code different pictures.
    # (numpy makes 0.45 UHD frames per second: at most 16 frames come from the generator, the rest of a larger batch are
    # those frames with every plane rolled down by 64 rows per repetition -- distinct pictures, coded by the oracle like any other)
    G = min(B, 16)
    if rank == 0 or B <= 2:
        frames = synth_fast(W, H, CFMT, BITS, 1234, frames=G)
    else:
        frames = synth_fast(W, H, CFMT, BITS, 1234, frames=2) + synth_fast(W, H, CFMT, BITS, 1234 + rank, frames=G - 2)
    if B > G:
        # (filled in place in ONE buffer: as a list of rolled copies joined at the end the same pictures cost a rank 90 s before it
        # touched the GPU, 70 of them in the kernel's page-fault handler -- VERDICT r5 item 8)
        rb0 = len(frames) // G
        a = np.frombuffer(frames, np.uint8).reshape(G, rb0)
        ny, nc = W * H * 2, (rb0 - W * H * 2) // 2
        cw = W if CFMT == "444" else W // 2
        buf = bytearray(B * rb0)
        out = np.frombuffer(buf, np.uint8).reshape(B, rb0)
        out[:G] = a
        for k in range(G, B):
            src, rows = a[k % G], 64 * (k // G)
            for lo, hi, rowb in ((0, ny, W * 2), (ny, ny + nc, cw * 2), (ny + nc, rb0, cw * 2)):
                sp, dp = src[lo:hi].reshape(-1, rowb), out[k, lo:hi].reshape(-1, rowb)
                r = rows % sp.shape[0]
                dp[r:] = sp[:sp.shape[0] - r]
                dp[:r] = sp[sp.shape[0] - r:]
        del out, a
        frames = buf
    rb = len(frames) // B

    # ---- CPU baseline first: nothing has touched the GPU yet, so forking worker processes is safe
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cores = os.cpu_count() or 1
        procs = args.cpu_procs or min(cores, B)
        cpu = cpu_reference(frames, rb, procs) + (cores, procs)
    # N > 1: EVERY rank has the oracle code some of ITS OWN pictures (slots 2..5: rank r's are from seed 1234 + r) in a forked
    # pool before it touches the GPU -- the parity verdict of an N-rank line is then against the oracle on every rank, not
    # only against the rank's own output in another slot.  (Not a baseline: nothing here is timed or reported.)
    oracle_slots = None
    if args.full and world > 1 and not args.no_rank_oracle:
        import multiprocessing as mp
        ks = [k for k in (2, 3, 4, 5) if k < B]
        if ks:
            with mp.get_context("fork").Pool(processes=len(ks)) as pool:
                oracle_slots = sorted(pool.map(_cpu_frame, [(k, bytes(frames[k * rb:(k + 1) * rb])) for k in ks], chunksize=1))

    if os.environ.get("VC2_BENCH_PREGPU_ONLY") == "1":   # (what a rank does before it touches the GPU, timed on its own)
        print(json.dumps({"pre_gpu_only": True, "rank": rank, "world": world, "pictures": B,
                          "seconds": round(time.perf_counter() - t_start, 2), "oracle_slots": len(oracle_slots or [])}), flush=True)
        return
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a MI355X: the HIP path has no CPU fallback")
    # rank -> HIP device: its local rank, or VC2_BENCH_DEVICE_MAP (comma list indexed by local rank; "0,0" = two ranks on one GPU)
    dev_map = [int(x) for x in os.environ.get("VC2_BENCH_DEVICE_MAP", "").split(",") if x.strip() != ""]
    dev_index = dev_map[local_rank] if local_rank < len(dev_map) else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    gloo = args.dist_backend == "gloo"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if gloo:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    red_dev = torch.device("cpu") if gloo else dev   # where the reduced scalars live

    import vc2hip_py
    hip = vc2hip_py.Vc2Hip(dev_index)
    fmt = vc2hip_py.picture_format(W, H, CFMT, BITS)
    cp = vc2hip_py.coding_params(hip.lib, fmt, KERNEL, DEPTH, U, A, q=Q, scalar=SCALAR)
    assert rb == hip.raw_picture_bytes(fmt)
    stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256

    host = torch.frombuffer(frames if isinstance(frames, bytearray) else bytearray(frames), dtype=torch.uint8)
    d_raw = host.to(dev)
    d_pay = torch.zeros(B * stride, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(B, dtype=torch.int64, device=dev)
    # THREE separately allocated output buffers, one per timed region: the physical placement of the
    # buffer the last inverse level writes moves that kernel by up to 15 %, and `value` should not be the
    # one draw a single allocation got -- it is the MEDIAN of the three regions, min and max beside it
    d_outs = [torch.zeros(B * rb, dtype=torch.uint8, device=dev) for _ in range(3 if args.full else 1)]
    d_out = d_outs[0]
    torch.cuda.synchronize()

    def enc():
        hip.encode_batch_dev(d_raw.data_ptr(), B, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())

    def dec():
        hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), B, fmt, cp, d_out.data_ptr())

    def step():
        enc()
        dec()

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, k):
        barrier()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        barrier()
        return time.perf_counter() - t0

    def headline(dt, coded):
        """the fields of a plain run's line (--full prints them first, then the rest)"""
        return {
            "metric": "Mpixels/s encode+decode, UHD-1 10-bit HQ_ConstQ",
            "value": round(W * H * B * world * args.steps / dt / 1e6, 1),
            "unit": "Mpixels/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int32",
            "dtype_note": "the reference's arithmetic: every transform, quantiser and code value is computed as int32 in registers; "
                          "the coefficient store between kernels holds int16 with an escape to int32 (exact for every input)",
            "data": f"synthetic (SURVEY Appendix-B generator, seed 1234; {B} distinct pictures per GPU" + (f": {G} generated, the others those rolled by 64 rows per repetition" if B > G else "") +
                    ("" if world == 1 else "; slots 2.. of rank r from seed 1234 + r") + ")",
            "config": {"workload": "BASELINE cfg2: UHD-1 3840x2160 4:2:2 10-bit HQ_ConstQ DD97 depth 4, -u 1 -a 2 -q 16 -S 2",
                       "pictures_per_gpu_per_step": B, "coded_bytes_per_picture": round(coded, 1), "streams": args.streams,
                       "parallelism": f"frame-parallel x{world}, no collective"},
        }

    if not args.full:
        # ---- a plain run: warm-up, exactly K timed steps, the outputs of the last one, the line
        if args.streams > 1:
            hip.set_streams(args.streams)
        for _ in range(max(1, args.warmup)):
            step()
        hip.sync()
        dt = timed(step, args.steps)
        hip.sync()  # raises on any device-side error flag
        if world > 1:
            tmax = torch.tensor([dt], dtype=torch.float64, device=red_dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)   # the slowest rank's time
            dt = tmax.item()
        if rank == 0:
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, torch, d_pay, stride, d_len, d_out, B, rb)
            print(json.dumps(headline(dt, int(d_len.sum().item()) / B)))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- the per-kernel table and the dominant kernel: ONE stream, the pictures of one launch (batch / streams), event pairs on
    # every launch, untimed.  (Paying for all ~30 event pairs of a step inside the timed region costs 4 % of it; and with
    # two streams a launch's duration includes what the other stream's kernels take from it -- the table is of kernels alone.)
    n_launch = max(1, B // max(1, min(args.streams, B)))   # pictures one launch processes

    def step_one_launch():
        hip.encode_batch_dev(d_raw.data_ptr(), n_launch, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
        hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), n_launch, fmt, cp, d_out.data_ptr())
    for _ in range(2):
        step_one_launch()
    hip.sync()
    hip.profile_reset()
    hip.profile_enable(True)
    for _ in range(3):
        step_one_launch()
    hip.sync()
    hip.profile_enable(False)
    pre = {k: v for k, v in hip.profile().items() if v[0] > 0 and k != "fill"}
    # the candidates for the step's longest kernel: the four longest of this first look; all four carry their event pairs
    # inside the timed region, and the table taken AFTER it (below) says which of them is the dominant one
    cands = sorted(pre, key=lambda k: -pre[k][1])[:4]
    hip.profile_reset()
    try:
        bus = torch.cuda.get_device_properties(dev_index)
        bus_id = "%04x:%02x:%02x.0" % (getattr(bus, "pci_domain_id", 0), bus.pci_bus_id, bus.pci_device_id)
    except Exception:
        bus_id = None
    clk = ClockSampler(bus_id)

    # ---- warm-up of the timed configuration: W untimed steps over the whole batch on `streams` streams
    if args.streams > 1:
        hip.set_streams(args.streams)
    for _ in range(max(1, args.warmup)):
        step()
    hip.sync()
    hip.profile_enable(True)

    # ---- timed region: exactly K steps; the dominant kernel's launches carry their event pairs (on the library's stream)
    hip.profile_reset()
    hip.profile_only(",".join(cands))
    clk_idle = clk.read()
    clk.start()
    region_dt = []
    for d_out in d_outs:             # (step / dec read the name at call time: each region decodes into its own buffer)
        region_dt.append(timed(step, args.steps))   # EXACTLY K steps between barrier + synchronize, three times
    clocks = clk.stop()
    hip.sync()  # collects the event pairs; raises on any device-side error flag
    if world > 1:
        rmax = torch.tensor(region_dt, dtype=torch.float64, device=red_dev)
        dist.all_reduce(rmax, op=dist.ReduceOp.MAX)   # every region: the slowest rank's time
        region_dt = rmax.tolist()
    dt = sorted(region_dt)[1]
    d_out = d_outs[region_dt.index(dt)]   # everything below (the other timings, the parity check) uses the median region's buffer
    same_out = all(torch.equal(d_outs[0], b) for b in d_outs[1:])
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, torch, d_pay, stride, d_len, d_out, B, rb)
    hip.profile_enable(False)
    hip.profile_only(None)
    prof = hip.profile()

    # ---- the per-kernel table, taken AFTER the timed region on the warm GPU (the table of round 4 was
    # taken from 3 steps right behind 2 warm launches and summed to 6 % more than the step it described): w_steps passes
    # with an event pair on every launch, the clocks sampled the same way
    if args.streams > 1:
        hip.set_streams(1)
    for _ in range(3):
        step_one_launch()
    hip.sync()
    w_steps = 10
    hip.profile_reset()
    hip.profile_enable(True)
    clk.start()
    for _ in range(w_steps):
        step_one_launch()
    hip.sync()
    clocks_table = clk.stop()
    hip.profile_enable(False)
    warm = {k: v for k, v in hip.profile().items() if v[0] > 0 and k != "fill"}
    dom = max(warm, key=lambda k: warm[k][1] / warm[k][0]) if warm else None   # the longest single launch
    if dom not in prof or prof[dom][0] == 0:   # (not among the candidates: the longest that was)
        dom = max((k for k in warm if k in prof and prof[k][0] > 0), key=lambda k: warm[k][1] / warm[k][0], default=None)
    if dom is None:
        raise SystemExit("no kernel of the timed region carried an event pair: nothing to price the roofline with")
    hip.profile_reset()
    if args.streams > 1:
        hip.set_streams(args.streams)

    # ---- beside it (never `value`): the same region without the per-kernel events; the two halves on their own
    dt_noev = timed(step, args.steps)
    dt_enc = timed(enc, args.steps)
    dt_dec = timed(dec, args.steps)
    # the same step over 32 pictures (rounds 1 - 4 quoted the metric at 32 per step; ADVICE r5: keep that number beside `value`)
    B32 = min(32, B)

    def step32():
        hip.encode_batch_dev(d_raw.data_ptr(), B32, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
        hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), B32, fmt, cp, d_out.data_ptr())
    dt_32 = None
    if not args.no_batch32:
        step32()
        dt_32 = timed(step32, args.steps)
        step()   # (the buffers hold the whole batch's results again for the parity check below)
        hip.sync()
    tmax = torch.tensor([dt_noev, dt_enc, dt_dec, dt_32 or 0.0], dtype=torch.float64, device=red_dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt_noev, dt_enc, dt_dec, dt_32 = tmax.tolist()

    # ---- parity of what was timed: EVERY slot of the batch, on EVERY rank; the verdicts are AND-reduced and a failure on
    # any rank suppresses the line
    lens = d_len.cpu().numpy().astype(np.int64)
    coded = int(lens.sum()) / B
    parity, failure = None, None
    if not same_out:
        failure = "the three timed regions' output buffers differ"
    if os.environ.get("VC2_BENCH_SABOTAGE") == "1" and B >= 2:   # tests/test_multi_rank_gpu.py: the guard must catch a wrong slot
        d_out.view(B, rb)[[0, 1]] = d_out.view(B, rb)[[1, 0]]
    out_host = d_out.cpu().numpy()
    pay_host = d_pay.cpu().numpy()
    if cpu is not None:   # (rank 0 of a one-rank run) against the oracle's bytes of every picture
        for (k, _, _, stream, sha_dec) in cpu[1]:
            pay = pay_host[k * stride:k * stride + int(lens[k])].tobytes()
            if pay != stream[-13 - len(pay):-13] or hashlib.sha256(out_host[k * rb:(k + 1) * rb].tobytes()).hexdigest() != sha_dec:
                failure = f"slot {k}: HIP output differs from the oracle"
                break
        parity = f"all {B} slots: slice payload and decoded picture byte for byte against the oracle"
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_digests.json")))["cfg2"]
    if failure is None and B >= 2 and hashlib.sha256(out_host[:2 * rb].tobytes()).hexdigest() != gold["decoded"]["sha256"]:
        failure = "decoded pictures 0-1 differ from the reference digest"
    if failure is None and oracle_slots:   # (N > 1) this rank's slots 2..5 against the oracle's bytes
        for (k, _, _, stream, sha_dec) in oracle_slots:
            pay = pay_host[k * stride:k * stride + int(lens[k])].tobytes()
            if pay != stream[-13 - len(pay):-13] or hashlib.sha256(out_host[k * rb:(k + 1) * rb].tobytes()).hexdigest() != sha_dec:
                failure = f"slot {k}: HIP output differs from the oracle"
                break
    if failure is None and parity is None:   # no CPU run: slots 0-1 against the reference digest, every slot must decode to
        # what it decodes to when the batch is coded again in another order (slot independence)
        perm = torch.arange(B - 1, -1, -1, device=dev)
        d_raw2 = d_raw.view(B, rb)[perm].contiguous().view(-1)
        d_out2 = torch.zeros_like(d_out)
        d_pay2 = torch.zeros_like(d_pay)
        d_len2 = torch.zeros_like(d_len)
        torch.cuda.synchronize()   # torch built these on ITS stream; the library reads them on its own
        hip.encode_batch_dev(d_raw2.data_ptr(), B, fmt, cp, d_pay2.data_ptr(), stride, d_len2.data_ptr())
        hip.decode_batch_dev(d_pay2.data_ptr(), stride, d_len2.data_ptr(), B, fmt, cp, d_out2.data_ptr())
        hip.sync()
        if not torch.equal(d_out2.view(B, rb)[perm].contiguous().view(-1), d_out):
            failure = "a picture decodes differently in another slot"
        elif not torch.equal(d_len2[perm], d_len):
            failure = "a picture codes to another length in another slot"
        parity = "slots 0-1 against the reference digest; " + \
                 (f"slots {oracle_slots[0][0]}-{oracle_slots[-1][0]} of every rank byte for byte against the oracle; " if oracle_slots else "") + \
                 "every slot against the same picture coded in another slot"
        del d_raw2, d_out2, d_pay2, d_len2
    del out_host, pay_host
    ok = torch.tensor([0 if failure else 1], dtype=torch.int32, device=red_dev)
    if world > 1:
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if failure:
        print(f"rank {rank}: {failure}: refusing to report a number", file=sys.stderr)
    if int(ok.item()) == 0:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        raise SystemExit(failure or "another rank's output failed its check: refusing to report a number")
    if world > 1:
        parity = f"every rank: {parity}; verdicts AND-reduced over {world} ranks (slots 2.. differ from rank to rank)"

    # ---- end to end: pictures start and end in pinned host memory; two streams, copies overlapped with kernels
    e2e = None
    if rank == 0 and world == 1 and not args.no_e2e:
        e2e = run_e2e(torch, vc2hip_py, dev, frames, rb, fmt, cp, stride, lens, B, d_out)

    other = None
    if rank == 0 and world == 1 and not args.no_other_configs:
        other = run_other_configs(torch, vc2hip_py, hip, dev, frames, rb, max(1, args.streams))

    pixels = W * H
    total_px = pixels * B * world * args.steps
    out = None
    if rank == 0:
        # algorithmic bytes: encode w*S + C, decode C + w*S per picture
        samples = W * H * 2  # 4:2:2
        alg_dir = 2 * samples + coded
        launches_per_step = B / n_launch
        kern_launch_ms = {k: v[1] / w_steps for k, v in warm.items()}    # one encode + decode of n_launch pictures, kernels alone
        kern_step_ms = {k: v * launches_per_step for k, v in kern_launch_ms.items()}
        dom_launches, dom_ms = prof[dom]                                  # the dominant kernel, live in the timed region
        dom_avg_s = dom_ms / dom_launches / 1e3
        per_launch = n_launch
        achieved = alg_dir * per_launch / dom_avg_s / 1e9
        solo_avg_s = warm[dom][1] / warm[dom][0] / 1e3                    # the same kernel with the GPU to itself
        solo_achieved = alg_dir * per_launch / solo_avg_s / 1e9
        path_achieved = 2 * alg_dir * B / (dt / args.steps) / 1e9         # the whole step: what the timed region sustained
        path_solo = 2 * alg_dir * n_launch / (sum(kern_launch_ms.values()) / 1e3) / 1e9
        # HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE in
        # separate runs, gfx950 correction applied).  Only valid for the kernel sources it was measured on.
        traffic, traffic_note, path_traffic = None, "no committed PMC profile", None
        for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True):
            try:
                pmc = json.load(open(f))
            except (OSError, ValueError):
                continue
            if pmc.get("csrc_digest") != csrc_digest():
                traffic_note = f"{os.path.basename(f)} was measured on other kernel sources (digest {pmc.get('csrc_digest')})"
                continue
            if pmc.get("pictures_per_launch") == per_launch and dom in pmc.get("kernels", {}):
                traffic = pmc["kernels"][dom]["hbm_bytes_per_launch"]
                # the whole path: every kernel of a step -- its launches per step (this run's own count) x its bytes per launch
                # (the PMC file), as counted (FETCH_SIZE + WRITE_SIZE) and with the guide's 2 x FETCH_SIZE
                path_traffic = {"as_counted": 0, "fetch_x2": 0}
                for k, v in warm.items():
                    n_k = v[0] / w_steps * launches_per_step   # launches of kernel k per step
                    rows = [r for name, r in pmc["kernels"].items() if name == k or name.startswith(k + "(")]
                    if not rows:
                        path_traffic = None
                        break
                    # (a name with several instantiations per pass, e.g. the levels below the first: the file holds their average)
                    path_traffic["as_counted"] += int(n_k * sum((r["FETCH_SIZE_KiB"] + r["WRITE_SIZE_KiB"]) * 1024 for r in rows) / len(rows))
                    path_traffic["fetch_x2"] += int(n_k * sum(r["hbm_bytes_per_launch"] for r in rows) / len(rows))
                traffic_note = f"committed profile {os.path.basename(f)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this bench), not collected by this run"
                break
        out = {
            **headline(dt, coded),
            "encode_only": {"value": round(total_px / dt_enc / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(dt_enc / args.steps * 1e3, 4)},
            "decode_only": {"value": round(total_px / dt_dec / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(dt_dec / args.steps * 1e3, 4)},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_note,
                         "kernel": dom, "kernel_avg_ms": round(dom_ms / dom_launches, 4),
                         "solo_achieved": round(solo_achieved, 1), "solo_frac": round(solo_achieved / HBM_PEAK_GBS, 4),
                         "solo_kernel_avg_ms": round(solo_avg_s * 1e3, 4),
                         "solo_note": "the same kernel, same pictures per launch, launched on ONE stream (untimed table pass): with "
                                      f"{args.streams} streams a launch shares the GPU with the other stream's kernels and `frac` prices that contention in",
                         "algorithmic_bytes_per_launch": int(alg_dir * per_launch),
                         "path_achieved_GBs": round(path_achieved, 1),
                         "path_frac": round(path_achieved / HBM_PEAK_GBS, 4),
                         "path_frac_note": "algorithmic bytes of a step / measured step time of the timed region",
                         "path_solo_frac": round(path_solo / HBM_PEAK_GBS, 4),
                         "path_algorithmic_bytes_per_step": int(2 * alg_dir * B),
                         "path_traffic_bytes": path_traffic,
                         "path_traffic_ratio": ({k: round(v / (2 * alg_dir * B), 2) for k, v in path_traffic.items()} if path_traffic else None),
                         "kernel_events": f"the {dom_launches} launches of `{dom}` inside the timed region (the event pairs of "
                                          f"{', '.join(cands)} ride in the timed region; the table after it names the longest)",
                         "kernel_in_run_ms": {k: round(prof[k][1] / prof[k][0], 4) for k in cands if k in prof and prof[k][0]},
                         "kernel_ms_per_step": {k: round(v, 4) for k, v in sorted(kern_step_ms.items())},
                         "kernel_ms_per_step_sum": round(sum(kern_step_ms.values()), 4),
                         "launch_gap_ms": round(dt / args.steps * 1e3 - sum(kern_step_ms.values()), 4),
                         "launch_gap_note": "ms_per_step of the timed region minus the sum of the table: what the step spends between its "
                                            "kernels (negative: the kernels ran faster inside the timed region than in the table pass)",
                         "kernel_ms_per_step_source": f"event pairs on every launch of {w_steps} untimed one-stream passes over {n_launch} pictures (one launch's worth) "
                                                      f"run right AFTER the timed region on the warm GPU, times {launches_per_step:g} launches per step: kernels alone, additive"},
            "clocks": {"timed_region": clocks, "table_pass": clocks_table,
                       "idle_before": (ClockSampler.summary([clk_idle]) if clk_idle else None),
                       "source": (f"{clk.dir}: freq1_input (sclk), freq2_input (mclk), power1_input, sampled every ~10 ms by a thread while the region runs"
                                  if clk.dir else "no readable amdgpu hwmon files for this device")},
            "value_regions": {"values": [round(total_px / t / 1e6, 1) for t in region_dt],
                              "min": round(total_px / max(region_dt) / 1e6, 1), "max": round(total_px / min(region_dt) / 1e6, 1),
                              "note": f"three timed regions of {args.steps} steps each, every one between barrier + synchronize, each decoding into "
                                      "its own separately allocated output buffer; `value` / `ms_per_step` are the MEDIAN region's"},
            "value_at_32_pictures_per_step": (None if not dt_32 else
                                              {"value": round(pixels * B32 * world * args.steps / dt_32 / 1e6, 1), "unit": "Mpixels/s",
                                               "ms_per_step": round(dt_32 / args.steps * 1e3, 4),
                                               "note": "the unit rounds 1 - 4 quoted; the same buffers, the first 32 pictures per step"}),
            "value_without_kernel_events": round(total_px / dt_noev / 1e6, 1),
            "parity_checked": parity,
            "e2e": e2e,
            "other_configs": other,
        }
        if cpu is not None:
            one, res, wall, cores, procs = cpu
            t_enc, t_dec = sum(r[1] for r in one), sum(r[2] for r in one)
            out["cpu_baseline"] = {
                "value": round(pixels * len(one) / (t_enc + t_dec) / 1e6, 3), "unit": "Mpixels/s", "cores": 1, "kind": "port",
                "sample": f"{len(one)} UHD-1 pictures of the same workload, encode {t_enc:.1f} s + decode {t_dec:.1f} s through oracle/ (1 thread)",
                "per_core_run": {"value": round(pixels * len(res) / wall / 1e6, 3), "unit": "Mpixels/s", "cores": procs,
                                 "host_cores": cores,
                                 "sample": f"all {len(res)} pictures of the batch, one process per core ({procs}), {wall:.1f} s wall; "
                                           f"mean {sum(r[1] + r[2] for r in res) / len(res):.2f} s per picture and core under load"},
                "port_vs_reference": PORT_VS_REFERENCE,
                "port_vs_reference_note": "oracle : reference speed on the same cores, measured in the build container (reference "
                                          "2.9 + 1.86 s, oracle 2.2 + 1.5 s per UHD frame); the reference cannot travel to the GPU box",
            }
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


OTHER_CFGS = {
    # name: geometry and coding parameters of BASELINE.json configs[0], [2], [3], [4]; B pictures per step.
    # B from the round-6 sweep (tools/batch_sweep.sh, one box, encode+decode Gpixel/s; VERDICT r5 item 7b -- rounds 1 - 5 ran these
    # lines at 16 (cfg 4: 4) pictures per step while the headline ran 128):
    #   cfg1  16 / 32 / 64 / 128: 51.6 / 62.0 / 69.1 / 73.3      cfg3  16 / 32 / 64 / 128: 73.7 / 82.6 / 88.3 / 93.5
    #   cfg4  4 / 8 / 16 / 32:    45.7 / 50.6 / 53.9 / 55.4      cfg5 (encode+decode there) 16 ... 256: 7.8 / 9.2 / 9.9 / 10.3 / 10.5
    # (the step amortises its ~16 launches, their ramps and tails; cfg 3 takes as many of the headline's pictures as exist)
    "cfg1": dict(w=1920, h=1080, cf="422", bits=10, wb=2, k="LeGall", d=2, u=2, a=4, B=128, kw=dict(q=12, scalar=1),
                 workload="BASELINE cfg1: 1920x1080 4:2:2 10-bit HQ_ConstQ LeGall depth 2, -u 2 -a 4 -q 12"),
    "cfg3": dict(w=3840, h=2160, cf="422", bits=10, wb=2, k="DD97", d=4, u=1, a=2, B=128, kw=dict(mode="HQ_CBR", s=8294400, scalar=2),
                 workload="BASELINE cfg3: UHD-1 3840x2160 4:2:2 10-bit HQ_CBR DD97 depth 4, -u 1 -a 2 -s 8294400 -S 2"),
    "cfg4": dict(w=7680, h=4320, cf="444", bits=12, wb=2, k="Fidelity", d=5, u=1, a=1, B=16, kw=dict(q=40, scalar=8),
                 workload="BASELINE cfg4: UHD-2 7680x4320 4:4:4 12-bit HQ_ConstQ Fidelity depth 5, -u 1 -a 1 -q 40 -S 8 (16 pictures on ONE GPU)"),
    "cfg5": dict(w=1920, h=1080, cf="422", bits=8, wb=1, k="LeGall", d=3, u=1, a=2, B=128, kw=dict(mode="LD", s=1036800),
                 workload="BASELINE cfg5: 1920x1080 4:2:2 8-bit LD LeGall depth 3, -u 1 -a 2 -s 1036800, DECODE only"),
}


def kernel_own_bytes(name, S, w, rawb, C, depth):
    """compulsory bytes of one kernel per picture: S samples, w bytes per store element, rawb bytes per raw
    sample, C coded bytes"""
    deep = sum(4.0 ** -l for l in range(1, depth))   # levels 1 .. depth-1 relative to level 0
    return {"dwt_level_first": (rawb + w) * S, "idwt_level_final": (rawb + w) * S, "dwt_level": 2 * w * S * deep, "idwt_level": 2 * w * S * deep,
            "hq_pack": w * S + C, "hq_unpack": C + w * S, "cbr_search": w * S, "ld_search": 2 * 4 * S, "ld_pack": 4 * S + C,
            "ld_unpack": C + 4 * S}.get(name)


def run_other_configs(torch, vc2hip_py, hip, dev, frames_cfg2, rb_cfg2, n_streams):
    """cfg 1, 3, 4 and 5 (decode) through the same device-resident batch path, 5 steps each.  Picture 0 of every batch is the
    SURVEY generator's frame 0 (what the reference digests were recorded on) and is checked against them (cfg 5: against
    the oracle); the other pictures of a batch are that frame rolled by 64 k rows (distinct content without minutes of
    numpy), cfg 3 takes the cfg-2 batch as it is.  A mismatch refuses the whole line."""
    import ctypes as C
    import numpy as np
    from synth import synth
    from vc2lib import load_oracle, make_params
    oracle = load_oracle()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_digests.json")))
    res = {}
    for name, c in OTHER_CFGS.items():
        w, h, cf, bits, wb, B = c["w"], c["h"], c["cf"], c["bits"], c["wb"], c["B"]
        fmt = vc2hip_py.picture_format(w, h, cf, bits, wb)
        cp = vc2hip_py.coding_params(hip.lib, fmt, c["k"], c["d"], c["u"], c["a"], **c["kw"])
        rb = hip.raw_picture_bytes(fmt)
        stride = (hip.max_payload_bytes(fmt, cp) + 255) // 256 * 256
        if name == "cfg3":
            B = min(B, len(frames_cfg2) // rb_cfg2)
            d_raw = torch.frombuffer(bytearray(frames_cfg2[:B * rb]), dtype=torch.uint8).to(dev)
        else:
            one = torch.frombuffer(bytearray(synth(w, h, cf, bits, 1234, frames=1, word_bytes=wb)), dtype=torch.uint8).to(dev)
            cw = w if cf == "444" else w // 2
            planes = [(0, w * h * wb, w * wb), (w * h * wb, (rb - w * h * wb) // 2, cw * wb), (w * h * wb + (rb - w * h * wb) // 2, (rb - w * h * wb) // 2, cw * wb)]
            pics = [one]
            for k in range(1, B):   # picture k: every plane rolled down by 64 k rows
                pics.append(torch.cat([torch.roll(one[o:o + n].view(-1, rowb), 64 * k, 0).reshape(-1) for (o, n, rowb) in planes]))
            d_raw = torch.cat(pics)
            del pics
        d_pay = torch.zeros(B * stride, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(B, dtype=torch.int64, device=dev)
        d_out = torch.zeros(B * rb, dtype=torch.uint8, device=dev)
        p = make_params(w, h, cf, bits, c["k"], c["d"], c["u"], c["a"], word_bytes=wb, **c["kw"])
        decode_only = name == "cfg5"
        if decode_only:   # the oracle's LD stream of frame 0 in every slot; the GPU's LD encoder must produce the same bytes
            raw0 = bytes(d_raw[:rb].cpu().numpy())
            stream = oracle.encode_stream(p, raw0, 1)
            want_dec, _ = oracle.decode_stream(p, stream, 1)
            nbytes = c["kw"]["s"]
            payload = np.frombuffer(stream[-13 - nbytes:-13], np.uint8)
            hp = torch.zeros(B, stride, dtype=torch.uint8)
            hp[:, :nbytes] = torch.from_numpy(payload.copy())
            d_pay.copy_(hp.view(-1))
            d_len.fill_(nbytes)
        torch.cuda.synchronize()

        def step():
            if not decode_only:
                hip.encode_batch_dev(d_raw.data_ptr(), B, fmt, cp, d_pay.data_ptr(), stride, d_len.data_ptr())
            hip.decode_batch_dev(d_pay.data_ptr(), stride, d_len.data_ptr(), B, fmt, cp, d_out.data_ptr())
        for _ in range(2):
            step()
        hip.sync()
        torch.cuda.synchronize()
        K = 5
        t0 = time.perf_counter()
        for _ in range(K):
            step()
        hip.sync()
        dt = (time.perf_counter() - t0) / K
        hip.profile_reset()
        hip.set_streams(1)         # the per-kernel table: kernels alone (one stream), steps outside the timed ones; the first
        hip.profile_enable(True)   # creates the event pairs and is discarded
        step()
        hip.sync()
        hip.profile_reset()
        for _ in range(3):
            step()
        hip.sync()
        hip.profile_enable(False)
        hip.set_streams(n_streams)   # what the timed steps of the next configuration run on
        prof = {k: v[1] / 3 for k, v in hip.profile().items() if v[0] > 0 and k != "fill"}
        hip.profile_reset()
        # ---- check picture 0 (and that the other slots are not copies of it)
        lens = d_len.cpu().numpy().astype(np.int64)
        dec0 = d_out[:rb].cpu().numpy().tobytes()
        if decode_only:
            ok = dec0 == want_dec
            got, _ = hip.encode_picture_hq(raw0, fmt, cp)
            ok = ok and got == payload.tobytes()
            checked = "picture 0 decoded == the oracle's decode of the oracle's LD stream; the GPU's LD encoder reproduces that stream"
        else:
            g = gold[name]
            pay0 = d_pay[:int(lens[0])].cpu().numpy().tobytes()
            hdr = np.zeros(64, np.uint8); n = C.c_size_t(); major = C.c_int()
            oracle.lib.vc2o_write_sequence_header_payload(C.byref(p), hdr.ctypes.data_as(C.c_void_p), 64, C.byref(n), C.byref(major))
            seq = bytes(hdr[:n.value])
            ph = np.zeros(64, np.uint8); m = C.c_size_t()
            oracle.lib.vc2o_write_hq_picture_header(0, p.kernel, c["d"], cp.x_slices, cp.y_slices, cp.prefix, cp.scalar, major.value,
                                                    ph.ctypes.data_as(C.c_void_p), 64, C.byref(m))

            def pi(code, nxt, prev):
                return b"BBCD" + bytes([code]) + nxt.to_bytes(4, "big") + prev.to_bytes(4, "big")
            n1, n2 = 13 + len(seq), 13 + m.value + len(pay0)
            stream = pi(0x00, n1, 0) + seq + pi(0xE8, n2, n1) + bytes(ph[:m.value]) + pay0 + pi(0x10, 0, n2)
            ok = hashlib.sha256(stream).hexdigest() == g["stream"]["sha256"] and hashlib.sha256(dec0).hexdigest() == g["decoded"]["sha256"]
            ok = ok and (B < 2 or not torch.equal(d_out[:rb], d_out[rb:2 * rb]))
            checked = "picture 0: stream (oracle header writers around the GPU payload) and decoded picture against the reference digests"
        if not ok:
            raise SystemExit(f"{name}: HIP output differs from the reference digest / the oracle: refusing to report a number")
        S = rb // wb
        coded = float(lens.mean())
        domk = max(prof, key=prof.get)
        own = kernel_own_bytes(domk, S, 4 if decode_only else 2, wb, coded, c["d"])
        alg = (4 if decode_only else 2) * S + coded   # per picture and direction
        res[name] = {"workload": c["workload"], "pictures_per_step": B, "steps": K,
                     "value": round(w * h * B / dt / 1e6, 1), "unit": "Mpixels/s " + ("decode" if decode_only else "encode+decode"),
                     "ms_per_step": round(dt * 1e3, 4),
                     "path_frac": round((1 if decode_only else 2) * alg * B / dt / 1e9 / HBM_PEAK_GBS, 4),
                     "dominant_kernel": domk, "dominant_kernel_ms": round(prof[domk], 4),
                     "dominant_kernel_own_GBs": (round(own * B / (prof[domk] / 1e3) / 1e9, 1) if own else None),
                     "dominant_kernel_frac": (round(own * B / (prof[domk] / 1e3) / 1e9 / HBM_PEAK_GBS, 4) if own else None),
                     "kernel_ms_per_step": {k: round(v, 4) for k, v in sorted(prof.items())},
                     "kernel_ms_per_step_source": "event pairs on every launch of 3 untimed ONE-stream steps (kernels alone, additive); "
                                                  f"the timed steps run on {n_streams} streams",
                     "coded_bytes_per_picture": round(coded, 1), "checked": checked}
        del d_raw, d_pay, d_len, d_out
        torch.cuda.empty_cache()
    return res


def run_e2e(torch, vc2hip_py, dev, frames, rb, fmt, cp, stride, lens, B, d_out):
    """Host memory to host memory.  Two HIP streams, each with its own library context and pinned staging buffers; a chunk
    of pictures goes H2D -> kernels -> D2H on one stream while the other stream works on the next chunk, so copies in
    both directions overlap with kernels.  Encode returns exactly the coded bytes (the lengths come back first)."""
    CH, NCH = 4, 8   # pictures per chunk, chunks timed (cycling over the batch's pictures)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    ctx = [vc2hip_py.Vc2Hip(dev.index or 0, stream=s.cuda_stream) for s in streams]
    h_raw = torch.frombuffer(bytearray(frames), dtype=torch.uint8).pin_memory()
    maxlen = int(lens.max())
    span = (maxlen + 255) // 256 * 256
    bufs = []
    for s in streams:
        bufs.append(dict(d_raw=torch.empty(CH * rb, dtype=torch.uint8, device=dev),
                         d_pay=torch.zeros(CH * stride, dtype=torch.uint8, device=dev),
                         d_len=torch.zeros(CH, dtype=torch.int64, device=dev),
                         d_out=torch.empty(CH * rb, dtype=torch.uint8, device=dev),
                         h_len=torch.zeros(CH, dtype=torch.int64).pin_memory(),
                         h_pay=torch.empty(CH * span, dtype=torch.uint8).pin_memory(),
                         h_out=torch.empty(CH * rb, dtype=torch.uint8).pin_memory()))
    nchunks_batch = B // CH

    def encode_chunk(i, c):
        b, s, h = bufs[i], streams[i], ctx[i]
        k0 = (c % nchunks_batch) * CH
        with torch.cuda.stream(s):
            b["d_raw"].copy_(h_raw[k0 * rb:(k0 + CH) * rb], non_blocking=True)
            h.encode_batch_dev(b["d_raw"].data_ptr(), CH, fmt, cp, b["d_pay"].data_ptr(), stride, b["d_len"].data_ptr())
            b["h_len"].copy_(b["d_len"], non_blocking=True)

    def encode_finish(i):
        b, s = bufs[i], streams[i]
        s.synchronize()   # the lengths are on the host (the other stream keeps the GPU busy meanwhile)
        with torch.cuda.stream(s):
            for j in range(CH):
                n = int(b["h_len"][j])
                b["h_pay"][j * span:j * span + n].copy_(b["d_pay"][j * stride:j * stride + n], non_blocking=True)

    def decode_chunk(i, c):
        b, s, h = bufs[i], streams[i], ctx[i]
        with torch.cuda.stream(s):
            for j in range(CH):
                n = int(b["h_len"][j])
                b["d_pay"][j * stride:j * stride + n].copy_(b["h_pay"][j * span:j * span + n], non_blocking=True)
            b["d_len"].copy_(b["h_len"], non_blocking=True)
            h.decode_batch_dev(b["d_pay"].data_ptr(), stride, b["d_len"].data_ptr(), CH, fmt, cp, b["d_out"].data_ptr())
            b["h_out"].copy_(b["d_out"], non_blocking=True)

    def run(fn_issue, fn_finish):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in range(NCH):
            i = c & 1
            if c >= 2 and fn_finish is None:
                streams[i].synchronize()   # the buffers of this stream are free again
            fn_issue(i, c)
            if fn_finish is not None:
                if c >= 1:
                    fn_finish(1 - i)
        if fn_finish is not None:
            fn_finish((NCH - 1) & 1)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    run(encode_chunk, encode_finish)          # warm-up (also leaves coded chunks in both streams' host buffers)
    te = run(encode_chunk, encode_finish)
    run(decode_chunk, None)
    td = run(decode_chunk, None)
    for h in ctx:
        h.sync()
    # ---- both directions at once: the link is full duplex (raw pictures go in for the encoder while decoded ones come out).
    # A second pair of streams / contexts / buffers decodes the chunks coded above while the first pair encodes.
    streams2 = [torch.cuda.Stream(device=dev) for _ in range(2)]
    ctx2 = [vc2hip_py.Vc2Hip(dev.index or 0, stream=s.cuda_stream) for s in streams2]
    bufs2 = []
    for i in range(2):
        b = bufs[i]
        bufs2.append(dict(d_pay=torch.zeros(CH * stride, dtype=torch.uint8, device=dev), d_len=torch.zeros(CH, dtype=torch.int64, device=dev),
                          d_out=torch.empty(CH * rb, dtype=torch.uint8, device=dev), h_len=b["h_len"].clone().pin_memory(),
                          h_pay=b["h_pay"].clone().pin_memory(), h_out=torch.empty(CH * rb, dtype=torch.uint8).pin_memory()))

    def decode_chunk2(i):
        b, s, h = bufs2[i], streams2[i], ctx2[i]
        with torch.cuda.stream(s):
            for j in range(CH):
                n = int(b["h_len"][j])
                b["d_pay"][j * stride:j * stride + n].copy_(b["h_pay"][j * span:j * span + n], non_blocking=True)
            b["d_len"].copy_(b["h_len"], non_blocking=True)
            h.decode_batch_dev(b["d_pay"].data_ptr(), stride, b["d_len"].data_ptr(), CH, fmt, cp, b["d_out"].data_ptr())
            b["h_out"].copy_(b["d_out"], non_blocking=True)

    def run_both():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in range(NCH):
            i = c & 1
            if c >= 2:
                streams2[i].synchronize()
            encode_chunk(i, c)
            decode_chunk2(i)
            if c >= 1:
                encode_finish(1 - i)
        encode_finish((NCH - 1) & 1)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    run_both()
    tb = run_both()
    for h in ctx + ctx2:
        h.sync()
    both_ok = all(torch.equal(bufs2[i]["h_out"], bufs[i]["h_out"]) for i in range(2))   # the same chunks decode to the same pictures
    if not both_ok:
        raise SystemExit("end-to-end pipeline: concurrent decode returned other pictures")
    for i in range(2):   # what came back on each stream is the decode of the chunk it encoded last
        k0 = ((NCH - 2 + i) % nchunks_batch) * CH
        if not torch.equal(bufs[i]["h_out"], d_out[k0 * rb:(k0 + CH) * rb].cpu()):
            raise SystemExit("end-to-end pipeline returned other pictures than the device-resident path")
    px = W * H * CH * NCH
    return {"encode": {"value": round(px / te / 1e6, 1), "unit": "Mpixels/s"},
            "decode": {"value": round(px / td / 1e6, 1), "unit": "Mpixels/s"},
            "encode+decode": {"value": round(px / (te + td) / 1e6, 1), "unit": "Mpixels/s"},
            "encode||decode": {"value": round(px / tb / 1e6, 1), "unit": "Mpixels/s (pictures encoded AND as many decoded in that time, both directions of the link at once)",
                               "host_link_GBs_each_way": round((rb + maxlen) * CH * NCH / tb / 1e9, 1)},
            "host_link_GBs": {"encode_in": round(rb * CH * NCH / te / 1e9, 1), "decode_out": round(rb * CH * NCH / td / 1e9, 1)},
            "method": f"pinned host buffers, 2 HIP streams x chunks of {CH} pictures, H2D / kernels / D2H of consecutive chunks overlapped; "
                      f"{CH * NCH} pictures per direction; bound by the PCIe Gen5 x16 link (33.2 MB in + ~9.4 MB out per picture)"}


if __name__ == "__main__":
    main()
