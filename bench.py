#!/usr/bin/env python3
"""bench.py - Mpixels/s of the embed + extract round trip at 4K on MI355X (BASELINE.json metric).

One STEP = one pass of the hot path over one device-resident batch: the fused embed kernel over
all frames of the batch, then the fused extract kernel over the stego frames it wrote
(+ for N > 1 the RCCL gather of the extracted packed bits to rank 0).  Inputs are synthetic,
generated on the device before the timed region.

Workload at N = 1 (config.workload): BASELINE.json configs[2], the configuration the metric is
quoted on - 3840x2160, 600 frames, 3 AC coefficients per block, delta 8, full-capacity payload.
With --gpus N every rank runs that batch on its own frames (weak scaling; frames are
independent units, the only exchange is the gather of extracted bits).

The timed mode is the product default ("guarded": what the drop-in operator and the video pipelines run - bit-identical to
the reference; --mode exact selects the lane-per-block pocketfft kernels, "fast" is an alias of the default).

Prints ONE JSON line (rank 0).  `roofline` is for the dominant kernel (embed): algorithmic bytes
per launch / its mean launch time measured with HIP events on the launch stream inside the timed
region.  `cpu_baseline` (N = 1 only) times the oracle - the vectorised SciPy restatement of the
reference's operator - on a bounded sample of the same frames on this box's host cores: one worker
process per core (up to 32) for `cpu_baseline`, one thread for `cpu_baseline_single_thread`.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(REPO, "secure-video-steganography-using-ecc-and-dct_amd")
for _p in (PKG_DIR, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)
SEED = 20250620


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=600, help="frames per GPU per step (weak scaling: every rank runs this batch)")
    ap.add_argument("--total-frames", type=int, default=0,
                    help="strong scaling: frames of the WHOLE job, divided over the ranks by svsdct.batch.shard_frames "
                         "(contiguous ranges, rank order = stream order); overrides --frames, e.g. --total-frames 2400 "
                         "--height 1080 --width 1920 --n-ac 10 for BASELINE configs[3], --total-frames 1200 --height 4320 "
                         "--width 7680 for configs[4]")
    ap.add_argument("--mode", default=None, choices=["fast", "guarded", "exact"],
                    help="transform mode of the timed embed / extract (default: guarded - what the drop-in operator and the "
                         "video pipelines run: bit-identical to the reference; at n_ac <= 15 fast is the same launch)")
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--n-ac", type=int, default=3)
    ap.add_argument("--delta", type=float, default=8.0)
    ap.add_argument("--cpu-frames", type=int, default=96,
                    help="frames in the CPU-baseline samples (all-core leg and single-thread leg; 0 = skip)")
    ap.add_argument("--rehearse-gloo", action="store_true",
                    help="rank-logic rehearsal on a box with fewer GPUs than ranks: gloo backend, ranks share "
                         "GPUs, collectives staged through host memory (numbers are NOT bench results)")
    ap.add_argument("--pmc-check", action="store_true",
                    help="measure roofline.traffic in THIS run instead of reading the committed capture: before this process touches "
                         "the GPU, two child processes run 2 steps of the same workload under `rocprofv3 --pmc FETCH_SIZE` / "
                         "`--pmc WRITE_SIZE` (+ --kernel-trace only); N = 1, needs rocprofv3 on PATH")
    ap.add_argument("--inject-gather-swap", action="store_true",
                    help="TEST HOOK: rank 0 swaps the first two slices of the gathered stream before it checks them - the run must "
                         "then end with a non-zero exit code (tests/test_bench_gpu.py)")
    ap.add_argument("--force-dist", action="store_true",
                    help="take the process-group path (RCCL gather included) even with one rank, so that a one-GPU box "
                         "exercises the collective calls")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, rank 0 writes what the last timed step returned as DIR/<name>.npy (float32 / "
                         "float64, at most 64 MiB in all; see dump_outputs) so that two builds can be compared output for output")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def job_plan(args, world: int) -> dict:
    """Who does what in a `world`-rank run of these arguments - pure arithmetic, no GPU, no torch (main() runs on it, and the
    CPU test tier dry-runs the documented multi-GPU commands through it): per-rank frame shares (contiguous, rank order =
    stream order), each rank's offset into the job's bit stream, the bytes every rank contributes to the gather (equal sizes:
    the largest share's packed bits) and the device memory a rank needs."""
    from svsdct import batch
    H, W, n_ac = args.height, args.width, args.n_ac
    if args.total_frames > 0:        # strong scaling: one clip divided over the ranks
        shares = [batch.shard_frames(args.total_frames, world, r) for r in range(world)]
    else:                            # weak scaling: every rank runs the N = 1 batch on its own frames
        shares = [(r * args.frames, args.frames) for r in range(world)]
    per_frame_bits = batch.capacity_bits(1, H, W, n_ac)
    gather_bytes = (max(c for _, c in shares) * per_frame_bits + 7) // 8
    ranks = []
    for first, count in shares:
        cap = count * per_frame_bits
        nbytes = (cap + 7) // 8
        ranks.append({"first_frame": first, "frames": count, "first_bit": first * per_frame_bits, "capacity_bits": cap,
                      "blocks": count * (H // 8) * (W // 8),
                      # gray + stego (+ the exact-mode stego rank 0 adds after the timed region) + payload + two extract buffers
                      "device_bytes": 3 * count * H * W + nbytes + 2 * max(nbytes, gather_bytes) + 64,
                      "embed_algorithmic_bytes": 2 * count * H * W + nbytes, "extract_algorithmic_bytes": count * H * W + nbytes})
    return {"world": world, "scaling": "strong" if args.total_frames > 0 else "weak", "shares": shares,
            "per_frame_bits": per_frame_bits, "gather_bytes_per_rank": gather_bytes,
            "bytes_received_by_rank0_per_step": world * gather_bytes if world > 1 else 0,
            "total_frames": sum(c for _, c in shares), "ranks": ranks}


def launch_ranks(args) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves - one process per GPU through
    torch.distributed.run, rendezvous on 127.0.0.1 - and relay what they print (rank 0's JSON line).  Runs BEFORE this
    process imports torch or touches HIP: the parent only waits.  -> exit code of the launcher."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    if args.force_dist:
        env["SVS_BENCH_FORCE_DIST"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def _cpu_worker(task):
    """One host core: the oracle (scipy.fftpack restatement of the reference operator) on its own frames."""
    first, count, h, w, n_ac, delta = task
    from oracle import qim_dct_oracle as orc                 # checker / baseline only
    from svsdct import batch, synth
    per = batch.capacity_bits(1, h, w, n_ac)
    frames = synth.synthetic_frames(count, h, w, seed=SEED, first_frame=first)
    bits = synth.synthetic_bits(count * per, seed=SEED, first_bit=first * per)
    t0 = time.perf_counter()
    stego, _ = orc.batch_embed(frames, delta, bits, n_ac)
    got = orc.batch_extract_bits(stego, delta, n_ac)
    return time.perf_counter() - t0, int((got != bits).sum())


_C_TOKEN = None


def _strip_c_comments(text: str) -> str:
    """C / C++ source without comments and with runs of white space collapsed (string literals are kept as they are)"""
    global _C_TOKEN
    if _C_TOKEN is None:
        import re
        _C_TOKEN = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', re.S)
    out = _C_TOKEN.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", text)
    return " ".join(out.split())


def kernel_source_sha() -> str:
    """sha256 over the kernel sources (csrc/*.hpp, *.hip, include/*.h) with comments and white space removed: ties a
    committed counter capture to the code of a build (a reworded comment does not make a capture stale)"""
    import hashlib
    h = hashlib.sha256()
    for d, pat in ((os.path.join(PKG_DIR, "csrc"), (".hpp", ".hip")), (os.path.join(REPO, "include"), (".h",))):
        for name in sorted(os.listdir(d)):
            if name.endswith(pat):
                with open(os.path.join(d, name), "r", encoding="utf-8", errors="replace") as fh:
                    h.update(name.encode() + b"\0" + _strip_c_comments(fh.read()).encode())
    return h.hexdigest()


def embed_kernel_label(mode: str, n_ac: int, delta: float) -> str:
    """Which kernel svs_embed_dev launches for these arguments - the predicate of csrc/svs_capi.hip (streaming = inside the
    guard's delta range, at most two coefficient rows, not the exact mode)"""
    n = max(0, min(int(n_ac), 63))
    rows = n // 8 + 1
    streaming = delta > 0 and n > 0 and 0.25 <= delta <= 4096.0 and rows <= 2 and mode != "exact"
    if not streaming:
        return "embed_exact_kernel (lane-per-block pocketfft arithmetic)"
    if rows == 1:
        return "embed_row1_kernel (one launch: integer-domain cheap arithmetic + in-kernel exact replay of undecided blocks; capped at 4 waves per SIMD)"
    return "embed_kernel<2> (one launch: two-row cheap arithmetic + in-kernel exact replay of undecided blocks)"


def stream_digest(buf, n_bytes: int):
    """Position-sensitive digest of the first n_bytes of a uint8 tensor (any device): two wrap-around 64-bit sums over its
    64-bit words, one plain, one weighted by 2 i + 1 - so slices that change hands between ranks, or pieces that move inside a
    slice, change it.  Every rank digests what it SENT, rank 0 what it RECEIVED: the gather's exit rule, correct at every
    delta (it never looks at the payload).  -> int64 tensor [2] on the tensor's device"""
    import torch
    pad = (-n_bytes) % 8
    x = buf[:n_bytes]
    if pad:
        x = torch.cat([x, torch.zeros(pad, dtype=torch.uint8, device=buf.device)])
    w = x.contiguous().view(torch.int64)
    idx = torch.arange(w.numel(), dtype=torch.int64, device=buf.device) * 2 + 1
    return torch.stack([w.sum(), (w * idx).sum()])


DUMP_LIMIT_BYTES = 64 << 20
DUMP_SAMPLE = 4 << 20       # values kept of an output larger than this: two float32 samples stay at 32 MiB


def dump_positions(n: int, seed: int):
    """Positions of an n-value output that --dump-outputs keeps: None (all of them, in order) when n <= DUMP_SAMPLE, else
    DUMP_SAMPLE positions drawn with replacement by numpy's default_rng(seed), sorted - the same for the same n in every run"""
    import numpy as np
    if n <= DUMP_SAMPLE:
        return None
    return np.sort(np.random.default_rng(seed).integers(0, n, DUMP_SAMPLE, dtype=np.int64))


def dump_outputs(out_dir, stego, packed, counts, frame_sse):
    """--dump-outputs: what the last timed step returned to its caller, as float32 / float64 .npy files in out_dir.
      stego.npy            stego pixels (the embed's output): [F, H, W], or the dump_positions(F*H*W, SEED) sample of the
                           flattened batch when it is larger than DUMP_SAMPLE pixels
      extracted.npy        the packed extracted bit stream, one value per byte (MSB-first bits, the extract's output; on rank 0
                           of a multi-rank run the gathered slices of every rank, each trimmed to its own bytes), or the
                           dump_positions(n_bytes, SEED + 1) sample of it
      stego_frame_sse.npy  float64 [F]: per-frame sum of squared differences between stego and cover over EVERY pixel
      counts.npy           float64 [bits embedded, bits extracted, payload bit errors over the whole stream]
    stego: uint8 device tensor [F, H, W]; packed: uint8 host array; counts: three ints; frame_sse: int64 tensor [F]"""
    import numpy as np
    import torch
    idx = dump_positions(stego.numel(), SEED)
    if idx is None:
        pixels = stego.cpu().numpy()
    else:
        pixels = stego.view(-1)[torch.from_numpy(idx).to(stego.device)].cpu().numpy()
    idx = dump_positions(packed.size, SEED + 1)
    arrays = {"stego": pixels.astype(np.float32),
              "extracted": (packed if idx is None else packed[idx]).astype(np.float32),
              "stego_frame_sse": frame_sse.cpu().numpy().astype(np.float64),
              "counts": np.asarray(counts, dtype=np.float64)}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def round_trip_verdict(parity_sample, bit_errors, delta, n_ac, gather_ok=None):
    """Exit rule of the bench (-> error text, or None when the run is good).  The round trip is WRONG when it loses payload
    bits the reference itself would not lose.  The reference is not error-free everywhere (delta = 4: 1.6 % BER on any input,
    SURVEY N5; many coefficients with clipping pixels), so the rule is parity with the oracle on the sample both ran - not
    "zero" (VERDICT r03 weak #9).  Without a CPU sample (--cpu-frames 0, N > 1) only a provably error-free setting can fail:
    the synthetic frames stay inside [16, 240) and 3 * 1.5 * delta * 0.1734 <= 12.5 for delta <= 16, so with n_ac <= 7 nothing
    clips and delta >= 8 cannot lose a bit.
    gather_ok (N > 1 / --force-dist): False when a slice rank 0 received differs from what its sender sent - fatal at every
    delta; the concatenation IS the path's output (extract_process.py:76,181)."""
    if gather_ok is False:
        return "the gathered bit stream on rank 0 differs from what the ranks sent (wrong slice, wrong order or damaged)"
    if parity_sample is not None:
        if parity_sample["gpu_round_trip_bit_errors_on_sample"] != parity_sample["oracle_round_trip_bit_errors_on_sample"]:
            return "payload bit errors in the round trip differ from the oracle's on the same frames"
        if parity_sample["gpu_extract_of_reference_stego_bit_mismatches"] != 0:
            return "bits extracted from the oracle's stego frames differ from the oracle's"
        return None
    if bit_errors != 0 and 8 <= delta <= 16 and n_ac <= 7:
        return "payload bit errors in the round trip"
    return None


def pmc_traffic_check(args):
    """--pmc-check: HBM bytes per embed launch of this workload from two FRESH child processes (never a re-exec of a process
    that has initialised the GPU; the program stands directly after `--`), one counter per pass as MI355X_MICROARCH.md
    prescribes: FETCH_SIZE (KiB; on gfx950 half the bytes of a coalesced stream - the factor is calibrated in the same pass
    on frame_sse_kernel's known 2 F H W bytes) and WRITE_SIZE (KiB; calibrated on fill_synthetic_kernel's F H W).
    -> (bytes per embed launch, description) or (None, why not)"""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 is not on PATH"
    px = args.frames * args.height * args.width
    work = ["--steps", "2", "--warmup", "1", "--cpu-frames", "0", "--frames", str(args.frames), "--height", str(args.height),
            "--width", str(args.width), "--n-ac", str(args.n_ac), "--delta", repr(args.delta)] + (["--mode", args.mode] if args.mode else [])
    means = {}
    tmp = tempfile.mkdtemp(prefix="svs_pmc_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, counter)
            env = dict(os.environ, TMPDIR=os.environ.get("TMPDIR", "/tmp"))
            res = subprocess.run([exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", out, "--",
                                  sys.executable, os.path.abspath(__file__)] + work, env=env, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                return None, f"rocprofv3 --pmc {counter} pass failed (exit {res.returncode})"
            acc = {}
            for path in glob.glob(os.path.join(out, "**", "*_counter_collection.csv"), recursive=True):
                with open(path) as fh:
                    for r in csv.DictReader(fh):
                        if r["Counter_Name"] == counter:
                            k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("svs::", "").split("<")[0]
                            acc.setdefault(k, []).append(float(r["Counter_Value"]))
            means[counter] = {k: sum(v) / len(v) for k, v in acc.items()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fetch, write = means["FETCH_SIZE"], means["WRITE_SIZE"]
    embed = next((k for k in ("embed_row1_kernel", "embed_kernel", "embed_exact_kernel") if k in fetch and k in write), None)
    if embed is None or "frame_sse_kernel" not in fetch or "fill_synthetic_kernel" not in write:
        return None, "the counter passes did not see the kernels they calibrate on"
    fetch_scale = 2 * px / (fetch["frame_sse_kernel"] * 1024)          # 2.0 on gfx950 (guide: FETCH_SIZE counts half)
    write_scale = px / (write["fill_synthetic_kernel"] * 1024)         # 1.0
    traffic = fetch[embed] * 1024 * fetch_scale + write[embed] * 1024 * write_scale
    return traffic, (f"measured in this run: two child passes `rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE --kernel-trace -- python bench.py "
                     f"--steps 2 ...` of this workload; {embed}; FETCH_SIZE x {fetch_scale:.4f} (calibrated on frame_sse_kernel), "
                     f"WRITE_SIZE x {write_scale:.4f} (fill_synthetic_kernel)")


def usable_cpus() -> int:
    """CPUs this process may actually use: scheduler affinity, further limited by a cgroup CPU quota if one is set
    (a GPU box hands each job a share of the host, not the 256 logical cores os.cpu_count() reports)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as fh:
                parts = fh.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(int(parts[0]) / int(parts[1]))))
            else:
                quota = int(parts[0])
                if quota > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
                        n = min(n, max(1, quota // int(fh.read())))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def cpu_baseline_all_cores(args):
    """BASELINE.md plan (b): one worker per core over frames.  Runs in worker processes forked BEFORE anything
    touches the GPU.  -> dict for the JSON line."""
    import multiprocessing as mp
    workers = max(1, min(usable_cpus(), 32, args.cpu_frames))
    per_worker = max(1, args.cpu_frames // workers)
    delta = args.delta if args.delta != int(args.delta) else int(args.delta)
    tasks = [(i * per_worker, per_worker, args.height, args.width, args.n_ac, delta) for i in range(workers)]
    with mp.get_context("fork").Pool(workers) as pool:
        out = pool.map(_cpu_worker, tasks)
    slowest = max(t for t, _ in out)
    frames = workers * per_worker
    return {"value": frames * args.height * args.width / slowest / 1e6, "unit": "Mpix/s", "cores": workers, "kind": "port",
            "payload_bit_errors": sum(e for _, e in out),
            "sample": f"{frames} frames of the workload ({per_worker} per worker, {workers} worker processes; the job may use "
                      f"{usable_cpus()} of the host's {os.cpu_count()} logical CPUs), embed + extract with the vectorised scipy.fftpack restatement "
                      f"(oracle/qim_dct_oracle.py); slowest worker {slowest:.2f} s"}


def main():
    args = parse_args()
    if "RANK" not in os.environ and (args.gpus > 1 or args.force_dist):
        # a profiler's preloaded library has initialised the GPU before this process started; starting the ranks from such
        # a process is the exec-after-GPU-init hop the pool forbids.  Counter passes are single-rank (tools/gpu_pmc.sh).
        if os.environ.get("ROCP_TOOL_LIBRARIES") or "rocprof" in os.environ.get("LD_PRELOAD", ""):
            raise SystemExit("bench.py: refusing to start ranks from a process running under rocprofv3; profile one rank "
                             "(python bench.py, no --gpus / --force-dist) or launch the ranks with torch.distributed.run "
                             "under the profiler yourself")
        raise SystemExit(launch_ranks(args))             # parent of the ranks: never initialises the GPU
    pmc_live = None
    if args.pmc_check and int(os.environ.get("WORLD_SIZE", "1")) == 1 and "RANK" not in os.environ:
        pmc_live = pmc_traffic_check(args)                   # child processes, before the first HIP call of this one
    cpu_parallel = None
    if args.cpu_frames > 0 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        cpu_parallel = cpu_baseline_all_cores(args)          # before the first HIP call of this process
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run")
    # launched by torch.distributed.run (RANK set): take the collective path even with one rank, so a
    # 1-GPU box can exercise the RCCL calls; plain `python bench.py` is the N = 1 line without a process group
    use_dist = world > 1 or ((args.force_dist or os.environ.get("SVS_BENCH_FORCE_DIST") == "1") and "RANK" in os.environ)
    if args.rehearse_gloo:
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.rehearse_gloo:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)     # "nccl" is RCCL on ROCm
    cdev = torch.device("cpu") if args.rehearse_gloo else dev     # where collective buffers live

    import ctypes as C

    from svsdct import batch, native
    from svsdct import dist as sdist
    from svsdct.native import Planes
    lib = native.load()                      # raises if the HIP library is missing - no fallback
    native.ensure_device(local_rank)

    H, W, n_ac, delta = args.height, args.width, args.n_ac, args.delta
    plan = job_plan(args, world)
    first_frame, F = plan["shares"][rank]
    if F == 0:
        raise SystemExit(f"--total-frames {args.total_frames} leaves rank {rank} of {world} without frames")
    mode = batch.resolve_mode(args.mode)     # unspecified = svsdct.batch.DEFAULT_MODE, what the drop-in operator and video loops run
    planes = Planes.contiguous(F, H, W)
    cap = batch.capacity_bits(F, H, W, n_ac)
    nbytes = (cap + 7) // 8
    stream = torch.cuda.current_stream().cuda_stream

    gray = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    stego = torch.empty_like(gray)
    payload = torch.zeros(nbytes + 8 - nbytes % 4, dtype=torch.uint8, device=dev)
    per_frame_bits = plan["per_frame_bits"]
    first_bit = plan["ranks"][rank]["first_bit"]             # this rank's offset in the job's bit stream
    # dist.gather wants equal sizes: every rank contributes the packed bits of the LARGEST share (ranks differ by at most one
    # frame under --total-frames; the tail of a smaller share is padding the check below ignores)
    shares = plan["shares"]
    gather_bytes = plan["gather_bytes_per_rank"]
    # extracted bits are double-buffered so that the gather of step k overlaps the kernels of step k+1
    ext_len = max(nbytes, gather_bytes)
    ext_bufs = [torch.zeros(ext_len + 8 - ext_len % 4, dtype=torch.uint8, device=dev) for _ in range(2 if use_dist else 1)]
    native.check(lib.svs_fill_synthetic_dev(gray.data_ptr(), C.byref(planes), SEED, first_frame, 16, 224, stream),
                 "fill_synthetic")
    native.check(lib.svs_fill_bits_dev(payload.data_ptr(), cap, SEED, first_bit, stream), "fill_bits")
    gathered = [None, None]
    if use_dist and rank == 0:
        gathered = [[torch.empty(gather_bytes, dtype=torch.uint8, device=cdev) for _ in range(world)] for _ in range(2)]
    pending = [None, None]
    torch.cuda.synchronize()
    step_no = [0]
    gather_wait = [0.0]       # host seconds this rank spent blocked on a gather's completion

    def step(ev=None):
        slot = step_no[0] % len(ext_bufs)
        step_no[0] += 1
        extracted = ext_bufs[slot]
        if ev:
            ev[0].record()
        used = batch.embed_device(gray.data_ptr(), stego.data_ptr(), planes, delta, n_ac, payload.data_ptr(), 0, cap,
                                  stream, mode=mode)
        if ev:
            ev[1].record()
        if pending[slot] is not None:
            tw = time.perf_counter()
            pending[slot].wait()          # the gather that last read this buffer must have finished
            gather_wait[0] += time.perf_counter() - tw
            pending[slot] = None
        got = batch.extract_device(stego.data_ptr(), planes, delta, n_ac, extracted.data_ptr(), extracted.numel(),
                                   stream, mode=mode)
        if ev:
            ev[2].record()
        if use_dist:
            # the path's one collective (RCCL over xGMI): packed bits of every rank to rank 0, in rank order;
            # asynchronous, so it runs beside the next step's kernels
            if args.rehearse_gloo:
                sdist.gather_packed(extracted.cpu(), gather_bytes, dst=0, recv=gathered[slot])
            else:
                pending[slot] = dist.gather(extracted[:gather_bytes], gathered[slot] if rank == 0 else None, dst=0,
                                            async_op=True)
        return used, got

    def drain():
        for i, w in enumerate(pending):
            if w is not None:
                tw = time.perf_counter()
                w.wait()
                gather_wait[0] += time.perf_counter() - tw
                pending[i] = None

    used = got = cap
    for _ in range(args.warmup):
        used, got = step()
    drain()
    assert (used, got) == (cap, cap)

    events = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    gather_wait[0] = 0.0
    t0 = time.perf_counter()
    for k in range(args.steps):
        used, got = step(events[k])
    drain()                                  # every gather of the timed steps has completed
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    embed_ms = sum(e[0].elapsed_time(e[1]) for e in events) / args.steps
    extract_ms = sum(e[1].elapsed_time(e[2]) for e in events) / args.steps
    per_rank = [[embed_ms, extract_ms, gather_wait[0] / args.steps * 1e3]]
    if use_dist:        # every rank's kernel times on rank 0: the SCALE record can show imbalance between GPUs
        mine = torch.tensor(per_rank[0], dtype=torch.float64, device=cdev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [[float(x) for x in t.tolist()] for t in allr]

    # ---- correctness of what was just timed (outside the timed region) -------------------------
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    last = (step_no[0] - 1) % len(ext_bufs)
    extracted = ext_bufs[last]
    native.check(lib.svs_bit_errors_dev(extracted.data_ptr(), payload.data_ptr(), cap, cnt.data_ptr(), stream), "ber")
    sse = torch.zeros(F, dtype=torch.int64, device=dev)
    native.check(lib.svs_frame_sse_dev(gray.data_ptr(), stego.data_ptr(), C.byref(planes), sse.data_ptr(), stream),
                 "sse")
    torch.cuda.synchronize()
    bit_errors = int(cnt.item())
    if args.dump_outputs and rank == 0:      # before the exact-mode leg below reuses the extract buffer
        if use_dist:
            packed = torch.cat([gathered[last][r][: (c * per_frame_bits + 7) // 8].cpu() for r, (_, c) in enumerate(shares)])
        else:
            packed = extracted[:nbytes].cpu()
        dump_outputs(args.dump_outputs, stego, packed.numpy(), (used, got, bit_errors), sse)
    gpu_sample_packed = None
    if rank == 0 and world == 1 and args.cpu_frames > 0:     # the timed extract's bits of the frames the oracle will redo below
        gpu_sample_packed = extracted[: (min(args.cpu_frames, F) * (cap // F) + 7) // 8].clone()
    if use_dist:
        t = torch.tensor([bit_errors], dtype=torch.int64, device=cdev)
        dist.all_reduce(t)
        bit_errors = int(t.item())
    import math
    sse0 = int(sse[0].item())
    psnr0 = float("inf") if sse0 == 0 else 10 * math.log10(255.0 ** 2 * H * W / sse0)
    gather_ok = gather_matches_payload = None
    if use_dist:
        # the collective's exit rule: every rank digests the slice it SENT in the last step, the digests are
        # all-gathered, rank 0 digests every slice it RECEIVED and compares it with its sender's - independent of delta and of
        # the payload (at delta = 4 the reference itself loses 1.67 % of the bits; a correct gather must still pass)
        sent = stream_digest(extracted.cpu() if args.rehearse_gloo else extracted, gather_bytes).to(cdev)
        all_sent = [torch.zeros_like(sent) for _ in range(world)]
        dist.all_gather(all_sent, sent)
        if rank == 0:
            slices = list(gathered[last])
            if args.inject_gather_swap and world > 1:
                slices[0], slices[1] = slices[1], slices[0]
            gather_ok = all(bool(torch.equal(stream_digest(slices[r], gather_bytes).cpu(), all_sent[r].cpu())) for r in range(world))
            # beside it, where it must hold (round_trip_verdict: 8 <= delta <= 16, n_ac <= 7): slice r is rank r's payload,
            # regenerated here from the counter-based generator - report only, the bit-error count above is the exit rule
            expect = torch.zeros(gather_bytes + 8 - gather_bytes % 4, dtype=torch.uint8, device=dev)
            padded = torch.zeros_like(expect)
            wrong = 0
            for r, (first_r, count_r) in enumerate(shares):
                bits_r = count_r * per_frame_bits
                native.check(lib.svs_fill_bits_dev(expect.data_ptr(), bits_r, SEED, first_r * per_frame_bits, stream), "fill_bits")
                padded[:gather_bytes] = slices[r].to(dev)
                native.check(lib.svs_bit_errors_dev(padded.data_ptr(), expect.data_ptr(), bits_r, cnt.data_ptr(), stream), "ber")
                torch.cuda.synchronize()
                wrong += int(cnt.item())
            gather_matches_payload = bool(wrong == 0)

    result = None
    if rank == 0:
        pixels_per_step = sum(c for _, c in shares) * H * W
        mpix_s = pixels_per_step * args.steps / elapsed / 1e6
        embed_bytes = F * H * W * 2 + nbytes            # read u8 + write u8 + packed payload
        extract_bytes = F * H * W + nbytes
        achieved = embed_bytes / (embed_ms * 1e-3) / 1e9
        # HBM bytes per embed launch from the PMC counters: NOT measured in this run (counters need their own rocprofv3
        # --pmc passes, tools/gpu_pmc.sh); taken from the committed summary of those passes when it is for this workload
        traffic, traffic_source = None, None
        tpath = os.path.join(REPO, "profiles", "hbm_traffic.json")
        if os.path.exists(tpath):
            try:
                with open(tpath) as fh:
                    tj = json.load(fh)
                same_workload = (tj.get("frames") == F and tj.get("height") == H and tj.get("width") == W and
                                 tj.get("n_ac", 3) == n_ac)
                same_kernels = tj.get("kernel_source_sha256") == kernel_source_sha()
                if same_workload and same_kernels:
                    traffic = tj.get("embed_bytes_per_launch")
                    traffic_source = {"file": "profiles/hbm_traffic.json", "captured": tj.get("captured"),
                                      "how": "rocprofv3 --pmc passes of this bench command (tools/gpu_pmc.sh), "
                                             "2 x FETCH_SIZE + WRITE_SIZE per embed launch; not measured in this run; the "
                                             "capture's kernel sources (sha256 of csrc/ + include/) are this build's"}
                elif same_workload:
                    traffic_source = {"file": "profiles/hbm_traffic.json", "captured": tj.get("captured"),
                                      "how": "STALE: captured from other kernel sources than this build's - traffic "
                                             "reported as null; re-run tools/gpu_pmc.sh + tools/pmc_summary.py"}
            except Exception:
                traffic, traffic_source = None, None
        if pmc_live is not None:                 # --pmc-check: this run's own counter passes replace the committed capture
            if pmc_live[0] is not None:
                traffic, traffic_source = pmc_live[0], {"how": pmc_live[1]}
            else:
                traffic_source = dict(traffic_source or {}, pmc_check_failed=pmc_live[1])
        result = {
            "metric": "Mpixels/sec embed+extract round-trip at 4K; payload bit-error rate (must be 0)",
            "value": mpix_s, "unit": "Mpix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong" if args.total_frames > 0 else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic" + (" (gloo rehearsal - not a result)" if args.rehearse_gloo else ""),
            "config": {"workload": (f"{W}x{H} x {args.total_frames} frames divided over {world} GPU(s)" if args.total_frames > 0
                                    else f"{W}x{H} x {F} frames per GPU") +
                                   f", {n_ac} AC coeffs/block, delta={delta:g}, full-capacity payload "
                                   f"({per_frame_bits} bits per frame), gray planes resident in HBM",
                       "frames_per_gpu": [c for _, c in shares] if args.total_frames > 0 else F,
                       "total_frames": sum(c for _, c in shares), "height": H, "width": W, "n_ac": n_ac, "delta": delta,
                       "mode": mode + (" (n_ac <= 15: the same launch as guarded - stego pixels bit-identical to the reference)"
                                       if mode == "fast" and n_ac <= 15 else ""),
                       "sharding": "frames" if world > 1 else "none",
                       "collective": ("gloo gather of packed bits through host memory (rehearsal)" if args.rehearse_gloo else
                                      "rccl gather of packed bits") if use_dist else "none"},
            "payload_bit_errors": bit_errors, "payload_ber": bit_errors / (sum(c for _, c in shares) * per_frame_bits),
            "psnr_frame0_db": psnr0,
            "kernel_ms": {"embed": embed_ms, "extract": extract_ms,
                          "per_rank": {"embed_min": min(r[0] for r in per_rank), "embed_max": max(r[0] for r in per_rank),
                                       "extract_min": min(r[1] for r in per_rank), "extract_max": max(r[1] for r in per_rank),
                                       "embed": [r[0] for r in per_rank], "extract": [r[1] for r in per_rank]}},
            "gather": ({"bytes_received_by_rank0_per_step": world * gather_bytes,
                        "host_wait_ms_per_step_rank0": per_rank[0][2],
                        "host_wait_ms_per_step_max_over_ranks": max(r[2] for r in per_rank),
                        "note": "asynchronous: the gather of step k runs beside the kernels of step k + 1; the wait is what "
                                "is left when its buffer is needed again (and at the end of the timed region)"}
                       if use_dist else None),
            "roofline": {"bound": "hbm", "kernel": embed_kernel_label(mode, n_ac, delta),
                         "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                         "algorithmic_bytes_per_launch": embed_bytes,
                         "extract_achieved": extract_bytes / (extract_ms * 1e-3) / 1e9,
                         # every rank's own embed launch against ITS algorithmic bytes (shares differ by at most one frame)
                         "per_rank": [{"rank": r, "frames": plan["ranks"][r]["frames"],
                                       "achieved": plan["ranks"][r]["embed_algorithmic_bytes"] / (per_rank[r][0] * 1e-3) / 1e9,
                                       "frac": plan["ranks"][r]["embed_algorithmic_bytes"] / (per_rank[r][0] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                       "extract_achieved": plan["ranks"][r]["extract_algorithmic_bytes"] / (per_rank[r][1] * 1e-3) / 1e9}
                                      for r in range(world)]},
        }
        if gather_ok is not None:
            result["gather_ok"] = gather_ok      # every slice rank 0 received has its sender's digest (fatal when false)
            result["gather_matches_payload"] = gather_matches_payload   # ... and is that rank's payload (must hold only where the
                                                                        # reference itself is error-free: 8 <= delta <= 16, n_ac <= 7)

    # ---- EXACT mode (pocketfft-identical arithmetic) timed on the same batch, reported beside the headline ------
    if rank == 0:
        ex_ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(3)]
        stego_x = torch.empty_like(gray)
        for e in ex_ev:
            e[0].record()
            batch.embed_device(gray.data_ptr(), stego_x.data_ptr(), planes, delta, n_ac, payload.data_ptr(), 0, cap,
                               stream, mode="exact")
            e[1].record()
            batch.extract_device(stego_x.data_ptr(), planes, delta, n_ac, extracted.data_ptr(), extracted.numel(),
                                 stream, mode="exact")
            e[2].record()
        native.check(lib.svs_bit_errors_dev(extracted.data_ptr(), payload.data_ptr(), cap, cnt.data_ptr(), stream), "ber")
        torch.cuda.synchronize()
        xe = min(e[0].elapsed_time(e[1]) for e in ex_ev)
        xx = min(e[1].elapsed_time(e[2]) for e in ex_ev)
        result["exact_mode"] = {"embed_ms": xe, "extract_ms": xx, "embed_GBps": embed_bytes / xe / 1e6,
                                "extract_GBps": extract_bytes / xx / 1e6,
                                "round_trip_Mpix_s": F * H * W / (xe + xx) / 1e3, "payload_bit_errors": int(cnt.item()),
                                "note": "bit-identical to the reference (stego pixels included); VALU-bound"}
        if world == 1 and args.cpu_frames > 0:
            result["exact_mode"]["_stego"] = stego_x[: min(args.cpu_frames, F)].cpu().numpy()
        del stego_x

    # ---- CPU baseline: the oracle on a bounded sample of the same frames (rank 0, N = 1 only) ----
    if rank == 0 and world == 1 and args.cpu_frames > 0:
        import numpy as np

        from oracle import qim_dct_oracle as orc            # checker / baseline only
        m = min(args.cpu_frames, F)
        sample = gray[:m].cpu().numpy()
        per = cap // F
        bits = np.unpackbits(payload[: (m * per + 7) // 8].cpu().numpy(), count=m * per)
        t0 = time.perf_counter()
        ref_stego, used = orc.batch_embed(sample, delta if delta != int(delta) else int(delta), bits, n_ac)
        t_embed = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref_bits = orc.batch_extract_bits(ref_stego, delta if delta != int(delta) else int(delta), n_ac)
        t_extract = time.perf_counter() - t0
        cpu_mpix = m * H * W / (t_embed + t_extract) / 1e6
        gpu_stego = stego[:m].cpu().numpy()
        psnr_ref = orc.psnr_u8(sample[0], ref_stego[0])
        result["cpu_baseline"] = cpu_parallel or {}
        result["cpu_baseline_single_thread"] = {
            "value": cpu_mpix, "unit": "Mpix/s", "cores": 1, "kind": "port",
            "sample": f"{m} of the {F} frames, embed {t_embed:.2f} s + extract {t_extract:.2f} s, vectorised "
                      f"scipy.fftpack restatement (oracle/qim_dct_oracle.py), 1 thread"}
        # context: the reference's own structure - a Python loop over blocks with four SciPy calls per
        # block - restated literally (oracle.frame_operator_loops), on a 240 x 320 crop of frame 0
        crop = np.ascontiguousarray(sample[0][:240, :320])
        cbits = bits[: (240 // 8) * (320 // 8) * min(n_ac, 63)]
        t0 = time.perf_counter()
        _, loop_stego, _ = orc.frame_operator_loops(crop, "embed", delta if delta != int(delta) else int(delta),
                                                    orc.bits_to_str(cbits), n_ac)
        orc.frame_operator_loops(loop_stego, "extract", delta if delta != int(delta) else int(delta), None, n_ac)
        t_loop = time.perf_counter() - t0
        result["cpu_literal_block_loop"] = {
            "value": crop.size / t_loop / 1e6, "unit": "Mpix/s", "cores": 1, "kind": "port",
            "sample": f"one 320x240 crop, embed + extract in {t_loop:.2f} s: per-block Python loop with scipy.fftpack calls, "
                      f"the shape of the reference's own code (context only)"}
        # the other direction: the GPU (the timed mode) reading the ORACLE's stego frames must give the oracle's bits
        ref_dev = torch.from_numpy(ref_stego).to(dev)
        planes_m = Planes.contiguous(m, H, W)
        batch.extract_device(ref_dev.data_ptr(), planes_m, delta, n_ac, extracted.data_ptr(), extracted.numel(), stream,
                             mode=mode)
        torch.cuda.synchronize()
        got_bits = np.unpackbits(extracted[: (m * per + 7) // 8].cpu().numpy(), count=m * per)
        gpu_sample_bits = np.unpackbits(gpu_sample_packed.cpu().numpy(), count=m * per)   # what the timed extract returned
        result["parity_sample"] = {
            "frames": m,
            "gpu_round_trip_bit_errors_on_sample": int((gpu_sample_bits != bits).sum()),
            "oracle_round_trip_bit_errors_on_sample": int((ref_bits != bits).sum()),
            "gpu_extract_of_reference_stego_bit_mismatches": int((got_bits != ref_bits).sum()),
            "bits_compared": int(m * per),
            "oracle_extract_of_gpu_stego_equals_payload": bool(np.array_equal(
                orc.batch_extract_bits(gpu_stego[:1], delta if delta != int(delta) else int(delta), n_ac), bits[:per])),
            "psnr_frame0_reference_db": psnr_ref, "psnr_frame0_delta_db": abs(psnr_ref - psnr0),
            "pixels_differing_from_reference": int((gpu_stego != ref_stego).sum()), "pixels": int(gpu_stego.size),
            "exact_mode_pixels_differing_from_reference": int((result["exact_mode"].pop("_stego") != ref_stego).sum())}

    if rank == 0:
        result.get("exact_mode", {}).pop("_stego", None)
        print(json.dumps(result))
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and result is not None:
        verdict = round_trip_verdict(result.get("parity_sample"), bit_errors, delta, n_ac, result.get("gather_ok"))
        if verdict:
            raise SystemExit(verdict)


if __name__ == "__main__":
    main()
