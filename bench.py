#!/usr/bin/env python3
"""bench.py — Mpix/s of the gfwarp hot path on N MI355X (one process per GPU).

    python bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over one synthetic frame: all planes of a 4K (3840x2160) u16 4:2:2 frame
(BASELINE.json configs[1], "C2": planar YUV422P16LE = 3 x Luma16, GoPro-style opencv_fisheye lens, per-row
rolling-shutter matrices) warped through libgfwarp's C ABI from buffers already resident in HBM.  The steps go to the
library the way a render loop hands it a clip: `gfw_undistort_clip` calls of `--clip` frames each (default 8; exactly K
frames are warped in the timed region), served by the context's run-time specialised kernel (GFW_OPT_JIT = 2: built
during the warm-up, `config.jit` reports the build) in launches of up to 8 frames.

Process model.  Started plainly, this file is a *launcher*: it spawns one worker process per GPU (RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* in the environment, rendezvous on 127.0.0.1), relays rank 0's JSON line and exits with the
workers' status; a worker set that dies abnormally fails the run (exit status != 0, no JSON line) unless `--retry` asks
for up to two more attempts, which the line then reports under `launcher`.  Started by `torch.distributed.run` (RANK already in the environment) it is a worker itself.  N >= 2 ranks
talk over RCCL (`nccl` backend); frames shard across ranks and no pixel ever crosses GPUs — the only collectives are a
broadcast of the clip-invariant block, a barrier either side of the timed region, a MAX of the elapsed time and an
all-gather of output checksums.

Modes: default = weak scaling (every rank warps its own K frames of C2); `--c5` = BASELINE.json configs[4]: a
10 000-frame clip whose frames are dealt round-robin to the ranks (strong scaling), each frame's per-row matrices built
on the device from the clip's quaternion tracks, a 64-bit checksum per frame — taken by the warp kernel where the pixels
leave (gfw_set_frame_checksums; `--sum-pass`: a gfw_checksum64 pass over each destination instead) — all-gathered at the end.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and reports the headline (`value` in Mpix/s,
`ms_per_step`, the workload in `config`); `--dump-outputs DIR` also writes what the last timed step computed (dump_outputs).
`--full` adds what takes time of its own beyond that:
  roofline     — algorithmic HBM bytes/launch (sum over planes of w*h*bpp read + written) over the
                 kernel's mean launch duration, measured with hipEvents on the launch stream (GFW_OPT_PROFILE) during
                 the timed region, against the 8 TB/s HBM3E peak;
  cpu_baseline — the oracle (C restatement of the reference CPU path, OpenMP over the host cores) timed on the same
                 frames, rank 0 at N=1 only;
  config.parity_vs_oracle — outputs of the LAST frames of the timed region itself, compared with the oracle.
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FMT, WIDTH, HEIGHT = "YUV422P16LE", 3840, 2160
N_RESIDENT = 64                  # distinct source frames + per-row matrix tables resident in HBM, cycled by the steps
                                 # (SURVEY.md 8d "64 distinct resident source frames cycled": 2.1 GB, far beyond L2 + MALL)
CLIP_FRAMES = 16                 # most frames gfw_undistort_clip puts into one launch (GFW_CLIP_FRAMES_MAX)
N_DST = 8                        # destination frame sets written round-robin (the frames of one clip launch are in flight together: one set each)
N_CHECK = 3                      # frames of the timed region compared with the oracle afterwards (--full)
DUMP_BUDGET_BYTES = 48 << 20     # --dump-outputs writes at most this much in all (C2's three planes as float32 are 66 MB: sampled)
TRAFFIC_FILE = os.path.join("profiles", "r06_c2_traffic.json")       # rocprofv3 PMC passes of the C2 workload; names the kernel source it was taken on (abi.kernel_source_id)


# coefficient sets of the other physical lens models (the ones tests/test_gpu_lens_models.py runs), for --lens-model
LENS_MODEL_K = {
    "opencv_standard": [0.12, -0.05, 0.001, 0.002, 0.01, 0.02, -0.01, 0.001, 0.0005, -0.0002, 0.0003, 0.0001],
    "poly3": [0.06], "poly5": [0.08, -0.02], "ptlens": [0.01, -0.03, 0.02], "insta360": [0.05, -0.01, 0.002, 0.001, -0.001, 0.6],
    "sony": [1.0, 0.01, -0.05, 0.02, 0.003, -0.001], "generic_polynomial": [1.0, 0.01, -0.05, 0.02, 0.003, -0.001, 0.0005, 0.0, 0.0, 0.0, 0.0, 0.0],
    "gopro": [0.0, 1.0, 0.01, -0.12, 0.02, 0.01, -0.004],
}


def parse_args(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: the roofline (hipEvent brackets in the timed region, --profile-every), the oracle's parity verdict on "
                         "the timed frames, the reference kernel's fixture through the timed call path, and the CPU baseline; a plain run does none of these")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last step computed (every destination plane of its frame, as float32) to DIR/<name>.npy; "
                         "planes beyond the size budget are replaced by a fixed, seeded sample of their pixels")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N >= 2 (nccl = RCCL; gloo for the 1-GPU test of the N-rank path)")
    ap.add_argument("--same-device", action="store_true", help="every rank uses cuda:0 (testing the N-rank path on a 1-GPU box; with --backend gloo)")
    ap.add_argument("--retry", action="store_true", help="launcher: re-run a worker set that died abnormally (GPU fault, signal) up to twice; "
                                                        "by default such a death fails the run")
    ap.add_argument("--no-retry", action="store_true", help=argparse.SUPPRESS)      # the default since round 3
    ap.add_argument("--jit", type=int, default=2, choices=(0, 1, 2),
                    help="GFW_OPT_JIT of the contexts: 2 (default) the per-clip specialised kernel is built during the warm-up; 0 ahead-of-time kernels only")
    ap.add_argument("--clip", type=int, default=0,
                    help="frames per gfw_undistort_clip call (resident-matrices workloads); 1 = one gfw_undistort_frame call per frame; 0 (default) = the largest "
                         "count from 16 down to 8 that divides --steps, so that the timed region has no runt launch (20 steps leave as 10 + 10, not 8 + 8 + 4: "
                         "round-5 verdict, weak #8), else 8")
    ap.add_argument("--preheat-ms", type=float, default=60.0,
                    help="untimed launches of the same workload for this long right before the timed region (declared in config.preheat_ms): "
                         "a 20-step region lasts 1.5 ms, shorter than the clock governor's ramp")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the oracle comparison of the last timed frames")
    ap.add_argument("--width", type=int, default=WIDTH)
    ap.add_argument("--height", type=int, default=HEIGHT)
    ap.add_argument("--fmt", default=FMT)
    ap.add_argument("--fov", type=float, default=1.0)
    ap.add_argument("--interp", type=int, default=2, help="2 bilinear (north-star), 4 bicubic, 8 Lanczos4 (the reference's render default, cli.rs:618)")
    ap.add_argument("--crop", action="store_true", help="C4: adaptive-zoom crop (fov 0.82 + non-zero translation2d)")
    ap.add_argument("--resident", type=int, default=N_RESIDENT, help="distinct source frames / matrix tables kept in HBM and cycled")
    ap.add_argument("--c1", action="store_true", help="C1: 1920x1080 NV12 (u8), one constant quaternion, matrix_count = 1 "
                                                      "(BASELINE.json configs[0], the reference's own CPU-runnable case)")
    ap.add_argument("--c5", action="store_true", help="C5: a --frames long 4K clip dealt round-robin to the ranks (strong scaling); per-row "
                                                      "matrices built on the device per frame; per-frame checksums all-gathered")
    ap.add_argument("--frames", type=int, default=10000, help="--c5: frames in the clip")
    ap.add_argument("--sum-pass", action="store_true",
                    help="--c5: take each frame's checksum with a gfw_checksum64 pass over its destination buffer (33 MB read back per C2 frame) instead of where the pixels "
                         "leave (gfw_set_frame_checksums, the default: the specialised kernel adds what it stores, no second pass)")
    ap.add_argument("--sum-stream", type=int, default=0, choices=(0, 1),
                    help="--c5: 0 (default) the per-frame checksums in order on the warp's stream; 1: on a stream of their own, beside the warp of the next launch (two groups of "
                         "destination sets ordered by events, one wave slot per SIMD left free for them) — built in round 5 to take the verification off the critical path and "
                         "measured SLOWER: 70.2 against 53.3 us per frame (the 66 MB reads of eight checksums beside a launch slow its warp from 42 to 50 us per frame and "
                         "the event chain serialises the rest: profiles/r05_bench_c5.txt)")
    ap.add_argument("--host-buffers", action="store_true",
                    help="PCIe-inclusive run: source and destination planes live in host memory (BufferSource::Cpu), every "
                         "call stages H2D, warps, copies D2H and synchronises — never the headline value")
    ap.add_argument("--profile-every", type=int, default=None,
                    help="bracket every N-th launch of the timed region with hipEvents for the roofline's kernel duration "
                         "(0 = none; default 8 with --full, else 0); the event pairs themselves cost GPU time between back-to-back kernels")
    ap.add_argument("--digital", default="", help="digital lens on top of the physical one (gopro_superview, gopro_hyperview, ...)")
    ap.add_argument("--lens-model", default="", help="physical lens model instead of opencv_fisheye (opencv_standard, poly3, poly5, ptlens, insta360, "
                                                     "sony, generic_polynomial, gopro): the fused kernel's generic-model body")
    ap.add_argument("--lca", type=float, default=1.0, help="lens_correction_amount (< 1: the blend of cpu_undistort.rs:429-460)")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--grid", type=int, default=0)
    ap.add_argument("--streams", type=int, default=1, choices=(1, 2, 4),
                    help="contexts (each with its own HIP stream) the frames are dealt to in turn: consecutive frames are independent, so the "
                         "occupancy tail of one frame's kernel can be filled by the next frame's workgroups (resident-matrices workloads only)")
    ap.add_argument("--per-plane", action="store_true",
                    help="the reference's own call sequence: one gfw_undistort_image per plane, each plane through a backend object (context) of its own "
                         "(rendering/mod.rs:494-545), asynchronous device buffers — GFW_OPT_COALESCE_PLANES turns the calls of a frame into one fused launch; "
                         "--clip N holds N assembled frames for one launch of the specialised kernel (GFW_OPT_COALESCE_FRAMES)")
    ap.add_argument("--frame-sync", action="store_true",
                    help="--per-plane on SYNCHRONOUS contexts (GFW_OPT_SYNCHRONOUS = 1, the reference's contract) with GFW_OPT_FRAME_SYNC: a frame's earlier planes are held, "
                         "its last plane's call launches the fused kernel and returns when the frame is complete")
    ap.add_argument("--build-matrices", action="store_true",
                    help="build every frame's per-row matrices on the device from quaternion tracks (gfw_build_matrices, "
                         "the 'next' row f-1) inside the timed region instead of using pre-packed resident tables")
    ap.add_argument("--build-batch", type=int, default=16, help="frames per gfw_build_matrices_batch call (1 = one gfw_build_matrices per frame "
                                                                 "on the auxiliary stream)")
    ap.add_argument("--upload-matrices", action="store_true",
                    help="upload the per-row matrices from host memory every frame (the reference's OpenCL backend does, "
                         "opencl.rs:406) instead of keeping the pre-packed tables of the clip resident in HBM")
    args = ap.parse_args(argv)
    if args.profile_every is None:
        args.profile_every = 8 if args.full else 0
    return args


# ---------------------------------------------------------------------------------------------- launcher
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launcher(args, argv):
    """Spawn one worker per GPU, relay rank 0's JSON line.  A worker set that dies abnormally (GPU fault, signal) fails the run;
    with --retry it is re-run — at most three attempts in all — and every failed attempt is reported in the line
    (`launcher.failures`)."""
    n = max(1, args.gpus)
    failures = []
    attempts = 3 if args.retry else 1
    for attempt in range(1, attempts + 1):
        env = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs, logs = [], []
        for r in range(n):
            e = dict(env, RANK=str(r), LOCAL_RANK=str(r))
            logs.append((tempfile.TemporaryFile(mode="w+"), tempfile.TemporaryFile(mode="w+")))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv + ["--worker"], env=e,
                                          stdout=logs[r][0], stderr=logs[r][1], text=True))
        # wait for all; if one rank dies the others would wait on a collective for ever: give them 10 s, then kill them
        dead_since = None
        while any(p.poll() is None for p in procs):
            if any(p.poll() not in (None, 0) for p in procs):
                dead_since = dead_since or time.time()
                if time.time() - dead_since > 10.0:
                    for p in procs:
                        if p.poll() is None:
                            p.kill()
            time.sleep(0.05)
        rcs = [p.returncode for p in procs]
        outs, errs = [], []
        for fo, fe in logs:
            fo.seek(0); fe.seek(0)
            outs.append(fo.read()); errs.append(fe.read())
            fo.close(); fe.close()
        out0 = outs[0]
        line = None
        for ln in (out0 or "").splitlines():
            if ln.startswith("{") and ln.rstrip().endswith("}"):
                line = ln
        if all(rc == 0 for rc in rcs) and line is not None:
            out = json.loads(line)
            out["launcher"] = {"ranks_spawned": n, "attempts": attempt, "failures": failures}
            for e in errs:
                if e:
                    sys.stderr.write(e)
            print(json.dumps(out), flush=True)
            return 0
        tail = " | ".join((e or "").strip().splitlines()[-1] if (e or "").strip() else "" for e in errs)
        failures.append({"attempt": attempt, "rcs": rcs, "stderr_tail": tail[-400:]})
        sys.stderr.write("[bench] attempt %d failed (rcs %s)\n" % (attempt, rcs))
        for e in errs:
            if e:
                sys.stderr.write(e)
        # only an abnormal death (signal, abort: GPU memory fault, runtime crash) is worth another attempt; an error the
        # worker reported itself (exit status 1..127) would only repeat
        if not any(rc < 0 or rc >= 128 for rc in rcs):
            break
    return 1


# ---------------------------------------------------------------------------------------------- worker
def host_threads():
    """(threads, why): the CPUs this process may actually use — the scheduler affinity, capped by the container's CFS quota (cgroup v2 cpu.max / v1
    cfs_quota_us).  More OpenMP threads than that only fight over the quota (profiles/r04_cpu_baseline_scan.txt: 61 Mpix/s on 16 threads, 42 on 128)."""
    n = os.cpu_count() or 1
    why = "%d hardware threads visible" % n
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None and quota < n:
        n = max(1, int(quota + 0.5))
        why += ", CFS quota of the container: %.1f CPUs" % quota
    return n, why


def dump_outputs(out_dir, arrays, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: each array as out_dir/<name>.npy in float32 (every pixel type the library writes is exact in it).  Arrays that exceed `budget`
    bytes together are each replaced by the same share of their elements, a sample drawn with a seed of the array's name and kept in index order:
    two runs with the same arguments write the same positions."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total, keep = sum(np.asarray(a).size for a in arrays.values()), budget // 4
    for name, a in arrays.items():
        a = np.asarray(a).astype(np.float32)
        if total > keep:
            idx = np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, a.size * keep // total, replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(out_dir, name + ".npy"), a)


class _FrameView:
    """What tests/_oracle.run_frame needs of a frame, with the pixels downloaded from the device."""

    def __init__(self, frame, src_planes, matrices):
        import numpy as np
        self.model, self.digital, self.matrices = frame.model, frame.digital, matrices
        self.planes = []
        for pl, src in zip(frame.planes, src_planes):
            q = dict(pl)
            q["src"] = src
            q["dst"] = np.full(pl["out_size"][2] * pl["out_size"][1], 0x5A, dtype=np.uint8)
            self.planes.append(q)


def worker(args):
    import numpy as np
    import torch
    from gyroflow_amd import abi, shard, synthetic as S, warp

    rank, local_rank, world = shard.env_rank()
    if world != max(1, args.gpus):
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (launch one rank per GPU)" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (libgfwarp has no CPU fallback)")
    dev_index = 0 if args.same_device else local_rank
    if dev_index >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d wants cuda:%d but only %d device(s) are visible" % (rank, dev_index, torch.cuda.device_count()))
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = shard.init(args.backend, rank, world, dev)
    if dist is not None:
        assert dist.get_world_size() == world, (dist.get_world_size(), world)
    cdev = dev if args.backend == "nccl" else "cpu"      # where the tiny control tensors of the collectives live

    lib = abi.load_library()
    if lib.gfw_set_device(dev_index) != 0:
        raise SystemExit("gfw_set_device failed: %s" % lib.gfw_last_error().decode())
    info = C.create_string_buffer(512)
    lib.gfw_get_info(info, 512)

    # ---- synthetic clip, produced directly in HBM ---------------------------------------------------------
    if args.c1:
        args.width, args.height, args.fmt = 1920, 1080, "NV12"
    auto_clip = args.clip <= 0
    if auto_clip:
        args.clip = 8
        if not (args.c5 or args.per_plane or args.host_buffers or args.upload_matrices or args.build_matrices):
            for cand in range(CLIP_FRAMES, 7, -1):
                if args.steps % cand == 0:
                    args.clip = cand
                    break
    global N_DST
    # the frames of a clip launch write one destination set each; clip launches dealt to S streams: a group of sets per stream
    N_DST = max(8, min(args.clip, CLIP_FRAMES)) * (args.streams if args.clip > 1 else 1)
    sum_stream_on = bool(args.c5 and args.sum_stream and args.clip > 1)
    sums_in_kernel = bool(args.c5 and not args.sum_pass and not sum_stream_on and args.streams == 1)
    if sum_stream_on:
        N_DST = 2 * min(args.clip, CLIP_FRAMES)         # two groups of destination sets: launch c + 1 writes one while the checksums of launch c read the other
    W, H = args.width, args.height
    readout = 0.0 if args.c1 else 16.0
    cquat = S.quat_from_euler_deg(5.0, 2.0, 3.0) if args.c1 else None
    fov = 0.82 if args.crop else args.fov
    ov = {"translation2d": (13.25, -7.5)} if args.crop else None
    lens = S.gopro_style_lens(W, H)
    if args.digital:
        lens["digital"] = args.digital
    if args.lens_model:
        k = LENS_MODEL_K[args.lens_model]
        lens["model"], lens["k"] = args.lens_model, k + [0.0] * (12 - len(k))
        if args.lens_model == "gopro":
            lens["r_limit"] = 2.5
    if args.lca != 1.0:
        ov = dict(ov or {}, lens_correction_amount=args.lca)
    NR = 4 if args.host_buffers else max(1, args.resident)
    if args.clip > 1 and NR > args.clip and NR % args.clip and args.resident == N_RESIDENT and not args.host_buffers:
        NR -= NR % args.clip                            # the source sets cycle in whole clip calls (each frame of a call writes its own destination set)
    device_built = args.build_matrices or args.c5
    # frame j of this rank: seed and timestamp of its own (seed = 0x9F10 + frame index); the C5 clip's
    # resident source frames are the clip's, the same on every rank
    seed_base = 0 if args.c5 else rank * 1000
    frames = [S.SyntheticFrame(args.fmt, W, H, seed=0x9F10 + seed_base + j, timestamp_ms=1000.0 + 33.3 * (seed_base + j), lens=dict(lens),
                               fov=fov, base_overrides=ov, interpolation=args.interp, readout_ms=readout,
                               constant_quat=cquat, pixels=args.host_buffers)
              for j in range(NR)]
    nplanes = len(frames[0].planes)
    types = [pl["pixel_type"] for pl in frames[0].planes]
    if args.host_buffers:
        d_src = None
        h_dst = [[pl["dst"].copy() for pl in frames[0].planes] for _ in range(N_DST)]
    else:
        d_src = [fr.device_planes(dev) for fr in frames]
        h_dst = None
    # destination sets: one contiguous allocation each (plane p at a 256-byte aligned offset), pre-filled like the host
    # copies — stride padding is never written by the warp
    sizes = [pl["out_size"][2] * pl["out_size"][1] for pl in frames[0].planes]
    offs = [0]
    for s in sizes:
        offs.append(S.align(offs[-1] + s, 256))
    dst_total = S.align(offs[-1], 256)
    d_dstbuf = [torch.full((dst_total,), 0x5A, dtype=torch.uint8, device=dev) for _ in range(N_DST)]
    d_dst = [[d_dstbuf[d][offs[p]:offs[p] + sizes[p]] for p in range(nplanes)] for d in range(N_DST)]
    if os.environ.get("GFW_BENCH_ADDR") and not args.host_buffers:      # diagnosis: where the resident sets landed (profiles/r06_c3_bimodal.txt)
        print("addr src0", [hex(t.data_ptr()) for t in d_src[0]], "src1", [hex(t.data_ptr()) for t in d_src[min(1, NR - 1)]],
              "dst", [hex(t.data_ptr()) for t in d_dstbuf[:3]], file=sys.stderr, flush=True)
    bufsets = []                                      # bufsets[j * N_DST + d]: source set j -> destination set d
    for j in range(NR):
        fr = frames[j]
        for d in range(N_DST):
            if args.host_buffers:
                bufsets.append([warp.host_buffers(pl["src"], pl["size"], h_dst[d][p], pl["out_size"]) for p, pl in enumerate(fr.planes)])
                continue
            bufsets.append([warp.device_buffers(d_src[j][p].data_ptr(), d_src[j][p].numel(), pl["size"],
                                                d_dst[d][p].data_ptr(), d_dst[d][p].numel(), pl["out_size"])
                            for p, pl in enumerate(fr.planes)])
    # clip-invariant block (lens + per-plane KernelParams template): rank 0's copy is the one every rank uses
    blob = shard.broadcast_bytes(dist, b"".join(bytes(pl["params"]) for pl in frames[0].planes), cdev)
    ksz = C.sizeof(abi.KernelParams)
    tmpl = [abi.KernelParams.from_buffer_copy(blob[k * ksz:(k + 1) * ksz]) for k in range(nplanes)]
    be = warp.Backend(tmpl[0], types[0], frames[0].model, frames[0].digital, bufsets[0][0])
    stream = torch.cuda.current_stream(dev)
    be.set_stream(stream.cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 1 if args.host_buffers else 0)
    if args.variant:
        be.set_option(abi.OPT_KERNEL_VARIANT, args.variant)
    if args.grid:
        be.set_option(abi.OPT_TUNE_GRID, args.grid)
    be.set_option(abi.OPT_JIT, args.jit)
    rows_n = frames[0].matrices.shape[0]
    nk = S.new_k(frames[0].lens, fov, W, H)

    def timing_for(ts_ms, t=None):
        t = t or abi.FrameTiming()
        t.timestamp_ms, t.frame_readout_time_ms, t.rows, t.readout_dim = ts_ms, readout, rows_n, H
        for i, v in enumerate(np.asarray(nk, dtype=np.float64).reshape(9)):
            t.new_k[i] = v
        return t

    BATCH = max(1, min(64, args.build_batch if not args.c5 else max(args.build_batch, 32)))
    if args.c5:
        total = max(1, args.frames)
        own = list(shard.frames_for_rank(rank, world, total))           # global frame indices of this rank, in order
        n_steps, n_warm = len(own), min(args.warmup, len(own))
    else:
        total, own = None, None
        n_steps, n_warm = args.steps, args.warmup

    def ts_of(f):                                      # clip time of global frame f (30 fps)
        return 1000.0 + 33.3 * f

    if device_built:
        t_end = ts_of((total if args.c5 else (n_steps + n_warm + BATCH + 2)) + 2) + 100.0
        org = S.sampled_track_fast(11, 0.0, t_end, 500.0)             # the clip's tracks: identical on every rank
        smo = S.sampled_track_fast(12, 0.0, t_end, 100.0, scale=0.25)
        be.set_quaternion_tracks(org, smo)
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        table0 = be.build_matrices(nk, 1000.0, readout, rows_n, H)     # context-owned table: a valid pointer for the pre-marshalled calls
        be.synchronize()
        calls = [warp.FrameCall(be, bufsets[i], tmpl, types, table0, rows_n) for i in range(NR * N_DST)]
        timings = (abi.FrameTiming * BATCH)()
        for t in timings:
            timing_for(0.0, t)
        tptrs = (C.c_void_p * BATCH)()
        batch_fn, ctxp = be.lib.gfw_build_matrices_batch, be.ctx
        one = timing_for(0.0)
        one_ref, tbl = C.byref(one), C.c_void_p(0)
        build_fn, tblref = be.lib.gfw_build_matrices, C.byref(tbl)
    elif args.upload_matrices:
        calls = [warp.FrameCall(be, bufsets[j * N_DST + (j % N_DST)], tmpl, types, frames[j].matrices) for j in range(NR)]
    else:
        d_mat = [torch.from_numpy(warp.pack_matrices(fr.matrices)).to(dev) for fr in frames]
        be.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        calls = [warp.FrameCall(be, bufsets[j * N_DST + (j % N_DST)], tmpl, types, d_mat[j].data_ptr(), rows_n) for j in range(NR)]
    plane_bes = []
    if args.per_plane:
        # the render loop's shape: plane p has a backend object of its own (plane 0's is `be`); the steps are per-plane gfw_undistort_image calls
        if device_built or args.host_buffers or args.streams > 1:
            raise SystemExit("bench.py: --per-plane runs with resident or per-frame uploaded matrices on one stream")
        hold = max(1, min(args.clip, CLIP_FRAMES, N_DST))
        for p in range(1, nplanes):
            b2 = warp.Backend(tmpl[p], types[p], frames[0].model, frames[0].digital, bufsets[0][p])
            b2.set_stream(stream.cuda_stream)
            b2.set_option(abi.OPT_SYNCHRONOUS, 0)
            if not args.upload_matrices:
                b2.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
            b2.set_option(abi.OPT_JIT, args.jit)
            plane_bes.append(b2)
        for b2 in [be] + plane_bes:
            b2.set_option(abi.OPT_COALESCE_FRAMES, hold)
            if args.frame_sync:                      # the reference's synchronous contract, relaxed to "the frame is complete when its last plane's call returns"
                b2.set_option(abi.OPT_SYNCHRONOUS, 1)
                b2.set_option(abi.OPT_FRAME_SYNC, 1)
        calls = [warp.PlaneCalls([be] + plane_bes, bufsets[j * N_DST + (j % N_DST)], tmpl,
                                 frames[j].matrices if args.upload_matrices else d_mat[j].data_ptr(), rows_n) for j in range(NR)]
    # --streams S: S contexts, each on a stream of its own, take the frames in turn.  Frame k writes destination set k mod N_DST and
    # S divides N_DST, so two frames that share a destination set always share a stream (ordered); everything else may overlap.
    n_streams = args.streams if not (device_built or args.upload_matrices or args.host_buffers or args.c5) else 1
    if n_streams > 1 and (NR % N_DST or N_DST % n_streams):
        raise SystemExit("bench.py: --streams %d needs --resident to be a multiple of %d (two streams would write one destination set unordered)" % (n_streams, N_DST))
    extra_bes, extra_streams, calls_by_stream = list(plane_bes), [], [calls]
    for _ in range(1, n_streams):
        st = torch.cuda.Stream(device=dev)
        b2 = warp.Backend(tmpl[0], types[0], frames[0].model, frames[0].digital, bufsets[0][0])
        b2.set_stream(st.cuda_stream)
        b2.set_option(abi.OPT_SYNCHRONOUS, 0)
        if args.variant:
            b2.set_option(abi.OPT_KERNEL_VARIANT, args.variant)
        if args.grid:
            b2.set_option(abi.OPT_TUNE_GRID, args.grid)
        b2.set_option(abi.OPT_MATRICES_ON_DEVICE, 2)
        b2.set_option(abi.OPT_JIT, args.jit)
        extra_bes.append(b2); extra_streams.append(st)
        calls_by_stream.append([warp.FrameCall(b2, bufsets[j * N_DST + (j % N_DST)], tmpl, types, d_mat[j].data_ptr(), rows_n) for j in range(NR)])
    all_bes = [be] + extra_bes

    # ---- clip mode: the steps reach the library as gfw_undistort_clip calls of `clip_n` frames (the frames of one call use distinct
    # destination sets: the specialised kernel takes up to 8 of them in one launch)
    clip_n = max(1, min(args.clip, CLIP_FRAMES) if device_built else min(args.clip, CLIP_FRAMES, NR))
    if args.upload_matrices or args.host_buffers or (device_built and not args.c5) or (NR % clip_n and not device_built):
        clip_n = 1
    if args.c5 and BATCH % clip_n:
        clip_n = 1
    if args.per_plane:
        clip_n = 1

    # what step k of this rank reads and writes: (global frame, source set, destination set)
    def plan(k):
        f = own[k] if args.c5 else k
        j = f % NR
        if device_built:
            if sum_stream_on:
                return f, j, (k % clip_n) + ((k // clip_n) % 2) * clip_n
            return f, j, (k % clip_n if clip_n > 1 else k % N_DST)
        return f, j, j % N_DST

    if args.c5:
        d_sums = torch.zeros(max(1, n_steps), dtype=torch.int64, device=dev)
        sum_fn, sum_base = be.lib.gfw_checksum64, d_sums.data_ptr()
        dst_ptrs = [b.data_ptr() for b in d_dstbuf]
    sum_stream, sum_ctxp, sums_done, be_sum = None, None, {}, None
    if sum_stream_on:
        # the verification off the warp's critical path: a context of its own on a stream of its own takes the checksums; the warp's persistent grid
        # (8 workgroups per CU by default) leaves one wave slot per SIMD so that the checksum kernel's workgroups find room beside it
        sum_stream = torch.cuda.Stream(dev)
        be_sum = warp.Backend(tmpl[0], types[0], frames[0].model, frames[0].digital, bufsets[0][0])
        be_sum.set_stream(sum_stream.cuda_stream)
        be_sum.set_option(abi.OPT_SYNCHRONOUS, 0)
        sum_ctxp = be_sum.ctx
        sums_done = {0: None, clip_n: None}
        if not args.grid:
            be.set_option(abi.OPT_TUNE_GRID, torch.cuda.get_device_properties(dev).multi_processor_count * 7)

    clip_cache = {}

    def clip_for(k0, ln):
        """pre-marshalled gfw_undistort_clip call for steps k0 .. k0+ln-1 (with --streams S, launch c goes to context c mod S)"""
        js = tuple(plan(k0 + i)[1] for i in range(ln))
        sidx = (k0 // clip_n) % n_streams
        par = ((k0 // clip_n) % 2) * clip_n if sum_stream_on else 0          # the launch's group of destination sets
        if par:
            sidx = -1                                   # (key only: the second group's calls)
        call = clip_cache.get((sidx, js))
        if call is None and sidx > 0:
            call = warp.ClipCall(all_bes[sidx], [bufsets[j * N_DST + (j % N_DST)] for j in js], tmpl, types, [d_mat[j].data_ptr() for j in js], rows_n)
            clip_cache[(sidx, js)] = call
        if call is None:
            if device_built:                            # C5: frame i of the call writes destination set i; its table pointer is set per call
                call = warp.ClipCall(be, [bufsets[j * N_DST + par + i] for i, j in enumerate(js)], tmpl, types, [table0] * ln, rows_n)
            else:
                call = warp.ClipCall(be, [bufsets[j * N_DST + (j % N_DST)] for j in js], tmpl, types, [d_mat[j].data_ptr() for j in js], rows_n)
            clip_cache[(sidx, js)] = call
        return call

    def clip_step(k0, ln):
        call = clip_for(k0, ln)
        if device_built:
            if k0 % BATCH == 0:                         # one launch builds the tables of the next BATCH frames, in order on the warp's stream
                for i in range(BATCH):
                    kk = min(k0 + i, n_steps - 1)
                    timings[i].timestamp_ms = ts_of(own[kk] if args.c5 else kk)
                rc = batch_fn(ctxp, timings, BATCH, tptrs)
                if rc != 0:
                    be._check(rc)
            for i in range(ln):
                call.marr[i] = tptrs[(k0 + i) % BATCH]
        if sum_stream_on:
            par = ((k0 // clip_n) % 2) * clip_n
            if sums_done[par] is not None:
                stream.wait_event(sums_done[par])       # this launch overwrites the sets launch c - 2 wrote: its checksums must have read them
            call()
            ev = torch.cuda.Event()
            ev.record(stream)
            sum_stream.wait_event(ev)
            for i in range(ln):                         # each frame's checksum on the second stream, beside the next launch's warp
                sum_fn(sum_ctxp, dst_ptrs[par + i], dst_total, sum_base + 8 * (k0 + i))
            sums_done[par] = torch.cuda.Event()
            sums_done[par].record(sum_stream)
            return
        call()
        if args.c5 and not sums_in_kernel:
            for i in range(ln):                         # each frame's checksum, in order on the same stream
                sum_fn(ctxp, dst_ptrs[i], dst_total, sum_base + 8 * (k0 + i))

    def step(k):
        f, j, d = plan(k)
        if device_built:
            call = calls[j * N_DST + d]
            if BATCH > 1:
                # every BATCH steps one launch builds the tables of the next BATCH frames, in order on the warp's stream
                if k % BATCH == 0:
                    for i in range(BATCH):
                        kk = min(k + i, n_steps - 1)
                        timings[i].timestamp_ms = ts_of(own[kk] if args.c5 else kk)
                    rc = batch_fn(ctxp, timings, BATCH, tptrs)
                    if rc != 0:
                        be._check(rc)
                call.mp = tptrs[k % BATCH]
            else:
                # the context builds this frame's table on its auxiliary stream (ring of tables) while the previous frame warps
                one.timestamp_ms = ts_of(f)
                rc = build_fn(ctxp, one_ref, None, tblref)
                if rc != 0:
                    be._check(rc)
                call.mp = tbl.value
            call()
            if args.c5 and not sums_in_kernel:
                sum_fn(ctxp, dst_ptrs[d], dst_total, sum_base + 8 * k)           # the frame's checksum, in order on the same stream
        elif n_streams > 1:
            calls_by_stream[k % n_streams][j]()
        else:
            calls[j]()

    ENQ_WINDOW = 256                                   # steps over which the host's own enqueue cost is read: beyond a few hundred frames in flight
    enq_mark = [None, 0]                               # the runtime's bounded rings make the host wait for the GPU, which is not host work

    def run_steps(n, bracket_every=0):
        """steps 0 .. n-1 of the workload, as clip calls or frame by frame; every bracket_every-th launch has its kernel time taken"""
        set_opt, ctxps = be.lib.gfw_set_option, [b.ctx for b in all_bes]
        enq_mark[0], enq_mark[1] = None, 0
        if sums_in_kernel:
            be.set_frame_checksums(sum_base, max(1, n_steps))            # step k's frame adds the checksum of what it writes to word k (the count restarts here)
        if clip_n > 1:
            for c, k0 in enumerate(range(0, n, clip_n)):
                ln = min(clip_n, n - k0)
                if enq_mark[0] is None and k0 >= ENQ_WINDOW:
                    enq_mark[0], enq_mark[1] = time.perf_counter(), k0
                if bracket_every and (c // n_streams) % 2 == 0:        # a launch carries clip_n frames: every other one (per stream) is bracketed
                    set_opt(ctxps[c % n_streams], abi.OPT_PROFILE, 1)
                    clip_step(k0, ln)
                    set_opt(ctxps[c % n_streams], abi.OPT_PROFILE, 0)
                else:
                    clip_step(k0, ln)
        elif bracket_every > 1:
            for k in range(n):
                if enq_mark[0] is None and k >= ENQ_WINDOW:
                    enq_mark[0], enq_mark[1] = time.perf_counter(), k
                if k % bracket_every == 0:
                    ctxp2 = ctxps[k % n_streams]
                    set_opt(ctxp2, abi.OPT_PROFILE, 1)
                    step(k)
                    set_opt(ctxp2, abi.OPT_PROFILE, 0)
                else:
                    step(k)
        else:
            for k in range(n):
                step(k)
        if args.per_plane:
            be.flush()                                   # frames still held for a launch (GFW_OPT_COALESCE_FRAMES) leave now: the region ends with a raw device synchronise

    run_steps(n_warm)
    torch.cuda.synchronize(dev)
    jit_state = be.jit_status()
    # declared, untimed pre-heat: the same launches for --preheat-ms, so that a short timed region runs at the clocks a long one does
    preheat_ms = 0.0
    if args.preheat_ms > 0 and n_steps > 0 and not args.host_buffers:
        t_ph = time.perf_counter()
        while (time.perf_counter() - t_ph) * 1e3 < args.preheat_ms:
            run_steps(min(n_steps, 4 * max(clip_n, 8)))
            torch.cuda.synchronize(dev)
        preheat_ms = (time.perf_counter() - t_ph) * 1e3
    if args.c5:
        d_sums.zero_()                                # gfw_checksum64 accumulates
    pe = args.profile_every
    if args.per_plane and pe != 1:
        pe = 0                                        # a launch happens inside the call of a frame's last plane (or later): brackets per step make no sense; --profile-every 1 brackets all
    for b in all_bes:
        b.set_option(abi.OPT_PROFILE, 1 if (pe == 1 and clip_n == 1) else 0)
        b.get_profile(reset=True)
    shard.barrier(dist)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run_steps(n_steps, pe)
    t_enq = time.perf_counter() - t0                 # host time to enqueue the steps (the GPU runs behind it)
    enq_steps = n_steps
    if enq_mark[0] is not None:                      # long runs: the first ENQ_WINDOW steps, before the queues fill and the host starts waiting for the GPU
        t_enq, enq_steps = enq_mark[0] - t0, enq_mark[1]
    torch.cuda.synchronize(dev)
    shard.barrier(dist)
    t1 = time.perf_counter()
    elapsed = t1 - t0
    kernel_ms, launches, prof_frames = 0.0, 0, 0
    for b in all_bes:
        km, ln, nf = b.get_profile_frames(reset=True)
        kernel_ms += km; launches += ln; prof_frames += nf
        b.set_option(abi.OPT_PROFILE, 0)
    elapsed = shard.reduce_max(dist, elapsed, cdev)

    def dst_host(d, p):
        return h_dst[d][p] if args.host_buffers else d_dst[d][p].cpu().numpy()

    # ---- checksums ------------------------------------------------------------------------------------------
    if args.c5:
        mine = d_sums[:n_steps].cpu().numpy().astype(np.int64)
        frame_sums, gathered = shard.assemble_frame_checksums(dist, [int(v) for v in mine], rank, world, total, cdev)
        frame_sums = np.asarray(frame_sums, dtype=np.int64)
        crc = zlib.crc32(frame_sums.tobytes())
        rank_crcs = [zlib.crc32(np.asarray(g, dtype=np.int64).tobytes()) for g in gathered]
    else:
        crc = 0
        last = plan(n_steps - 1)[2]
        for p in range(nplanes):
            crc = zlib.crc32(dst_host(last, p).tobytes(), crc)
        rank_crcs = [g[0] for g in shard.gather_checksums(dist, [crc], cdev)]
        crc = shard.reduce_checksum(dist, crc, cdev)

    # ---- what the last timed step computed (--dump-outputs): the destination planes of its frame, pixels as a caller of the path receives them
    if args.dump_outputs and rank == 0:
        last, planes_out = plan(n_steps - 1)[2], {}
        for p, pl in enumerate(frames[0].planes):
            ow, oh, ostride = pl["out_size"]
            rows_b = dst_host(last, p)[:oh * ostride].reshape(oh, ostride)[:, :ow * pl["params"].bytes_per_pixel]
            planes_out["plane%d" % p] = np.ascontiguousarray(rows_b).view(abi.PIXEL_TYPES[types[p]][1])
        dump_outputs(args.dump_outputs, planes_out)

    luma_px = frames[0].luma_pixels()
    alg_bytes = frames[0].algorithmic_bytes()
    frames_done = total if args.c5 else n_steps * world
    value = luma_px * frames_done / elapsed / 1e6
    cfg_name = ("custom" if (args.lens_model or args.lca != 1.0 or args.digital) else "C5" if args.c5 else "C1" if args.c1 else "C2" if (W, H, args.fmt, args.crop) == (3840, 2160, FMT, False) else
                "C3" if (W, H, args.fmt) == (7680, 4320, FMT) else "C4" if args.crop else "custom")
    how = (" — HOST buffers: H2D + warp + D2H + sync per frame (PCIe-inclusive)" if args.host_buffers else
           " (matrices re-uploaded per frame)" if args.upload_matrices else
           " (per-row matrices built on the device every frame from quaternion tracks, %d frames per build launch)" % BATCH if device_built else "")
    workload = "%s: %dx%d %s, LENS GoPro-style lens, rolling shutter matrix_count=%d, %s, %d distinct source frames%s resident in HBM%s" % (
        cfg_name, W, H, args.fmt, rows_n, {2: "bilinear", 4: "bicubic", 8: "Lanczos4"}.get(args.interp, str(args.interp)), NR,
        "" if device_built else " + per-row matrix tables", how)
    workload = workload.replace("LENS", (args.lens_model or "opencv_fisheye") + (" + " + args.digital if args.digital else "") +
                                ("" if args.lca == 1.0 else " (lens correction %g)" % args.lca))
    if args.c5:
        workload += "; %d-frame clip dealt round-robin to %d rank(s), one 64-bit checksum per frame (%s)" % (
            total, world, "taken by the warp kernel where the pixels leave: gfw_set_frame_checksums" if sums_in_kernel else "a gfw_checksum64 pass over each destination buffer")
    if clip_n > 1:
        workload += "; steps handed to the library as gfw_undistort_clip calls of %d frames" % clip_n
    if args.per_plane:
        workload += ("; the reference's call sequence: %d gfw_undistort_image calls per frame (one per plane, each plane its own context), asynchronous, coalesced by the "
                     "library into one fused launch per %d frame(s)" % (nplanes, max(1, min(args.clip, CLIP_FRAMES, N_DST))))
    out = {
        "metric": "Mpix/s (4K u16 YUV, rolling-shutter warp)" if not args.c1 else "Mpix/s (1080p u8 NV12 warp)",
        "value": round(value, 2), "unit": "Mpix/s", "n_gpus": world, "steps": n_steps, "warmup": n_warm,
        "ms_per_step": round(elapsed / max(n_steps, 1) * 1e3, 5), "higher_is_better": True, "scaling": "strong" if args.c5 else "weak",
        "vs_baseline": None, "dtype": "f32 coordinates, %s pixels" % np.dtype(abi.PIXEL_TYPES[types[0]][1]).name, "data": "synthetic",
        "config": {"workload": workload + ("" if n_streams == 1 else "; frames dealt to %d contexts / HIP streams in turn (bracketed kernel times overlap their neighbours)" % n_streams),
                   "streams_per_rank": n_streams, "frames_per_rank": n_steps, "frames_total": frames_done, "parallelism": "frame-sharded x%d" % world,
                   "backend": warp.last_backend(), "checksum": crc, "rank_checksums": rank_crcs,
                   "host_enqueue_ms_per_step": round(t_enq / max(enq_steps, 1) * 1e3, 5),
                   "clip_frames_per_call": clip_n, "per_plane_calls": bool(args.per_plane), "preheat_ms": round(preheat_ms, 1),
                   "jit": {"mode": args.jit, "state": {0: "none", 1: "compiling", 2: "ready", 3: "failed"}.get(jit_state[0], str(jit_state[0])),
                           "compile_ms": round(jit_state[1], 1), "log": jit_state[2][-300:] if jit_state[0] == 3 else ""},
                   "device": info.value.decode(), "collectives": (args.backend if dist is not None else "none (1 rank)")},
    }
    if launches:
        per_launch_ms = kernel_ms / launches
        fpl = max(prof_frames, launches) / launches                 # frames per bracketed launch (a clip launch carries up to 8)
        achieved = alg_bytes * fpl / (per_launch_ms * 1e-3) / 1e9
        # HBM bytes per launch: rocprofv3 PMC passes cannot run inside bench.py; the stored figure of this exact workload is quoted
        traffic, tsrc = None, None
        tpath = os.path.join(ROOT, TRAFFIC_FILE)
        if (W, H, args.fmt, args.interp, args.crop, args.variant, args.host_buffers, bool(args.digital or args.lens_model or args.lca != 1.0)) == (WIDTH, HEIGHT, FMT, 2, False, 0, False, False) and os.path.exists(tpath):
            tj = json.load(open(tpath))                  # per frame; a launch carries fpl of them
            if tj.get("kernel_source_id") and tj.get("kernel_source_id") == abi.kernel_source_id():
                traffic = int((tj["fetch_size_kib_per_frame"] * tj["fetch_correction"] + tj["write_size_kib_per_frame"]) * 1024 * fpl)
                tsrc = "%s (stored rocprofv3 PMC passes of this workload on this kernel source, not measured in this run)" % TRAFFIC_FILE
            else:                                        # counters of another kernel say nothing about this one: no figure rather than a stale one
                tsrc = "%s was taken on kernel source %s, the loaded library is %s: not quoted" % (TRAFFIC_FILE, tj.get("kernel_source_id"), abi.kernel_source_id())
        out["roofline"] = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": tsrc,
                           "kernel": warp.last_backend(), "kernel_ms_per_launch": round(per_launch_ms, 5),
                           "frames_per_launch": round(fpl, 3), "kernel_ms_per_frame": round(per_launch_ms / fpl, 5),
                           "algorithmic_bytes_per_launch": int(alg_bytes * fpl), "launches": launches}

    # ---- parity of the timed region's own output, and the CPU baseline (rank 0, --full) ---------------------------------
    if rank == 0 and args.full and not (args.no_parity and (args.no_cpu_baseline or world > 1)):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _oracle as O
        checks, seen_d = [], set()
        for k in range(n_steps - 1, max(n_steps - 1 - min(N_CHECK, N_DST - 1), -1), -1):
            f, j, d = plan(k)
            if d in seen_d:                           # a later step overwrote this destination set
                break
            seen_d.add(d)
            if device_built:
                # the table this frame used: rebuilt from the same tracks / timestamp (the builder is deterministic)
                tab = torch.empty(rows_n * 16, dtype=torch.float32, device=dev)
                be.set_option(abi.OPT_SYNCHRONOUS, 1)
                be.build_matrices(nk, ts_of(f), readout, rows_n, H, out_ptr=tab.data_ptr())
                be.set_option(abi.OPT_SYNCHRONOUS, 0)
                mats = np.ascontiguousarray(tab.cpu().numpy().reshape(rows_n, 16)[:, :14])
            else:
                mats = frames[j].matrices
            src = [pl["src"] for pl in frames[j].planes] if args.host_buffers else [t.cpu().numpy() for t in d_src[j]]
            checks.append((k, f, d, _FrameView(frames[j], src, mats)))
        checks.reverse()
        got = {d: [dst_host(d, p).copy() for p in range(nplanes)] for (_, _, d, _) in checks}
        refs = {}
        if not args.no_parity:
            bad = []
            for k, f, d, view in checks:
                refs[k] = O.run_frame(view)
                if not all(np.array_equal(refs[k][p], got[d][p]) for p in range(nplanes)):
                    bad.append(k)
                    diff = [np.flatnonzero(refs[k][p] != got[d][p]) for p in range(nplanes)]
                    print("bench: step %d differs from the oracle: %s bytes per plane, first at %s" % (k, [int(x.size) for x in diff], [int(x[0]) if x.size else None for x in diff]), file=sys.stderr)
                if args.c5 and sums_in_kernel:
                    # the checksum of the bytes WRITTEN (the pixels: stride padding and the gaps between planes stay out), each at its place in its 64-bit word
                    want = 0
                    for p, pl in enumerate(frames[0].planes):
                        ow, oh, ostride = pl["out_size"]
                        body = np.zeros(S.align(sizes[p], 8), np.uint8)
                        rows_v = body[:oh * ostride].reshape(oh, ostride)
                        rows_v[:, :ow * pl["params"].bytes_per_pixel] = refs[k][p][:oh * ostride].reshape(oh, ostride)[:, :ow * pl["params"].bytes_per_pixel]
                        want += int(body.view(np.int64).sum(dtype=np.int64))
                    want = int(np.array([want & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.int64)[0])
                    if want != int(mine[k]):
                        bad.append(("checksum", k))
                elif args.c5:
                    want = int(np.concatenate([np.pad(refs[k][p], (0, offs[p + 1] - offs[p] - sizes[p]), constant_values=0x5A) for p in range(nplanes)]
                                              + [np.full(dst_total - offs[-1], 0x5A, np.uint8)]).view(np.int64).sum(dtype=np.int64))
                    if want != int(mine[k]):
                        bad.append(("checksum", k))
            out["config"]["parity_vs_oracle"] = "bit-exact" if not bad else "MISMATCH at steps %s" % bad
            out["config"]["parity_checked"] = "outputs of timed steps %s (frames %s) vs oracle/gfw_oracle.c, all planes" % (
                [c[0] for c in checks], [c[1] for c in checks])
        # ... and against the reference itself: source frame 0 of the default workload is the frame whose output the reference's OWN kernel (its
        # OpenCL source compiled for the host cores, tests/golden/make_ref_golden.py) froze as tests/golden/ref_golden.json — one more launch
        # through the timed region's own call path, compared with numbers no restatement stands behind
        fixture = os.path.join(ROOT, "tests", "golden", "ref_golden.json")
        c2_default = (W, H, args.fmt, args.interp, args.crop, args.variant, args.host_buffers, bool(args.digital or args.lens_model or args.lca != 1.0),
                      args.fov, seed_base, device_built, n_streams) == (WIDTH, HEIGHT, FMT, 2, False, 0, False, False, 1.0, 0, False, 1)
        if not args.no_parity and c2_default and os.path.exists(fixture):
            want = json.load(open(fixture))["c2_yuv422p16_3840x2160_rs"]["planes"]
            if clip_n > 1:
                clip_step(0, min(clip_n, NR))
            else:
                step(0)
            torch.cuda.synchronize()
            crcs = [zlib.crc32(dst_host(0, p).tobytes()) for p in range(nplanes)]
            out["config"]["parity_vs_reference_kernel"] = ("bit-exact: CRC32 of all %d planes of frame 0 = tests/golden/ref_golden.json[c2_yuv422p16_3840x2160_rs], written by "
                                                           "the reference's opencl_undistort.cl compiled for the host" % nplanes) if crcs == want else "MISMATCH %s != %s" % (crcs, want)
        if world == 1 and not args.no_cpu_baseline:
            # The reference's CPU path as this box's host cores run it: oracle/gfw_oracle.c, its row loop instantiated per (sampler, pixel type) like the
            # Rust original's <I, T>, all planes of a frame in ONE parallel region (static chunks of 4 rows), one thread per CPU the container may use
            # (host_threads: the GPU boxes show 256 hardware threads and grant a CFS quota of 16 — round 3 ran 128 threads into that quota and reported
            # 0.32 Mpix/s per thread where a thread does 3.8-4.6).  profiles/r04_cpu_baseline_scan.txt: how it scales.
            hw, why = host_threads()
            runners = [O.FrameRunner(c[3], nthreads=hw) for c in checks]
            for i in range(2):
                runners[i % len(runners)].run()                           # warm-up: first touch of the outputs by the threads that keep writing them
            if not args.no_parity:
                for (k, f, d, view), r in zip(checks, runners):           # the timed form must write what the checker's form wrote (bytes the warp never writes aside)
                    outs = r.run()
                    for p in range(nplanes):
                        w_, h_, st_ = view.planes[p]["out_size"]
                        bpp_ = view.planes[p]["params"].bytes_per_pixel
                        a = outs[p].reshape(h_, st_)[:, :w_ * bpp_]; b2 = refs[k][p].reshape(h_, st_)[:, :w_ * bpp_]
                        assert np.array_equal(a, b2), "cpu_baseline: the whole-frame entry point differs from the per-plane oracle (plane %d)" % p
            times = []
            c0 = time.perf_counter()
            while len(times) < 5 or (time.perf_counter() - c0 < 10.0 and len(times) < 64):
                a = time.perf_counter()
                runners[len(times) % len(runners)].run()
                times.append(time.perf_counter() - a)
            med = float(np.median(times))
            # one thread, for the per-thread figure (a bounded sample: 1/16 of the frame's rows would need another entry point; one full frame instead, once)
            one = O.FrameRunner(checks[0][3], nthreads=1)
            a = time.perf_counter(); one.run(); t_one = time.perf_counter() - a
            O.FrameRunner(checks[0][3], nthreads=hw).run()               # (the thread count is a process-wide setting of the OpenMP runtime: back to all)
            out["cpu_baseline"] = {"value": round(luma_px / med / 1e6, 3), "unit": "Mpix/s", "cores": hw, "kind": "port",
                                   "per_thread": round(luma_px / med / 1e6 / hw, 4), "one_thread": round(luma_px / t_one / 1e6, 3),
                                   "sample": "median of %d frames of the same workload (2 warm-ups) through oracle/gfw_oracle.c's whole-frame entry point: row loop instantiated per "
                                             "(sampler, pixel type), one OpenMP region over all planes, static chunks of 4 rows, %d threads (%s); "
                                             "mean %.3f Mpix/s; the same frame on ONE thread: %.2f Mpix/s" % (len(times), hw, why, luma_px * len(times) / sum(times) / 1e6, luma_px / t_one / 1e6)}
    for b in extra_bes:
        b.close()
    if be_sum is not None:
        be_sum.close()
    be.close()
    if rank == 0:
        print(json.dumps(out), flush=True)
    shard.finish(dist)


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    if args.worker or "RANK" in os.environ:
        worker(args)
        return 0
    return launcher(args, argv)


if __name__ == "__main__":
    sys.exit(main())
