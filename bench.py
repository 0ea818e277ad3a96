#!/usr/bin/env python3
"""Whole-hot-path benchmark: unlabeled-pool sweep + diversity selection (BASELINE.json metric
"unlabeled scenes scored+selected/sec", reported in frames/s; 1 scene = 40 frames).

One *step* = one full pass of the hot path over the rank's pool: every frame is voxelized,
run through the FPNVoxelNet detector (sparse encoder, MFMA neck/head, decode + rotated NMS)
and reduced to its 512-d BEV embedding; embeddings are all-gathered (RCCL) when N > 1; then
SpatialTemporalFeatureSelector builds the spatial (kNN geodesic), temporal and feature (L1)
maps and runs the greedy k-center under the cost budget.  Workload at N=1 = BASELINE.json
configs[1]: the 64-scene pool (2,560 frames), budget 600.  With N > 1 ranks the workload is
BASELINE.json configs[2]'s shape: every rank sweeps 88 scenes = 3,520 frames (weak scaling) and the
selector sees N x 3,520 frames with budget 1200 -- at N = 8 that is the full nuScenes pool
(704 scenes, 28,160 frames).  Point clouds are synthetic and resident in HBM before the timed
region; weights are seeded random-init (no checkpoints offline).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
--dump-outputs DIR writes what the last timed step returned (rank 0): embeddings.npy (the swept 512-d BEV embeddings,
float32; a fixed seeded row sample, with its row indices in embeddings_rows.npy, when the whole array would exceed
DUMP_EMBED_BYTES) and selected.npy (the selected frame indices in pick order, float64).  Inputs and weights are seeded,
so two builds run with the same arguments can be compared output for output.
N > 1: either under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (the driver's way), or
plain `python bench.py --gpus N`, which starts that launcher itself as a child process; `--gpus N` under a WORLD_SIZE that
is not N is refused, and so is a run whose all-reduce counts a different number of ranks (launch_or_refuse).
"""
import argparse
import json
import os
import pickle
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SCENES_PER_RANK = 64              # N = 1: BASELINE configs[1]
SCENES_PER_RANK_MULTI = 88        # N > 1: BASELINE configs[2] (8 x 88 scenes = the full 28,160-frame pool)
FRAMES_PER_SCENE = 40
BUDGET = 600
BUDGET_MULTI = 1200
HBM_PEAK_GBS = 8000.0             # MI355X_MICROARCH.md: HBM3E ~8 TB/s
DENSE_GFLOP_PER_FRAME = 67.6      # neck 63.7 + heads 3.96 (2*MAC, fp32)
MFMA_F32_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
MFMA_BF16_PEAK_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 MFMA peak (no sparsity)
DUMP_EMBED_BYTES = 48 << 20       # --dump-outputs: above this the embeddings are written as a seeded row sample


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scenes", type=int, default=None,
                    help="scenes per rank (default 64 at N=1 = configs[1]; 88 at N>1 = configs[2] per rank)")
    ap.add_argument("--batch", type=int, default=128, help="frames per detector launch")
    ap.add_argument("--budget", type=int, default=None,
                    help="cost budget (default 600; scaled down for pools under 64 scenes, whose "
                         "total labelling cost is below 600)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-from-files", action="store_true",
                    help="skip the extra step that sweeps the same number of frames from .bin files on tmpfs "
                         "through the streaming loader (value_from_files)")
    ap.add_argument("--no-bevfusion", action="store_true",
                    help="skip the two untimed BEVFusion legs (value_bevfusion_lidar = configs[3], "
                         "value_bevfusion_camera_lidar = configs[4])")
    ap.add_argument("--no-extra-math", action="store_true",
                    help="skip the one extra step (outside the timed region) under AL3D_MATH=bf16x6 (value_bf16x6)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's outputs as DIR/<name>.npy (rank 0)")
    ap.add_argument("--launch-check", action="store_true",
                    help="launcher rehearsal (no GPU needed): rendezvous, count the ranks, print a line with value null "
                         "and \"launch_check\": true, exit -- what tests/test_bench_launcher.py runs over gloo")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def dump_outputs(out_dir, feats, selected):
    """The last timed step's results as a caller of the hot path receives them: the embeddings and the picks."""
    os.makedirs(out_dir, exist_ok=True)
    emb = feats.detach().to("cpu", torch.float32).numpy()
    if emb.nbytes > DUMP_EMBED_BYTES:
        n_rows = DUMP_EMBED_BYTES // (emb.shape[1] * emb.itemsize)
        rows = np.sort(np.random.default_rng(0).choice(emb.shape[0], size=n_rows, replace=False))
        emb = emb[rows]
        np.save(os.path.join(out_dir, "embeddings_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "embeddings.npy"), np.ascontiguousarray(emb))
    np.save(os.path.join(out_dir, "selected.npy"), np.asarray(list(selected), dtype=np.float64))


def launch_or_refuse(args):
    """`--gpus N` must never mislabel itself (reference contract: env:// ranks, tools/active_select.py:94-103).
    * N > 1 and no WORLD_SIZE in the environment: start `python -m torch.distributed.run --nproc-per-node N bench.py ...`
      as a CHILD process (never exec: see the GPU box's rule on exec after GPU initialisation; nothing has touched the
      GPU yet at this point), relay its output and exit with its code.
    * WORLD_SIZE present and != N: refuse, naming the command to use.
    Returns only when this process is one of exactly N ranks."""
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None:
        if args.gpus <= 1:
            return
        import socket
        import subprocess
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        print(f"[bench] --gpus {args.gpus} without WORLD_SIZE: launching {' '.join(cmd[1:9])} bench.py ...",
              file=sys.stderr, flush=True)
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.exit(subprocess.run(cmd, env=env).returncode)
    if int(env_world) != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={env_world}: refusing to print a mislabelled line.  Use\n"
              f"  python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 "
              f"--master-port P bench.py --gpus {args.gpus} ...\n(or plain `python bench.py --gpus {args.gpus}`, "
              f"which starts that launcher itself)", file=sys.stderr)
        sys.exit(2)


def launch_check(args):
    """Rendezvous + rank census only (CPU-capable: gloo when AL3D_DIST_BACKEND=gloo or no GPU is visible)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    seen = 1
    if world > 1:
        backend = os.environ.get("AL3D_DIST_BACKEND", "nccl")
        if backend == "nccl":
            local = int(os.environ.get("LOCAL_RANK", "0"))
            torch.cuda.set_device(local)
            dist.init_process_group(backend="nccl", init_method="env://", device_id=torch.device("cuda", local))
            ones = torch.ones(1, dtype=torch.int64, device=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend, init_method="env://")
            ones = torch.ones(1, dtype=torch.int64)
        dist.all_reduce(ones)
        seen = int(ones.item())
        dist.barrier()
    ok = seen == args.gpus
    if rank == 0:
        print(json.dumps({"launch_check": True, "value": None, "n_gpus": world, "ranks_seen": seen,
                          "gpus_requested": args.gpus, "ok": ok}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    sys.exit(0 if ok else 3)


class ConvTimer:
    """HIP-event timing of the dominant kernel family (conv2d_mfma_kernel) on the stream it is
    launched on; events bracket each neck+head region, which launches nothing else."""

    def __init__(self):
        self.pairs, self.launches, self.frames = [], 0, 0
        self.enabled = False

    def wrap(self, model):
        neck_fwd, head_fwd = model.neck.forward, model.bbox_head.forward
        timer = self

        def neck(x, out_pair=False):                   # the detector looks for `out_pair` in this signature (pair pixels to the head)
            if not timer.enabled:
                return neck_fwd(x, out_pair=out_pair)
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
            y = neck_fwd(x, out_pair=out_pair)
            timer._e0, timer._b = e0, x.shape[0]
            return y

        def head(x, finetune=False, **kw):
            r = head_fwd(x, finetune=finetune, **kw)
            if timer.enabled:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                timer.pairs.append((timer._e0, e1))
                timer.launches += 12 + 1 + 1 + 1      # 12 conv3x3, conv1x1, deconv (4 phases), fused head
                timer.frames += timer._b
            return r

        model.neck.forward = neck
        model.bbox_head.forward = head
        # the dominant kernel by itself: HIP events around every launch of the streamed 3x3 kernel in its f32-out form
        # (conv3x3_f16x3_frag_kernel<0>: nine of the neck's eleven 3x3 launches), on the stream it is launched on
        from al3d import detector_ops as D
        conv_fn = D.conv2d_nhwc
        timer.dom = []

        def conv(x, w, *a, **k):
            if not (timer.enabled and getattr(w, "kind", None) == "frag3x3" and not k.get("io", 0)):
                return conv_fn(x, w, *a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = conv_fn(x, w, *a, **k)
            e1.record()
            timer.dom.append((e0, e1, 2.0 * y.shape[0] * y.shape[1] * y.shape[2] * w.cout * w.cin * 9))
            return y

        D.conv2d_nhwc = conv

    def result(self):
        if not self.pairs:
            return None
        from al3d import detector_ops as D
        ms = sum(a.elapsed_time(b) for a, b in self.pairs)
        flops = self.frames * DENSE_GFLOP_PER_FRAME * 1e9
        tf = flops / (ms * 1e-3) / 1e12
        out = dict(bound="mfma", achieved=round(tf, 2), unit="TFLOP/s", traffic=None,
                   launches=self.launches, avg_launch_us=round(ms * 1e3 / max(self.launches, 1), 2),
                   gflop_per_frame=DENSE_GFLOP_PER_FRAME)
        if D.MATH == "f16x3":
            # fp32-class arithmetic on the f16 matrix cores: every algorithmic MAC executes as three
            # f16 MFMA products (the f16 and bf16 dense peaks are equal), so peak/3 bounds it.
            out.update(kernel="conv3x3_f16x3_frag_kernel<0>",
                       kernel_family="conv3x3_f16x3_frag_kernel (11 of 15 launches) + conv2d_f16x3_dma2_kernel "
                                     "(stride-2, 1x1, deconv, fused head)",
                       peak=round(MFMA_BF16_PEAK_TFLOPS / 3, 1),
                       peak_basis="2500 TFLOP/s dense f16 MFMA / 3 f16 products per fp32-class MAC",
                       frac=round(3 * tf / MFMA_BF16_PEAK_TFLOPS, 4), mfma_products_per_mac=3,
                       executed_tflops=round(3 * tf, 1), f16_mfma_peak=MFMA_BF16_PEAK_TFLOPS,
                       fp32_mfma_peak=MFMA_F32_PEAK_TFLOPS,
                       vs_fp32_mfma_peak=round(tf / MFMA_F32_PEAK_TFLOPS, 3))
            if getattr(self, "dom", None):
                dms = sum(a.elapsed_time(b) for a, b, _ in self.dom)
                dtf = sum(f for _, _, f in self.dom) / (dms * 1e-3) / 1e12
                out.update(frac_family=out["frac"], achieved_family=out["achieved"],
                           frac_dominant=round(3 * dtf / MFMA_BF16_PEAK_TFLOPS, 4), achieved_dominant=round(dtf, 2),
                           dominant_launches=len(self.dom), dominant_avg_launch_us=round(dms * 1e3 / len(self.dom), 2),
                           frac_note="frac / achieved = the 15-launch neck+head family (all dense flops / the region's time); "
                                     "frac_dominant / achieved_dominant = conv3x3_f16x3_frag_kernel<0> alone (its own "
                                     "launches' flops / its own launches' HIP-event time)")
        elif D.MATH == "bf16x6":
            # fp32-faithful arithmetic on the bf16 matrix cores: every algorithmic MAC executes as
            # six bf16 MFMA products, so the bf16 peak bounds the *executed* rate.
            out.update(kernel="conv3x3_bf16x6_halo_kernel",
                       kernel_family="conv3x3_bf16x6_halo_kernel (11 of 15 launches) + conv2d_bf16x6_kernel "
                                     "(stride-2, 1x1, deconv, fused head)",
                       peak=round(MFMA_BF16_PEAK_TFLOPS / 6, 1),
                       peak_basis="2500 TFLOP/s dense bf16 MFMA / 6 bf16 products per fp32-faithful MAC",
                       frac=round(6 * tf / MFMA_BF16_PEAK_TFLOPS, 4), mfma_products_per_mac=6,
                       executed_tflops=round(6 * tf, 1), bf16_mfma_peak=MFMA_BF16_PEAK_TFLOPS,
                       fp32_mfma_peak=MFMA_F32_PEAK_TFLOPS,
                       vs_fp32_mfma_peak=round(tf / MFMA_F32_PEAK_TFLOPS, 3))
        else:
            out.update(kernel="conv2d_mfma_kernel", peak=MFMA_F32_PEAK_TFLOPS,
                       frac=round(tf / MFMA_F32_PEAK_TFLOPS, 4))
        for pmc in ("r05_pmc_hbm_traffic.json", "r04_pmc_hbm_traffic.json", "r03_pmc_hbm_traffic.json", "r02_pmc_hbm_traffic.json",
                    "r01_pmc_hbm_traffic.json"):
            pmc = os.path.join(ROOT, "profiles", pmc)
            if not os.path.exists(pmc):      # PMC passes are separate runs (rocprofv3 --pmc); see DESIGN.md
                continue
            try:
                recs = json.load(open(pmc))
                # the counter file names the instantiation ("...<0, 2>"); the line names the family member ("...<0>")
                rec = recs.get(out["kernel"]) or next((v for k, v in recs.items() if k.startswith(out["kernel"][:-1] + ",")), None)
                if rec:
                    out["traffic"] = round(rec["hbm_mb_corrected"] * 1e6)
                    out["traffic_detail"] = {k: rec[k] for k in ("fetch_mb_raw", "fetch_mb_x2", "write_mb", "launches",
                                                                 "correction", "hbm_mb_fetch_as_counted", "hbm_mb_fetch_x2",
                                                                 "algorithmic_mb", "x2_applies", "ratio_as_counted",
                                                                 "ratio_x2", "fetch_factor", "loader_shape",
                                                                 "ratio_corrected") if k in rec}
                    out["traffic_note"] = rec.get("note", "") + " (" + os.path.basename(pmc) + ")"
                    break
            except Exception:
                pass
        return out


class SparseTimer:
    """HIP-event timing of every sparse-conv launch (the 21 layers of FPNSpMiddleResNetFHD,
    det3d/models/backbones/scn.py:331-369) on the stream it is launched on, plus the algorithmic
    work of each layer from the measured rulebook: pairs = valid (output row, tap)
    entries, flops = 2 * pairs * Cin * Cout, bytes = pairs * (Cin + Cout) * 4 + n_out * Cout * 4 +
    K * Cin * Cout * 4."""

    def __init__(self):
        self.enabled = False
        self.events = []            # (layer index within the batch, e0, e1)
        self.layers = None          # per layer: dict(cin, cout, K, n_out, pairs) of ONE batch
        self._i = 0

    def wrap(self, model):
        bb = model.backbone
        conv = bb._conv
        timer = self

        def timed(*a, **k):
            if not timer.enabled:
                return conv(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            conv(*a, **k)
            e1.record()
            timer.events.append((timer._i, e0, e1))
            timer._i += 1

        bb._conv = timed
        run = bb._run

        def run_wrapped(*a, **k):
            timer._i = 0
            return run(*a, **k)

        bb._run = run_wrapped

    def measure_rulebook(self, model, example):
        """Pairs per layer of one batch (outside the timed region)."""
        bb = model.backbone
        with torch.no_grad():
            book = bb.rulebook_for(example["coordinates"], len(example["num_voxels"]), example["shape"][0])
        layers, seen = [], {}
        n_prev = int(example["coordinates"].shape[0])
        for step, b in zip(bb._plan, book["steps"]):
            if step["kind"] == "stage_end":
                continue
            m = step["mod"]
            n_in, n_prev = (b["n"] if step["kind"] == "subm" else n_prev), b["n"]
            key = b["nbr"].data_ptr()
            if key not in seen:
                seen[key] = int((b["nbr"][:, :max(b["n"], 1)] >= 0).sum().item()) if b["n"] else 0
            layers.append(dict(cin=m.in_channels, cout=m.out_channels, K=b["K"], n_out=b["n"], n_in=n_in, pairs=seen[key],
                               kind=step["kind"], residual=bool(step.get("residual"))))
        self.layers = layers
        self.batch_frames = len(example["num_voxels"])

    def result(self):
        if not self.events or not self.layers:
            return None
        nl = len(self.layers)
        ms = [0.0] * nl
        cnt = [0] * nl
        for i, e0, e1 in self.events:
            ms[i % nl] += e0.elapsed_time(e1)
            cnt[i % nl] += 1
        rows, tot_flop, tot_bytes, tot_ms, tot_unique = [], 0.0, 0.0, 0.0, 0.0
        for L, t, c in zip(self.layers, ms, cnt):
            if c == 0:
                continue
            us = t * 1e3 / c
            flop = 2.0 * L["pairs"] * L["cin"] * L["cout"]
            byts = L["pairs"] * (L["cin"] + L["cout"]) * 4.0 + L["n_out"] * L["cout"] * 4.0 + \
                L["K"] * L["cin"] * L["cout"] * 4.0
            # bytes that must cross HBM once: input rows + output rows (+ residual rows) + weights
            uniq = (L["n_in"] * L["cin"] + L["n_out"] * L["cout"] * (2 if L["residual"] else 1)) * 4.0 + \
                L["K"] * L["cin"] * L["cout"] * 4.0
            tot_unique += uniq
            rows.append(dict(cin=L["cin"], cout=L["cout"], K=L["K"], n_out=L["n_out"], pairs=L["pairs"],
                             n_in=L["n_in"], valid=round(L["pairs"] / max(1, L["n_out"] * L["K"]), 3), avg_us=round(us, 1),
                             tflops=round(flop / us / 1e6, 1), gather_gbs=round(byts / us / 1e3, 1),
                             unique_mb=round(uniq / 1e6, 1), unique_gbs=round(uniq / us / 1e3, 1)))
            tot_flop += flop
            tot_bytes += byts
            tot_ms += us / 1e3
        tf = tot_flop / tot_ms / 1e9
        gbs = tot_bytes / tot_ms / 1e6
        from al3d import detector_ops as D
        prod = {"f16x3": 3, "bf16x6": 6}.get(D.MATH)
        peak = MFMA_BF16_PEAK_TFLOPS / prod if prod else MFMA_F32_PEAK_TFLOPS
        return dict(kernel="sp_conv family (21 launches per batch)", bound="hbm (gather) below 64 channels, mfma at 128",
                    frames_per_launch=self.batch_frames, ms_per_batch=round(tot_ms, 3),
                    ms_per_frame=round(tot_ms / self.batch_frames, 4),
                    algorithmic_gflop_per_frame=round(tot_flop / self.batch_frames / 1e9, 3),
                    algorithmic_mb_per_frame=round(tot_bytes / self.batch_frames / 1e6, 2),
                    achieved_tflops=round(tf, 1), mfma_peak_tflops=round(peak, 1), frac_mfma=round(tf / peak, 4),
                    hbm_peak_gbs=HBM_PEAK_GBS,
                    unique_mb_per_frame=round(tot_unique / self.batch_frames / 1e6, 2),
                    unique_gbs=round(tot_unique / tot_ms / 1e6, 1), frac_hbm=round(tot_unique / tot_ms / 1e6 / HBM_PEAK_GBS, 4),
                    gather_gbs=round(gbs, 1),
                    bytes_note="frac_hbm = unique bytes (input rows + output rows + residual rows + weights: what must cross "
                               "HBM once) / time / 8 TB/s.  gather_gbs is SURVEY 8d's per-layer formula, which prices every "
                               "gathered (row, tap) pair as memory traffic (a gather/GEMM/scatter formulation): gathers here "
                               "are L2 / LDS-DMA hits, so it is a gather rate, not HBM traffic, and is not divided by the "
                               "HBM peak",
                    measured="HIP events around each sparse-conv launch of the timed steps (rank 0); pairs from "
                             "the rulebook of one batch (every batch holds the same base frames)",
                    layers=rows)


def write_pool_files(tmp, infos, logs):
    ip = os.path.join(tmp, "infos.pkl")
    with open(ip, "wb") as f:
        pickle.dump(infos, f)
    lp = os.path.join(tmp, "log.json")
    with open(lp, "w") as f:
        json.dump(logs, f)
    bp = os.path.join(tmp, "buffer.json")
    with open(bp, "w") as f:
        json.dump({"0": []}, f)
    return ip, lp, bp


def from_files_leg(cfg, model, anchors, n_frames, batch, dev):
    """Sweep n_frames frames through FileSweepLoader from a synthetic on-disk pool (tools/write_synthetic_pool.py,
    written to tmpfs): frames/s of the sweep alone with file reads, H2D, merge and voxelization included."""
    import shutil
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from write_synthetic_pool import write_pool
    from al3d.datasets import FileSweepLoader
    from al3d.sweep import sweep_embeddings
    from al3d.datasets.file_loader import usable_cores
    root = tempfile.mkdtemp(prefix="al3d_pool_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        scenes = (n_frames + FRAMES_PER_SCENE - 1) // FRAMES_PER_SCENE
        infos, _ = write_pool(root, scenes, base=16)
        infos = infos[:n_frames]
        threads = max(2, min(12, usable_cores() - 2))
        loader = FileSweepLoader(infos, cfg.voxel_generator, anchors, batch_size=batch, device=dev, root=root,
                                 threads=threads, depth=2)
        sweep_embeddings(model, loader, dev, num_frames=len(infos))             # warm-up pass (pinned buffers, page cache)
        torch.cuda.synchronize()
        loader.bytes_read = 0
        t0 = time.perf_counter()
        emb = sweep_embeddings(model, loader, dev, num_frames=len(infos))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"frames_per_s": round(len(infos) / dt, 2), "frames": len(infos), "reader_threads": threads,
                "file_gb_per_s": round(loader.bytes_read / dt / 1e9, 2), "mb_per_frame": round(loader.bytes_read / len(infos) / 1e6, 2),
                "finite": bool(torch.isfinite(emb).all()),
                "what": "sweep only (no selection), 10 .bin files per frame on tmpfs -> reader pool -> pinned staging -> "
                        "H2D -> al3d_merge_sweeps_batch_f32 -> voxelizer -> detector, two-stream pipeline"}
    finally:
        shutil.rmtree(root, ignore_errors=True)


SWIN_T_GFLOP_PER_SAMPLE = 194.0   # 6 cameras of 256 x 704: token GEMMs 187 + window attention 7 (2*MAC)


def bevfusion_lidar_leg(dev, frames=96, batch=32):
    """BASELINE configs[3] on one GPU (pattern: bevfusion/tools/benchmark.py:52-84, warm-up then timed iterations):
    the BEVFusion lidar-only voxelnet_0p075 embedding sweep -- 0.075 m voxels, 1440 x 1440 x 41 grid, 160k-voxel cap --
    over a small resident synthetic pool; frames/s of the sweep (no selection)."""
    from al3d import sweep as S, synthetic
    from al3d.datasets import DeviceSweepLoader, PoolFrames
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_lidar_spatial_temporal_feature.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    model = model.to(dev).eval()
    pool = PoolFrames.from_synthetic(frames, dev, num_base=8, seed=1)
    loader = DeviceSweepLoader(pool, cfg.voxel_generator, None, batch, device=dev)
    ex = next(iter(loader))
    voxels = float(ex["num_voxels"].float().mean())
    del ex
    S.sweep_embeddings(model, loader, dev, frames)                     # warm-up: weight packing, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    emb = S.sweep_embeddings(model, loader, dev, frames)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"value": round(frames / dt, 2), "unit": "frames/s", "frames": frames, "batch": batch,
            "voxels_per_frame": round(voxels), "finite": bool(torch.isfinite(emb).all()),
            "what": "BEVFusion lidar-only voxelnet_0p075 embedding sweep (sparse encoder -> SECOND/SECONDFPN -> GAP), "
                    "synthetic frames resident in HBM, AL3D_PIPELINE as the headline"}


def bevfusion_camera_lidar_from_files(cfg, model, frames, batch, dev):
    """The same sweep fed from an mmdet3d-format pool on tmpfs (tools/write_synthetic_pool.py --cameras: ten .bin files and
    six 1600 x 900 JPEGs per sample): reader pool + BEVFusion merge rule + range filter + voxelizer for the lidar side; split
    JPEG decoding (entropy decoding on host threads, the rest on the device) + device resize / crop / normalise (PIL's bicubic
    as an integer kernel) for the cameras."""
    import shutil
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from write_synthetic_pool import write_camera_lidar_pool
    from al3d.datasets import CameraLidarFileLoader
    from al3d.datasets.file_loader import usable_cores
    from al3d.sweep import sweep_embeddings
    root = tempfile.mkdtemp(prefix="al3d_campool_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        scenes = (frames + FRAMES_PER_SCENE - 1) // FRAMES_PER_SCENE
        infos, _ = write_camera_lidar_pool(root, scenes, base=2)
        infos = infos[:frames]
        loader = CameraLidarFileLoader(infos, cfg.voxel_generator, None, batch_size=batch, device=dev, root=root,
                                       threads=max(2, min(8, usable_cores() // 4)))
        sweep_embeddings(model, loader, dev, num_frames=len(infos))             # warm-up (page cache, pinned buffers)
        torch.cuda.synchronize()
        loader.images_decoded = 0
        t0 = time.perf_counter()
        emb = sweep_embeddings(model, loader, dev, num_frames=len(infos))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return {"frames_per_s": round(len(infos) / dt, 2), "frames": len(infos), "images_per_s": round(loader.images_decoded / dt, 1),
                "decode_threads": loader._pool._max_workers, "finite": bool(torch.isfinite(emb).all()),
                "images_split_decoded": int(getattr(loader, "images_split", 0)),
                "what": "sweep only; per sample 10 lidar .bin files + 6 JPEG frames of 1600 x 900 on tmpfs; split JPEG "
                        "decoding: Huffman entropy decoding on host threads, IDCT / upsampling / colour conversion on the "
                        "device (byte-identical to Pillow; 113 frames/s with Pillow decoding everything in round 4)"}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def bevfusion_camera_lidar_leg(dev, frames=48, batch=16):
    """BASELINE configs[4] on one GPU: the registered ``BEVFusion`` detector (Swin-T -> LSS-FPN -> depth LSS view transform;
    sparse lidar encoder; ConvFuser; SECOND/SECONDFPN decoder; 512-d fused-BEV embedding; examples/active/
    bevfusion_camera_lidar_spatial_temporal_feature.py) swept by ``sweep_embeddings`` over ``CameraLidarSweepLoader`` batches
    of synthetic inputs of the configured shapes (6 cameras of 256 x 704, 0.075 m voxels) with seeded weights: frames/s of
    the embedding sweep, per-stage ms per sample (HIP events, one extra forward), the Swin-T stage against the f16x3 roof."""
    from al3d import sweep as S, synthetic
    from al3d.datasets import CameraLidarSweepLoader, PoolFrames
    from al3d.models import build_detector
    from al3d.utils import Config
    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "bevfusion_camera_lidar_spatial_temporal_feature.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model.lidar, seed=0)
    for i, m in enumerate((model.camera_backbone, model.camera_neck, model.vtransform, model.fuser)):
        synthetic.seed_modules_(m, 30 + i)
    model = model.to(dev).eval()
    pool = PoolFrames.from_synthetic(frames, dev, num_base=min(frames, 4), seed=1)
    loader = CameraLidarSweepLoader(pool, cfg.voxel_generator, None, batch, device=dev)
    S.sweep_embeddings(model, loader, dev, frames)                     # warm-up: weight packing, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    emb = S.sweep_embeddings(model, loader, dev, frames)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ex = next(iter(loader))
    with torch.no_grad():
        model._run(ex, ex["img"], ex["points"], ex["lidar2image"], ex["camera_intrinsics"], ex["camera2lidar"],
                   ex["img_aug_matrix"], ex["lidar_aug_matrix"], timed=True)
    stage = {k: round(v / batch, 3) for k, v in model.stage_ms.items()}
    swin_ms = stage.get("camera backbone (Swin-T)", 0.0)
    roof = None
    if swin_ms > 0:
        ach = SWIN_T_GFLOP_PER_SAMPLE / swin_ms                       # GFLOP / ms = TFLOP/s
        peak = MFMA_BF16_PEAK_TFLOPS / 3.0
        roof = {"stage": "camera backbone (Swin-T)", "bound": "mfma", "achieved": round(ach, 1), "peak": round(peak, 1),
                "unit": "TFLOP/s", "frac": round(ach / peak, 3),
                "note": "algorithmic flops (194 GFLOP per sample) / stage time from HIP events; peak = dense f16 MFMA "
                        "2.5 PFLOP/s / 3 products per MAC (f16x3); stages 0-1 run fused attention / MLP halves (VALU-issue bound), "
                        "stages 2-3 token GEMMs with K = 384 / 768"}
    try:
        files = bevfusion_camera_lidar_from_files(cfg, model, frames, batch, dev)
    except Exception as e:                                              # the figure is auxiliary: never fail the line
        files = {"error": repr(e)}
    return {"value": round(frames / dt, 2), "unit": "frames/s", "frames": frames, "batch": batch, "ms_per_sample": stage,
            "voxels_per_frame": round(float(ex["num_voxels"].float().mean())), "finite": bool(torch.isfinite(emb).all()),
            "roofline": roof, "from_files": files,
            "what": "BEVFusion camera+lidar swint_v0p075 convfuser: fused-BEV embedding sweep (sweep_embeddings over "
                    "CameraLidarSweepLoader), synthetic inputs, seeded weights, no detection head; every stage on this "
                    "build's HIP kernels"}


def cpu_baseline(cfg, model_cpu_state, infos, feats, sample_frames=8):
    """Oracle (CPU port) timed on the host: a bounded sample of the same workload.
    sweep: `sample_frames` synthetic frames through oracle voxelize + oracle sparse encoder +
    torch-CPU dense neck/head + oracle NMS; selection: the oracle selector on the full pool
    metadata with the device embeddings.  Reported as pool-frames / (N * t_frame + t_select)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    oracle.build()
    import cpu_port
    return cpu_port.run(cfg, model_cpu_state, infos, feats, sample_frames)


def main():
    args = parse()
    launch_or_refuse(args)              # before anything touches the GPU
    if args.launch_check:
        launch_check(args)
    global BUDGET
    if os.environ.get("AL3D_STACKDUMP_AFTER"):
        # diagnosis aid for runs under a profiler (a counter pass of round 3 hung under the two-stream pipeline and left no
        # trace of where): every N seconds the Python stacks of all threads go to stderr, so a stuck pass shows its wait
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["AL3D_STACKDUMP_AFTER"]), repeat=True, file=sys.stderr)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.scenes is None:
        args.scenes = SCENES_PER_RANK if world == 1 else SCENES_PER_RANK_MULTI
    if args.budget is not None:
        BUDGET = args.budget
    elif world > 1 and args.scenes * world >= SCENES_PER_RANK:
        BUDGET = BUDGET_MULTI
    elif args.scenes * world < SCENES_PER_RANK:
        BUDGET = max(10, BUDGET * args.scenes * world // SCENES_PER_RANK)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # Rehearsal knob: AL3D_DIST_BACKEND=gloo lets several ranks share cuda:0 of a one-GPU box (device
    # tensors over gloo) to exercise the N>1 control flow; the real runs use RCCL, one GPU per rank.
    backend = os.environ.get("AL3D_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local = 0
    if world > 1:
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", init_method="env://",
                                    device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend, init_method="env://")
    assert torch.cuda.is_available(), "bench.py needs a ROCm device"
    dev = torch.device("cuda", local if world > 1 else 0)
    torch.cuda.set_device(dev)

    from al3d import synthetic
    from al3d.datasets import DeviceSweepLoader, PoolFrames, generate_task_anchors
    from al3d.models import build_detector
    from al3d.selectors import build_selector
    from al3d.utils import Config

    cfg = Config.fromfile(os.path.join(ROOT, "examples", "active", "cbgs_spatial_temporal_feature.py"))
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    synthetic.seeded_init_(model, seed=0)
    cpu_state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev).eval()
    timer = ConvTimer()
    timer.wrap(model)
    sp_timer = SparseTimer()
    sp_timer.wrap(model)
    anchors = generate_task_anchors(cfg.tasks, cfg.target_assigner.anchor_generators, [1, 128, 128])

    per_rank = args.scenes * FRAMES_PER_SCENE
    n_total = per_rank * world
    infos, logs = synthetic.make_pool(args.scenes * world, seed=0)
    # every rank holds its contiguous shard of the pool in HBM (seeded per rank)
    pool = PoolFrames.from_synthetic(per_rank, dev, num_base=16, seed=1000 + rank)
    my_index = list(range(rank * per_rank, (rank + 1) * per_rank))

    class ShardLoader(DeviceSweepLoader):
        """Local frame j is dataset frame my_index[j] (contiguous block per rank)."""
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.sampler = my_index

    loader = ShardLoader(pool, cfg.voxel_generator, anchors, batch_size=args.batch, device=dev)
    tmp = tempfile.mkdtemp(prefix="al3d_bench_")
    ip, lp, bp = write_pool_files(tmp, infos, logs)
    sel_cfg = dict(cfg.selector)
    sel_cfg.update(budget=BUDGET, buffer_file=bp, infos_origin=ip, logs_file=lp, buffer_path="",
                   distance_store_file=None, pred=True)

    state = {}

    def step():
        random.seed(3407)                       # tools/active_select.py:76-80 of the reference
        sel = build_selector(dict(sel_cfg, detector=model, dataloader=loader))
        t0 = time.perf_counter()
        feats = sel.buffer_pred(local_rank=dev.index)
        sel.pred = False
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sel._features = lambda device, kwargs: feats      # reuse the swept embeddings
        sel.select_samples(local_rank=dev.index)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        state.update(feats=feats, selected=sel.selected_index[sel.current_budget],
                     sweep_s=t1 - t0, select_s=t2 - t1)

    for _ in range(args.warmup):
        step()
    ranks_seen = 1
    if world > 1:
        # RCCL sanity before the timed region: an all-reduce of ones must count every rank
        ones = torch.ones(1, dtype=torch.int64, device=dev)
        dist.all_reduce(ones)
        ranks_seen = int(ones.item())
        dist.barrier()
    if ranks_seen != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the all-reduce counted {ranks_seen} rank(s)")
    torch.cuda.synchronize()
    timer.enabled = sp_timer.enabled = rank == 0
    t0 = time.perf_counter()
    sweep_s = select_s = 0.0
    for _ in range(args.steps):
        step()
        sweep_s += state["sweep_s"]
        select_s += state["select_s"]
        if os.environ.get("AL3D_BENCH_MEM") == "1" and rank == 0:      # dev aid: allocator growth per step
            print(f"[mem] reserved {torch.cuda.memory_reserved() / 2**30:.1f} GiB, allocated "
                  f"{torch.cuda.memory_allocated() / 2**30:.1f} GiB", file=sys.stderr)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    timer.enabled = sp_timer.enabled = False
    rank_sweep_s = [sweep_s / args.steps]
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        mine = torch.tensor([sweep_s / args.steps], dtype=torch.float64, device=dev)
        allt = torch.empty(world, dtype=torch.float64, device=dev)
        dist.all_gather_into_tensor(allt, mine)
        rank_sweep_s = [round(float(v), 4) for v in allt.tolist()]

    if rank == 0:
        value = n_total * args.steps / elapsed
        verified = None if args.no_verify else verify_selection(infos, state["feats"], state["selected"])
        first_selected = list(state["selected"])
        first_feats = state["feats"]
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, first_feats, first_selected)
        out = {
            "metric": "unlabeled frames scored+selected/sec (whole node; 40 frames = 1 scene); "
                      + {True: "selected set equals the CPU oracle's", False: "SELECTED SET DIFFERS FROM THE CPU ORACLE",
                         None: "selection not verified (--no-verify)"}[verified],
            "value": round(value, 2), "unit": "frames/s", "scenes_per_s": round(value / FRAMES_PER_SCENE, 3),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 2), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": _DTYPE[_math()],
            "data": "synthetic",
            "config": {"workload": f"{args.scenes * world}-scene nuScenes-shaped pool ({n_total} frames, "
                                   f"10-sweep ~250k-point clouds resident in HBM), FPNVoxelNet sweep + "
                                   f"SpatialTemporalFeatureSelector budget {BUDGET} "
                                   + ("(BASELINE configs[1])" if world == 1 and args.scenes == SCENES_PER_RANK else
                                      f"(BASELINE configs[2] shape: {args.scenes} scenes per rank x {world} ranks"
                                      + ("= the full pool)" if args.scenes * world == 704 else ")")),
                       "frames_per_rank": per_rank, "batch": args.batch,
                       "weights": "seeded random-init (al3d.synthetic.seeded_init_, seed 0)"},
            "breakdown_s_per_step": {"sweep+allgather": round(sweep_s / args.steps, 4),
                                     "select": round(select_s / args.steps, 4)},
            "selected_frames": len(state["selected"]),
            "ranks_seen": ranks_seen, "sweep_s_per_rank": rank_sweep_s,
        }
        roof = timer.result()
        if roof:
            from al3d import sweep as _sweep
            roof["measured"] = ("HIP events around every neck+head region of the timed steps"
                                + {"split": "; the sparse half of the next batch runs concurrently on a second stream "
                                            "(AL3D_PIPELINE=split), so these durations include that contention",
                                   "ahead": "; the next batch's voxelization + rulebook (small latency-bound kernels) "
                                            "run on a second stream meanwhile"}.get(_sweep.PIPELINE, ""))
            out["roofline"] = roof
        try:
            sp_timer.measure_rulebook(model, next(iter(loader)))
            roof_sp = sp_timer.result()
            if roof_sp:
                out["roofline_sparse"] = roof_sp
        except Exception as e:           # a report, never a reason to lose the line
            out["roofline_sparse"] = {"error": repr(e)}
        if verified is not None:
            out["selected_equals_oracle"] = verified
        if world == 1 and not args.no_extra_math and _math() == "f16x3":
            # the strict-range arithmetic (full fp32 exponent range, six bf16 products per MAC) on the same
            # workload: one extra step outside the timed region, so the driver record carries both
            try:
                from al3d import detector_ops as D
                D.MATH = "bf16x6"
                step()                                  # re-packs the weights (untimed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                out["value_bf16x6"] = round(n_total / dt, 2)
                out["value_bf16x6_note"] = ("frames/s of one step under AL3D_MATH=bf16x6 (exact 3-way bf16 split, "
                                            "6 MFMA products per MAC, full fp32 range), same workload, same process")
                # the selection is a discrete function of tolerance-bound embeddings: report how far the two
                # arithmetics' picks agree (identical prefix + set overlap), not just a yes/no
                other = list(state["selected"])
                same_prefix = next((i for i, (a, b) in enumerate(zip(first_selected, other)) if a != b),
                                   min(len(other), len(first_selected)))
                out["selection_f16x3_vs_bf16x6"] = {
                    "identical": bool(other == first_selected), "identical_prefix": same_prefix,
                    "common": len(set(other) & set(first_selected)), "of": len(first_selected),
                    "max_abs_embedding_diff": float((state["feats"] - first_feats).abs().max())}
            except Exception as e:
                out["value_bf16x6"] = {"error": repr(e)}
            finally:
                D.MATH = "f16x3"
        if world == 1 and not args.no_from_files:
            # I/O-inclusive sweep: the same number of frames read from .bin files (tmpfs) by the native reader pool,
            # merged + voxelized on device one batch ahead of the detector.  Reported next to
            # `value`, never as `value` (the headline keeps its inputs resident in HBM).
            try:
                out["value_from_files"] = from_files_leg(cfg, model, anchors, per_rank, args.batch, dev)
            except Exception as e:
                out["value_from_files"] = {"error": repr(e)}
        if world == 1 and not args.no_bevfusion:
            # BASELINE configs[3] / configs[4] on the same GPU, outside the timed region (N = 1 only)
            for key, leg in (("value_bevfusion_lidar", bevfusion_lidar_leg),
                             ("value_bevfusion_camera_lidar", bevfusion_camera_lidar_leg)):
                try:
                    torch.cuda.empty_cache()
                    out[key] = leg(dev)
                except Exception as e:
                    out[key] = {"error": repr(e)}
        if world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(cfg, cpu_state, infos, first_feats.cpu().numpy())
            except Exception as e:       # the baseline is a report, never a reason to lose the line
                out["cpu_baseline"] = {"error": repr(e)}
        print(json.dumps(order_line(out)))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def order_line(out):
    """The driver keeps the first ~2,000 characters of the line: contract keys, the parity verdict, the strict-range
    and from-files numbers, the roofline's and the CPU baseline's numbers go first; prose and per-layer tables after."""
    head = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "selected_equals_oracle", "ranks_seen", "value_bf16x6"]
    line = {k: out[k] for k in head if k in out}
    ff = out.get("value_from_files")
    if isinstance(ff, dict):
        line["value_from_files"] = ff.get("frames_per_s", ff)
    for key in ("value_bevfusion_lidar", "value_bevfusion_camera_lidar"):
        leg = out.get(key)
        if isinstance(leg, dict) and "value" in leg:
            line[key + "_fps"] = leg["value"]
            if isinstance(leg.get("from_files"), dict):
                line[key + "_from_files_fps"] = leg["from_files"].get("frames_per_s")
    roof = out.get("roofline")
    if isinstance(roof, dict):
        first = ["bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "frac_dominant", "achieved_dominant",
                 "dominant_avg_launch_us", "avg_launch_us", "launches"]
        line["roofline"] = {k: roof[k] for k in first if k in roof}
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        line["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "sample") if k in cb} or cb
    sp = out.get("roofline_sparse")
    if isinstance(sp, dict) and "ms_per_batch" in sp:
        line["sparse_ms_per_batch"] = sp["ms_per_batch"]
        line["sparse_frac_mfma"] = sp.get("frac_mfma")
    line["config"] = out.get("config")
    if isinstance(roof, dict):
        line["roofline_detail"] = {k: v for k, v in roof.items() if k not in line["roofline"]}
    if isinstance(cb, dict):
        rest = {k: v for k, v in cb.items() if k not in line["cpu_baseline"]}
        if rest:
            line["cpu_baseline_detail"] = rest
    for k, v in out.items():
        if k not in line and k not in ("roofline", "cpu_baseline"):
            line[k] = v
    return line


_DTYPE = {
    "f32": "f32",
    "bf16x6": "f32 (exact 3-way bf16 split, 6 MFMA products per MAC, f32 accumulate)",
    "f16x3": "f32 (2-way f16 split of every operand, 3 MFMA products per MAC, f32 accumulate; sparse "
             "encoder, dense neck and head)",
}


def _math():
    from al3d import detector_ops as D
    return D.MATH


def verify_selection(infos, feats, selected):
    """Checker (not timed, rank 0 only, no collectives): the oracle selector must pick the same
    frames.  Pools up to 6,000 frames are recomputed end to end on the CPU; above that the O(N^2 C)
    oracle maps are too slow, so 48 sampled rows of every device map are compared bit for bit
    with oracle rows and the oracle's greedy loop runs on the (host copy of the) device map."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    oracle.build()
    from al3d import selector_ops as ops, synthetic
    cfgm, run_id, n_boxes = synthetic.pool_arrays(infos)
    n = len(infos)
    xy = np.stack([(-(c[:3, 3].T @ c[:3, :3]))[:2] for c in cfgm])
    random.seed(3407)
    first = random.choice(range(n))
    box = np.array([int(b) * 0.04 for b in n_boxes], dtype=np.float64)
    if n <= 6000:
        F = oracle.l1_map_f32(feats.cpu().numpy(), 2)
        S = oracle.spatial_map(xy, 8)
        D = oracle.combine(n, spatial=S, temporal_id=run_id, feat=F, normalize="exp", aggregate="sum",
                           lambda_t=1.0, lambda_f=1.0)
        rc, picks = oracle.greedy(D, [], first, box, 0.12, 0.0, float(BUDGET))
        return bool(rc == 0 and picks.tolist() == list(selected))
    dev = feats.device
    d, i = ops.knn_2d(torch.from_numpy(xy).to(dev), 9)
    S = ops.apsp_knn(d, i)
    F = ops.l1_distance(feats, 2, shard=False)        # rank-0-only checker: no collectives
    D = ops.combine_maps(n, spatial=S, temporal_id=torch.from_numpy(run_id).to(dev), feat=F,
                         normalize="exp", aggregate="sum", lambda_t=1.0, lambda_f=1.0)
    rows = np.unique(np.linspace(0, n - 1, 48).astype(np.int64))
    kd, ki = oracle.knn(xy, 9)
    indptr, indices, w = oracle.knn_csr(kd, ki)
    fnp = feats.cpu().numpy()
    ok = True
    for r in rows:
        s_row = oracle.apsp(indptr, indices, w, int(r), int(r) + 1)[0]
        f_row = np.zeros(n, dtype=np.float32)
        acc = np.zeros(n, dtype=np.float32)
        for c in range(fnp.shape[1]):                      # canonical order c = 0..C-1, float32
            acc += np.abs(fnp[:, c] - fnp[r, c])
        f_row = acc
        ok &= np.array_equal(S[r].cpu().numpy().view(np.int64), s_row.view(np.int64))
        ok &= np.array_equal(F[r].cpu().numpy().view(np.int32), f_row.view(np.int32))
        # combined map row: the oracle's row-block combine on the oracle rows
        d_row = oracle.combine_rows(n, int(r), spatial_rows=s_row[None], temporal_id=run_id, feat_rows=f_row[None],
                                    normalize="exp", aggregate="sum", lambda_t=1.0, lambda_f=1.0)[0]
        ok &= np.array_equal(D[r].cpu().numpy().view(np.int64), d_row.view(np.int64))
    Dh = D.cpu().numpy()
    del S, F, D
    rc, picks = oracle.greedy(Dh, [], first, box, 0.12, 0.0, float(BUDGET))
    return bool(ok and rc == 0 and picks.tolist() == list(selected))


if __name__ == "__main__":
    main()
