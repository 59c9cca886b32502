#!/usr/bin/env python3
"""bench.py -- training images/sec of PackNet-SAN + depth-edge loss at 384x1280, bf16 compute, on N MI355X.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = zero_grad + forward (dropout 0.5, random whole-batch flip) + silog/edge loss + backward + bucketed RCCL
gradient all-reduce (N > 1) + fused Adam, on a synthetic batch of 8 frames per GPU that is already resident in HBM
(SURVEY.md 8(d) recipe).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line (value, ms_per_step, ...).  The backward pass adds a few
weight-gradient tails with fp32 atomics, so the parameters drift apart from run to run; the last timed step therefore starts
from the initial parameters and random-number state (restored in place, as the optimizer writes parameters), and what it
computes is the same in every run with the same arguments.  --dump-outputs DIR writes that step's outputs (loss terms,
inverse-depth maps) as DIR/<name>.npy.

--full adds the measurements that take runs of their own: "roofline" for the dominant kernel family (MFMA implicit-GEMM
convolutions; algorithmic FLOPs / HIP-event time of every launch), "roofline_hbm": the same for the HBM-bound GroupNorm+ELU family (algorithmic bytes / HIP-event time against 8 TB/s), the host's enqueue cost of unthrottled
steps, and, at N = 1, the all-reduce layout, "cpu_baseline": the CPU oracle (oracle/) timed on this box's host cores on a
bounded sample, and "parity" against that oracle.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The training step keeps two HIP streams busy (main chain + weight-gradient stream) and RCCL adds its own; ROCm maps streams
# onto GPU_MAX_HW_QUEUES hardware queues (default 4) and two streams that share one queue serialise -- measured: the
# weight-gradient overlap is lost (31 -> 37 ms/step) as soon as a process group exists.  Must be set before HIP initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2500.0     # MI355X_MICROARCH.md: ~2.5 PF dense bf16 MFMA
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8, help="frames per GPU")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--mode", choices=["train", "infer"], default="train")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=2)
    ap.add_argument("--dump-conv", type=str, default="", help="write per-launch conv timings (shape, ms, TFLOP/s) to this file (--full)")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--full", action="store_true",
                    help="also run the per-kernel timing, unthrottled host-enqueue steps, all-reduce layout, CPU baseline and parity check")
    args = ap.parse_args()
    if args.dump_conv and not (args.full and not args.no_kernel_timing):
        ap.error("--dump-conv needs the per-kernel timing of --full")
    return args


DUMP_BUDGET_ELEMS = 60 * 2**20 // 4                # --dump-outputs: float32 elements in all (under 64 MB with the .npy headers)


def _output_arrays(out, prefix=""):
    """name -> tensor for every tensor in a step's output (nested dicts / lists flattened: inv_depths_0, metrics_edge_loss, ...)"""
    items = out.items() if isinstance(out, dict) else enumerate(out) if isinstance(out, (list, tuple)) else ()
    res = {}
    for k, v in items:
        name = "%s%s" % (prefix, k)
        if torch.is_tensor(v):
            res[name] = v
        elif isinstance(v, (dict, list, tuple)):
            res.update(_output_arrays(v, name + "_"))
    return res


def snapshot_outputs(out):
    """Host copies (float32) of the step's outputs, right after the timed steps: later work (the --full passes) runs more
    steps and may reuse the device buffers."""
    return {k: v.detach().float().cpu().numpy().reshape(v.shape) for k, v in _output_arrays(out).items()}


def dump_outputs(arrays, path):
    """Writes each array as path/<name>.npy.  Arrays are kept whole while they fit the 64 MB budget; what does not fit is
    reduced to a fixed sample (seeded, the same element indices on every run of the same arguments), stored 1-D."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    left, names = DUMP_BUDGET_ELEMS, sorted(arrays, key=lambda k: (arrays[k].size, k))
    for i, name in enumerate(names):
        a = np.asarray(arrays[name], dtype=np.float32)
        cap = left // (len(names) - i)
        if a.size > cap:
            idx = np.sort(np.random.default_rng(20240611).choice(a.size, cap, replace=False))
            a = a.reshape(-1)[idx]
        left -= a.size
        np.save(os.path.join(path, name + ".npy"), a)


class ConvTimer:
    """HIP-event bracket around every conv launch (events are recorded on the stream the kernels run on)."""

    def __init__(self, K):
        self.K, self.records, self.enabled = K, [], False
        lib = K.lib
        self._orig = {}
        # (round 5: + the two LDS-patch forward entry points of round 4's late steps -- iconv1 / iconv2 with the rank-1 term inside, the 3x3 data
        #  gradient that carries the 1x1 shortcut's -- which the round-4 line left out of the family: ~0.5 ms of conv kernels per step)
        for name in ("mte_conv2d_igemm", "mte_conv2d_wgrad", "mte_conv2d_patch_fwd", "mte_conv2d_patch_wgrad",
                     "mte_conv2d_stem_fwd", "mte_conv2d_stem_wgrad", "mte_conv2d_patch_fwd_rank1", "mte_conv2d_patch_fwd_plus1x1"):
            self._orig[name] = getattr(lib, name)
        self._optional = ("mte_gn_tail_fwd", "mte_gn_stats_from_records", "mte_conv2d_patch_fwd_gn", "mte_conv2d_igemm_unshuffle")   # (entry points an older build of the library lacks: same-box A/B of two libraries with ONE bench.py)
        for name in ("mte_conv2d_patch_fwd_gn", "mte_conv2d_igemm_unshuffle"):   # round 5 / round 6 (the folded pack layers' data gradient without the shuffle pass behind it); round 5: LDS-patch launches that also leave GroupNorm records
            try:
                self._orig[name] = getattr(lib, name)
            except AttributeError:
                pass
        self.untimed = {}               # mte_conv2d_* launches seen during the conv timing pass that are NOT in the family (a new entry point someone forgot here)
        self.hbm_records = []           # (name, e0, e1, algorithmic bytes) of the GroupNorm+ELU passes (HBM-bound family)
        for name in ("mte_gn_stats", "mte_gn_elu_fwd", "mte_gn_elu_bwd", "mte_gn_tail_fwd", "mte_gn_stats_from_records"):
            try:
                self._orig[name] = getattr(lib, name)
            except AttributeError:
                if name not in self._optional:
                    raise
        self.loss_records = []          # the fused depth-edge loss stencils ("reported as HBM GB/s vs 8.0 TB/s")
        for name in ("mte_edge_loss_fwd", "mte_edge_loss_bwd", "mte_edge_loss_multi_fwd", "mte_edge_loss_multi_bwd"):
            self._orig[name] = getattr(lib, name)

    def install(self):
        K = self.K
        outer = self

        class Proxy:
            def __getattr__(self_, name):
                fn = getattr(outer._lib, name)
                hbm_family = name.startswith("mte_gn_") or name.startswith("mte_edge_loss_")
                if name.startswith("mte_conv2d_") and name not in outer._orig and outer.enabled == "conv" and not name.endswith(("_supported", "_ok", "_elems", "_repack", "_nine_tap")):
                    def counted(*args):
                        outer.untimed[name] = outer.untimed.get(name, 0) + 1
                        return fn(*args)
                    return counted
                if name not in outer._orig or not outer.enabled or hbm_family != (outer.enabled == "hbm"):
                    return fn

                def timed(*args):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(*args)
                    e1.record()
                    if name.startswith("mte_edge_loss_multi_"):
                        # (scales, nscales, B, ...): ONE launch for all scales; fwd reads pred + edge + normal (12 B/px), bwd the same +
                        # the gradient write (16 B/px); the fused silog adds the ground-truth depth read of scale 0 (4 B/px)
                        import ctypes as _ct
                        S_, B_ = args[1], args[2]
                        sc_ = (outer.K._EdgeScale * S_).from_address(args[0])
                        fwd_ = name.endswith("_fwd")
                        px_ = sum(B_ * s_.H * s_.W for s_ in sc_)
                        maps_ = 2 + bool(sc_[0].normal) + bool(sc_[0].mask) + (0 if fwd_ else 1)
                        gt_ = args[9] if fwd_ else args[10]
                        outer.loss_records.append((name, e0, e1, 4.0 * maps_ * px_ + (4.0 * B_ * sc_[0].H * sc_[0].W if gt_ else 0.0)))
                        return
                    if name.startswith("mte_edge_loss_"):
                        # fwd (pred, edge, normal, mask, sums, gmap, B, H, W, ...): reads pred + edge (+ normal, + mask) = 4 B each;
                        # bwd (pred, edge, normal, mask, coef, gout, dpred, B, H, W, ...): the same reads + 4 B gradient write
                        fwd_ = name.endswith("_fwd")
                        B_, H_, W_ = args[6:9] if fwd_ else args[7:10]
                        maps = 2 + bool(args[2]) + bool(args[3]) + (0 if fwd_ else 1)
                        outer.loss_records.append((name, e0, e1, 4.0 * maps * B_ * H_ * W_))
                        return
                    if name.startswith("mte_gn_"):
                        # algorithmic bytes: every tensor the pass must touch once (2 B/element in bf16)
                        if name == "mte_gn_stats_from_records":   # (rec, tiles_per_sample, stats, B, stream): reads the records
                            outer.hbm_records.append((name, e0, e1, 128.0 * args[1] * args[3]))
                            return
                        if name == "mte_gn_tail_fwd":       # (y1, ld1, stats1, gamma1, beta1, y2, ld2, scale2, t, ldt, stats_t, gamma_t, beta_t, z, ldz, B, HW, C, eps, dtype, stream)
                            (B_, HW_, C_), dt_ = args[15:18], args[19]
                            tensors = 5                                         # read y1, y2, write t; read t, write z
                        elif name == "mte_gn_stats":        # (y1, ld1, y2, ld2, scale2, stats, B, HW, C, dtype, stream)
                            has2, (B_, HW_, C_, dt_) = bool(args[2]), args[6:10]
                            tensors = 1 + has2                                  # read y1 (+ y2)
                        elif name == "mte_gn_elu_fwd":      # (y1, ld1, y2, ld2, scale2, stats, stats_ready, gamma, beta, z, ldz, B, HW, C, eps, dtype, stream)
                            has2, (B_, HW_, C_), dt_ = bool(args[2]), args[11:14], args[15]
                            tensors = 1 + has2 + 1                              # read y1 (+ y2), write z
                        else:                               # (dz, lddz, y1, ld1, y2, ld2, scale2, stats, gamma, beta, red, d1, ldd1, d2, ldd2, ..., B, HW, C, eps, dtype, stream)
                            has2, hasd2, (B_, HW_, C_), dt_ = bool(args[4]), bool(args[13]), args[18:21], args[22]
                            tensors = 2 * (2 + has2) + 1 + hasd2                # reduce + apply each read dz, y1 (+ y2); write d1 (+ d2)
                        outer.hbm_records.append((name, e0, e1, float(tensors) * B_ * HW_ * C_ * (2 if dt_ == 0 else 4)))
                        return
                    if name == "mte_conv2d_patch_fwd_rank1":     # (x, ldx, w, bias, y, ldy, B, H, W, Cin_p, N, inv, w1, stride, stream): 3x3 (+ the map's 16-slot MFMA step)
                        shp = tuple(args[6:11]) + (3, 3)
                    elif name == "mte_conv2d_patch_fwd_plus1x1":  # (dy, lddy, w, bias, dx, lddx, B, H, W, Cin_p, N, dy3, lddy3, w3, C3, stream): 3x3 over Cin_p + 1x1 over C3 channels
                        B_, H_, W_, Ci_, N_ = args[6:11]
                        outer.records.append((name, e0, e1, 2.0 * B_ * H_ * W_ * N_ * (9 * Ci_ + args[14]), (B_, H_, W_, Ci_, N_, 3, 3)))
                        return
                    elif name == "mte_conv2d_igemm":
                        shp = args[7:14]           # (x, ldx, w, bias, y, ldy, out_f32, B, H, W, Cin_p, N, KH, KW, ...)
                    elif name == "mte_conv2d_igemm_unshuffle":
                        shp = args[5:12]           # (x, ldx, w, y, ldy, B, H, W, Cin_p, N, KH, KW, ...)
                    elif name in ("mte_conv2d_patch_fwd", "mte_conv2d_patch_fwd_gn"):
                        shp = args[6:13]           # (x, ldx, w, bias, y, ldy, B, H, W, Cin_p, N, KH, KW, ...)
                    elif name == "mte_conv2d_stem_fwd":
                        shp = args[6:9] + (8,) + args[9:12]      # (x, ldx, wf, bias, y, ldy, B, H, W, N, KH, KW, stream): 8 input channels
                    elif name == "mte_conv2d_stem_wgrad":
                        shp = args[7:10] + (8,) + args[10:13]    # (x, ldx, dy, lddy, dw, stage_parts, parts_out, B, H, W, N, KH, KW, stream)
                    else:
                        shp = args[7:14]           # (x, ldx, dy, lddy, dw, stage_parts, parts_out, B, H, W, Cin_p, N, KH, KW, ...)
                    B, H, W, Cin_p, N, KH, KW = shp
                    outer.records.append((name, e0, e1, 2.0 * B * H * W * Cin_p * N * KH * KW, tuple(shp)))
                return timed
        self._lib = K.lib
        K.lib = Proxy()

    def hbm_summary(self):
        t = sum(e0.elapsed_time(e1) for _, e0, e1, _ in self.hbm_records) * 1e-3
        return len(self.hbm_records), t, sum(r[3] for r in self.hbm_records)

    def loss_summary(self):
        t = sum(e0.elapsed_time(e1) for _, e0, e1, _ in self.loss_records) * 1e-3
        return len(self.loss_records), t, sum(r[3] for r in self.loss_records)

    def summary(self):
        out = {}
        for name, e0, e1, fl, _ in self.records:
            d = out.setdefault(name, [0, 0.0, 0.0])
            d[0] += 1
            d[1] += e0.elapsed_time(e1) * 1e-3
            d[2] += fl
        return out


def pmc_traffic_per_launch(args, B, H, W, launches_per_step, key="conv_family_MB_per_step"):
    """HBM-side bytes per launch of a kernel family: the family's bytes per step from the committed rocprofv3 PMC passes
    (FETCH_SIZE x2 + WRITE_SIZE, collected in separate runs by tools/pmc_traffic.sh as MI355X_MICROARCH.md prescribes; bench.py
    cannot read PMCs itself) divided by the launches per step THIS run counted -- the same launches `achieved` and
    `launches_per_step` are quoted over (the PMC side also sees the split-K finish kernels: round-3 verdict, item 10).
    Only reported for the workload the passes were taken on."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(path) or not launches_per_step:
        return None
    with open(path) as f:
        d = json.load(f)
    if (d.get("mode"), d.get("batch"), d.get("height"), d.get("width"), d.get("dtype")) != (args.mode, B, H, W, args.dtype):
        return None
    mb = d.get(key)
    # the figure is quoted only while THIS run counts the launches per step the PMC passes were taken with (round-4 advisor: a stale numerator
    # over a live denominator); older files without the count are not used
    rec = d.get(key.replace("_MB_per_step", "_api_launches_per_step"))
    if mb is None or rec is None or abs(rec - launches_per_step) > 0.51:
        return None
    return mb * 1e6 / launches_per_step


def conv_flops_per_image(H, W):
    """Algorithmic conv FLOPs per image forward (285.27 GMAC at 384x1280, scales with pixels)."""
    return 2.0 * 285.27e9 * (H * W) / (384.0 * 1280.0)


def conv2d_flops_per_image(H, W):
    """conv2d-only share (281.16 GMAC: total minus the 4.11 GMAC of the conv3d stencils, which are VALU kernels)."""
    return 2.0 * 281.16e9 * (H * W) / (384.0 * 1280.0)


def device_batch(B, H, W, seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device=device)
    batch = {"rgb": r(B, 3, H, W)}
    batch["depth"] = (r(B, 1, H, W) < 0.05).float() * (1.0 + 79.0 * r(B, 1, H, W))
    for s in range(4):
        sfx = "" if s == 0 else "_%d" % s
        h, w = H >> s, W >> s
        batch["edge" + sfx] = (r(B, 1, h, w) < 0.03).float() * r(B, 1, h, w)
        batch["normal" + sfx] = (r(B, 1, h, w) * 2 - 1) * math.pi
    return batch


def cpu_baseline(H, W, steps):
    """The CPU oracle (verified against the reference's golden vectors) timed on this host: B=1 training step,
    fp32, all physical cores."""
    from oracle import packnet_oracle as po, loss_oracle as lo
    try:
        import psutil
        cores = psutil.cpu_count(logical=False) or os.cpu_count()
    except Exception:
        cores = os.cpu_count()
    cores = min(cores, 128)
    torch.set_num_threads(cores)
    P = {k: v.clone().requires_grad_(True) for k, v in po.reference_init_params().items()}
    names = [k for k in P if k not in ("weight", "bias")]
    opt = torch.optim.Adam([P[k] for k in names], lr=1e-4)
    batch = lo.synthetic_batch(1, H, W, seed=0)
    times = []
    for it in range(steps + 1):
        t0 = time.perf_counter()
        opt.zero_grad()
        g = torch.Generator().manual_seed(it)
        keeps = {}
        for li, nb in zip((2, 3, 4, 5), po.NUM_BLOCKS):
            c = (po.N2, po.N3, po.N4, po.N5)[li - 2]
            for b in range(nb):
                keeps["encoder.conv%d.%d" % (li, b)] = (torch.rand(1, c, generator=g) >= 0.5).float() * 2.0
        inv = po.packnet_san01(batch["rgb"], P, training=True, channel_keeps=keeps)["inv_depths"]
        loss = lo.semisup_edge_model_loss(inv, batch)["loss"].sum()
        loss.backward()
        opt.step()
        times.append(time.perf_counter() - t0)
    t = sum(times[1:]) / max(1, len(times) - 1)
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    return {"value": 1.0 / t, "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": "%d timed B=1 %dx%d fp32 training steps (fwd+loss+bwd+Adam) of the CPU oracle after 1 warm-up; %s" % (steps, H, W, model)}


def parity_check(net, K, H, W):
    """Measured parity of the benchmarked arithmetic against the CPU oracle AT the benchmark resolution: one eval frame through
    the HIP path in bf16 (the timed mode) and in fp32 validation mode, same weights, element-wise relative error of the
    full-resolution inverse depth (|a - b| / max(|b|, rms b)).  north_star asks 1e-3: met in fp32 mode; bf16 STORAGE of ~60
    stacked conv/GroupNorm layers holds ~2e-3 mean / a few 1e-2 max per pixel (tests/test_gpu_oracle_fullsize.py)."""
    from oracle import packnet_oracle as po, loss_oracle as lo
    P = {k: v.detach().float().cpu() for k, v in net.state_dict().items()}
    rgb = lo.synthetic_batch(1, H, W, seed=77)["rgb"]
    with torch.no_grad():
        ref = po.packnet_san01(rgb, P, training=False)["inv_depths"][0][0].double()
    floor = float(ref.pow(2).mean().sqrt())
    out = {"frame": "1x3x%dx%d eval forward vs CPU oracle, weights of the benchmarked network" % (H, W)}
    was_training = net.training
    net.eval()
    try:
        for mode in ("bf16", "fp32"):
            K.set_compute_dtype(mode)
            with torch.no_grad():
                got = net(rgb.cuda())["inv_depths"][0][0].double().cpu()
            err = (got - ref).abs() / ref.abs().clamp(min=floor)
            out[mode] = {"inv_depth_max_elem_rel": float(err.max()), "inv_depth_mean_elem_rel": float(err.mean())}
    finally:
        net.train(was_training)
    return out


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # MTE_BENCH_DIST_SELFTEST=1 (development aid, under torch.distributed.run --nproc-per-node 1): take every multi-rank
    # code path -- RCCL init, barrier, broadcast, bucketed all-reduce in backward, MAX-reduce of the time -- with one rank
    dist_on = world > 1 or bool(os.environ.get("MTE_BENCH_DIST_SELFTEST"))
    if dist_on:
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    dev = torch.device("cuda", local_rank if world > 1 else 0)
    torch.cuda.set_device(dev)

    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "mindtheedge_amd", "csrc", "libmte_hip.so")):
        if rank == 0:
            ge.build()
        if dist_on:
            dist.barrier()
    from mindtheedge_amd import kernels as K
    from mindtheedge_amd.networks.depth.PackNetSAN01 import PackNetSAN01
    from mindtheedge_amd.models.SemiSupEdgeModel import SemiSupEdgeModel
    from mindtheedge_amd.losses.grad_loss import GradLoss
    from mindtheedge_amd.trainers.data_parallel import FlatParameters, BucketedAllReduce, FusedAdam, broadcast_parameters
    import random

    K.set_compute_dtype(args.dtype)
    knobs = [kv.split("=") for kv in filter(None, os.environ.get("MTE_DEBUG_KNOBS", "").split(","))]
    if knobs:                                            # development A/B knobs, e.g. "2=8,3=4096": only libmte_hip_dev.so has them
        from mindtheedge_amd import _lib
        K.lib.switch(_lib.DEV_LIB_PATH, True)
        for k, v in knobs:
            K.lib.mte_debug_set(int(k), int(v))
    if os.environ.get("MTE_NO_SIDE_STREAM"):
        K.use_wgrad_side_stream(False)
    torch.manual_seed(42)                                # default_config.py:16 seed; xavier init per PackNetSAN01.init_weights
    net = PackNetSAN01(dropout=0.5, version="1A").to(dev)
    model = SemiSupEdgeModel(supervised_loss_weight=1.0, depth_edges_loss_weight=1.0, supervised_method="sparse-silog",
                             supervised_num_scales=1, edges_depth_edge_loss_all_scales=True, flip_lr_prob=0.5)
    model.add_depth_net(net)
    model.add_edge_loss(GradLoss("cross_entropy", True, [], 10.0, 1.0))
    B, H, W = args.batch, args.height, args.width
    batch = device_batch(B, H, W, seed=1234 + rank, device=dev)
    random.seed(100 + rank)
    torch.manual_seed(1000 + rank)                       # decorrelated per-rank dropout masks

    timer = None
    if args.full and not args.no_kernel_timing:
        timer = ConvTimer(K)
        timer.install()

    kept = {}                          # the output dict of the last timed step (--dump-outputs)
    restore_start = None
    if args.mode == "train":
        model.train()
        flat = FlatParameters(net.parameters())
        broadcast_parameters(flat)
        reducer = BucketedAllReduce(flat, force=True) if dist_on else None
        opt = FusedAdam(flat, lr=1e-4, reducer=reducer)
        start = {"params": flat.flat.clone(), "cuda_rng": torch.cuda.get_rng_state(dev), "cpu_rng": torch.get_rng_state(),
                 "py_rng": random.getstate()}

        def restore_start():
            """The initial parameters and random-number state (dropout masks, flip draw) back in place for the last timed step.
            Ordered like the optimizer's own parameter write: after the side streams' work (the weight packs being rebuilt from
            the previous parameters), then the packs are invalidated and rebuilt."""
            for st in K._side["streams"]:
                ev = torch.cuda.Event()
                ev.record(st)
                torch.cuda.current_stream().wait_event(ev)
            flat.flat.copy_(start["params"])
            K.bump_weights_epoch()
            K.prefetch_weight_packs()
            torch.cuda.set_rng_state(start["cuda_rng"], dev)
            torch.set_rng_state(start["cpu_rng"])
            random.setstate(start["py_rng"])

        boundary = []                      # MTE_BENCH_BOUNDARY=1 (development): GPU time from the end of Adam to the first kernel of the next forward
        if os.environ.get("MTE_BENCH_BOUNDARY"):
            _img = K.image_to_act
            state = {"adam": None}

            def image_to_act(*a, **k):
                if state["adam"] is not None:
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    boundary.append((state["adam"], e))
                    state["adam"] = None
                return _img(*a, **k)
            K.image_to_act = image_to_act
            import mindtheedge_amd.networks.layers.packnet.layers01 as _l01
            _l01.K = K

        def eager_step(keep=False):
            opt.zero_grad()
            out = model(batch)
            out["loss"].backward()
            opt.step()
            if os.environ.get("MTE_BENCH_BOUNDARY"):
                state["adam"] = torch.cuda.Event(enable_timing=True)
                state["adam"].record()
            if keep:
                kept["out"] = out
            return out["loss"]
        step, launch_mode = eager_step, "eager"
        if dist_on:
            launch_mode = "eager (bucketed RCCL all-reduce is issued from grad-ready callbacks)"
        elif not os.environ.get("MTE_BENCH_GRAPH"):
            # measured on MI355X / ROCm 7.2 (profiles/README.md, round 2): the captured step replays at 45 ms against 29.7 ms eager -- the
            # runtime executes the graph's parallel branches (main chain | weight-gradient stream) one after the other and a replay
            # of ~1000 nodes costs the host 22 ms -- so the eager two-stream schedule stays the default; MTE_BENCH_GRAPH=1 replays
            launch_mode = "eager"
        else:
            # the whole step (zero_grad + forward + loss + backward + Adam + weight-pack prefetch, ~1000 launches) replayed from
            # two HIP graphs, one per outcome of the host-side flip draw; falls back to the eager step in this process
            from mindtheedge_amd.utils.graph import GraphedTrainStep
            graphed = GraphedTrainStep(model, opt, batch)
            if graphed.graphed:
                def graph_step(keep=False):
                    out = graphed()
                    if keep:
                        kept["out"] = out
                    return out["loss"]
                step, launch_mode = graph_step, "hip_graph"
            else:
                launch_mode = "eager (capture failed: %s)" % graphed.error
                print("bench.py: HIP-graph capture of the training step failed, running eagerly: %s" % graphed.error, file=sys.stderr)
    else:
        launch_mode = "eager"
        eager_step = None
        model.eval()

        def step(keep=False):
            with torch.no_grad():
                out = model(batch)
            if keep:
                kept["out"] = out
            return out["inv_depths"][0][0]

    def sync():
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        last = step()
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if i == args.steps - 1 and restore_start is not None:
            restore_start()
        last = step(keep=i == args.steps - 1)
    host_dt = time.perf_counter() - t0                   # time the host needed to ENQUEUE the steps (it runs ahead of the GPU)
    torch.cuda.synchronize()
    dt_local = time.perf_counter() - t0                  # this rank's own steps done (before the barrier): straggler spread across ranks
    sync()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(snapshot_outputs(kept.pop("out")), args.dump_outputs)
    host_free_dt = None
    if args.full:
        # the host's own cost per step: three steps enqueued right after a sync (empty queues: `host_dt` above also contains the time the
        # host spends blocked on full hardware queues while it runs ahead of the GPU)
        t1 = time.perf_counter()
        for _ in range(3):
            last = step()
        host_free_dt = (time.perf_counter() - t1) / 3
        sync()
    if args.mode == "train" and boundary:
        gaps = [a.elapsed_time(b) for a, b in boundary[-args.steps + 1:]]
        print("step boundary (end of Adam -> image conversion of the next step), ms: min %.3f median %.3f max %.3f"
              % (min(gaps), sorted(gaps)[len(gaps) // 2], max(gaps)), file=sys.stderr)
    # Per-kernel HIP-event timing runs on `ksteps` further steps of the same workload, outside the clocked region:
    # an event pair around each of the ~280 conv launches per step costs ~50 us of GPU idle each (14 ms/step), which
    # would distort `value`; the kernel durations themselves are unaffected by the gaps.
    ksteps = 0
    overlapped_records = []
    if timer:
        # the weight-gradient side stream is switched off for these steps: with kernels of two streams sharing the CUs an
        # event pair measures contention, not the kernel
        K.use_wgrad_side_stream(False)
        ksteps = min(args.steps, 3)
        kstep = eager_step if eager_step is not None else step      # launch by launch: the event pairs need the eager path
        for family in ("conv", "hbm"):           # separate steps per family: the event pairs of one must not space out the other
            timer.enabled = family
            for _ in range(ksteps):
                kstep()
            sync()
        timer.enabled = False
        K.use_wgrad_side_stream(not os.environ.get("MTE_NO_SIDE_STREAM"))
        # the same event pairs with the two-stream schedule ON: what the conv kernels cost while they share the CUs with the other
        # queue (the schedule `value` is measured on) -> roofline.frac_overlapped
        serial_records = timer.records
        timer.records = []
        timer.enabled = "conv"
        for _ in range(ksteps):
            kstep()
        sync()
        timer.enabled = False
        overlapped_records, timer.records = timer.records, serial_records
    if dist_on:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
        tl = torch.tensor([dt_local, -dt_local], device=dev, dtype=torch.float64)
        dist.all_reduce(tl, op=dist.ReduceOp.MAX)
        rank_ms = (-float(tl[1]) / args.steps * 1e3, float(tl[0]) / args.steps * 1e3)
    else:
        rank_ms = (dt_local / args.steps * 1e3,) * 2
    final = float(last.detach().float().sum()) if args.mode == "train" else float(last.float().mean())

    if rank == 0:
        ms = dt / args.steps * 1e3
        value = B * world * args.steps / dt
        res = {"metric": ("training images/sec, PackNet-SAN+edge-loss %dx%d %s" if args.mode == "train"
                          else "inference images/sec, PackNet-SAN %dx%d %s") % (H, W, args.dtype),
               "value": value, "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype,
               "data": "synthetic (SURVEY.md 8(d): rgb U[0,1), 5% sparse depth, soft thin edges, uniform normals; xavier init seed 42)",
               "config": {"workload": ("T8: PackNet-SAN + silog + 4-scale depth-edge loss training step" if args.mode == "train" else
                                       "I%d: PackNet-SAN depth inference" % B) + ", %dx%d, %d frames/GPU, dropout 0.5, flip 0.5" % (H, W, B),
                          "global_batch": B * world, "height": H, "width": W,
                          "parallelism": "dp%d (bucketed RCCL all-reduce overlapped with backward)" % world if world > 1 else "single GPU"},
               "final_loss" if args.mode == "train" else "mean_inv_depth": final,
               "host_enqueue_ms_per_step": host_dt / args.steps * 1e3,
               "step_launch": launch_mode,
               # fastest / slowest rank's own ms per step, measured to its local device sync BEFORE the closing barrier: the spread
               # is straggler time, to be read beside allreduce.allreduce_exposed_ms (both are inside ms_per_step)
               "rank_ms_per_step_min": rank_ms[0], "rank_ms_per_step_max": rank_ms[1]}
        if host_free_dt is not None:
            res["host_enqueue_unthrottled_ms_per_step"] = host_free_dt * 1e3
        passes = 3.0 if args.mode == "train" else 1.0
        step_flops = conv_flops_per_image(H, W) * B * passes
        res["mfma_fraction_of_step"] = step_flops / (ms * 1e-3) / (BF16_DENSE_PEAK_TFLOPS * 1e12)
        if timer and args.dump_conv:
            rows = [(e0.elapsed_time(e1), name, shp, fl) for name, e0, e1, fl, shp in timer.records[:len(timer.records) // max(ksteps, 1)]]
            with open(args.dump_conv, "w") as f:
                for ms_, name, shp, fl in sorted(rows, reverse=True):
                    f.write("%8.3f ms %7.1f TF  %-24s B,H,W,Cin_p,N,KH,KW=%s\n" % (ms_, fl / ms_ / 1e9, name, shp))
                hrows = [(e0.elapsed_time(e1), name, by) for name, e0, e1, by in timer.hbm_records[:len(timer.hbm_records) // max(ksteps, 1)]]
                for ms_, name, by in sorted(hrows, reverse=True):
                    f.write("%8.3f ms %7.2f TB/s  %-24s %.1f MB\n" % (ms_, by / ms_ / 1e9, name, by / 1e6))
        if timer:
            s = timer.summary()
            tot_t = sum(v[1] for v in s.values())
            tot_f = sum(v[2] for v in s.values())
            n = sum(v[0] for v in s.values())
            if tot_t > 0:
                peak = BF16_DENSE_PEAK_TFLOPS if args.dtype == "bf16" else 157.3
                alg = conv2d_flops_per_image(H, W) * B * passes * ksteps          # algorithmic conv2d FLOPs of the timed launches
                ach = alg / tot_t / 1e12
                res["roofline"] = {"bound": "mfma", "kernel": "conv2d MFMA family (mte_conv2d_igemm fwd+dgrad (+ _unshuffle), mte_conv2d_wgrad, "
                                                              "mte_conv2d_patch_fwd (+ _gn, _rank1, _plus1x1), mte_conv2d_patch_wgrad, mte_conv2d_stem_fwd, mte_conv2d_stem_wgrad)",
                                   "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                                   "traffic": pmc_traffic_per_launch(args, B, H, W, n / ksteps),
                                   "launches_per_step": n / ksteps, "avg_launch_ms": tot_t / n * 1e3,
                                   "conv_ms_per_step": tot_t / ksteps * 1e3, "timed_steps": ksteps,
                                   "frac_overlapped": (alg / (sum(e0.elapsed_time(e1) for _, e0, e1, _, _ in overlapped_records) * 1e-3) / 1e12 / peak)
                                   if overlapped_records else None,
                                   "conv_ms_per_step_overlapped": (sum(e0.elapsed_time(e1) for _, e0, e1, _, _ in overlapped_records) / ksteps)
                                   if overlapped_records else None,
                                   "algorithmic_flops_per_step": alg / ksteps, "executed_flops_per_step": tot_f / ksteps,
                                   # mte_conv2d_* launches seen during the timing pass that this family does NOT time (must be empty: rounds 4 and 5 each
                                   # added an entry point and read a `frac` that was too high until it was listed above)
                                   "untimed_conv_entry_points": dict(timer.untimed),
                                   "by_kernel": {k: {"launches_per_step": v[0] / ksteps, "ms_per_step": v[1] / ksteps * 1e3,
                                                     "executed_tflops": v[2] / v[1] / 1e12 if v[1] > 0 else None} for k, v in s.items()}}
            hn, ht, hb = timer.hbm_summary()
            if ht > 0:
                # second roofline object: the HBM-bound GroupNorm+ELU family (26 of the 84 GB a step moves), same method --
                # algorithmic bytes of the timed launches / HIP-event time, against the 8 TB/s HBM3E peak
                res["roofline_hbm"] = {"bound": "hbm", "kernel": "GroupNorm(16)+ELU family (mte_gn_stats (+ _from_records), mte_gn_elu_fwd, mte_gn_elu_bwd, mte_gn_tail_fwd)",
                                       "achieved": hb / ht / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": hb / ht / 1e9 / HBM_PEAK_GBS,
                                       "traffic": pmc_traffic_per_launch(args, B, H, W, hn / ksteps, "gn_family_MB_per_step"),
                                       "launches_per_step": hn / ksteps, "ms_per_step": ht / ksteps * 1e3,
                                       "algorithmic_bytes_per_step": hb / ksteps, "timed_steps": ksteps}
                ln, lt, lb = timer.loss_summary()
                if lt > 0:      # the fused Sobel / direction-select / balanced-BCE stencils of the depth-edge loss, 4 scales fwd + bwd
                    res["roofline_hbm"]["edge_loss_stencils"] = {"achieved": lb / lt / 1e9, "unit": "GB/s", "frac": lb / lt / 1e9 / HBM_PEAK_GBS,
                                                                  "launches_per_step": ln / ksteps, "ms_per_step": lt / ksteps * 1e3,
                                                                  "algorithmic_bytes_per_step": lb / ksteps}
        if args.mode == "train":
            # data-parallel readiness (spec horovod_trainer.py:53-55): the bucket / message layout the gradient
            # all-reduce uses, the order the buckets were launched in during the last backward and the device time the step
            # waited for RCCL in finish() -- at N = 1 (--full) the layout of the same network is reported without a collective
            if reducer is not None:
                res["allreduce"] = {"rccl_ranks": dist.get_world_size(), "backend": dist.get_backend(), **reducer.describe(),
                                    "allreduce_exposed_ms": reducer.exposed_ms(), "gradient_mb": round(flat.total * 4 / 2**20, 1)}
            elif args.full:
                layout = BucketedAllReduce(flat)
                res["allreduce"] = {"rccl_ranks": 1, "backend": None, **layout.describe(), "allreduce_exposed_ms": 0.0,
                                    "gradient_mb": round(flat.total * 4 / 2**20, 1)}
        if args.full and world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(H, W, args.cpu_steps)
            try:
                res["parity"] = parity_check(net, K, H, W)
            finally:
                K.set_compute_dtype(args.dtype)
        print(json.dumps(res))
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
