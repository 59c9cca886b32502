// Which kernels a GroupNorm pass gets: the decision and nothing else.  No HIP in here -- plain C++17, so that a CPU test can print the plan of any shape
// (tests/test_gn_launch_table_cpu.py).  norm_act.hip fills a GnProblem, calls plan_gn and launches the plan it gets (launch_gn there); the two queries that tell
// Python whether the forward pass takes its own statistics ask the same function.
#pragma once

#ifndef MTE_OK
#define MTE_OK 0
#define MTE_ERR_ARG (-1)
#define MTE_ERR_LAUNCH (-2)
#define MTE_ERR_UNSUPPORTED (-3)
#endif
// record slots per sample of a statistics buffer: common.hpp's definition, repeated for the stand-alone build (the preprocessor refuses a second one that differs)
#define MTE_GN_SLOTS(B) ((B) >= 8 ? 64 : 512 / (B))

constexpr int GN_PLAN_GROUPS = 16;           // GroupNorm(16, C)
// A slab workgroup runs load -> reduce -> apply -> store back to back with the CU to itself (1024 threads), and only B*16
// of them exist: measured (tools/gn_bench.py, B = 8, bf16) it wins 3x on the 12x40 layers (6.8 vs 19 us forward, 19 vs 37 us
// backward), ties at 24x80 and loses at 48x160, where the streaming kernels overlap their phases across workgroups.
constexpr long GN_SLAB_MAX = 1024L * 4;      // 16-byte chunks of one (sample, group) slab

// Development knobs.  The library has one instance (norm_act.hip); mte_debug_set (libmte_hip_dev.so only) writes it through gn_knob_set.
struct GnKnobs {
    // keys 2, 3: ~8 workgroups of 256 threads per CU across the batch (target), at least min_rows pixels per thread row: a thread's rows are consumed in
    // serial batches of GN_U loads, so long runs leave the short low-resolution launches latency-bound; the backward kernels pay a per-workgroup flush of
    // 2-3 C atomics and prefer fewer, longer workgroups (the forward and statistics kernels take at most 16 rows)
    int min_rows = 32, target = 2048;
    int slab = 1;                            // key 13: 0 = stream kernels only
    // key 14: two-pass kernels read the same tensors twice.  Blocks are dispatched in blockIdx order, i.e. sample after sample: when the second pass walks the
    // samples in the OPPOSITE order it starts on the bytes the first pass touched last, which are still in the 256 MB Infinity Cache (a full-resolution
    // 32-channel activation is 252 MB per tensor at T8: in the same order nothing of the first pass survives to the second)
    int zigzag = 1;
    int cluster = 1;                         // key 25, values below 1000: 0 = no cluster kernels
    unsigned spin_max = 1u << 24;            // key 25, value 1000 + n: bound of the cluster kernels' arrival poll (tests force the give-up path with it)
};
inline int gn_knob_set(GnKnobs& k, int key, int value) {
    switch (key) {
    case 2: if (value < 1) return MTE_ERR_ARG; k.min_rows = value; return MTE_OK;
    case 3: if (value < 1) return MTE_ERR_ARG; k.target = value; return MTE_OK;
    case 13: k.slab = value; return MTE_OK;
    case 14: k.zigzag = value; return MTE_OK;
    case 25: if (value >= 1000) k.spin_max = (unsigned)(value - 1000); else k.cluster = value; return MTE_OK;
    }
    return MTE_ERR_ARG;
}

enum class GnPass {
    Stats,                                   // mte_gn_stats
    TailStats,                               // first launch of mte_gn_tail_fwd: inner apply + statistics of the sum
    FwdApply,                                // mte_gn_elu_fwd with ready statistics, and the second launch of mte_gn_tail_fwd
    FwdSingle,                               // mte_gn_elu_fwd without: one kernel takes the statistics and applies them, or nothing does
    Bwd,                                     // mte_gn_elu_bwd
};
enum class GnSecond { None, Input, ScaledOutput };   // a second input tensor y2 / (backward only) one input whose gradient also leaves scaled, d2 = scale2 * d1

// What the choice depends on
struct GnProblem {
    int elem_size;                           // 2 = bf16, 4 = fp32
    int B, HW, C;
    GnPass pass;
    GnSecond second;
    bool dbias;                              // backward: a bias gradient is wanted
    bool after_tail;                         // FwdApply: the launch before was the tail's statistics pass, which ended on the LAST sample
};

enum class GnForm { Stream, Slab, Cluster, Unsupported };
enum : unsigned {                            // GnPlan.clears, in the order they go out
    GN_CLEAR_RED = 1, GN_CLEAR_DBIAS = 2,    // backward, every form (the bias gradient only where one is wanted)
    GN_CLEAR_DGAMMA_DBETA = 4,               // the slab and cluster kernels ADD each sample's part (the stream kernels overwrite them)
    GN_CLEAR_TICKETS = 8,                    // the statistics passes' arrival counters
    GN_CLEAR_RECORDS = 16,                   // the cluster's exchange words live in the record area of the statistics buffer and must be zero at entry
};
struct GnLaunch { unsigned grid_x = 0, grid_y = 1; int block = 0; long lds = 0; int reverse = 0; };

// What gets launched
struct GnPlan {
    int rc = MTE_OK;                         // otherwise nothing is launched
    GnForm form = GnForm::Stream;
    int NT = 256, NCH = 0, CL = 0;           // template parameters: threads (1024: statistics and slab kernels), chunks per thread and workgroups per slab
    int cps_shift = 0;                       // slab, cluster: log2(chunks per pixel inside one group)
    int blocks_per_sample = 0;               // stream
    int per_launch = 0, launches = 1;        // cluster: samples per launch, and how many launches take the batch
    int kernels = 0; GnLaunch launch[2];     // one kernel; the stream backward has two (reduce, then apply)
    unsigned clears = 0;                     // GN_CLEAR_*: what must be zero first and is cleared unless the caller pre-zeroed it (MTE_OPT_GN_PREZEROED)
};

inline bool gn_single_pass(const GnPlan& pl) { return pl.form == GnForm::Slab || pl.form == GnForm::Cluster; }

inline bool gn_shape_ok(int C, int elem_size) {
    const int per16 = 16 / elem_size;
    if (C < GN_PLAN_GROUPS || C % GN_PLAN_GROUPS != 0 || C % per16 != 0) return false;
    const int cpr = C / per16;               // 16-byte chunks of a pixel: the stream kernels' thread map wants a divisor of 256
    return cpr <= 256 && 256 % cpr == 0;
}

namespace gn_plan_detail {

inline long cdivl(long a, long b) { return (a + b - 1) / b; }

// workgroups per sample of a stream kernel of NT threads: the target spread over the batch, at least min_rows pixel rows per thread
inline int stream_blocks(const GnProblem& p, const GnKnobs& k, int NT, bool cap_rows, bool cap_slots) {
    const int rstep = NT / (p.C / (16 / p.elem_size));
    const int min_rows = k.min_rows < 1 ? 1 : cap_rows && k.min_rows > 16 ? 16 : k.min_rows;
    long want = cdivl((long)k.target * 256 / NT, p.B);
    const long maxb = cdivl(p.HW, (long)min_rows * rstep);
    if (want > maxb) want = maxb;
    if (cap_slots && want > MTE_GN_SLOTS(p.B)) want = MTE_GN_SLOTS(p.B);      // one record slot per workgroup
    return (int)(want < 1 ? 1 : want);
}

// slab geometry: a group must be whole 16-byte chunks (1, 2, 4 or 8 per pixel); -> chunks of one slab, or 0 if not a slab shape
inline long slab_chunks(const GnProblem& p, const GnKnobs& k, int* cps_shift) {
    const int per16 = 16 / p.elem_size, gs = p.C / GN_PLAN_GROUPS;
    if (!k.slab || gs % per16 != 0 || gs > 32) return 0;
    const int cps = gs / per16;
    if (cps != 1 && cps != 2 && cps != 4 && cps != 8) return 0;
    int sh = 0;
    while ((1 << sh) < cps) ++sh;
    *cps_shift = sh;
    return (long)p.HW * cps;
}

// cluster geometry for a slab of more than GN_SLAB_MAX chunks: CL workgroups of 256 threads, NCH chunks per thread.
// regs = 16-byte registers a thread holds per chunk.  -> false: not a cluster shape
inline bool cluster(const GnProblem& p, const GnKnobs& k, int sh, int regs, GnPlan& pl) {
    if (!k.cluster) return false;
    // the registers decide the workgroups per slab: <= 128 VGPRs without spills (measured on the compiler's report) = 12 sixteen-byte data
    // registers per thread, so four workgroups per CU stay resident
    int nmax = 8;
    while (nmax * regs > 12) nmax >>= 1;
    // (measured, tools/gn_bench.py: clusters of 16 with the batch in two launches of 4 samples -- 256 channels at 48x160 backward, 128 at 96x320
    //  forward -- run 1.4-2.3x SLOWER than the streaming kernels: 66 vs 48 us, 89 vs 38 us; a cluster pays only when ONE launch of <= 8
    //  workgroups per slab covers 8 samples)
    int cl = 2;
    while (cl < 8 && (cdivl(p.HW, cl) << sh) > 256L * nmax) cl <<= 1;
    const long per_wg = cdivl(p.HW, cl) << sh;             // chunks of the largest pixel range
    if (per_wg > 256L * nmax || 2 + 2 * cl > MTE_GN_SLOTS(p.B) * 2) return false;
    int nch = 2;
    while (256L * nch < per_wg) nch <<= 1;
    // every LIVE workgroup of a launch must be resident (1024 of 256 threads): samples per launch; the batch goes out in several launches
    const int per_launch = 8;                              // (the block map would also deal 4, 2 or 1 samples to the 8 XCD labels)
    if (per_launch * GN_PLAN_GROUPS * cl > 1024) return false;
    if (cdivl(p.B, per_launch) > 4) return false;          // more than four launches: the streaming kernels are the better form
    pl.form = GnForm::Cluster; pl.NT = 256; pl.NCH = nch; pl.CL = cl; pl.cps_shift = sh;
    pl.per_launch = per_launch; pl.launches = (int)cdivl(p.B, per_launch);
    pl.kernels = 1; pl.launch[0] = {(unsigned)(per_launch * GN_PLAN_GROUPS * cl), 1, 256, 0, 0};
    return true;
}

// the stream kernels of 256 threads
inline void stream(const GnProblem& p, const GnKnobs& k, bool forward, GnPlan& pl) {
    pl.form = GnForm::Stream; pl.NT = 256;
    pl.blocks_per_sample = stream_blocks(p, k, 256, forward, false);
    pl.kernels = 1; pl.launch[0] = {(unsigned)pl.blocks_per_sample, (unsigned)p.B, 256, 0, 0};
}

}  // namespace gn_plan_detail

// Odd rules kept on purpose, each as the kernels were measured: the backward holds one 16-byte register more per chunk than the forward (2 + second input
// against 1 + second input), so one shape can be a cluster going forward and stream kernels going back; a scaled second output never takes a slab (the slab
// kernels have no such instance; the cluster kernels do); the forward and statistics kernels cap min_rows at 16; eight chunks per thread exist only in the
// forward without a second input.
// A cluster starts above GN_SLAB_MAX = 4096 chunks and a workgroup holds at most 256 * nmax of them, so of the cluster instances norm_act.hip has (NCH 2 / 4 / 8
// x CL 2 / 4 / 8 / 16) the plan can return only these: forward without a second input (nmax 8) NCH 8 with CL 4 or 8; forward with one, and every backward
// (nmax 4), NCH 4 with CL 8.  The others stay instantiated and unreached, as they were.
inline GnPlan plan_gn(const GnProblem& p, const GnKnobs& k) {
    using namespace gn_plan_detail;
    GnPlan pl;
    if ((p.elem_size != 2 && p.elem_size != 4) || p.B < 1 || p.HW < 0 || !gn_shape_ok(p.C, p.elem_size)) { pl.form = GnForm::Unsupported; pl.rc = MTE_ERR_ARG; return pl; }
    const bool two = p.second == GnSecond::Input;
    switch (p.pass) {
    case GnPass::Stats:
    case GnPass::TailStats:                                 // 1024 threads: the same number of threads as `target` workgroups of 256 would be
        pl.NT = 1024;
        pl.blocks_per_sample = stream_blocks(p, k, 1024, true, true);
        // Stats: the producing conv wrote sample 0 first, start on the freshest bytes; TailStats: the inner layer's statistics pass ended on sample 0
        pl.kernels = 1; pl.launch[0] = {(unsigned)pl.blocks_per_sample, (unsigned)p.B, 1024, 0, p.pass == GnPass::Stats ? k.zigzag : 0};
        pl.clears = GN_CLEAR_TICKETS;
        return pl;
    case GnPass::FwdApply:
        stream(p, k, true, pl);
        pl.launch[0].reverse = p.after_tail ? k.zigzag : 0;      // (... and the statistics pass ended on sample 0)
        return pl;
    case GnPass::FwdSingle:
    case GnPass::Bwd: {
        const bool bwd = p.pass == GnPass::Bwd;
        if (bwd) pl.clears = GN_CLEAR_RED | (p.dbias ? GN_CLEAR_DBIAS : 0u);
        int sh = 0;
        const long n = slab_chunks(p, k, &sh);
        if (n > 0 && n <= GN_SLAB_MAX && !(bwd && p.second == GnSecond::ScaledOutput)) {
            pl.form = GnForm::Slab; pl.NT = 1024; pl.NCH = n <= 1024L * 2 ? 2 : 4; pl.cps_shift = sh;
            // the 16 group-workgroups of a sample on one XCD: whole sets of 8 samples
            pl.kernels = 1; pl.launch[0] = {(unsigned)(8L * GN_PLAN_GROUPS * cdivl(p.B, 8)), 1, 1024, 0, 0};
        } else if (n > GN_SLAB_MAX && cluster(p, k, sh, (bwd ? 2 : 1) + (two ? 1 : 0), pl)) {
            if (!bwd) pl.clears = GN_CLEAR_RECORDS;
        } else if (bwd) {
            stream(p, k, false, pl);
            pl.kernels = 2; pl.launch[1] = pl.launch[0];
            pl.launch[0].lds = 4L * p.C * 2;
            pl.launch[1].lds = p.dbias ? 4L * p.C : 0;
            pl.launch[1].reverse = k.zigzag;                // the apply pass starts where the reduce pass ended
            return pl;
        } else {
            pl.rc = MTE_ERR_ARG;                            // a stream apply needs ready statistics: form stays Stream, nothing is launched
            return pl;
        }
        if (bwd) pl.clears |= GN_CLEAR_DGAMMA_DBETA;
        return pl;
    }
    }
    pl.form = GnForm::Unsupported; pl.rc = MTE_ERR_ARG;
    return pl;
}
