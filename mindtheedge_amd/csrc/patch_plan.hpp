// Which kernel an LDS-patch convolution call gets: the decision and nothing else.  No HIP in here -- plain C++17, so that a CPU test can print the plan of any
// shape (tests/test_patch_launch_table_cpu.py).  The entry points of conv_patch.hip fill a PatchProblem, call plan_patch and hand the plan to launch_patch_plan
// there; the three queries (mte_conv2d_patch_supported, _wgrad_supported, _fwd_rank1_ok) are the plan's return code.
#pragma once
#include <stddef.h>

#ifndef MTE_OK
#define MTE_OK 0
#define MTE_ERR_ARG (-1)
#define MTE_ERR_LAUNCH (-2)
#define MTE_ERR_UNSUPPORTED (-3)
#endif

// Workgroup groups of the weight-gradient launches WHEN THEY SHARE THE CHIP with the data-gradient chain (MTE_OPT_WGRAD_SHARES_CHIP; round 5, same-box
// step times with the two-stream schedule, profiles/r05_side_queue_width.txt):
// 512 -> 256 groups: 23.25 -> 23.16 ms per step (192: the same, 128: 23.60); the wide (65..128-output) variant 256 -> 128: a further -0.08 ms.  Fewer,
// longer workgroups leave CUs to the data-gradient chain and halve the slabs the unpack pass adds up.
// (end of round 5, after the kernel's instruction diet: 256 -> 22.75 ms per step, 192 -> 22.67, 160 -> 22.65, 128 -> 22.95 on one box; 23.24 / 23.13 / -- on another: 192)
#ifndef MTE_PATCH_WGRAD_WGS
#define MTE_PATCH_WGRAD_WGS 192
#endif
#ifndef MTE_PATCH_WGRAD_WIDE_WGS
#define MTE_PATCH_WGRAD_WIDE_WGS 128
#endif

constexpr int PATCH_TH = 8, PATCH_TW = 32;   // output tile (pixels); the tall forward tiles have 16 rows, the three-slice and the wide weight gradients 4

// Development knobs.  The library has one instance (conv_patch.hip); mte_debug_set(11, value) (libmte_hip_dev.so only) writes it through patch_knob_set, which
// finds the member by the range the value is in.
struct PatchKnobs {
    int tall = 1;                            // value < 100: 0 = 8-row forward tiles everywhere
#ifdef MTE_PATCH_FWD1
    int fwd2 = 0;                            // (diagnostic builds: tools/patch_stamps.py v1)
#else
    int fwd2 = 1;                            // 400 + v: 0 = the first form of the forward kernel
#endif
    // Round 6: every forward form runs on v_mfma_f32_16x16x32_bf16 (M16); the 32x32x16 forms of rounds 1-5 are instantiated in the development library only
    // (tests/test_gpu_conv_variants.py compares the two).  Same-box A/B per layer: profiles/r06_m16_ab.txt, profiles/r06_inloop_clock.txt.
    int m16 = 1;                             // 500 + v: 0 = the 5x5 / 7x7 second form on v_mfma_f32_32x32x16_bf16
    int m16_3 = 1;                           // 700 + v: 0 = the 3x3 / 1x1 second form on v_mfma_f32_32x32x16_bf16
    int m16_f1 = 1;                          // 600 + v: 0 = the first form on v_mfma_f32_32x32x16_bf16
    int wgrad_8w = 1;                        // 200 + v: 0 = four waves per workgroup everywhere
    int wgrad_wide = 1;                      // 300 + v: 0 = 65..128 output channels stay on the generic weight gradient
    int wgrad_wgs = MTE_PATCH_WGRAD_WGS;     // any other value >= 100: workgroups of a weight-gradient launch (the wide variant: MTE_PATCH_WGRAD_WIDE_WGS, compile time only)
};
constexpr int PATCH_KNOB_RESET = -1;         // every member back to its default: what mte_debug_set(33, .) passes on
inline int patch_knob_set(PatchKnobs& k, int value) {
    if (value == PATCH_KNOB_RESET) k = PatchKnobs{};
    else if (value >= 700 && value < 710) k.m16_3 = value - 700;
    else if (value >= 600 && value < 610) k.m16_f1 = value - 600;
    else if (value >= 500 && value < 510) k.m16 = value - 500;
    else if (value >= 400 && value < 410) k.fwd2 = value - 400;
    else if (value >= 300 && value < 310) k.wgrad_wide = value - 300;
    else if (value >= 200 && value < 210) k.wgrad_8w = value - 200;
    else if (value >= 100) k.wgrad_wgs = value;
    else k.tall = value;
    return MTE_OK;
}

enum class PatchOp { Fwd, FwdGn, FwdRank1, FwdPlus1x1, Wgrad };

// What the choice depends on
struct PatchProblem {
    PatchOp op;
    int B, H, W, Cin_p, N, KH, KW;           // (FwdRank1, FwdPlus1x1: 3 x 3)
    long ldx;                                // pixel stride of x: only the second form's 2 GiB descriptor bound reads it
    bool accumulate;                         // Fwd, FwdGn: y += conv
    bool bias_aligned;                       // the bias pointer is null or on a 16-byte boundary (the second form reads it in 16-byte groups)
    int C2;                                  // FwdPlus1x1: channels of the 1x1 term
    int parts_cap;                           // Wgrad: slabs the stage has room for
    bool wgrad_shares_chip;                  // Wgrad: MTE_OPT_WGRAD_SHARES_CHIP
};

// What gets launched
struct PatchPlan {
    int rc = MTE_OK;                         // otherwise nothing is launched
    bool wgrad = false;
    // forward: conv_patch_fwd2_kernel<K, NT, TALL, R1, ACC, EXTRA, M16> (second) or conv_patch_fwd_kernel<K, NT, TALL, ACC, EXTRA, M16>
    bool second = false;
    int K = 0, NT = 0;
    bool TALL = false, R1 = false, ACC = false, EXTRA = false, M16 = false;
    int rows = 0, tiles_per_sample = 0;      // tile rows; tiles (= GroupNorm records) per sample
    // weight gradient: conv_patch_wgrad_kernel<K, NT, SL, NW, NH, THW>
    int SL = 0, NW = 0, NH = 0, THW = 0;
    int nslices = 0, groups = 0, parts_out = 1;
    long part_stride = 0;                    // > 0: one slab per group
    size_t clear_bytes = 0;                  // > 0: dw is zeroed first (the groups add into it)
    unsigned grid_x = 0, grid_y = 1; int block = 256; size_t lds = 0;
};

// The instance a plan names, as one integer: the template arguments in the kernel's own order
constexpr long patch_fwd_key(int K, int NT, bool TALL, bool ACC, bool EXTRA, bool M16) { return ((((1L * 8 + K) * 4 + NT) * 2 + TALL) * 8 + ACC * 2 + EXTRA) * 2 + M16; }
constexpr long patch_fwd2_key(int K, int NT, bool TALL, bool R1, bool ACC, bool EXTRA, bool M16) {
    return ((((2L * 8 + K) * 4 + NT) * 2 + TALL) * 8 + R1 * 4 + ACC * 2 + EXTRA) * 2 + M16;
}
constexpr long patch_wgrad_key(int K, int NT, int SL, int NW, int NH, int THW) { return ((((3L * 8 + K) * 4 + NT) * 4 + SL) * 16 + NW) * 64 + NH * 16 + THW; }
inline long patch_key(const PatchPlan& pl) {
    if (pl.wgrad) return patch_wgrad_key(pl.K, pl.NT, pl.SL, pl.NW, pl.NH, pl.THW);
    return pl.second ? patch_fwd2_key(pl.K, pl.NT, pl.TALL, pl.R1, pl.ACC, pl.EXTRA, pl.M16) : patch_fwd_key(pl.K, pl.NT, pl.TALL, pl.ACC, pl.EXTRA, pl.M16);
}

// bf16, C_out <= 64, W % 32 == 0, k in {1, 3, 5, 7}: what every entry point but the wide weight gradient covers
inline bool patch_shape_ok(int W, int Cin_p, int N, int KH, int KW) {
    if (KH == 7 && N > 32) return false;             // 13 taps x 2 tiles of accumulators per wave would spill in wgrad
    return W % PATCH_TW == 0 && Cin_p % 8 == 0 && N % 8 == 0 && N <= 64 && KH == KW && (KH == 1 || KH == 3 || KH == 5 || KH == 7);
}
// weight gradient only: 65..128 output channels, 3x3, at least one 64-channel slice pair (the wide variant of conv_patch_wgrad_kernel)
inline bool patch_wgrad_wide_ok(const PatchKnobs& k, int W, int Cin_p, int N, int KH, int KW) {
    return k.wgrad_wide && W % PATCH_TW == 0 && Cin_p % 8 == 0 && Cin_p >= 64 && N % 8 == 0 && N > 64 && N <= 128 && KH == 3 && KW == 3;
}

namespace patch_plan_detail {

// tiles of `rows` x PATCH_TW pixels (W % PATCH_TW == 0).  -> false: more of them than a grid's x takes (the parent cast the product to unsigned, and a wrapped
// count sends the kernels out of range: refused here)
inline bool count_tiles(const PatchProblem& p, int rows, long& per_sample, long& all) {
    per_sample = (long)(p.W / PATCH_TW) * (((long)p.H + rows - 1) / rows);
    if (per_sample > 0x7fffffffL || per_sample < -0x7fffffffL) return false;
    all = per_sample * p.B;
    return all >= 0 && all <= 0x7fffffffL;
}

// The second (buffer-descriptor) form of the forward kernel.  Same-box A/B over the network's shapes (tools/conv_shape_bench.py): 7x7 -12..-15 %, 5x5 -8..-12 %,
// 3x3 with 32 outputs -4..-12 %, 3x3 with 64 outputs -8 % from three slices on; with one or two slices the first form wins by 8-15 % (167 VGPRs, three
// workgroups per CU, against 244), and the 1x1 layers are HBM-bound either way.  (With the rank-1 term and with the 1x1 term K is 3: N <= 32 || Cin_p > 64.)
// It addresses the input through a buffer descriptor (< 2 GiB) and reads the bias in 16-byte groups.
inline bool second_form(const PatchProblem& p, const PatchKnobs& k, int K, int NT) {
    return k.fwd2 && (K >= 5 || (K == 3 && (NT == 1 || p.Cin_p > 64))) && (((long)p.B * p.H * p.W - 1) * p.ldx + p.Cin_p) * 2 < 0x7ff00000L && p.bias_aligned;
}
// 16-row tiles: one output tile only, and at 5x5 / 7x7 one input slice only
inline bool tall_tiles(const PatchProblem& p, const PatchKnobs& k, int K, int NT) { return NT == 1 && k.tall && (p.Cin_p <= 32 || K <= 3) && p.H >= 16; }

inline PatchPlan refuse(PatchPlan pl, int rc) { pl.rc = rc; return pl; }

}  // namespace patch_plan_detail

// Every rule in the order the entry points had them.  Kept as they were: B < 1, H < 1 and W < 1 are refused nowhere (an empty grid, which the launch then
// reports); the rank-1 entry point answers MTE_ERR_UNSUPPORTED for everything its _ok query refuses, a bad shape included, and has no first form; FwdGn refuses
// N % 16 != 0 as MTE_ERR_UNSUPPORTED after the shape test; `accumulate` picks the ACC instance only where neither R1 nor EXTRA is set.  New: a tile count beyond
// a grid's x, and a weight gradient with no input slice (Cin_p < 1: the parent divided by zero), are MTE_ERR_ARG.
inline PatchPlan plan_patch(const PatchProblem& p, const PatchKnobs& k) {
    using namespace patch_plan_detail;
    PatchPlan pl;
    const bool ok = patch_shape_ok(p.W, p.Cin_p, p.N, p.KH, p.KW);
    long per_sample = 0, tiles = 0;
    if (p.op != PatchOp::Wgrad) {
        pl.K = p.KH; pl.NT = p.N <= 32 ? 1 : 2;
        pl.R1 = p.op == PatchOp::FwdRank1; pl.EXTRA = p.op == PatchOp::FwdPlus1x1;
        if (!ok || (pl.EXTRA && (p.C2 < 8 || p.C2 % 8 != 0))) return refuse(pl, pl.R1 ? MTE_ERR_UNSUPPORTED : MTE_ERR_ARG);
        if (p.op == PatchOp::FwdGn && p.N % 16 != 0) return refuse(pl, MTE_ERR_UNSUPPORTED);      // whole groups
        pl.second = second_form(p, k, pl.K, pl.NT);
        if (pl.R1 && (!pl.second || (p.H & 1) || (p.W & 1))) return refuse(pl, MTE_ERR_UNSUPPORTED);     // (the caller then writes the term with mte_rank1_conv_fwd)
        pl.TALL = tall_tiles(p, k, pl.K, pl.NT);
        pl.ACC = p.accumulate && !pl.R1 && !pl.EXTRA;
        pl.M16 = (pl.second ? (pl.K >= 5 ? k.m16 : k.m16_3) : k.m16_f1) != 0;
        pl.rows = pl.TALL ? 16 : PATCH_TH;
        if (!count_tiles(p, pl.rows, per_sample, tiles)) return refuse(pl, MTE_ERR_ARG);
        pl.tiles_per_sample = (int)per_sample;
        pl.grid_x = (unsigned)tiles;
        return pl;
    }
    pl.wgrad = true;
    if (ok) {
        // two slices per workgroup where the accumulators still fit (3x3 and 1x1; 5x5 with C_out <= 32) and there is more than one slice
        // eight waves (two per SIMD on the one workgroup a CU holds) where a wave still gets enough accumulator units: two output
        // tiles per unit, or >= 32 units.  Same-box A/B per launch: 7x7 32->32 @384x1280 0.510 -> 0.388 ms, 3x3 64->64 @192x640
        // 0.146 -> 0.108, 5x5 256->64 @96x320 0.272 -> 0.205; the one-tile launches with 18 / 25 units lose 14-20 % and stay on four.
        const int K = pl.K = p.KH, NT = pl.NT = p.N <= 32 ? 1 : 2;
        pl.NH = 1; pl.THW = 8;
        if (K == 3 && p.Cin_p > 64 && p.Cin_p <= 96 && k.wgrad_8w) {
            // 65..96 input channels (iconv1: the 72-channel decoder concat): all three 32-channel slices in ONE workgroup -- the 192-byte
            // pixel rows of the two-slice layout are exactly full, dy is read once instead of once per slice pair (0.40 -> 0.29 ms)
            // round 6: the same for 64 outputs (iconv2: the 96-channel concat @192x640) -- 27 (tap, slice) units over 8 waves instead of two slice groups of 18, the
            // second one half empty: a third fewer MFMA steps (0.191 -> 0.147 ms, profiles/r06_lowres_split.txt; 4-row tiles: with 8 rows the staged next tile pushed it past 256 VGPRs)
            pl.SL = 3; pl.NW = 8; pl.THW = NT == 2 ? 4 : 8;
        } else {
            pl.SL = (K <= 3 || (K == 5 && NT == 1)) && p.Cin_p > 32 ? 2 : 1;
            const int units = K * K * pl.SL;
            pl.NW = units >= 16 && (NT == 2 || units >= 32) && k.wgrad_8w ? 8 : 4;
        }
    } else {
        if (!patch_wgrad_wide_ok(k, p.W, p.Cin_p, p.N, p.KH, p.KW)) return refuse(pl, MTE_ERR_ARG);
        pl.K = 3; pl.NT = 2; pl.SL = 2; pl.NW = 8; pl.NH = 2; pl.THW = 4;
    }
    const int K = pl.K, PH = pl.THW + K - 1, PW = PATCH_TW + K - 1;
    const int XRS = pl.SL == 1 ? 64 : 192, YRS = pl.NT * pl.NH == 1 ? 64 : (pl.NT * pl.NH == 2 ? 192 : 320);
    pl.lds = (size_t)(PH * PW * XRS + pl.THW * PATCH_TW * YRS);
    const long nslices = ((long)p.Cin_p + 32 * pl.SL - 1) / (32 * pl.SL);
    if (nslices < 1 || !count_tiles(p, pl.THW, per_sample, tiles)) return refuse(pl, MTE_ERR_ARG);
    // ~2 workgroups per CU in total; the 147 KB wide variant (NH = 2) holds one per CU: one round of workgroups, half the slabs to add up
    // (alone on the chip -- MTE_OPT_WGRAD_SHARES_CHIP off -- twice the groups: the round-4 geometry)
    const long want = (long)(pl.NH == 2 ? MTE_PATCH_WGRAD_WIDE_WGS : k.wgrad_wgs) * (p.wgrad_shares_chip ? 1 : 2);
    long groups = (want + nslices - 1) / nslices;
    if (groups > tiles) groups = tiles;
    if (groups > p.parts_cap) groups = p.parts_cap < 1 ? 1 : p.parts_cap;   // one slab per workgroup group, always (round 4: no fp32-atomic combine on this launch path)
    pl.nslices = (int)nslices; pl.groups = (int)groups;
    if (groups > 1 && groups <= p.parts_cap) {                              // one partial gradient per group, summed by the unpack pass
        pl.part_stride = (long)p.N * K * K * p.Cin_p;
        pl.parts_out = pl.groups;
    } else {
        pl.clear_bytes = sizeof(float) * (size_t)p.N * K * K * p.Cin_p;
    }
    pl.grid_x = (unsigned)groups; pl.grid_y = (unsigned)nslices; pl.block = pl.NW * 64;
    return pl;
}
