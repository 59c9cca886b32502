// Which kernel a weight-gradient call (mte_conv2d_wgrad) gets, with how many pixel splits and slabs: the decision and nothing else.  No HIP in here -- plain
// C++17, so that a CPU test can print the plan of any shape (tests/test_wgrad_launch_table_cpu.py).  mte_conv2d_wgrad (conv_igemm.hip) fills a WgradProblem,
// calls plan_wgrad and hands the plan to launch_wgrad_plan there (the nine-tap instances: wgrad9_launch, conv_wgrad9.hip); the query
// mte_conv2d_wgrad_nine_tap is wgrad_nine_tap_rk, the rule the plan asks.
#pragma once
#include <stddef.h>

#ifndef MTE_OK
#define MTE_OK 0
#define MTE_ERR_ARG (-1)
#define MTE_ERR_LAUNCH (-2)
#define MTE_ERR_UNSUPPORTED (-3)
#endif

// Workgroups of 256 threads the LDS-DMA forms aim for (pixel splits): ~4 per CU (or 1 of 1024 threads); three quarters of that beside the data-gradient chain
// (MTE_OPT_WGRAD_SHARES_CHIP; end of round 5, same box, ms per step: 512 -> 22.85, 384 -> 22.70, 256 -> 22.79, 768 -> 22.77 -- profiles/r05_side_queue_width.txt)
#ifndef MTE_WGRAD_WGS
#define MTE_WGRAD_WGS 512
#endif
// Workgroups the nine-tap kernel aims for per launch when the caller runs the weight gradients BESIDE the data-gradient chain (MTE_OPT_WGRAD_SHARES_CHIP): HALF the chip.
// With one workgroup per CU this kernel's 96 KB of LDS, 512 threads and whole register file take every CU away from the main queue's kernels for its whole length
// and it writes twice the slabs (what the main queue loses is less the CUs than the clock: profiles/r05_overlap_probe.txt).  Same-box step times (profiles/r05_side_queue_width.txt): 256 -> 23.59 ms, 192 -> 23.50, 128 -> 23.26, 96 -> 23.35, 64 -> 23.79.
// Alone on the chip (option off: serial profiling runs, a binding without a second stream) it takes one workgroup per CU.
#ifndef MTE_W9_WGS
#define MTE_W9_WGS 128
#endif

constexpr int WGRAD_RING = 4;                // LDS ring slots of the LDS-DMA and nine-tap kernels (WG_RING, conv_igemm.hip)
constexpr int WGRAD_REG_WGS = 1024;          // workgroups the register-staged forms aim for: >= ~4 per CU
constexpr int WGRAD9_LDS = WGRAD_RING * (8 + 16) * 1024;     // the nine-tap kernel's ring: dy 8 KiB + x patch 16 KiB per slot
constexpr long WGRAD_DESC_BOUND = 0x7ff00000L;               // bytes a buffer descriptor of the LDS-DMA kernels addresses

// Development knobs.  The library has one instance (conv_igemm.hip); mte_debug_set(key, value) (libmte_hip_dev.so only) writes it through wgrad_knob_set.
struct WgradKnobs {
    int dma = 1;                             // key 4: 0 = the register-staged kernel everywhere
    int big = 1;                             // key 8: 0 = 4-wave 64 x 128 / 128 x 128 tiles only; any other value = the 256 x 256 / 256 x 128 / 128 x 256 tiles too
                                             // (4x fewer re-reads of dy / x; pays once the pixel splits are few: wgs)
    int wgs = MTE_WGRAD_WGS;                 // key 9: workgroups aimed for (pixel splits)
    int nine_tap = 1;                        // key 26: 0 = the generic per-tap kernel everywhere, 2 = 2 x 16 K-steps before 1 x 32
    int nine_tap_wgs = MTE_W9_WGS;           // key 27: workgroups aimed for per shared-chip launch (0 = one per CU)
};
constexpr int WGRAD_KNOB_RESET = 33;         // key 33: every member back to its default, as for the other families
inline bool wgrad_knob_set(WgradKnobs& k, int key, int value) {
    switch (key) {
    case 4: k.dma = value; return true;
    case 8: k.big = value; return true;
    case 9: k.wgs = value; return true;
    case 26: k.nine_tap = value; return true;
    case 27: k.nine_tap_wgs = value; return true;
    case WGRAD_KNOB_RESET: k = WgradKnobs{}; return true;
    default: return false;
    }
}

// What the choice depends on
struct WgradProblem {
    int elem_size;                           // 2 = bf16, 4 = fp32; anything else: MTE_ERR_UNSUPPORTED
    int B, H, W, Cin_p, N, KH, KW;
    long ldx, ldy;                           // pixel strides of x and dy: only the descriptor bounds read them
    int parts_cap;                           // slabs the stage has room for
    bool has_parts_out;                      // the caller passed parts_out (without it nobody could add slabs up: no nine-tap kernel)
    bool shares_chip;                        // MTE_OPT_WGRAD_SHARES_CHIP
    int cus;                                 // compute units of the device
};

enum class WgradFamily { NineTap, Dma, Reg };      // conv_wgrad9_kernel<RK>, conv_wgrad_dma_kernel<WNO, WC, TNO, TC, FL>, conv_wgrad_kernel<T, WNO, WC, TNO, TC, FL>

// What gets launched
struct WgradPlan {
    int rc = MTE_OK;                         // otherwise nothing is launched
    WgradFamily family = WgradFamily::Reg;
    int rk = 0;                              // nine-tap: 1 = 1 x 32 K-steps, 2 = 2 x 16
    int WNO = 0, WC = 0, TNO = 0, TC = 0;    // the others: waves and 32 x 32 wave tiles along the output and the input channels
    bool row_aligned = false;                // FL: 32-pixel blocks that do not cross image rows
    int tiles_n = 0, tiles_c = 0, splits = 1;
    int blocks_per_split = 0;                // Dma, Reg: pixel blocks of 32
    int base = 0, units = 0, units_per_split = 0;      // nine-tap: tiles_n * tiles_c; K-steps of 32 pixels, all and per pixel split
    long part_stride = 0;                    // > 0: one slab per pixel split
    int parts_out = 1;
    size_t clear_bytes = 0;                  // > 0: slab 0 is zeroed first (the splits add into it): the register-staged family with more than one split, nothing else
    unsigned grid = 0; int threads = 256; size_t lds = 0;
    bool lds_optin = false;                  // the launch asks for `lds` bytes of dynamic LDS first (mte_allow_lds in wgrad9_launch): the nine-tap kernel's 96 KiB
};

// The instance a plan names, as one integer: the switch of launch_wgrad_plan is over it
constexpr int wgrad_key(WgradFamily f, int elem_size, int WNO, int WC, int TNO, int TC) { return (((((int)f * 8 + elem_size) * 8 + WNO) * 8 + WC) * 8 + TNO) * 8 + TC; }
inline int wgrad_key(const WgradPlan& pl, int elem_size) {
    return pl.family == WgradFamily::NineTap ? wgrad_key(pl.family, 2, pl.rk, 0, 0, 0) : wgrad_key(pl.family, pl.family == WgradFamily::Dma ? 2 : elem_size, pl.WNO, pl.WC, pl.TNO, pl.TC);
}

// The nine-tap kernel's shapes: bf16, 3x3, whole tiles of 128 output x 64 input channels, rows of whole K-steps.  0: not that kernel's; 1: 1 x 32 K-steps; 2: 2 x 16.
// 1 x 32 K-steps where the rows allow it: measured 2-4 % faster on the 48x160 layers than 2 x 16 ones although they stage 15 patch pieces against 12
// (development knob 26 = 2: 2 x 16 first).  This is mte_conv2d_wgrad_nine_tap.
inline int wgrad_nine_tap_rk(const WgradKnobs& k, int elem_size, int H, int W, int Cin_p, int N, int KH, int KW) {
    if (elem_size != 2 || KH != 3 || KW != 3 || H < 1 || W < 1 || Cin_p < 1 || N < 1) return 0;
    if (!k.nine_tap || N % 128 != 0 || Cin_p % 64 != 0) return 0;
    const bool ok2 = W % 16 == 0 && H % 2 == 0, ok1 = W % 32 == 0;
    return k.nine_tap == 2 ? (ok2 ? 2 : (ok1 ? 1 : 0)) : (ok1 ? 1 : (ok2 ? 2 : 0));
}

namespace wgrad_plan_detail {
inline WgradPlan refuse(WgradPlan pl, int rc) { pl.rc = rc; return pl; }
inline void tile(WgradPlan& pl, int WNO, int WC, int TNO, int TC) { pl.WNO = WNO; pl.WC = WC; pl.TNO = TNO; pl.TC = TC; }
}  // namespace wgrad_plan_detail

// Every rule in the order mte_conv2d_wgrad, wgrad9_launch, dispatch_wgrad and the two launch_wgrad templates had them.  Kept as they were: the register-staged
// forms ignore parts_cap and add into slab 0 after clearing it (*parts_out = 1); even kernel sizes are not refused; a missing parts_out skips the nine-tap kernel;
// a parts_cap below 1 counts as 1 for the LDS-DMA forms.  Knob 8 = 3 (256 x 256 on eight waves: measured 20-30 % slower in round 4, never adopted, no longer
// built) now means what every other non-zero value means.  The LDS-DMA forms never clear: their splits never exceed the slabs there is room for.  The pixel
// count times a stride is taken to stay inside a long, as the kernels' own addressing needs.
// New, all MTE_ERR_ARG: B, H, W, N, Cin_p, KH or KW below 1 (the parent divided by zero), a grid beyond what `unsigned` holds, a count of tiles, pixel blocks or
// K-steps beyond what `int` holds (the parent cast them unchecked), and cus < 1 (the launch path never passes that: it has a fallback beside its query).
inline WgradPlan plan_wgrad(const WgradProblem& p, const WgradKnobs& k) {
    using namespace wgrad_plan_detail;
    WgradPlan pl;
    if (p.Cin_p % 8 != 0 || p.N % 8 != 0) return refuse(pl, MTE_ERR_ARG);
    if (p.B < 1 || p.H < 1 || p.W < 1 || p.N < 1 || p.Cin_p < 1 || p.KH < 1 || p.KW < 1 || p.cus < 1) return refuse(pl, MTE_ERR_ARG);
    if (p.elem_size != 2 && p.elem_size != 4) return refuse(pl, MTE_ERR_UNSUPPORTED);
    const long es = p.elem_size, taps = (long)p.KH * p.KW, BH = (long)p.B * p.H;
    if (taps > 0x7fffffffL || BH > 0x7fffffffffffL / p.W) return refuse(pl, MTE_ERR_ARG);
    const long M = BH * p.W;
    const bool dy_fits = ((M - 1) * p.ldy + p.N) * es < WGRAD_DESC_BOUND;

    // round 5: the 3x3 layers with >= 64 / 128 channels take all nine taps from one staged patch (conv_wgrad9.hip)
    const int rk = p.parts_cap >= 1 && p.has_parts_out ? wgrad_nine_tap_rk(k, p.elem_size, p.H, p.W, p.Cin_p, p.N, p.KH, p.KW) : 0;
    if (rk && ((M + 2 * p.W + 16) * p.ldx) * 2 < WGRAD_DESC_BOUND && dy_fits) {
        pl.family = WgradFamily::NineTap; pl.rk = rk;
        const long base = (long)(p.N / 128) * (p.Cin_p / 64), units = M / 32;
        if (base > 0x7fffffffL || units > 0x7fffffffL) return refuse(pl, MTE_ERR_ARG);
        // one workgroup per CU (96 KB of LDS, 512 threads): pixel splits so that tiles x splits ~ the CU count, at least 12 K-steps each
        const long target = p.shares_chip && k.nine_tap_wgs > 0 ? k.nine_tap_wgs : p.cus;
        long splits = (target + base / 2) / base;
        if (splits < 1) splits = 1;
        if (splits > p.parts_cap) splits = p.parts_cap;
        if (splits > units / 12) splits = units / 12 > 0 ? units / 12 : 1;
        const long per_split = ((units + splits - 1) / splits + 3) & ~3L;     // the main loop is unrolled over its four ring slots
        splits = (units + per_split - 1) / per_split;
        if (per_split > 0x7fffffffL || base * splits > 0xffffffffL) return refuse(pl, MTE_ERR_ARG);
        pl.tiles_n = p.N / 128; pl.tiles_c = p.Cin_p / 64; pl.base = (int)base; pl.units = (int)units; pl.units_per_split = (int)per_split;
        pl.splits = pl.parts_out = (int)splits;
        pl.part_stride = (long)p.N * 9 * p.Cin_p;
        pl.grid = (unsigned)(base * splits); pl.threads = 512; pl.lds = WGRAD9_LDS; pl.lds_optin = true;
        return pl;
    }

    // The LDS-DMA ring kernel (bf16, both operands inside a descriptor); the register-staged one stays for fp32 validation mode, > 2 GiB tensors and <= 32 channels
    const bool fits = ((M + p.KW) * p.ldx + p.Cin_p) * es < WGRAD_DESC_BOUND && dy_fits;
    const bool dma = p.elem_size == 2 && k.dma && fits && p.N > 32 && p.Cin_p > 32;
    pl.family = dma ? WgradFamily::Dma : WgradFamily::Reg;
    if (dma) {
        if (k.big && p.N % 256 == 0 && p.Cin_p % 256 == 0) tile(pl, 4, 4, 2, 2);           // 256 x 256, 16 waves
        else if (k.big && p.N % 256 == 0 && p.Cin_p >= 128) tile(pl, 4, 2, 2, 2);          // 256 x 128, 8 waves
        else if (k.big && p.N >= 128 && p.Cin_p % 256 == 0) tile(pl, 2, 4, 2, 2);          // 128 x 256, 8 waves
        else if (p.N <= 64) tile(pl, 2, 2, 1, 2);                                          // cout 64 x cin 128
        else tile(pl, 2, 2, 2, 2);                                                         // cout 128 x cin 128
    } else {
        if (p.N <= 32) tile(pl, 1, 4, 1, 1);                                               // cout 32 x cin 128
        else if (p.N <= 64) tile(pl, 2, 2, 1, 2);                                          // cout 64 x cin 128
        else tile(pl, 2, 2, 2, 2);                                                         // cout 128 x cin 128
    }
    const int BNO = pl.WNO * pl.TNO * 32, BC = pl.WC * pl.TC * 32;
    pl.threads = dma ? pl.WNO * pl.WC * 64 : 256;
    if (dma) pl.lds = (size_t)WGRAD_RING * 32 * (BNO + BC) * 2;
    else {
        const long ry = BNO * es, rx = BC * es;                                            // LDS rows padded to an odd multiple of 64 bytes
        pl.lds = (size_t)(2 * 32 * ((ry % 128 == 64 ? ry : ry + 64) + (rx % 128 == 64 ? rx : rx + 64)));
    }
    const long tiles_n = ((long)p.N + BNO - 1) / BNO, tiles_c = ((long)p.Cin_p + BC - 1) / BC;
    if (tiles_n * tiles_c > 0xffffffffL / taps) return refuse(pl, MTE_ERR_ARG);
    const long base_wgs = tiles_n * tiles_c * taps;
    // row-aligned 32-pixel blocks waste MFMA work when W is not a multiple of 32 (W = 40: 37 %): use them for wide rows only (and inside a descriptor)
    pl.row_aligned = (p.W % 32 == 0 || p.W >= 160) && fits;
    const long nblk = pl.row_aligned ? BH * (((long)p.W + 31) / 32) : (M + 31) / 32;
    const long max_splits = (nblk + 15) / 16;                   // at least 16 pixel blocks per workgroup
    const long cap = p.parts_cap < 1 ? 1 : p.parts_cap;
    const long want = dma ? (p.shares_chip ? (long)k.wgs * 3 / 4 : (long)k.wgs) * 256 / pl.threads : WGRAD_REG_WGS;
    long splits = (want + base_wgs - 1) / base_wgs;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    if (dma && !p.shares_chip) {
        // alone on the chip the launch runs in whole rounds of (CUs x workgroups per CU): 50 tiles x 6 splits = 300 one-per-CU workgroups took two rounds, the second
        // 17 % full (5x5 512 -> 128 @48x160: 0.366 ms at 550 TFLOP/s; 5 splits = 250 workgroups: one round).  Among the split counts around the one above take the
        // cheapest in rounds per split; ties go to fewer partial slabs.
        long per_cu = (long)(160 * 1024 / pl.lds);
        if (per_cu > 2048 / pl.threads) per_cu = 2048 / pl.threads;
        if (per_cu < 1) per_cu = 1;
        const long slots = per_cu * p.cus;
        long best = splits; double best_cost = 1e30;
        for (long sc = splits > 2 ? splits - 2 : 1; sc <= splits + 2 && sc <= max_splits && sc <= cap; ++sc) {
            const double cost = (double)((base_wgs * sc + slots - 1) / slots) / (double)sc;
            if (cost < best_cost * 0.98) { best_cost = cost; best = sc; }
        }
        splits = best;
    }
    // one partial gradient per pixel split (plain stores, summed in part order by the unpack pass): never more splits than the caller's stage
    // has parts -- round 4: the fp32-atomic combine that used to take over beyond stage_parts is gone from this kernel's launch path, the
    // weight gradient is a fixed-order sum (the atomics cost 0.4 ms per step when they were the default, and made the result order-dependent)
    if (dma && splits > cap) splits = cap;
    const long per_split = (nblk + splits - 1) / splits;
    splits = (nblk + per_split - 1) / per_split;
    if (per_split > 0x7fffffffL || base_wgs * splits > 0xffffffffL) return refuse(pl, MTE_ERR_ARG);
    pl.tiles_n = (int)tiles_n; pl.tiles_c = (int)tiles_c; pl.blocks_per_split = (int)per_split; pl.splits = (int)splits;
    const long slab = (long)p.N * taps * p.Cin_p;               // (inside a long: base_wgs fits 32 bits and a tile has at most 2^16 elements)
    if (dma && splits > 1) { pl.part_stride = slab; pl.parts_out = (int)splits; }
    else if (splits > 1) pl.clear_bytes = sizeof(float) * (size_t)slab;
    pl.grid = (unsigned)(base_wgs * splits);
    return pl;
}
