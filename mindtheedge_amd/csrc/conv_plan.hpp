// Which kernel an implicit-GEMM convolution gets: the decision and nothing else.  No HIP in here -- plain C++17, so that a CPU test can print the plan of any
// shape (tests/test_conv_launch_table_cpu.py).  conv_igemm.hip fills an IgemmProblem, calls plan_igemm and launches the plan it gets (launch_plan there).
#pragma once

#ifndef MTE_OK
#define MTE_OK 0
#define MTE_ERR_ARG (-1)
#define MTE_ERR_LAUNCH (-2)
#define MTE_ERR_UNSUPPORTED (-3)
#endif

// 1 (default): the main loops issue v_mfma_f32_32x32x16_bf16; 0: the 32x32x8 loop the ablation arms were written for (conv_igemm.hip)
#ifndef MTE_IGEMM_MFMA16
#define MTE_IGEMM_MFMA16 1
#endif
// Default 51 = 19 | 32: TAP-major.  The slice-major order of round 5 (ConvArgs.kslice) cuts the implicit GEMM's fetches beyond L2 (the nine tap sweeps
// of a 64-channel slice re-use the lines of the first), but those fetches were Infinity-Cache hits, not HBM reads: same box, the training step takes
// 24.80 ms with it and 24.77 ms without, and in isolation the kernels are 5 % SLOWER (a tap change, i.e. new lane offsets, every K-tile): 6.74 against
// 6.43 ms over the step's launches (profiles/r05_igemm8_korder.txt).  It stays selectable: knob 23 without bit 5, or -DMTE_IGEMM8_DEFAULT=19.
#ifndef MTE_IGEMM8_DEFAULT
#define MTE_IGEMM8_DEFAULT 51
#endif

// Development knobs of the choice.  The library has one instance (conv_igemm.hip); mte_debug_set (libmte_hip_dev.so only) writes it through igemm_knob_set.
struct IgemmKnobs {
    int dma = 1;                 // key 0: tile loader -- 1 = LDS-DMA ring with buffer descriptors where possible, 2 = pointer DMA only, 0 = register staging
    int pair_ksteps = 72;        // key 19: see the two-workgroup ring of the 256 x 128 tile in plan_igemm
    int ablate = 0;              // key 17: main-loop ablation, see ABL in conv_igemm.hip (the arms exist only in a development build with -DMTE_IGEMM_MFMA16=0)
    int ring6 = 0;               // key 15, for the 8-wave 256 x 128 tile: 1 = 6-slot ring, 3 = 3-slot ring with two workgroups per CU
    int big_min_tiles = 224;     // key 7: tiles from which the 256-row / 192-row forms of the older kernel are taken
    int igemm8 = MTE_IGEMM8_DEFAULT;   // key 23: bit 0 = 8-phase 256 x 256 kernel, bit 1 = its 256 x 128 form, bit 2 every eligible launch, bit 5 (32) tap-major K order
                                 // (the default; without it: slice-major where Cin_p % 64 == 0); bits 3 / 4 belonged to the tile-walking form, removed in round 5
    int n32_dma = 1;             // key 32: N <= 32 on the two-wave LDS-DMA form
    int igemm8_split_bn128 = 64; // key 29: see the split-K rule of the 8-phase kernels
    int igemm8_min_tiles = 200;  // key 24
    int pp = 1;                  // key 21: 0 = the 16-wave one-barrier loop on the 256 x 256 tile
    int big = 3;                 // key 6: 0 128x128 only, 1 + 256x128, 2 + 256x256, 3 + 192x96
    int igemm8_one = 1;          // key 28: 0 = the two-state loop everywhere
};
constexpr int MTE_KNOB_IGEMM_RESET = 33;     // key 33: every field back to its default (tests restore with it instead of repeating defaults)

// -> false: not one of this struct's keys
inline bool igemm_knob_set(IgemmKnobs& k, int key, int value) {
    switch (key) {
    case 0: k.dma = value; return true;
    case 6: k.big = value; return true;
    case 7: k.big_min_tiles = value; return true;
    case 15: k.ring6 = value; return true;
    case 17: k.ablate = value; return true;
    case 19: k.pair_ksteps = value; return true;
    case 21: k.pp = value; return true;
    case 23: k.igemm8 = value; return true;
    case 24: k.igemm8_min_tiles = value; return true;
    case 28: k.igemm8_one = value; return true;
    case 29: k.igemm8_split_bn128 = value; return true;
    case 32: k.n32_dma = value; return true;
    case MTE_KNOB_IGEMM_RESET: k = IgemmKnobs{}; return true;
    }
    return false;
}

// What the choice depends on (GEMM view: M = B*H*W pixels, N output channels, K = KH*KW*Cin_p)
struct IgemmProblem {
    int elem_size;               // 2 = bf16, 4 = fp32
    long M;
    int N, Cin_p, KH, KW;
    long ldx;                    // elements per input pixel
    int out_f32;
    bool sparse;                 // ConvArgs.rows: the active-site form
    int unshuffle_c;             // ConvArgs.unshuffle_c (0 = off)
    int solo;                    // ConvArgs.solo
    bool has_ws; long ws_elems;  // split-K workspace: a pointer was passed, its fp32 elements
};

// Tile forms.  The first eight are conv_igemm_kernel<T, WM, WN, TM, TN, ...> (WM x WN waves of TM x TN 32 x 32 blocks), the last two conv_igemm8_kernel<BN, ...>.
enum class IgemmForm {
    T128x32,                     // <4, 1, 1, 1>: four waves, register-staged (its B stage misses the LDS-DMA loader's (BN * 4) % threads == 0)
    T128x32_W2,                  // <2, 1, 2, 1>: two waves of 64 x 32
    T128x64,                     // <2, 2, 2, 1>
    T128x128,                    // <2, 2, 2, 2>
    T192x96,                     // <2, 3, 3, 1>: six waves
    T256x128,                    // <4, 2, 2, 2>: eight waves
    T256x256_PP,                 // <2, 4, 4, 2>: eight waves of 128 x 64 in the ping-pong loop
    T256x256_W16,                // <4, 4, 2, 2>: sixteen waves, one-barrier loop
    P8_256x256, P8_256x128,      // the 8-phase kernels (conv_igemm8.hip), 512 threads
};
struct IgemmTile { int WM, WN, TM, TN; };
inline IgemmTile igemm_tile(IgemmForm f) {
    switch (f) {
    case IgemmForm::T128x32: return {4, 1, 1, 1};
    case IgemmForm::T128x32_W2: return {2, 1, 2, 1};
    case IgemmForm::T128x64: return {2, 2, 2, 1};
    case IgemmForm::T128x128: return {2, 2, 2, 2};
    case IgemmForm::T192x96: return {2, 3, 3, 1};
    case IgemmForm::T256x128: return {4, 2, 2, 2};
    case IgemmForm::T256x256_PP: return {2, 4, 4, 2};
    case IgemmForm::T256x256_W16: return {4, 4, 2, 2};
    default: return {0, 0, 0, 0};
    }
}

// What gets launched
struct IgemmPlan {
    int rc = MTE_OK;             // MTE_ERR_UNSUPPORTED: nothing is launched
    int elem_size = 2;
    IgemmForm form = IgemmForm::T128x128;
    int loader = 0;              // LD: 0 register staging, 1 pointer LDS-DMA, 2 buffer-descriptor LDS-DMA (the 8-phase kernels: always 2)
    int ring = 4, wpc = 1;       // RING slots and workgroups per CU (MINW) of conv_igemm_kernel: 4 / 1, or 3 / 4 and 6 / 1 on the 256 x 128 tile
    int ablate = 0;              // ABL arm, 0 = none
    int one = 0, kslice = 0;     // 8-phase kernels: one tap state per K-tile (ONE); slice-major K order (SM, ConvArgs.kslice)
    int splits = 1;              // ConvArgs.splits
    unsigned grid = 0; int threads = 0, lds_bytes = 0;
    bool lds_optin = false;      // ask for lds_bytes of dynamic LDS first (mte_allow_lds)
    bool finish = false;         // splitk_finish_kernel follows, finish_grid workgroups of 256
    unsigned finish_grid = 0;
};

// split-K factor for small-M / huge-K layers (pack5.conv: 120 tiles for 256 CUs); 1 = no split
inline int choose_splits(long tiles, int ksteps, long M, int N, long ws_elems, int nthr = 256) {
    const long want = 768L * 256 / nthr;               // ~3 four-wave workgroups per CU, or their equivalent in larger ones
    if (tiles >= want / 2 || ws_elems < M * N || N % 4 != 0) return 1;
    long s = (want + tiles - 1) / tiles;
    const long max_s = ksteps / 16;                    // keep >= 16 K-steps (1 KiB of K per row) per split
    if (s > max_s) s = max_s;
    if (s > ws_elems / (M * N)) s = ws_elems / (M * N);   // one [M][N] slab per split
    return (int)(s < 1 ? 1 : s);
}

// Does the buffer-descriptor LDS-DMA loader (LD = 2) apply: the knob asks for it, a K-step of 64 bytes never straddles a filter tap, and both operands lie
// inside what a buffer descriptor with 32-bit offsets addresses.  Every tile form asks this one question.  (The parent had four spellings: two spelled the
// bf16 case out, which this covers; the 8-phase launcher also refused M >= 0x7fffff00, which the first bound implies for every ldx >= 1 and is kept beside
// its caller below.)  mte_conv2d_igemm_unshuffle asks LESS before it plans -- the knob and the channel multiple, not the bounds: an un-shuffled launch past
// the bounds is taken by the pointer-DMA loader (LD = 1), which stages its result in LDS all the same.
inline bool igemm_dma_fits(const IgemmProblem& p, const IgemmKnobs& k) {
    const long es = p.elem_size;
    return k.dma == 1 && p.Cin_p % (int)(64 / es) == 0 && ((p.M - 1) * p.ldx + p.Cin_p) * es < 0x7ff00000L && (long)p.N * p.KH * p.KW * p.Cin_p * es < 0x7ff00000L;
}

namespace igemm_plan_detail {

inline void finish_after(IgemmPlan& pl, const IgemmProblem& p) {
    pl.finish = pl.splits > 1;
    long g = (p.M * p.N / 4 + 255) / 256; if (g > 4096) g = 4096;
    pl.finish_grid = (unsigned)g;
}

// conv_igemm_kernel on the tile `form`: loader, ring and split-K.  ws_elems: what of the workspace this form may use (0 = no split).
inline IgemmPlan plan_tile(IgemmForm form, long ws_elems, const IgemmProblem& p, const IgemmKnobs& k, bool dev_build) {
    IgemmPlan pl;
    pl.elem_size = p.elem_size; pl.form = form;
    const IgemmTile t = igemm_tile(form);
    const int BM = t.WM * t.TM * 32, BN = t.WN * t.TN * 32, NTHR = t.WM * t.WN * 64;
    const bool bf16 = p.elem_size == 2;
    const long tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
    const int ksteps = (p.KH * p.KW * (p.Cin_p / (16 / p.elem_size)) + 3) / 4;
    pl.splits = (p.has_ws && !p.out_f32 && !p.sparse) ? choose_splits(tiles, ksteps, p.M, p.N, ws_elems, NTHR) : 1;
    pl.threads = NTHR;
    pl.grid = (unsigned)(tiles * pl.splits);
    finish_after(pl, p);
    const bool dma_stage = (BN * 4) % NTHR == 0;       // the LDS-DMA loaders' B stage
    // the un-shuffled output is written from the LDS image of the result, which only the LDS-DMA forms stage; no K split
    if (p.unshuffle_c && (pl.splits != 1 || p.out_f32 || p.sparse || !bf16 || BN % 32 != 0 || !dma_stage || !k.dma)) { pl.rc = MTE_ERR_UNSUPPORTED; return pl; }
    if (dma_stage && k.dma) {
        const bool fast = igemm_dma_fits(p, k);
        pl.loader = fast ? 2 : 1;
        pl.lds_bytes = 4 * (BM + BN) * 64;
        const bool square = (BM == 256 && BN == 128) || (BM == 128 && BN == 128) || (BM == 256 && BN == 256);
        if (dev_build && !MTE_IGEMM_MFMA16 && bf16 && square && fast && k.ablate) {
            pl.ablate = k.ablate >= 1 && k.ablate <= 6 ? k.ablate : 7;
            return pl;
        }
        if (bf16 && form == IgemmForm::T256x128 && fast) {
            // two 74 KB workgroups per CU (3-slot ring): always for solo launches; beside the weight-gradient stream only for short
            // reductions over several rounds of tiles, where the prologue / epilogue share is largest (same-box step 30.46 -> 30.30 ms;
            // for every launch it costs the step 0.2 ms)
            const bool pair = p.solo || (ksteps <= k.pair_ksteps && tiles >= 512);
            if (k.ring6 == 3 || (k.ring6 == 0 && pair)) { pl.ring = 3; pl.wpc = 4; pl.lds_bytes = 3 * (BM + BN) * 64; pl.lds_optin = true; }
            else if (k.ring6 == 1) { pl.ring = 6; pl.lds_bytes = 6 * (BM + BN) * 64; pl.lds_optin = true; }
        }
        return pl;
    }
    if (NTHR != 256) { pl.rc = MTE_ERR_UNSUPPORTED; return pl; }      // (register staging exists for four waves only)
    pl.loader = 0;
    pl.lds_bytes = 2 * (BM + BN) * 64;
    return pl;
}

}  // namespace igemm_plan_detail

// dev_build: MTE_DEV -- the slice-major K order of the 8-phase kernels and the ablation arms exist only in that build
inline IgemmPlan plan_igemm(const IgemmProblem& p, const IgemmKnobs& k, bool dev_build) {
    using namespace igemm_plan_detail;
    using F = IgemmForm;
    if (p.elem_size != 2 && p.elem_size != 4) { IgemmPlan pl; pl.rc = MTE_ERR_UNSUPPORTED; return pl; }
    if (p.unshuffle_c && !(p.elem_size == 2 && k.dma == 1 && p.Cin_p % 32 == 0)) { IgemmPlan pl; pl.rc = MTE_ERR_UNSUPPORTED; return pl; }   // (see igemm_dma_fits)
    if (p.elem_size == 2) {
        // 256 x 128 tile, 8 waves: 24 KB of operands per K-step feed twice the MFMA work of a 128 x 128 tile (16 KB).  The
        // 4-wave kernel runs at ~14 TB/s of L2->LDS traffic with three stages in flight -- the latency-bandwidth product,
        // not the MFMA pipe, bounds it -- so fewer bytes per flop is the lever.  Needs the buffer-DMA loader and enough
        // tiles to cover the CUs.
        const long tiles_big = ((p.M + 255) / 256) * ((p.N + 127) / 128);
        const bool dma_ok = igemm_dma_fits(p, k);
        // (odd widths -- 72 / 104 / 200 input channels of the decoder concats as data-gradient N -- take the tile that covers
        //  them in ONE column block: the padded columns cost the same MFMA work as two narrower blocks, A is read once)
        const long n256 = (p.N + 255) / 256;
        const long t256 = ((p.M + 255) / 256) * n256;
        const bool wide = p.N > 128 && (p.N % 256 == 0 || p.N % 256 > 128);
        const int ksteps = p.KH * p.KW * (p.Cin_p / 32);
        // few tiles but a huge reduction (pack4/pack5.conv: K = 9 x 4096 / 8192): the big tiles keep their bytes-per-flop
        // advantage when the K range is split over workgroups (one fp32 slab per split in the workspace, then the finish kernel)
        const bool can_split = p.has_ws && p.ws_elems >= 2 * p.M * p.N && p.N % 4 == 0;
        long smax = can_split ? p.ws_elems / (p.M * p.N) : 1;                  // one [M][N] slab per split
        if (smax > 8) smax = 8;
        const long reach256 = t256 * (can_split ? (ksteps / 16 < smax ? (ksteps / 16 > 0 ? ksteps / 16 : 1) : smax) : 1);
        // ---- round 4: the 8-phase kernels (conv_igemm8.hip) take every launch the 256-row tiles took
        if (k.igemm8 && dma_ok && !p.out_f32 && !p.sparse && p.N > 64 && !p.unshuffle_c) {
            const int nkt = (ksteps + 1) / 2;                                                      // K-tiles of 64
            int bn = 0, splits = 1;
            // Same-box A/B against the older tile forms over the training step's shapes (tools/igemm8_check.py bench; profiles/r04_igemm8_ab.txt):
            // one workgroup per CU, so a launch of SEVERAL rounds of tiles pays prologue + epilogue (~ 6 K-tiles' worth) per round, where the
            // 256 x 128 kernel it replaces runs two workgroups per CU: short reductions over many tiles stay with the older forms.
            if (k.igemm8 & 4) {                                                                    // (development: every eligible launch)
                if (wide && t256 >= k.igemm8_min_tiles) bn = 256;
                else if (tiles_big >= k.igemm8_min_tiles) bn = 128;
            } else if (wide && (k.igemm8 & 1) && t256 >= k.igemm8_min_tiles) {
                if (nkt >= (t256 <= 256 ? 18 : 36)) bn = 256;
            } else if ((k.igemm8 & 2) && tiles_big >= k.igemm8_min_tiles && tiles_big <= 256 && nkt >= 36) bn = 128;
            if (!bn && wide && (k.igemm8 & 1) && can_split && t256 < 128 && ksteps >= 32) {        // few tiles, long reduction: split K
                bn = 256;
                long tsp = t256;
                // Round 6: very few tiles AND a short reduction (the 512-channel 12x40 / 24x80 layers: K = 4608) -> 256 x 128 tiles with half the K splits.  Such a
                // launch is dominated by its fp32 slabs (8 x 7.9 MB written and read back for a 3.9 MB result at 12x40); half the slabs: 41.7 -> 35.2 us forward,
                // 39.7 -> 33.4 data gradient at 512 -> 512 @12x40, 55.9 -> 52.4 at 512 -> 256 @24x80.  With a long reduction (pack4 / pack5.conv: K = 36,864 /
                // 73,728) the slabs do not matter and the narrower tile loses 15 % (265 -> 305 us): profiles/r06_lowres_split.txt.  Knob 29 = tile bound (0: off).
                if (t256 <= k.igemm8_split_bn128 && ksteps <= 288) { bn = 128; tsp = tiles_big; }
                long sp = 256 / tsp;                                                               // one round of workgroups
                if (sp > smax) sp = smax;
                if (sp > ksteps / 16) sp = ksteps / 16;                                            // >= 8 K-tiles per split
                const int per = (int)((ksteps + sp - 1) / (sp < 1 ? 1 : sp));
                splits = (ksteps + per - 1) / per;                                                 // (no empty split)
            }
            // round 5: 64-channel slices outer, taps inner where asked for and the channels allow it (ConvArgs.kslice; knob 23 bit 5 = tap-major, the order of
            // every other tile form and the default -- see IgemmKnobs.igemm8).  Measured slower: development library only (tests, tools/igemm8_locality.py); a
            // product build asked for it takes the older forms.  The tile-walking (persistent) form of round 4 is gone: it was 15-20 % slower per launch than
            // one workgroup per tile and no launch used it.
            const int kslice = (!(k.igemm8 & 32) && p.Cin_p % 64 == 0) ? 1 : 0;
            // what the 8-phase kernels cover (16-byte output chunks; 32-bit row index) -- outside it the older forms below take the launch
            if (bn && p.N % 8 == 0 && p.M < 0x7fffff00L && (!kslice || dev_build)) {
                IgemmPlan pl;
                pl.elem_size = 2; pl.form = bn == 256 ? F::P8_256x256 : F::P8_256x128;
                pl.loader = 2; pl.kslice = kslice; pl.splits = splits;
                // one tap state for both K-halves where they can never straddle a tap: 64-channel granularity and a split range that starts on an even K-step
                pl.one = !kslice && k.igemm8_one && p.Cin_p % 64 == 0 && (splits == 1 || ((ksteps + splits - 1) / splits) % 2 == 0);
                pl.threads = 512;
                pl.lds_bytes = 2 * (4 * 128 * 64 + 4 * (bn / 2) * 64); pl.lds_optin = true;
                pl.grid = (unsigned)(((p.M + 255) / 256) * ((p.N + bn - 1) / bn) * splits);
                finish_after(pl, p);
                return pl;
            }
        }
        if (k.big >= 2 && dma_ok && !p.out_f32 && wide &&
            (t256 >= k.big_min_tiles || (can_split && t256 < 96 && reach256 >= 160))) {   // (96: below it choose_splits does split)
            // enough tiles without a K split: 8 waves of 128 x 64 in the ping-pong loop (same-box A/B per layer: 256 -> 256 3x3 @48x160
            // 70.2 -> 66 us, 384 -> 256 106 -> 95-101, 5x5 64 -> 256 @96x320 226 -> 212, 128 -> 512 @48x160 203 -> 189); the split-K
            // launches (few tiles, short per-split reductions) lose with it and keep the 16-wave one-barrier loop
            if (k.pp && t256 >= k.big_min_tiles) return plan_tile(F::T256x256_PP, 0, p, k, dev_build);
            return plan_tile(F::T256x256_W16, t256 >= k.big_min_tiles ? 0 : p.ws_elems, p, k, dev_build);
        }
        // 65..96 columns (the 72-channel decoder concat as data-gradient N): a 192 x 96 tile of 6 waves wastes a quarter of
        // the MFMA work instead of the 44 % a 128-wide tile does
        if (k.big >= 3 && dma_ok && !p.out_f32 && p.N > 64 && p.N <= 96 && ((p.M + 191) / 192) >= k.big_min_tiles)
            return plan_tile(F::T192x96, 0, p, k, dev_build);
        if (k.big && dma_ok && !p.out_f32 && p.N > 64 && tiles_big >= k.big_min_tiles)
            return plan_tile(F::T256x128, 0, p, k, dev_build);
        // round 6: two waves of 64 x 32 where the LDS-DMA loader applies (its B stage needs (BN * 4) % threads == 0, which the four-wave 128 x 32 form misses: that
        // one stages through registers) -- the 32-output band convolutions of the folded pack layers (K = 25 x 512)
        if (p.N <= 32 && k.n32_dma && dma_ok && !p.out_f32) return plan_tile(F::T128x32_W2, p.ws_elems, p, k, dev_build);
    }
    return plan_tile(p.N <= 32 ? F::T128x32 : p.N <= 64 ? F::T128x64 : F::T128x128, p.ws_elems, p, k, dev_build);
}
