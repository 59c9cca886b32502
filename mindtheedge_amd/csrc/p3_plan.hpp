// Which kernel a conv3d pack / unpack call gets: the decision and nothing else.  No HIP in here -- plain C++17, so that a CPU test can print the plan of any
// shape (tests/test_p3_launch_table_cpu.py).  The six entry points of pack3d.hip fill a P3Problem, call plan_p3 and hand the plan to launch_p3plan there.
#pragma once
#include <stddef.h>

#ifndef MTE_OK
#define MTE_OK 0
#define MTE_ERR_ARG (-1)
#define MTE_ERR_LAUNCH (-2)
#define MTE_ERR_UNSUPPORTED (-3)
#endif
#ifndef MTE_DT_BF16
#define MTE_DT_BF16 0
#define MTE_DT_F32 1
#endif
#ifndef MTE_P3W_WGS
#define MTE_P3W_WGS 512      // workgroups of the conv3d weight-gradient launches (side queue; end of round 5, after the kernel's instruction diet, same box: 768 -> 22.00 ms per step, 512 -> 21.94, 384 -> 21.97, 256 -> 22.09)
#endif

// LDS tiles keep 8 pad elements (16 B) after the D depths of every pixel: with a power-of-two pixel stride the 16-byte window
// reads of a wave (64..1024 B apart) fall on a few banks only -- SQ_LDS_BANK_CONFLICT was 47-84 % of the LDS-active cycles.
#define LDP(D) ((D) + 8)

// P3Knobs.mfma_data: which data paths run on the matrix cores (bf16, and only while lds >= 2).  The product value is 239 = every bit but P3_ONE_BF16_WEIGHT:
// pack forward and unpack forward as taps-in-K GEMMs, pack backward data as a banded GEMM, unpack backward data banded for C = 64 and by LDS-DMA with four
// waves for C = 32, the conv3d weights split into bf16 hi + lo parts.  P3_UNPACK_FWD stays set but decides nothing there: the taps-in-K form comes first in
// the ladder and takes every C the banded forward accepts.
// Contract of P3_ONE_BF16_WEIGHT (HILO = false instances; development build only): each conv3d weight is rounded ONCE to bf16, to nearest even, and no lo part
// is multiplied; products, sums and the store are as in every other form.  The result is the operation on the rounded weights, exactly
// (tests/test_gpu_conv3d_exact.py checks it bit for bit), and differs from the hi + lo forms wherever w != bf16(w).
enum : int {
    P3_UNPACK_BWD_DATA = 1,          // bit 0: unpack backward data as a banded GEMM (C = 32, 64)
    P3_UNPACK_BWD_DATA_DMA = 2,      // bit 1: ... by LDS-DMA of the raw records for C = 32
    P3_DMA_4_WAVES = 4,              // bit 2: ... with 4 waves per workgroup (0: 2 waves x 4 rows, measured slower)
    P3_UNPACK_FWD = 8,               // bit 3: unpack forward as a banded GEMM, persistent workgroups (C = 32, 64)
    P3_ONE_BF16_WEIGHT = 16,         // bit 4: the conv3d weights as ONE bf16 value in every banded form (no lo part: half the MFMAs)
    P3_UNPACK_FWD_TAPS_K = 32,       // bit 5: unpack forward with the spatial taps in K (C = 32 .. 256)
    P3_PACK_FWD_TAPS_K = 64,         // bit 6: pack forward in that form (C % 32 == 0)
    P3_PACK_BWD_DATA = 128,          // bit 7: pack backward data as a banded GEMM (C % 32 == 0)
    P3_MFMA_DATA_PRODUCT = 239,
};

// Development knobs.  The library has one instance (pack3d.hip); mte_debug_set(1, value) (libmte_hip_dev.so only) writes it through p3_knob_set, which
// finds the member by the range the value is in.
struct P3Knobs {
    int lds = 2;                             // value < 100: 0 = gather kernels, 1 = LDS-tiled (plane by plane), 2 = + four-plane unpack backward data and the matrix-core forms
    int small_tiles = 1;                     // 100 + v: 0 = the larger tile table of p3_tile; also whole (not halved) unpack weight-gradient tiles under a cap of 512 workgroups
    int mfma = 1;                            // 200 + v: 0 = conv3d weight gradients on the fp32 VALU (LDS kernels)
    int mfma_data = P3_MFMA_DATA_PRODUCT;    // 300 + bits: P3_* above
    int mfma_threads = 512;                  // 1000 + n: threads per workgroup of the matrix-core weight gradient
    int persist_wgs = 1024;                  // 2000 + n: workgroups of the persistent banded unpack forward (a multiple of 8: tile % 8 = XCD)
    int tr_passes = 4;                       // 3000 + v, v = 1 / 2 / 4: output passes of the taps-in-K unpack forward
    int weight_wgs = MTE_P3W_WGS;            // (compile time only) workgroups of the matrix-core weight gradient
};
constexpr int P3_KNOB_RESET = -1;            // every member back to its default: what mte_debug_set(33, .) passes on
inline int p3_knob_set(P3Knobs& k, int value) {
    if (value == P3_KNOB_RESET) k = P3Knobs{};
    else if (value >= 3000) k.tr_passes = value == 3001 ? 1 : value == 3002 ? 2 : 4;
    else if (value >= 2000) k.persist_wgs = value - 2000;
    else if (value >= 1000) k.mfma_threads = value - 1000;
    else if (value >= 300) k.mfma_data = value - 300;
    else if (value >= 200) k.mfma = value - 200;
    else if (value >= 100) k.small_tiles = value - 100;
    else k.lds = value;
    return MTE_OK;
}

enum class P3Op { PackFwd, PackBwdData, PackBwdWeight, UnpackFwd, UnpackBwdData, UnpackBwdWeight };

// What the choice depends on.  B, H, W, C: the UN-packed side tensor (pack: the layer's input; unpack: the conv3d's input)
struct P3Problem {
    P3Op op;
    int dtype;                               // MTE_DT_*
    int B, H, W, C;
    long ldx, ldo;                           // pixel strides of the un-packed side and of the feature side: only the 1 << 30 element bounds of the buffer-addressed forms read them
};

enum class P3Form {
    Gather,                                  // one thread per (pixel, 8 channels), P3Args; bf16 and fp32
    Lds,                                     // LDS-tiled fp32-VALU stencil, one feature plane at a time
    Lds4,                                    // ... all four planes staged at once (unpack backward data, C <= 128)
    Mfma,                                    // banded-operand GEMM
    Dma32,                                   // ... fed by LDS-DMA (unpack backward data, C = 32)
    TapsK,                                   // GEMM with the spatial taps in K
    WeightMfma, WeightLds,                   // weight gradient on the matrix cores / on the fp32 VALU
};

// What gets launched
struct P3Plan {
    int rc = MTE_OK;                         // otherwise no kernel is launched
    P3Op op = P3Op::PackFwd;
    P3Form form = P3Form::Gather;
    bool f32 = false;                        // Gather: the element type
    int CPT = 0, C = 0, HILO = 0, WAVES = 0, NH = 0;     // template parameters of the instance, 0 where it has none of that name (TH below is one for TapsK)
    int TH = 0, TW = 0, tiles_h = 0, tiles_w = 0, ntiles = 0;      // P3LArgs: tile geometry
    int dshift = 0, tshift = 0;              // P3LArgs, weight forms: log2(depth pairs per pixel) or -1 when not a power of two; log2(TW)
    long total = 0;                          // P3Args (Gather): threads with work
    unsigned grid_x = 0, grid_y = 1; int block = 256; size_t lds = 0;
    bool clear_dwb = false;                  // dwb[112] is zeroed first (also where rc says the element type is unknown: the parent cleared before it looked)
};

// The instance a plan names, as one integer: operation, form and the template arguments in the kernel's own order (element type: 0 = bf16, 1 = float)
constexpr long p3_key(P3Op op, P3Form form, int t0 = 0, int t1 = 0, int t2 = 0) {
    return ((((long)op * 8 + (long)form) * 1024 + t0) * 1024 + t1) * 1024 + t2;
}
inline long p3_key(const P3Plan& pl) {
    const bool pack = pl.op == P3Op::PackFwd || pl.op == P3Op::PackBwdData || pl.op == P3Op::PackBwdWeight;
    switch (pl.form) {
    case P3Form::Gather: return pack ? p3_key(pl.op, pl.form, pl.f32, pl.CPT) : p3_key(pl.op, pl.form, pl.f32);
    case P3Form::Mfma: return pack ? p3_key(pl.op, pl.form, pl.HILO) : p3_key(pl.op, pl.form, pl.C, pl.HILO);
    case P3Form::Dma32: return p3_key(pl.op, pl.form, pl.WAVES, pl.HILO);
    case P3Form::TapsK: return pack ? p3_key(pl.op, pl.form, pl.TH, pl.NH) : p3_key(pl.op, pl.form, pl.C, pl.TH, pl.NH);
    default: return p3_key(pl.op, pl.form);
    }
}

inline bool p3_ok(int C) { const int cb = C >> 3; return C % 8 == 0 && cb >= 1 && cb <= 64 && (cb & (cb - 1)) == 0; }

// ---- tiles.  Pack forms tile the PACKED volume [H/2][W/2] of D = 4C depths, unpack forms the volume [H][W] of C depths
struct P3Tile { int TH, TW; };
inline P3Tile p3_tile(int C, int small_tiles) {      // LDS pack stencils: TH*TW*C = 2048 (small) / 4096
    if (small_tiles) {
        if (C <= 32) return {4, 16};
        if (C <= 64) return {4, 8};
        if (C <= 128) return {2, 8};
        if (C <= 256) return {2, 4};
        return {2, 2};
    }
    if (C <= 32) return {8, 16};
    if (C <= 64) return {4, 16};
    if (C <= 128) return {4, 8};
    if (C <= 256) return {2, 8};
    return {2, 4};
}
inline P3Tile up_tile(int C) {                       // LDS unpack stencils: TH*TW*C = 16384 (2 items of 32 depths per thread)
    if (C <= 32) return {16, 32};
    if (C <= 64) return {8, 32};
    if (C <= 128) return {8, 16};
    if (C <= 256) return {4, 16};
    return {4, 8};
}
inline P3Tile up4_tile(int C) {                      // four planes at once: TH*TW*C = 4096 (one 16-depth item per thread), the same ~46-61 KB of LDS
    if (C <= 32) return {8, 16};
    if (C <= 64) return {4, 16};
    return {4, 8};
}
// bytes of `planes` halo tiles of D bf16 depths per pixel: what every LDS stencil and weight-gradient kernel stages
inline size_t p3_halo_bytes(P3Tile t, int D, int planes = 1) { return (size_t)planes * (t.TH + 2) * (t.TW + 2) * LDP(D) * 2; }
inline size_t p3_lds_bytes(int C, int small_tiles) { return p3_halo_bytes(p3_tile(C, small_tiles), 4 * C); }
inline size_t up_lds_bytes(int C) { return p3_halo_bytes(up_tile(C), C); }
inline size_t up4_lds_bytes(int C) { return p3_halo_bytes(up4_tile(C), C, 4); }

namespace p3_plan_detail {

// tiles of t over an [h][w] volume per sample.  -> false: more than an int of them (the parent's product overflowed, and a wrapped count sends the kernels
// out of range: refused here)
inline bool set_tiles(P3Plan& pl, P3Tile t, int h, int w, int B) {
    pl.TH = t.TH; pl.TW = t.TW;
    pl.tiles_h = (int)(((long)h + t.TH - 1) / t.TH); pl.tiles_w = (int)(((long)w + t.TW - 1) / t.TW);
    const long n = (long)pl.tiles_h * pl.tiles_w;
    if (n > 0x7fffffffL || n < -0x7fffffffL || n * B > 0x7fffffffL || n * B < -0x7fffffffL) { pl.rc = MTE_ERR_ARG; pl.clear_dwb = false; return false; }
    pl.ntiles = (int)(n * B);
    return true;
}
inline int ilog2_exact(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }      // v a power of two
inline int min_int(int a, int b) { return a < b ? a : b; }

// one workgroup of 256 threads per tile of an LDS form
inline P3Plan& lds_form(P3Plan& pl, P3Form form, size_t lds) {
    pl.form = form; pl.grid_x = (unsigned)pl.ntiles; pl.lds = lds;
    return pl;
}
// the gather kernels: one thread per (pixel, 8 channels), or per 4 channels where CPT = 4; the weight gradients walk the work with a capped grid, y = kh
inline P3Plan& gather(P3Plan& pl, const P3Problem& p, long pixels, int CPT, long cap) {
    pl.form = P3Form::Gather; pl.CPT = CPT; pl.f32 = p.dtype == MTE_DT_F32;
    pl.total = pixels * (p.C / 8) * (CPT == 4 ? 2 : 1);
    const long threads = cap && pl.total >= cap ? cap : pl.total;
    pl.grid_x = (unsigned)((threads + 255) / 256); pl.grid_y = cap ? 3 : 1;
    if (p.dtype != MTE_DT_BF16 && p.dtype != MTE_DT_F32) pl.rc = MTE_ERR_UNSUPPORTED;
    return pl;
}
// the weight forms: D depths per pixel of the staged volume
inline void weight_shifts(P3Plan& pl, int D) {
    const int dpairs = D / 16;
    pl.dshift = (dpairs & (dpairs - 1)) == 0 ? ilog2_exact(dpairs) : -1;
    pl.tshift = ilog2_exact(pl.TW);
}

}  // namespace p3_plan_detail

// Every rule in the order the entry points had them.  Kept as they were: only the pack forward refuses odd H / W (the pack gradients halve them silently);
// B < 1, H < 1 and W < 1 are refused nowhere (an empty grid, which the launch then reports); C = 16 (and 8) gets the plane-by-plane LDS kernels for pack and the
// gather kernels for unpack; C = 512 gets them too except in the pack forward and backward data, which are matrix-core forms for every C % 32 == 0; fp32 always
// gets the gather kernels; an element type the library does not have is MTE_ERR_UNSUPPORTED only after the shape tests, and after the weight gradients' clear.
inline P3Plan plan_p3(const P3Problem& p, const P3Knobs& k) {
    using namespace p3_plan_detail;
    P3Plan pl;
    pl.op = p.op;
    const int B = p.B, H = p.H, W = p.W, C = p.C;
    if (!p3_ok(C) || (p.op == P3Op::PackFwd && ((H & 1) || (W & 1)))) { pl.rc = MTE_ERR_ARG; return pl; }
    const bool bf16 = p.dtype == MTE_DT_BF16;
    const bool lds2 = bf16 && k.lds >= 2;                   // what every matrix-core data form and the four-plane kernel ask first
    const int one = (k.mfma_data & P3_ONE_BF16_WEIGHT) ? 0 : 1;     // HILO of the banded forms
    const long lim = 1L << 30;                              // elements a buffer-addressed tensor may span
    const long slabs = 4 * C / 128;                         // depth slabs of 128 of the packed volume: grid = tiles x slabs
    switch (p.op) {
    case P3Op::PackFwd:
        if (lds2 && (k.mfma_data & P3_PACK_FWD_TAPS_K) && C % 32 == 0) {
            if (!set_tiles(pl, {2, 16}, H / 2, W / 2, B)) return pl;
            if (pl.ntiles * slabs < lim) {
                pl.NH = 4;
                lds_form(pl, P3Form::TapsK, (size_t)4 * 18 * 448 + (size_t)8 * 1024).grid_x = (unsigned)(pl.ntiles * slabs);
                return pl;
            }
        }
        if (bf16 && k.lds && C <= 512) {
            if (!set_tiles(pl, p3_tile(C, k.small_tiles), H / 2, W / 2, B)) return pl;
            return lds_form(pl, P3Form::Lds, p3_lds_bytes(C, k.small_tiles));
        }
        return gather(pl, p, (long)B * (H / 2) * (W / 2), C <= 256 ? 4 : 8, 0);
    case P3Op::PackBwdData:
        if (lds2 && (k.mfma_data & P3_PACK_BWD_DATA) && C % 32 == 0 && ((long)B * (H / 2) * (W / 2) - 1) * p.ldo + 16L * C < lim) {
            if (!set_tiles(pl, {4, 16}, H / 2, W / 2, B)) return pl;
            if (pl.ntiles * slabs < lim) {
                pl.HILO = one;
                lds_form(pl, P3Form::Mfma, (size_t)7 * 20 * 256).grid_x = (unsigned)(pl.ntiles * slabs);
                return pl;
            }
        }
        if (bf16 && k.lds && C <= 512) {
            if (!set_tiles(pl, p3_tile(C, k.small_tiles), H / 2, W / 2, B)) return pl;
            return lds_form(pl, P3Form::Lds, p3_lds_bytes(C, k.small_tiles));
        }
        return gather(pl, p, (long)B * (H / 2) * (W / 2), C <= 256 ? 4 : 8, 0);
    case P3Op::PackBwdWeight:
        pl.clear_dwb = true;
        if (bf16 && k.lds && C <= 512) {
            if (!set_tiles(pl, p3_tile(C, k.small_tiles), H / 2, W / 2, B)) return pl;
            weight_shifts(pl, 4 * C);
            if (k.mfma) {
                lds_form(pl, P3Form::WeightMfma, p3_lds_bytes(C, k.small_tiles) + 16).grid_x = (unsigned)min_int(pl.ntiles, k.weight_wgs);
                pl.block = k.mfma_threads;
                return pl;
            }
            lds_form(pl, P3Form::WeightLds, p3_lds_bytes(C, k.small_tiles)).grid_x = (unsigned)min_int(pl.ntiles, 512);
            return pl;
        }
        return gather(pl, p, (long)B * (H / 2) * (W / 2), C <= 256 ? 4 : 8, 256L * 1024);
    case P3Op::UnpackFwd:
        if (lds2 && (k.mfma_data & P3_UNPACK_FWD_TAPS_K) && (C == 32 || C == 64 || C == 128 || C == 256)) {
            if (!set_tiles(pl, {256 / C, 16}, H, W, B)) return pl;
            const int rs = (C * 2) % 128 == 64 ? C * 2 : C * 2 + 64;     // bytes of a staged pixel row, off the 128-byte bank period
            pl.C = C; pl.NH = k.tr_passes;
            return lds_form(pl, P3Form::TapsK, (size_t)(pl.TH + 2) * 18 * rs + (size_t)pl.TH * 16 * 8 * C / pl.NH);
        }
        if (lds2 && (k.mfma_data & P3_UNPACK_FWD) && (C == 32 || C == 64) && ((long)B * H * W - 1) * p.ldx + C < lim) {
            if (!set_tiles(pl, {C == 32 ? 8 : 4, 16}, H, W, B)) return pl;
            pl.C = C; pl.HILO = one;
            lds_form(pl, P3Form::Mfma, (size_t)2 * (((pl.TH + 2) * 18 + 15) / 16) * (C / 8 + 2) * 256).grid_x = (unsigned)min_int(pl.ntiles, k.persist_wgs);      // two tile buffers
            return pl;
        }
        return gather(pl, p, (long)B * H * W, 0, 0);
    case P3Op::UnpackBwdData:
        if (lds2 && (k.mfma_data & P3_UNPACK_BWD_DATA) && (C == 32 || C == 64)) {
            if (!set_tiles(pl, {C == 32 ? 8 : 4, 16}, H, W, B)) return pl;
            if (C == 32 && (k.mfma_data & P3_UNPACK_BWD_DATA_DMA) && ((long)B * 4 * H * W - 1) * p.ldo + 32 < lim) {
                pl.WAVES = (k.mfma_data & (P3_ONE_BF16_WEIGHT | P3_DMA_4_WAVES)) ? 4 : 2;      // (the one-value weights exist with four waves only)
                pl.HILO = one;
                lds_form(pl, P3Form::Dma32, (size_t)180 * 256).block = 64 * pl.WAVES;
                return pl;
            }
            pl.C = C; pl.HILO = one;
            return lds_form(pl, P3Form::Mfma, (size_t)4 * (pl.TH + 2) * (pl.TW + 2) * (C + 16) * 2);
        }
        if (lds2 && C % 32 == 0 && C <= 128) {
            if (!set_tiles(pl, up4_tile(C), H, W, B)) return pl;
            return lds_form(pl, P3Form::Lds4, up4_lds_bytes(C));
        }
        if (bf16 && k.lds && C % 32 == 0 && C <= 512) {
            if (!set_tiles(pl, up_tile(C), H, W, B)) return pl;
            return lds_form(pl, P3Form::Lds, up_lds_bytes(C));
        }
        return gather(pl, p, (long)B * H * W, 0, 0);
    case P3Op::UnpackBwdWeight:
        pl.clear_dwb = true;
        if (bf16 && k.lds && C % 32 == 0 && C <= 512) {
            P3Tile t = up_tile(C);
            if (k.small_tiles && t.TH >= 4) t.TH /= 2;      // kernels with generic item loops: half the LDS, twice the resident blocks
            if (!set_tiles(pl, t, H, W, B)) return pl;
            weight_shifts(pl, C);
            if (k.mfma) {
                lds_form(pl, P3Form::WeightMfma, p3_halo_bytes(t, C) + 16).grid_x = (unsigned)min_int(pl.ntiles, k.weight_wgs);
                pl.block = k.mfma_threads;
                return pl;
            }
            lds_form(pl, P3Form::WeightLds, p3_halo_bytes(t, C)).grid_x = (unsigned)min_int(pl.ntiles, k.small_tiles ? 1024 : 512);
            return pl;
        }
        return gather(pl, p, (long)B * H * W, 0, 256L * 2048);
    }
    pl.rc = MTE_ERR_ARG;
    return pl;
}
