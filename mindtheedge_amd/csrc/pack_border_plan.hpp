// Index arithmetic of the folded pack layers' exact border (csrc/pack_border.hip), free of HIP so that the host tests compile it alone.
//
// The folded convolution evaluates conv3d on the zero-extended packed tensor everywhere, the reference zeroes conv3d's result T outside the
// H2 x W2 image.  conv3d reaches one pixel, so outside the image T depends on the data only on the RING at distance 1:
//     y_ref(p) = y_fold(p) - sum_{t : p+t on the ring} W[t] . U(p+t) - sum_{t : p+t outside} S[t],     U = T - b3 on the ring.
// Ring lines (edge e): 0 top row y' = -1, 1 bottom row y' = H2, both over x' = -1 .. W2 (corners included, position i = x' + 1);
//                      2 left column x' = -1, 3 right column x' = W2, both over y' = 0 .. H2-1 (position i = y').
// Border pixels: j = distance to the near edge < pad = k/2.  A pixel j away from an edge meets that edge's ring line with ONE tap row / column.
// Pixel classes per axis: 0 .. pad-1 = that far from the low edge, pad = interior, 2 pad - j = j away from the high edge (needs extent >= 2 pad).
#pragma once

#ifndef PB_HD
#ifdef __HIPCC__
#define PB_HD __host__ __device__ inline
#else
#define PB_HD inline
#endif
#endif

#define PB_CLASS_SPLITS 64     // partial sums per pixel class (mte_pack_border_class_sums)
#define PB_RING_BLOCKS 64      // workgroups per edge of the ring stencil's weight gradient

// ---- the ring stencil ------------------------------------------------------------------------------------------------------------------
PB_HD int pb_edge_len(int e, int H2, int W2) { return e < 2 ? W2 + 2 : H2; }
// packed-image pixel (h, w) that tap a = 0..2 along edge e reads at ring position i; false = outside the image (contributes nothing)
PB_HD bool pb_edge_src(int e, int i, int a, int H2, int W2, int* h, int* w) {
    if (e < 2) { *h = e == 0 ? 0 : H2 - 1; *w = i + a - 2; return *w >= 0 && *w < W2; }
    *w = e == 2 ? 0 : W2 - 1; *h = i + a - 1; return *h >= 0 && *h < H2;
}
// index into K3[4][3][3][3] = [f][kd][dh][dw]: across the edge only the tap that reaches back into the image counts
PB_HD int pb_k3_index(int e, int f, int kd, int a) {
    const int fix = (e == 0 || e == 2) ? 2 : 0;
    return e < 2 ? ((f * 3 + kd) * 3 + fix) * 3 + a : ((f * 3 + kd) * 3 + a) * 3 + fix;
}
// is pixel (h, w) on the source line of edge e?  If so, tap a of ring position i = *along + *off - a reads it (for the i that lie inside the edge's length)
PB_HD bool pb_edge_of_pixel(int e, int h, int w, int H2, int W2, int* along, int* off) {
    if (e < 2) { *along = w; *off = 2; return h == (e == 0 ? 0 : H2 - 1); }
    *along = h; *off = 1; return w == (e == 2 ? 0 : W2 - 1);
}

// ---- the border GEMMs --------------------------------------------------------------------------------------------------------------------
// tap row (column) with which a pixel j away from the near (far = 0) / far (far = 1) edge meets that edge's ring line
PB_HD int pb_tap(int far, int j, int pad) { return far ? pad + 1 + j : pad - 1 - j; }
// GEMM column of (far, j, co): the edges and distances are stacked in the output-channel dimension
PB_HD int pb_col(int far, int j, int co, int pad, int Co) { return (far * pad + j) * Co + co; }
// the (far, j) whose tap is t; false for the centre tap, which never leaves the image
PB_HD bool pb_tap_owner(int t, int pad, int* far, int* j) {
    if (t == pad) return false;
    *far = t > pad; *j = t > pad ? t - pad - 1 : pad - 1 - t;
    return true;
}
PB_HD int pb_class(int r, int n, int pad) { return r < pad ? r : (n - 1 - r < pad ? 2 * pad - (n - 1 - r) : pad); }
PB_HD bool pb_tap_outside(int cls, int t, int pad) { return cls < pad ? t < pad - cls : (cls > pad ? t > 3 * pad - cls : false); }
PB_HD int pb_class_count(int cls, int n, int pad) { return cls == pad ? n - 2 * pad : 1; }     // pixels of a class along one axis
PB_HD int pb_class_first(int cls, int n, int pad) { return cls < pad ? cls : (cls == pad ? pad : n - 1 - (2 * pad - cls)); }

// border pixels in a fixed order: pad top rows, pad bottom rows, then the left and right columns between them
PB_HD long pb_border_count(int H2, int W2, int pad) { return 2L * pad * W2 + 2L * pad * (H2 - 2 * pad); }
PB_HD void pb_border_pixel(long idx, int H2, int W2, int pad, int* r, int* x) {
    const long rows = 2L * pad * W2;
    if (idx < rows) { const int q = (int)(idx / W2); *x = (int)(idx % W2); *r = q < pad ? q : H2 - 2 * pad + q; return; }
    idx -= rows;
    const int q = (int)(idx % (2 * pad));
    *r = pad + (int)(idx / (2 * pad)); *x = q < pad ? q : W2 - 2 * pad + q;
}
PB_HD bool pb_shape_ok(int H2, int W2, int k) { return (k & 1) && k >= 3 && H2 >= 2 * (k / 2) && W2 >= 2 * (k / 2); }

// ---- the forward ring GEMMs as ONE grouped split-K launch (mte_pack_border_gemm_fwd) -------------------------------------------------------
// Line-batch (far', b) only ever uses the output columns (far, j, co) with far == far' (border_apply_kernel reads no others), so the two GEMMs of a layer are
// four independent ones of half the width: group g = 2 * family + far, family 0 = ring rows (n = W2 + 2 positions per line), 1 = ring columns (n = H2);
//     out[far * B * n + m][far * Ng + c] = sum_{t < k, ch < Cin} x[far * B * n + m + t - pad][ch] * w[far * Ng + c][t][ch]      (the tap stays inside line m / n)
// with M = B * n rows, Ng = pad * Co columns and K = k * Cin.  One grid covers the PBG_BM x PBG_BN tiles of the four groups times `splits` slices of K;
// a slice is a whole number of K-steps (PBG_KSTEP channels of one tap), every slice but the last has `per_split` of them, none is empty.  Slice s writes
// its partial tile into slab s of its family: fp32 [splits][2B][n][N], N = 2 Ng, the layout of the unsplit ring terms (the cross blocks far != far' are never
// written and never read); the consumer adds the slabs in slice order.  No atomics, no tickets, no workgroup waits for another.
// All four groups take the SAME split count: every workgroup then runs the same number of K-steps, and what the launch takes is one workgroup's time as
// long as they all fit the chip at once (the three training layers have 54-106 tiles: 3-5 slices give 270-318 workgroups of 20-40 K-steps).
#define PBG_BM 128             // tile rows (ring positions)
#define PBG_BN 64              // tile columns (output channels of one edge)
#define PBG_KSTEP 32           // channels per K-step: one MFMA reduction, 64 bytes of a row
#define PBG_STAGE 2            // K-steps staged per barrier; per_split is a multiple of it when there is more than one slice
#define PBG_RING 3             // LDS slots of one stage each: PBG_RING - 1 stages in flight
#define PBG_MAX_SPLITS 8
#define PBG_MIN_KSTEPS 16      // a slice shorter than this is not worth its slab: K below twice that (K < 1024) is not split

// elements of one slab of a family (0 rows, 1 columns): [2B][n][N]
PB_HD long pb_gemm_slab_elems(int family, int B, int H2, int W2, int Co, int k) { return 2L * B * (family ? H2 : W2 + 2) * (2 * (k / 2) * Co); }

struct PbGemmPlan {
    int rc;                    // 0, or -3 (MTE_ERR_UNSUPPORTED): a shape this launch does not take
    int bm, bn;                // tile form
    int ksteps;                // K-steps of the whole reduction, k * Cin / PBG_KSTEP
    int per_split;             // K-steps per slice (the last slice: the rest, at least one)
    int splits[4];             // slices per group (equal, see above)
    int M[4];                  // rows per group
    int n[4];                  // positions per line
    int tiles_m[4], tiles_n;   // tiles per group along M, along Ng
    int block0[5];             // first workgroup of each group; block0[4] = grid
    int grid, threads, lds_bytes;
    int Ng, N, Cin, taps, pad, B;
    long slab[2];              // elements of one slab per family: 2B * n * N
    long ws_off[2];            // first element of each family's slabs in the workspace
    long ws_elems;             // fp32 elements of the workspace
};

// force_splits > 0 (tests): that many slices where K has them, whatever the shape
inline PbGemmPlan plan_pack_border_gemm(int B, int H2, int W2, int Cin, int Co, int k, bool bf16, int cus, int force_splits = 0) {
    PbGemmPlan p = {};
    p.rc = -3;
    if (!bf16 || B <= 0 || Co <= 0 || Co % 8 != 0 || Cin <= 0 || Cin % PBG_KSTEP != 0 || k > 5 || !pb_shape_ok(H2, W2, k)) return p;
    const long lines = 2L * B * ((long)W2 + 2 > H2 ? (long)W2 + 2 : H2);
    if (lines * Cin >= (1L << 30) || lines * 2 * (k / 2) * Co >= (1L << 30) || 2L * (k / 2) * Co * k * Cin >= (1L << 30)) return p;   // 32-bit element indices in the kernel
    p.rc = 0;
    p.bm = PBG_BM; p.bn = PBG_BN; p.threads = 256;
    p.lds_bytes = PBG_RING * PBG_STAGE * (PBG_BM + PBG_BN) * 64;
    p.B = B; p.Cin = Cin; p.taps = k; p.pad = k / 2; p.Ng = p.pad * Co; p.N = 2 * p.Ng;
    p.ksteps = k * (Cin / PBG_KSTEP);
    p.tiles_n = (p.Ng + PBG_BN - 1) / PBG_BN;
    int tiles = 0;
    for (int g = 0; g < 4; ++g) {
        p.n[g] = g < 2 ? W2 + 2 : H2;
        p.M[g] = B * p.n[g];
        p.tiles_m[g] = (p.M[g] + PBG_BM - 1) / PBG_BM;
        tiles += p.tiles_m[g] * p.tiles_n;
    }
    int want = cus > tiles ? (cus + tiles - 1) / tiles : 1;
    if (want > PBG_MAX_SPLITS) want = PBG_MAX_SPLITS;
    if (want > p.ksteps / PBG_MIN_KSTEPS) want = p.ksteps / PBG_MIN_KSTEPS;
    if (force_splits > 0) want = force_splits < p.ksteps ? force_splits : p.ksteps;
    if (want < 1) want = 1;
    p.per_split = (p.ksteps + want - 1) / want;
    if (want > 1) p.per_split = (p.per_split + PBG_STAGE - 1) / PBG_STAGE * PBG_STAGE;
    const int splits = (p.ksteps + p.per_split - 1) / p.per_split;         // no empty slice
    for (int g = 0; g < 4; ++g) {
        p.splits[g] = splits;
        p.block0[g] = g ? p.block0[g - 1] + p.tiles_m[g - 1] * p.tiles_n * splits : 0;
    }
    p.block0[4] = p.grid = p.block0[3] + p.tiles_m[3] * p.tiles_n * splits;
    for (int f = 0; f < 2; ++f) p.slab[f] = pb_gemm_slab_elems(f, B, H2, W2, Co, k);
    p.ws_off[0] = 0; p.ws_off[1] = splits * p.slab[0];
    p.ws_elems = splits * (p.slab[0] + p.slab[1]);
    return p;
}
// workgroup -> (group, slice, tile): a group's workgroups are slice-major, then tile rows, then tile columns
PB_HD void pb_gemm_block(const PbGemmPlan& p, int block, int* g, int* split, int* tile_m, int* tile_n) {
    int gg = 0;
    while (gg < 3 && block >= p.block0[gg + 1]) ++gg;
    const int tiles = p.tiles_m[gg] * p.tiles_n;
    int idx = block - p.block0[gg];
    *g = gg; *split = idx / tiles;
    idx -= *split * tiles;
    *tile_m = idx / p.tiles_n; *tile_n = idx - *tile_m * p.tiles_n;
}
// K-steps [*s0, *s1) of slice s
PB_HD void pb_gemm_slice(int ksteps, int per_split, int s, int* s0, int* s1) {
    *s0 = s * per_split;
    *s1 = *s0 + per_split < ksteps ? *s0 + per_split : ksteps;
}
// workspace element of (group g, slice s, row m of the group, column c of the group)
PB_HD long pb_gemm_ws_index(const PbGemmPlan& p, int g, int s, int m, int c) {
    const int f = g >> 1, far = g & 1;
    return p.ws_off[f] + s * p.slab[f] + ((long)far * p.M[g] + m) * p.N + far * p.Ng + c;
}
