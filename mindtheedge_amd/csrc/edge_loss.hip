// Fused depth-edge loss and silog loss for gfx950 (fp32 NCHW maps with C = 1, i.e. plain [B,H,W]).
//
// Edge loss = GradLoss.forward with edge_loss_type 'cross_entropy' (packnet_sfm/losses/grad_loss.py:122-219)
// fused with inv2depth (utils/depth.py:104-121) and GradLayer (grad_loss.py:20-31,65-95):
//   depth = 1/max(inv,1e-6) -> 4 Sobel responses (v,h,lr,rl; zero pad) -> per-pixel direction chosen by the
//   edge-normal angle (or sqrt(v^2+h^2+1e-6) without normals) -> p = sigmoid(g - thresh)
//   -> pos = -e log(p+1e-3), neg = -(1-e) log(1-p+1e-3) -> per-sample class-balance alpha -> weighted mean.
// Silog = SupervisedLoss 'sparse-silog', one scale (losses/supervised_loss.py:57-69,155-216).
//
// The reference issues 4 conv2d + ~20 masking kernels + torch.unique (host syncs) per scale.  Here ONE forward launch
// covers all four scales (+ the silog sums, which read the same full-resolution inverse depth) and ONE backward launch
// writes all four gradients (+ the silog gradient):
//   * workgroup = one 64 x 32-pixel tile of one (scale, sample); the tile + halo of the prediction is staged in LDS as
//     DEPTH (the reciprocal is taken once per pixel, halo overhead 10 % / 20 %); a thread owns 4 consecutive pixels of a
//     row, so every global access is a 16-byte load / store (1 KiB per wave instruction);
//   * every global load of a workgroup (tile + halo, labels, normals) is issued before its first use, so a workgroup pays
//     one memory latency, not one per phase;
//   * sums: fp32 per thread and per wave, fp64 per workgroup; a workgroup leaves ONE 128-byte record, the last workgroup of a
//     (scale, sample) to arrive (agent-scope ticket) adds that image's <= 240 records in a fixed order, and the LAST of those computes
//     alpha, the loss scalars and the backward coefficients on the device from an LDS copy of the 32 images' sums (one thread per
//     scale): no reduce / finalize launches, no host sync, no floating-point atomics -- losses and coefficients are bit-reproducible
//     (round 4; rounds 1-3 added each value with one fp64 atomic per workgroup: 1,680 adds on one cache line per full-resolution
//     image cost half of the launch, and the single-thread scalar tail another 15 us: forward 73 -> see profiles/README.md).
// HBM-bound: 12 B/pixel forward (inv, edge, normal), 16 B/pixel backward (+4 B gradient write).
//
// This file holds the generic kernels (every runtime flag: masks, magnitude mode, probability maps, unaligned widths), the stand-alone silog
// kernels and every entry point.  edge_fast.hpp holds what the kernels share (launch description, record / ticket tail, finish) and the kernels of
// the training configuration, template <int NBR>: <1> behind mte_edge_loss_multi_*, <2> behind mte_edge_loss_pair_* (two predictions, one label set).
#include "edge_fast.hpp"

int g_mte_loss_prezeroed = 0;

namespace {

struct EdgeScale : TileGrid {
    const float* pred;                  // inv-depth (from_inv), depth, or probability map
    const float* edge; const float* normal; const float* mask;    // normal / mask nullable
    float* gmap;                        // forward: optional edge-strength map output
    float* dpred;                       // backward output
    int vec;                            // 16-byte accesses are legal (W % 4 == 0, aligned bases)
};
struct EdgeMulti : LossLaunch {         // one prediction per label set
    EdgeScale s[MAXS];
    int from_inv, is_grad, is_sigmoid, finalize;
};

// ---------------- forward -----------------------------------------------------------------------------------------

// FAST = the training configuration on every scale (16-byte accesses legal, inverse depth in, Sobel + normals + sigmoid, no mask):
// the flags are compile-time there.  The generic instantiation carries every runtime flag -- its body is ~10k instructions
// (scalar and vector access paths, magnitude / probability / mask branches), several times what the instruction cache likes.
template <bool FAST>
__global__ __launch_bounds__(256, FAST ? 4 : 2) void edge_loss_fwd_kernel(EdgeMulti a) {
    __shared__ __attribute__((aligned(16))) float sd[(TH + 2) * LS];
    __shared__ float sred[4][NP];
    __shared__ int s_last;
    const BlockId id = decode_block(a);
    const EdgeScale& sc = a.s[id.s];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = (tid & 15) * 4, r0 = tid >> 4;                   // this thread's 4 pixels: columns c..c+3 of rows r0 and r0 + 16
    const bool has_mask = FAST ? false : sc.mask != nullptr;
    const bool silog = a.gt_depth != nullptr && id.s == 0;
    const int vec = FAST ? 1 : sc.vec;
    const bool is_grad = FAST ? true : a.is_grad != 0, is_sigmoid = FAST ? true : a.is_sigmoid != 0;
    const bool has_normal = FAST ? true : sc.normal != nullptr;
    const int from_inv = FAST ? 1 : a.from_inv;
    const long img = (long)id.b * sc.H;

    float acc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) acc[i] = 0.f;
    // a workgroup walks `tiles_per_wg` consecutive tiles of its image and keeps the sums in registers: the record / ticket round trips
    // at the end (two dependent trips to the memory side, ~5 us with the slot held) are paid once per 3 tiles instead of per tile
    for (int t = id.t0; t < id.t1; ++t) {
    const int x0 = (t % sc.tiles_x) * TW, y0 = (t / sc.tiles_x) * TH;
    if (t != id.t0) __syncthreads();                              // the previous tile's window reads are done
        // every global load of the workgroup first: one memory latency for the tile, the labels and the normals together
        DepthTile<1> tile;
        if (is_grad) tile.issue(sc, vec, id.b, x0, y0);
        f32x4_t e4[2], n4[2], m4[2], d4[2], i4[2];
    #pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int gy = y0 + r0 + 16 * ps;
            const bool ok = gy < sc.H;
            e4[ps] = ok ? load4(sc.edge, img + gy, x0 + c, sc.W, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (has_normal && is_grad) n4[ps] = ok ? load4(sc.normal, img + gy, x0 + c, sc.W, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (has_mask) m4[ps] = ok ? load4(sc.mask, img + gy, x0 + c, sc.W, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (silog) {
                d4[ps] = ok ? load4(a.gt_depth, img + gy, x0 + c, sc.W, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
                i4[ps] = ok ? load4(sc.pred, img + gy, x0 + c, sc.W, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
            if (!is_grad) i4[ps] = ok ? load4(sc.pred, img + gy, x0 + c, sc.W, vec) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        if (is_grad) tile.commit(sc, from_inv, x0, y0, sd);
        __syncthreads();

#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int ly = r0 + 16 * ps, gy = y0 + ly;
        if (gy >= sc.H) continue;
        float w[3][6];
        if (is_grad) window(sd, ly + 1, c, w);
        f32x4_t g4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x0 + c + k >= sc.W) { g4[k] = 0.f; continue; }
            float g;
            if (is_grad) {
                float sh, sv, srl, slr;
                sobel4(w, k, sh, sv, srl, slr);
                if (has_normal) {
                    const int code = direction_code(n4[ps][k]);
                    g = fabsf(code == 0 ? sh : (code == 1 ? sv : (code == 2 ? srl : slr)));
                } else {
                    g = sqrtf(sv * sv + sh * sh + 1e-6f);
                }
            } else {
                g = i4[ps][k];
            }
            g4[k] = g;
            // p = 1 / (1 + t), 1 - p = t p with t = exp(-(g - thresh)): the reference forms 1 - p by subtraction in float32, which
            // loses everything once p rounds towards 1 (g - thresh > ~8); t p is exact to an ulp and agrees wherever that is defined
            float p, omp;
            if (is_sigmoid) { const float t = fast_exp(-(g - a.thresh)); p = rcpf(1.f + t); omp = t * p; }
            else { p = g; omp = 1.f - g; }
            const float e = e4[ps][k];
#if defined(MTE_EDGE_ABLATE) && (MTE_EDGE_ABLATE & 2)
            const float pos = -e * g, neg = -(1.f - e) * g;          // diagnostic: no exp / rcp / log
#else
            const float pos = -e * fast_log(p + 0.001f), neg = -(1.f - e) * fast_log(omp + 0.001f);
#endif
            acc[2] += pos; acc[3] += neg;
            if (has_mask) {
                const float m = m4[ps][k];
                const float keep = m != 0.f ? 1.f : 0.f;
                acc[0] += e * m; acc[1] += (1.f - e) * m;
                acc[4] += pos * keep; acc[5] += neg * keep;
                acc[6] += m == 0.f ? 1.f : 0.f; acc[7] += m == 1.f ? 1.f : 0.f; acc[8] += (m != 0.f && m != 1.f) ? 1.f : 0.f; acc[9] += m;
            } else {
                acc[0] += e; acc[1] += 1.f - e;
            }
            if (silog) {
                const float d = d4[ps][k];
                if (d > 0.f) {
                    const float gt = rcpf(fmaxf(d, 1e-6f));           // feeds a log: 1 ulp here is 6e-8 absolute there
                    const float dl = fast_log((i4[ps][k] + 1e-5f) * 10.f) - fast_log(gt * 10.f);
                    acc[10] += dl; acc[11] = fmaf(dl, dl, acc[11]); acc[12] += 1.f;
                }
            }
        }
        if (!FAST && sc.gmap) store4(sc.gmap, img + gy, x0 + c, sc.W, vec, g4);
    }
    }   // tiles of this workgroup
#if defined(MTE_EDGE_ABLATE) && (MTE_EDGE_ABLATE & 1)
    { float tt = 0.f; for (int i = 0; i < NP; ++i) tt += acc[i]; if (tt == 123.456f) a.losses[0] = tt; return; }      // diagnostic: no reductions, atomics, tickets
#endif
    forward_tail<1, true>(a, id, acc, has_mask, silog, a.finalize != 0, sd, sred, &s_last);
}

// single-scale finalize (GradLoss called on its own): accumulators [B][NP] -> loss (accumulated into *loss_acc with factor
// out_scale) and backward coefficients
__global__ void edge_loss_finalize_kernel(const double* __restrict__ sums, int B, long numel, float weight, float pos_to_neg,
                                          int has_mask, float out_scale, float* __restrict__ loss_acc, float* __restrict__ loss_this,
                                          float* __restrict__ coef) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const PlainView R0{sums};
    const ScaleStats st = scale_stats(R0, 0, B, has_mask != 0, (double)numel);
    double total = 0.0;
    for (int b = 0; b < B; ++b) total += sample_term(weight, pos_to_neg, R0, (long)b * NP, st, coef, b);
    coef[2 * B] = st.binary ? 1.f : 0.f;
    const float l = (float)((double)weight * total / st.nvalid);
    if (loss_this) *loss_this = l;
    if (loss_acc) *loss_acc += out_scale * l;
}

// ---------------- backward ----------------------------------------------------------------------------------------
// Transposed Sobel.  d s_code(p) / d depth(p + t) for tap t = (dy, dx) is  h: dx (2 - |dy|), v: dy (2 - |dx|), rl: dx - dy, lr: dx + dy.  With the
// four tap patterns X[t] = dx, Y[t] = dy, Xc[t] = dx [dy = 0], Yc[t] = dy [dx = 0] these are h = X + Xc, v = Y + Yc, rl = X - Y, lr = X + Y, so
//   d loss / d depth(q) = sum_t  A(q - t) X[t] + B(q - t) Y[t] + C(q - t) Xc[t] + D(q - t) Yc[t]
// with per-pixel planes A = G [code != v], B = G (v: 1, rl: -1, lr: 1, h: 0), C = G [code = h], D = G [code = v].  X and Y are separable
// (column sums of A, row differences of B shared by the 4 pixels of a thread), Xc / Yc touch one row / one column, and C, D need no storage:
// C = A where B = 0, D = B where A = 0 (G = 0 makes all four vanish).  ~80 instructions per 4 pixels; the per-tap select by the neighbour's
// code it replaces (rounds 1-3) took ~420.  Magnitude mode (no normals): A = C = the h part, B = D = the v part.
template <bool FAST>
__global__ __launch_bounds__(256) void edge_loss_bwd_kernel(EdgeMulti a) {
    // depth on the tile + 2-pixel halo; the planes A, B of G = d loss / d s(p) on the tile + 1-pixel halo
    __shared__ __attribute__((aligned(16))) float sd[(TH + 4) * LS];
    __shared__ __attribute__((aligned(16))) float sga[(TH + 2) * LS], sgb[(TH + 2) * LS];        // planes A and B (see above)
    const BlockId id = decode_block(a);                            // one tile per workgroup (tiles_per_wg = 1)
    const EdgeScale& sc = a.s[id.s];
    const int x0 = (id.t0 % sc.tiles_x) * TW, y0 = (id.t0 / sc.tiles_x) * TH;
    const int tid = threadIdx.x;
    const int c = (tid & 15) * 4, r0 = tid >> 4;
    const long img = (long)id.b * sc.H;
    const float go = a.gout ? a.gout[id.s] : 1.f;
    const float* coef = a.coef + (long)id.s * (2 * a.B + 1);
    const float cpos = coef[2 * id.b] * go, cneg = coef[2 * id.b + 1] * go;
    const bool use_keep = FAST ? false : (coef[2 * a.B] != 0.f && sc.mask != nullptr);
    const bool silog = a.gt_depth != nullptr && id.s == 0;
    const bool magnitude = FAST ? false : sc.normal == nullptr;
    const int vec = FAST ? 1 : sc.vec;
    const bool is_grad = FAST ? true : a.is_grad != 0, is_sigmoid = FAST ? true : a.is_sigmoid != 0;
    const int from_inv = FAST ? 1 : a.from_inv;

    // ---- every global load of the workgroup is issued here: depth tile, labels / normals of the G region, inputs of the output phase
    constexpr int GITEMS = (TH + 2) * (TW / 4 + 2), NG = (GITEMS + 255) / 256;     // G region: interior groups of 4 + two halo columns per row
    DepthTile<2> tile;
    f32x4_t ge[NG], gn[NG], gm[NG];
    f32x4_t inv4[2], d4[2], oe4[2], om4[2];
    if (is_grad) {
        tile.issue(sc, vec, id.b, x0, y0);
#pragma unroll
        for (int k = 0; k < NG; ++k) {
            const int i = tid + k * 256;
            const int ly = i / (TW / 4 + 2), q = i % (TW / 4 + 2);               // q < 16: interior group, 16 / 17: left / right halo column
            const int gy = y0 + ly - 1;
            const bool group = q < TW / 4;
            const int j0 = group ? q * 4 : (q == TW / 4 ? -1 : TW);
            ge[k] = f32x4_t{0.f, 0.f, 0.f, 0.f}; gn[k] = ge[k]; gm[k] = f32x4_t{1.f, 1.f, 1.f, 1.f};
            if (i < GITEMS && (unsigned)gy < (unsigned)sc.H) {
                if (group) {
                    ge[k] = load4(sc.edge, img + gy, x0 + j0, sc.W, vec);
                    if (!magnitude) gn[k] = load4(sc.normal, img + gy, x0 + j0, sc.W, vec);
                    if (use_keep) gm[k] = load4(sc.mask, img + gy, x0 + j0, sc.W, vec);
                } else if ((unsigned)(x0 + j0) < (unsigned)sc.W) {
                    const long idx = (img + gy) * sc.W + x0 + j0;
                    ge[k][0] = sc.edge[idx];
                    if (!magnitude) gn[k][0] = sc.normal[idx];
                    if (use_keep) gm[k][0] = sc.mask[idx];
                }
            }
        }
    }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int gy = y0 + r0 + 16 * ps;
        const bool ok = gy < sc.H && x0 + c < sc.W;
        const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
        inv4[ps] = ok ? load4(sc.pred, img + gy, x0 + c, sc.W, vec) : z;
        if (silog) d4[ps] = ok ? load4(a.gt_depth, img + gy, x0 + c, sc.W, vec) : z;
        if (!is_grad) {
            oe4[ps] = ok ? load4(sc.edge, img + gy, x0 + c, sc.W, vec) : z;
            om4[ps] = (ok && use_keep) ? load4(sc.mask, img + gy, x0 + c, sc.W, vec) : f32x4_t{1.f, 1.f, 1.f, 1.f};
        }
    }
    if (is_grad) {
        tile.commit(sc, from_inv, x0, y0, sd);
        __syncthreads();
#pragma unroll
        for (int kq = 0; kq < NG; ++kq) {
            const int i = tid + kq * 256;
            if (i >= GITEMS) break;
            const int ly = i / (TW / 4 + 2), q = i % (TW / 4 + 2);
            const int gy = y0 + ly - 1;
            const bool group = q < TW / 4;
            const int j0 = group ? q * 4 : (q == TW / 4 ? -1 : TW);
            const int np = group ? 4 : 1;
            const f32x4_t e4 = ge[kq], n4 = gn[kq], m4 = gm[kq];
            const bool rowok = (unsigned)gy < (unsigned)sc.H;
            float w[3][6];
            if (group) window(sd, ly + 1, j0, w);
            else {                                                            // single column: centre it at window column 1
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int k = 0; k < 3; ++k) w[r][k] = sd[(ly + r) * LS + 4 + j0 - 1 + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= np) break;
                const int gx = x0 + j0 + k;
                float ga = 0.f, gb = 0.f;       // planes A (X coefficient) and B (Y coefficient)
                if (rowok && (unsigned)gx < (unsigned)sc.W) {
                    float sh, sv, srl, slr;
                    sobel4(w, k, sh, sv, srl, slr);
                    float g, da, db = 0.f;        // d g / d s_a, d g / d s_b
                    int code = 0;
                    if (!magnitude) {
                        code = direction_code(n4[k]);
                        const float s = code == 0 ? sh : (code == 1 ? sv : (code == 2 ? srl : slr));
                        g = fabsf(s);
                        da = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
                    } else {
                        g = sqrtf(sv * sv + sh * sh + 1e-6f);
                        da = sv / g; db = sh / g;                  // a = v, b = h
                    }
                    float p, omp;                  // p and 1 - p without cancellation (see the forward kernel)
                    if (is_sigmoid) { const float t = fast_exp(-(g - a.thresh)); p = rcpf(1.f + t); omp = t * p; }
                    else { p = g; omp = 1.f - g; }
                    const float e = e4[k];
                    const float keep = (use_keep && m4[k] == 0.f) ? 0.f : 1.f;
                    const float dp = is_sigmoid ? p * omp : 1.f;
                    const float dg = keep * dp * (-cpos * e * rcpf(p + 0.001f) + cneg * (1.f - e) * rcpf(omp + 0.001f));
                    if (magnitude) { ga = dg * db; gb = dg * da; }             // h part, v part
                    else {
                        const float G = dg * da;
                        ga = code != 1 ? G : 0.f;
                        gb = code == 1 ? G : (code == 2 ? -G : (code == 3 ? G : 0.f));
                    }
                }
                const int o = ly * LS + 4 + j0 + k;
                sga[o] = ga; sgb[o] = gb;
            }
        }
        __syncthreads();
    }
    const float m1 = silog ? a.silog_aux[0] : 0.f, ksl = silog ? a.silog_aux[1] * (a.silog_gout ? a.silog_gout[0] : 1.f) : 0.f;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int ly = r0 + 16 * ps, gy = y0 + ly;
        if (gy >= sc.H || x0 + c >= sc.W) continue;
        f32x4_t out = {0.f, 0.f, 0.f, 0.f};
        if (is_grad) {
            // the 3 x 6 windows of the planes around the 4 pixels; window column j = image column c - 1 + j, pixel k sits at column k + 1
            float wa[3][6], wb[3][6];
            window(sga, ly + 1, c, wa);
            window(sgb, ly + 1, c, wb);
            float ca[6], eb[6], cc1[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                ca[j] = (wa[0][j] + wa[1][j]) + wa[2][j];                                   // column sums of A
                eb[j] = wb[0][j] - wb[2][j];                                                // row above - row below of B
                cc1[j] = magnitude ? wa[1][j] : (wb[1][j] == 0.f ? wa[1][j] : 0.f);         // C on the centre row
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // source p at window (r, k + cc) reaches q = (1, k + 1) with t = q - p = (1 - r, 1 - cc)
                const float d0 = magnitude ? wb[0][k + 1] : (wa[0][k + 1] == 0.f ? wb[0][k + 1] : 0.f);       // D above / below q
                const float d2 = magnitude ? wb[2][k + 1] : (wa[2][k + 1] == 0.f ? wb[2][k + 1] : 0.f);
                float dd = (ca[k] - ca[k + 2]) + ((eb[k] + eb[k + 1]) + eb[k + 2]) + (cc1[k] - cc1[k + 2]) + (d0 - d2);
                if (from_inv) {
                    const float inv = inv4[ps][k];
                    const float d = rcpf(fmaxf(inv, 1e-6f));
                    dd = inv >= 1e-6f ? -dd * d * d : 0.f;
                }
                out[k] = dd;
            }
        } else {
            const f32x4_t e4 = oe4[ps], m4 = om4[ps];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float g = inv4[ps][k];
                float p, omp;
                if (is_sigmoid) { const float t = fast_exp(-(g - a.thresh)); p = rcpf(1.f + t); omp = t * p; }
                else { p = g; omp = 1.f - g; }
                const float keep = (use_keep && m4[k] == 0.f) ? 0.f : 1.f;
                const float dp = is_sigmoid ? p * omp : 1.f;
                out[k] = keep * dp * (-cpos * e4[k] * rcpf(p + 0.001f) + cneg * (1.f - e4[k]) * rcpf(omp + 0.001f));
            }
        }
        if (silog) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = d4[ps][k];
                if (d > 0.f) {
                    const float gt = rcpf(fmaxf(d, 1e-6f));           // feeds a log: 1 ulp here is 6e-8 absolute there
                    const float pi = inv4[ps][k] + 1e-5f;
                    const float dl = fast_log(pi * 10.f) - fast_log(gt * 10.f);
                    out[k] += ksl * (dl - 0.85f * m1) * rcpf(pi);
                }
            }
        }
        store4(sc.dpred, img + gy, x0 + c, sc.W, vec, out);
    }
}

// ---------------- silog (stand-alone: SupervisedLoss used without the edge loss) -------------------------------------
__global__ __launch_bounds__(256) void silog_fwd_kernel(const float* __restrict__ inv, const float* __restrict__ depth, long n, double* __restrict__ sums) {
    __shared__ double sred[4][3];
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float d = depth[i];
        if (d > 0.f) {
            const float g = 1.f / fmaxf(d, 1e-6f);
            const float dl = logf((inv[i] + 1e-5f) * 10.f) - logf(g * 10.f);
            s1 += dl; s2 += (double)dl * dl; cnt += 1.0;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s1 = wave_sum_d(s1); s2 = wave_sum_d(s2); cnt = wave_sum_d(cnt);
    if (lane == 0) { sred[wave][0] = s1; sred[wave][1] = s2; sred[wave][2] = cnt; }
    __syncthreads();
    if (threadIdx.x < 3) atomicAdd(&sums[threadIdx.x], sred[0][threadIdx.x] + sred[1][threadIdx.x] + sred[2][threadIdx.x] + sred[3][threadIdx.x]);
}
// loss = 10 sqrt(E[d^2] - 0.85 E[d]^2);  aux = (mean, 10/sqrt(S)/n)
__global__ void silog_finalize_kernel(const double* __restrict__ sums, float out_scale, float* __restrict__ loss_acc, float* __restrict__ loss_this, float* __restrict__ aux) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double n = sums[2];
    const double m1 = sums[0] / n, m2 = sums[1] / n;
    const double S = m2 - 0.85 * m1 * m1;
    const float l = (float)(sqrt(S) * 10.0);
    if (loss_this) *loss_this = l;
    if (loss_acc) *loss_acc += out_scale * l;
    aux[0] = (float)m1;
    aux[1] = (float)(10.0 / sqrt(S) / n);
}
__global__ void silog_bwd_kernel(const float* __restrict__ inv, const float* __restrict__ depth, const float* __restrict__ aux,
                                 const float* __restrict__ gout, float* __restrict__ dinv, long n, int accumulate) {
    const float m1 = aux[0], k = aux[1] * (gout ? gout[0] : 1.f);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float d = depth[i];
        float gr = 0.f;
        if (d > 0.f) {
            const float g = 1.f / fmaxf(d, 1e-6f);
            const float pi = inv[i] + 1e-5f;
            const float dl = logf(pi * 10.f) - logf(g * 10.f);
            gr = k * (dl - 0.85f * m1) / pi;
        }
        dinv[i] = accumulate ? dinv[i] + gr : gr;
    }
}

// public scale records of include/mte_kernels.h
struct mte_edge_scale_t { const float* pred; const float* edge; const float* normal; const float* mask; float* gmap; float* dpred; int H, W; };
struct mte_edge_pair_scale_t { const float* pred[2]; float* dpred[2]; const float* edge; const float* normal; int H, W; };

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Grid geometry of a launch from H, W of its scales: tiles, first workgroup and workgroups per image of each.  nbr: records per workgroup.
// -> workgroups of the launch, or MTE_ERR_ARG where an int no longer indexes the records
template <typename A> int place_scales(A& a, int nscales, int B, bool backward, int nbr) {
    const int T = backward ? 1 : FWD_TILES_PER_WG;
    long blocks = 0;
    for (int s = 0; s < nscales; ++s) {
        TileGrid& o = a.s[s];
        o.tiles_x = (o.W + TW - 1) / TW; o.tiles_y = (o.H + TH - 1) / TH;
        o.first_block = (int)blocks;
        o.groups = (o.tiles_x * o.tiles_y + T - 1) / T;
        blocks += (long)o.groups * B;
        if (blocks > 0x7fffffffL / (nbr * REC)) return MTE_ERR_ARG;
    }
    a.nscales = nscales; a.B = B; a.nblocks = (int)blocks; a.tiles_per_wg = T;
    return (int)blocks;
}

// -> workgroups, or MTE_ERR_ARG
int setup_scales(EdgeMulti& a, const mte_edge_scale_t* scales, int nscales, int B, bool backward) {
    if (!scales || nscales < 1 || nscales > MAXS || B < 1) return MTE_ERR_ARG;
    for (int s = 0; s < nscales; ++s) {
        const mte_edge_scale_t& in = scales[s];
        if (!in.pred || !in.edge || in.H < 1 || in.W < 1 || (backward && !in.dpred)) return MTE_ERR_ARG;
        EdgeScale& o = a.s[s];
        o.pred = in.pred; o.edge = in.edge; o.normal = in.normal; o.mask = in.mask; o.gmap = backward ? nullptr : in.gmap; o.dpred = in.dpred;
        o.H = in.H; o.W = in.W;
        o.vec = in.W % 4 == 0 && aligned16(in.pred) && aligned16(in.edge) && aligned16(in.normal) && aligned16(in.mask) &&
                aligned16(in.gmap) && aligned16(in.dpred);
    }
    return place_scales(a, nscales, B, backward, 1);
}
// -> workgroups, MTE_ERR_ARG, or (check_config) MTE_ERR_UNSUPPORTED where a scale is outside the training configuration
int setup_scales(FastArgs<2>& a, const mte_edge_pair_scale_t* scales, int nscales, int B, bool backward, bool check_config) {
    if (!scales || nscales < 1 || nscales > MAXS || B < 1) return MTE_ERR_ARG;
    bool supported = true;
    for (int s = 0; s < nscales; ++s) {
        const mte_edge_pair_scale_t& in = scales[s];
        if (!in.pred[0] || !in.pred[1] || !in.edge || in.H < 1 || in.W < 1 || (backward && (!in.dpred[0] || !in.dpred[1]))) return MTE_ERR_ARG;
        if (!in.normal || in.W % 4 != 0 || !aligned16(in.pred[0]) || !aligned16(in.pred[1]) || !aligned16(in.edge) || !aligned16(in.normal) ||
            (backward && (!aligned16(in.dpred[0]) || !aligned16(in.dpred[1]))))
            supported = false;
        FastScale<2>& o = a.s[s];
        for (int br = 0; br < 2; ++br) { o.pred[br] = in.pred[br]; o.dpred[br] = in.dpred[br]; }
        o.edge = in.edge; o.normal = in.normal;
        o.H = in.H; o.W = in.W;
    }
    const int blocks = place_scales(a, nscales, B, backward, 2);
    return blocks >= 0 && check_config && !supported ? MTE_ERR_UNSUPPORTED : blocks;
}

// every scale in the training configuration (edge_fast.hpp)?
bool fast_config(const EdgeMulti& a) {
    if (!a.from_inv || !a.is_grad || !a.is_sigmoid) return false;
    for (int s = 0; s < a.nscales; ++s)
        if (!a.s[s].vec || !a.s[s].normal || a.s[s].mask || a.s[s].gmap) return false;
    return true;
}
// the same launch for the one-branch fast kernels
FastArgs<1> fast_args(const EdgeMulti& a) {
    FastArgs<1> f{};
    static_cast<LossLaunch&>(f) = a;
    for (int s = 0; s < a.nscales; ++s) {
        const EdgeScale& in = a.s[s];
        static_cast<TileGrid&>(f.s[s]) = in;
        f.s[s].pred[0] = in.pred; f.s[s].dpred[0] = in.dpred; f.s[s].edge = in.edge; f.s[s].normal = in.normal;
    }
    return f;
}

// workspace of a forward launch, in doubles: [nbr][nscales][B][NP] sums, the tickets (a 16-byte multiple), one record per (workgroup, branch)
long results_elems(int nbr, int nscales, int B) { return ((long)nbr * nscales * B * NP + 1) & ~1L; }
long counter_elems(int nscales, int B) { return (((long)nscales * B + 1) * 4 + 15) / 16 * 2; }
long work_elems(const LossLaunch& a, int nbr) { return results_elems(nbr, a.nscales, a.B) + counter_elems(a.nscales, a.B) + (long)a.nblocks * nbr * REC; }
// points the launch into `work` and zeroes sums + tickets (the records are overwritten) unless they are handed in zeroed
bool carve_work(LossLaunch& a, double* work, int nbr, hipStream_t stream) {
    const long r = results_elems(nbr, a.nscales, a.B), c = counter_elems(a.nscales, a.B);
    a.results = work; a.counter = (unsigned*)(work + r); a.records = work + r + c;
    return g_mte_loss_prezeroed || mte_memset_async(work, 0, sizeof(double) * (r + c), stream) == hipSuccess;
}
void set_forward(LossLaunch& a, float thresh, float weight, float pos_to_neg, const float* gt_depth, float* losses, float* coef, float* silog_loss, float* silog_aux) {
    a.thresh = thresh; a.weight = weight; a.pos_to_neg = pos_to_neg; a.gt_depth = gt_depth; a.losses = losses; a.coef = coef;
    a.silog_loss = silog_loss; a.silog_aux = silog_aux;
}
void set_backward(LossLaunch& a, float thresh, const float* coef, const float* gout, const float* gt_depth, const float* silog_aux, const float* silog_gout) {
    a.thresh = thresh; a.coef = (float*)coef; a.gout = gout; a.gt_depth = gt_depth; a.silog_aux = (float*)silog_aux; a.silog_gout = silog_gout;
}

}  // namespace

extern "C" {

// doubles of workspace for a forward launch over these scales: [nscales][B][13] sums + the arrival tickets + one 16-double record per workgroup
long mte_edge_loss_work_elems(const void* scales, int nscales, int B) {
    EdgeMulti a{};
    return setup_scales(a, (const mte_edge_scale_t*)scales, nscales, B, false) < 0 ? -1 : work_elems(a, 1);
}

// Forward of `nscales` (<= 4) depth-edge losses in ONE launch, the silog loss of scale 0 fused in when gt_depth != NULL.
// losses[s] <- weight * balanced BCE of scale s; coef [nscales][2B+1] <- backward coefficients; silog_loss / silog_aux[2].
int mte_edge_loss_multi_fwd(const void* scales, int nscales, int B, int from_inv, int is_grad, int is_sigmoid, float thresh,
                            float weight, float pos_to_neg, const float* gt_depth, double* work, float* losses, float* coef,
                            float* silog_loss, float* silog_aux, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    EdgeMulti a{};
    a.fences = g_mte_handoff_fences;
    const int blocks = setup_scales(a, (const mte_edge_scale_t*)scales, nscales, B, false);
    if (blocks < 0 || !work || !losses || !coef || (gt_depth && (!silog_loss || !silog_aux))) return MTE_ERR_ARG;
    if (gt_depth && !aligned16(gt_depth)) a.s[0].vec = 0;
    a.from_inv = from_inv; a.is_grad = is_grad; a.is_sigmoid = is_sigmoid; a.finalize = 1;
    set_forward(a, thresh, weight, pos_to_neg, gt_depth, losses, coef, silog_loss, silog_aux);
    if (!carve_work(a, work, 1, stream)) return MTE_ERR_LAUNCH;
    if (fast_config(a)) hipLaunchKernelGGL(edge_fwd_fast_kernel<1>, dim3(blocks), dim3(256), 0, stream, fast_args(a));
    else hipLaunchKernelGGL(edge_loss_fwd_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}

// Backward of the same: dpred of every scale <- gout[s] * d loss_s / d pred_s (+ silog_gout * d silog / d pred_0 on scale 0).
int mte_edge_loss_multi_bwd(const void* scales, int nscales, int B, int from_inv, int is_grad, int is_sigmoid, float thresh,
                            const float* coef, const float* gout, const float* gt_depth, const float* silog_aux, const float* silog_gout,
                            hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    EdgeMulti a{};
    a.fences = g_mte_handoff_fences;
    const int blocks = setup_scales(a, (const mte_edge_scale_t*)scales, nscales, B, true);
    if (blocks < 0 || !coef || (gt_depth && !silog_aux)) return MTE_ERR_ARG;
    if (gt_depth && !aligned16(gt_depth)) a.s[0].vec = 0;
    a.from_inv = from_inv; a.is_grad = is_grad; a.is_sigmoid = is_sigmoid;
    set_backward(a, thresh, coef, gout, gt_depth, silog_aux, silog_gout);
    if (fast_config(a)) hipLaunchKernelGGL(edge_bwd_fast_kernel<1>, dim3(blocks), dim3(256), 0, stream, fast_args(a));
    else hipLaunchKernelGGL(edge_loss_bwd_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}

// ---- two predictions (RGB, RGB+LiDAR) against one label set, training configuration only: MTE_ERR_UNSUPPORTED for anything else, and the caller
//      makes two mte_edge_loss_multi_* calls.  Outputs are [2][...] of the single launch's; each branch is bit-equal to a single launch of it.
// doubles of workspace: [2][nscales][B][13] sums + the arrival tickets + two 16-double records per workgroup
long mte_edge_loss_pair_work_elems(const void* scales, int nscales, int B) {
    FastArgs<2> a{};
    return setup_scales(a, (const mte_edge_pair_scale_t*)scales, nscales, B, false, false) < 0 ? -1 : work_elems(a, 2);
}

int mte_edge_loss_pair_fwd(const void* scales, int nscales, int B, float thresh, float weight, float pos_to_neg, const float* gt_depth,
                           double* work, float* losses, float* coef, float* silog_loss, float* silog_aux, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    FastArgs<2> a{};
    a.fences = g_mte_handoff_fences;
    const int blocks = setup_scales(a, (const mte_edge_pair_scale_t*)scales, nscales, B, false, true);
    if (blocks == MTE_ERR_UNSUPPORTED) return MTE_ERR_UNSUPPORTED;
    if (blocks < 0 || !work || !losses || !coef || (gt_depth && (!silog_loss || !silog_aux))) return MTE_ERR_ARG;
    if (gt_depth && !aligned16(gt_depth)) return MTE_ERR_UNSUPPORTED;
    set_forward(a, thresh, weight, pos_to_neg, gt_depth, losses, coef, silog_loss, silog_aux);
    if (!carve_work(a, work, 2, stream)) return MTE_ERR_LAUNCH;
    hipLaunchKernelGGL(edge_fwd_fast_kernel<2>, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}

int mte_edge_loss_pair_bwd(const void* scales, int nscales, int B, float thresh, const float* coef, const float* gout, const float* gt_depth,
                           const float* silog_aux, const float* silog_gout, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    FastArgs<2> a{};
    a.fences = g_mte_handoff_fences;
    const int blocks = setup_scales(a, (const mte_edge_pair_scale_t*)scales, nscales, B, true, true);
    if (blocks == MTE_ERR_UNSUPPORTED) return MTE_ERR_UNSUPPORTED;
    if (blocks < 0 || !coef || (gt_depth && !silog_aux)) return MTE_ERR_ARG;
    if (gt_depth && !aligned16(gt_depth)) return MTE_ERR_UNSUPPORTED;
    set_backward(a, thresh, coef, gout, gt_depth, silog_aux, silog_gout);
    hipLaunchKernelGGL(edge_bwd_fast_kernel<2>, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}

// ---- single-scale entry points (GradLoss / GradLayer called directly): the same kernels with one scale
// doubles the caller must provide as `sums`: [B][13] sums (6 class-balance / BCE sums, 4 mask statistics, 3 unused) + the tickets + one 16-double record per workgroup
long mte_edge_loss_sums_elems(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return -1;
    EdgeMulti a{};
    a.s[0].H = H; a.s[0].W = W;
    return place_scales(a, 1, B, false, 1) < 0 ? -1 : work_elems(a, 1);
}

// Forward pass of one scale.  sums: mte_edge_loss_sums_elems(B, H, W) doubles (content on entry ignored).  gmap nullable.
int mte_edge_loss_fwd(const float* pred, const float* edge, const float* normal, const float* mask, double* sums, float* gmap,
                      int B, int H, int W, int from_inv, int is_grad, int is_sigmoid, float thresh, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!pred || !edge || !sums) return MTE_ERR_ARG;
    mte_edge_scale_t one{pred, edge, normal, mask, gmap, nullptr, H, W};
    EdgeMulti a{};
    a.fences = g_mte_handoff_fences;
    const int blocks = setup_scales(a, &one, 1, B, false);
    if (blocks < 0) return MTE_ERR_ARG;
    a.from_inv = from_inv; a.is_grad = is_grad; a.is_sigmoid = is_sigmoid; a.finalize = 0; a.thresh = thresh;
    if (!carve_work(a, sums, 1, stream)) return MTE_ERR_LAUNCH;
    hipLaunchKernelGGL(edge_loss_fwd_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}
// loss_this (nullable) <- weight * balanced BCE;  *loss_acc (nullable) += out_scale * loss;  coef: [2B + 1] floats
int mte_edge_loss_finalize(const double* sums, int B, long numel, float weight, float pos_to_neg, int has_mask,
                           float out_scale, float* loss_acc, float* loss_this, float* coef, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!sums || !coef) return MTE_ERR_ARG;
    hipLaunchKernelGGL(edge_loss_finalize_kernel, dim3(1), dim3(64), 0, stream, sums, B, numel, weight, pos_to_neg, has_mask, out_scale, loss_acc, loss_this, coef);
    return mte_check_launch();
}
// dpred <- gout * d loss / d pred  (gout: device scalar, nullable = 1)
int mte_edge_loss_bwd(const float* pred, const float* edge, const float* normal, const float* mask, const float* coef, const float* gout,
                      float* dpred, int B, int H, int W, int from_inv, int is_grad, int is_sigmoid, float thresh, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!pred || !edge || !coef || !dpred) return MTE_ERR_ARG;
    mte_edge_scale_t one{pred, edge, normal, mask, nullptr, dpred, H, W};
    return mte_edge_loss_multi_bwd(&one, 1, B, from_inv, is_grad, is_sigmoid, thresh, coef, gout, nullptr, nullptr, nullptr, stream);
}

// sums[3] doubles (zeroed here); aux[2] floats
int mte_silog_fwd(const float* inv, const float* depth, long n, double* sums, float out_scale, float* loss_acc, float* loss_this, float* aux, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!inv || !depth || !sums || !aux) return MTE_ERR_ARG;
    if (mte_memset_async(sums, 0, sizeof(double) * 3, stream) != hipSuccess) return MTE_ERR_LAUNCH;
    long g = (n + 255) / 256; if (g > 1024) g = 1024; if (g < 1) g = 1;
    hipLaunchKernelGGL(silog_fwd_kernel, dim3((unsigned)g), dim3(256), 0, stream, inv, depth, n, sums);
    hipLaunchKernelGGL(silog_finalize_kernel, dim3(1), dim3(64), 0, stream, sums, out_scale, loss_acc, loss_this, aux);
    return mte_check_launch();
}
int mte_silog_bwd(const float* inv, const float* depth, const float* aux, const float* gout, float* dinv, long n, int accumulate, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!inv || !depth || !aux || !dinv) return MTE_ERR_ARG;
    long g = (n + 255) / 256; if (g > 4096) g = 4096; if (g < 1) g = 1;
    hipLaunchKernelGGL(silog_bwd_kernel, dim3((unsigned)g), dim3(256), 0, stream, inv, depth, aux, gout, dinv, n, accumulate);
    return mte_check_launch();
}

}  // extern "C"
