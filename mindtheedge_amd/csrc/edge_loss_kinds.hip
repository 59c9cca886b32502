// The other edge-loss choices of GradLoss (packnet_sfm/losses/grad_loss.py:139-156), one scale per launch, fp32 NCHW maps with C = 1:
//   kind 0  'cross_entropy'       class-balanced BCE of comp_cross_entropy (grad_loss.py:161-219; edge_loss.hip computes the same sums)
//   kind 1  'attention_loss'      attention_loss2(p, t, m, False) (losses/attention_loss.py:21-49): focal-style weighted BCE, ONE alpha =
//                                 count(t == 0) / (count(t == 1) + count(t == 0)) over the whole batch
//   kind 2  'spatially_adaptive'  attention_loss2(p, t, m, True): per-pixel alpha = 1 - box15(t) / 225 (zero padding), 0.5 where that is
//                                 >= 1.0f (an all-negative window)
//   + dice ('dice' in the type string, grad_loss.py:151-156): 1000 (sum p^2 + sum t^2 + 1e-4) / (2 sum p t + 1e-4) / N, unmasked, not detached
//   loss = weight * (base + dice);  p = sigmoid(g - thresh) (or g itself), g = GradLayer of depth (or the input itself), depth = inv2depth(pred)
//   when from_inv.
//
// Layout (edge_loss.hip's generic kernels, single scale): a workgroup is one 64 x 32-pixel tile of one sample; a thread owns 4 consecutive pixels
// of rows r0 and r0 + 16 (16-byte accesses when W % 4 == 0); the prediction tile + halo is staged in LDS as DEPTH.  Kind 2 also stages the label
// tile with a 7-pixel halo (8 in the backward, whose alpha is needed on the 1-pixel G halo too) and forms the 15 x 15 box sum separably in LDS:
// binary labels give exact integer sums.
//
// Sums: fp32 per thread and per wave, fp64 per workgroup; the workgroup writes ONE record, the last workgroup of a sample to arrive (agent-scope
// ticket, returning vector atomics only) adds the sample's records in a fixed order, the last of those computes alpha, the loss and the backward
// coefficients in device memory.  No floating-point atomics, no host sync, bit-reproducible.  The attention loss factors as
// (alpha A + (1 - alpha) B) / N with A = sum m t 4^sqrt(1 - pc) bce, B = sum m (1 - t) 4^sqrt(pc) bce, so one pass suffices before the global
// alpha is known.  The backward recomputes p (and the box alpha) on the tile + halo, applies torch's BCE backward
// w (p - t) / max(p (1 - p), 1e-12) / N (+ the dice derivative), the sigmoid derivative p (1 - p), the transposed direction-selected Sobel
// stencil and the derivative of inv2depth.
#include "common.hpp"
#include "edge_direction.hpp"
#include "edge_tile.hpp"
#include "handoff.hpp"

namespace {

constexpr int NP = 13;                  // partial sums per workgroup (see the forward kernel)
constexpr int BR = 7;                   // box radius: 15 x 15 window
constexpr int NC = 4;                   // leading backward coefficients: alpha, weight / N, dice c1, dice c2

struct KindArgs {
    const float* pred; const float* edge; const float* normal; const float* mask;    // normal / mask nullable
    float* gmap;                        // forward: optional edge-strength map
    float* dpred;                       // backward output
    int B, H, W, tiles_x, tiles_y, vec;
    int kind, dice, from_inv, is_grad, is_sigmoid, fences;
    float thresh, weight, pos_to_neg;
    double* results;                    // [B][NP] sums of each sample (zeroed by the launcher)
    unsigned* counter;                  // [0] sample ticket, [1 + b] workgroup ticket of sample b (zeroed by the launcher)
    double* records;                    // [B * tiles][REC]
    float* loss;                        // forward out: the loss scalar
    float* coef;                        // forward out / backward in: [NC + 2B + 1]
    const float* gout;                  // backward: upstream gradient of the loss (device, nullable = 1)
};

// ---- 15 x 15 box alpha (attention_loss.py:27-31) ------------------------------------------------------------------------------------
// alpha on tile rows -AH .. TH+AH-1, columns -AH .. TW+AH-1 -> alpha[(ly + AH) * ACOLS + j + AH].  lab: ROWS x COLS floats (the alpha plane
// reuses it once the row sums are formed), hs: ROWS x ACOLS floats.
template <int AH> struct Box {
    static constexpr int R = AH + BR, ROWS = TH + 2 * R, COLS = TW + 2 * R, AROWS = TH + 2 * AH, ACOLS = TW + 2 * AH;
};
template <int AH> __device__ void box_alpha(const KindArgs& a, int b, int x0, int y0, float* lab, float* hs) {
    using G = Box<AH>;
    const float* img = a.edge + (long)b * a.H * a.W;
    for (int i = threadIdx.x; i < G::ROWS * G::COLS; i += 256) {
        const int r = i / G::COLS, j = i - r * G::COLS;
        const int gy = y0 - G::R + r, gx = x0 - G::R + j;
        lab[i] = ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) ? img[(long)gy * a.W + gx] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < G::ROWS * G::ACOLS; i += 256) {
        const int r = i / G::ACOLS, j = i - r * G::ACOLS;
        const float* p = lab + r * G::COLS + j;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * BR + 1; ++k) s += p[k];
        hs[i] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < G::AROWS * G::ACOLS; i += 256) {
        const int r = i / G::ACOLS, j = i - r * G::ACOLS;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * BR + 1; ++k) s += hs[(r + k) * G::ACOLS + j];
        const float v = 1.f - s / 225.f;
        lab[i] = v >= 1.f ? 0.5f : v;                              // float32(1 - 1e-14) == 1.0f
    }
    __syncthreads();
}

// ---- per-pixel loss terms -------------------------------------------------------------------------------------------------------------
// kind 0: p and 1 - p as edge_loss.hip forms them (1 - p = t p, no cancellation)
__device__ __forceinline__ void prob_ce(const KindArgs& a, float g, float& p, float& omp) {
    if (a.is_sigmoid) { const float t = fast_exp(-(g - a.thresh)); p = rcpf(1.f + t); omp = t * p; }
    else { p = g; omp = 1.f - g; }
}
// kinds 1, 2: torch's sigmoid and torch's 1 - p (p == 1.0f at large responses, where the BCE term saturates at -100)
__device__ __forceinline__ float prob_att(const KindArgs& a, float g) { return a.is_sigmoid ? 1.f / (1.f + expf(-(g - a.thresh))) : g; }
// focal factors 4^sqrt(1 - pc), 4^sqrt(pc), pc = clamp(p, 1e-14, float32(1 - 1e-14) = 1)
__device__ __forceinline__ void focal(float p, float& f1, float& f0) {
    const float pc = fminf(fmaxf(p, 1e-14f), 1.f);
    f1 = exp2f(2.f * sqrtf(1.f - pc));
    f0 = exp2f(2.f * sqrtf(pc));
}

struct BwdCoef { float alpha, gw, c1, c2, cpos, cneg; bool use_keep; };

// d loss / d g of one pixel (al: the pixel's box alpha for kind 2)
__device__ __forceinline__ float dloss_dg(const KindArgs& a, const BwdCoef& k, float g, float e, float m, float al) {
    if (a.kind == 0) {
        float p, omp;
        prob_ce(a, g, p, omp);
        const float keep = (k.use_keep && m == 0.f) ? 0.f : 1.f;
        const float dp = a.is_sigmoid ? p * omp : 1.f;
        float d = -k.cpos * e * rcpf(p + 0.001f) + k.cneg * (1.f - e) * rcpf(omp + 0.001f);
        if (a.dice) return keep * dp * d + dp * (k.c1 * p - k.c2 * e);
        return keep * dp * d;
    }
    const float p = prob_att(a, g), omp = 1.f - p;
    float f1, f0;
    focal(p, f1, f0);
    const float alpha = a.kind == 1 ? k.alpha : al;
    float w = e * alpha * f1 + (1.f - e) * (1.f - alpha) * f0;
    if (a.mask) w *= m;
    float d = k.gw * (p - e) / fmaxf(omp * p, 1e-12f) * w;      // torch's BCE backward, then the weight
    if (a.dice) d += k.c1 * p - k.c2 * e;
    return a.is_sigmoid ? d * omp * p : d;                      // sigmoid backward: grad (1 - y) y
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// Sums of a workgroup (slot: kind 0 | kinds 1, 2):  0: sum e m | A (kind 2: the weighted loss itself)   1: sum (1 - e) m | B
//   2: pos | count(t == 1)   3: neg | count(t == 0)   4, 5: pos, neg on mask != 0   6..9: count(m == 0), count(m == 1), count(other m), sum m
//   10, 11, 12: sum p^2, sum t^2, sum p t (dice)
template <typename V> __device__ void finalize(const KindArgs& a, const V& R) {
    double T[NP];
#pragma unroll
    for (int v = 0; v < NP; ++v) T[v] = 0.0;
    for (int b = 0; b < a.B; ++b)
        for (int v = 0; v < NP; ++v) T[v] += R((long)b * NP + v);
    const double N = (double)a.B * a.H * a.W;
    float* coef = a.coef;
    double base;
    if (a.kind == 0) {                                           // comp_cross_entropy, as edge_loss.hip's finalize
        const bool binary = a.mask != nullptr && T[8] == 0.0 && T[6] > 0.0 && T[7] > 0.0;       // unique(mask) == {0, 1}
        const double nvalid = binary ? T[9] : N;
        double wneg_total = 0.0;
        for (int b = 0; b < a.B; ++b) wneg_total += (double)(float)R((long)b * NP + 1);
        double total = 0.0;
        for (int b = 0; b < a.B; ++b) {
            const float wp = (float)R((long)b * NP), wn = (float)R((long)b * NP + 1);
            const float alpha = wneg_total == 0.0 ? 1.f : wn / (wp + wn);
            const double P = binary ? R((long)b * NP + 4) : R((long)b * NP + 2), Q = binary ? R((long)b * NP + 5) : R((long)b * NP + 3);
            total += (double)a.pos_to_neg * alpha * P + (double)(1.f - alpha) * Q;
            coef[NC + 2 * b] = (float)((double)a.weight * a.pos_to_neg * alpha / nvalid);
            coef[NC + 2 * b + 1] = (float)((double)a.weight * (1.f - alpha) / nvalid);
        }
        coef[NC + 2 * a.B] = binary ? 1.f : 0.f;
        base = total / nvalid;
        coef[0] = 0.f;
    } else if (a.kind == 1) {
        const float npos = (float)T[2], nneg = (float)T[3];
        const float alpha = nneg / (npos + nneg);                   // attention_loss.py:25-27
        coef[0] = alpha;
        base = ((double)alpha * T[0] + (double)(1.f - alpha) * T[1]) / N;
    } else {
        coef[0] = 0.f;
        base = T[0] / N;
    }
    coef[1] = (float)((double)a.weight / N);
    double dice = 0.0;
    coef[2] = coef[3] = 0.f;
    if (a.dice) {
        const double num = T[10] + T[11] + 1e-4, den = 2.0 * T[12] + 1e-4;
        dice = 1000.0 * num / den / N;
        coef[2] = (float)((double)a.weight * 2000.0 / (den * N));               // d dice / d p = c1 p - c2 t
        coef[3] = (float)((double)a.weight * 2000.0 * num / (den * den * N));
    }
    *a.loss = (float)((double)a.weight * (base + dice));
}
struct LdsView { const double* l; __device__ __forceinline__ double operator()(long i) const { return l[i]; } };
struct MemView { const double* g; __device__ __forceinline__ double operator()(long i) const { return handoff::read(g + i); } };

// workgroup sums -> record -> sample sums -> loss (sd: >= 256 doubles of dead LDS)
__device__ void forward_tail(const KindArgs& a, int b, float acc[NP], double* sd, int sd_elems, float (*sred)[NP], int* s_last_p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    volatile int* s_last = s_last_p;                               // handoff::arrive broadcasts through it
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const float s = wave_sum_dpp(acc[i]);
        if (lane == 0) sred[wave][i] = s;
    }
    __syncthreads();
    if (tid < NP) {
        const double v = (double)sred[0][tid] + (double)sred[1][tid] + (double)sred[2][tid] + (double)sred[3][tid];
        handoff::publish(a.records + (long)blockIdx.x * REC + tid, v);
    }
    const int per_image = a.tiles_x * a.tiles_y;
    if (!handoff::arrive([&] { return a.counter + 1 + b; }, [&] { return per_image; }, a.fences, a.fences, s_last)) return;
    // last workgroup of sample b: value v = tid % 16 of records k, k + 16, ... (k = tid / 16), then the 16 part sums in order
    {
        const int v = tid & 15, k = tid >> 4;
        const double* rec = a.records + (long)b * per_image * REC + v;
        double part = 0.0;
        if (v < NP) {
#pragma unroll 4
            for (int j = k; j < per_image; j += 16) part += handoff::read(rec + (long)j * REC);
        }
        sd[k * 16 + v] = part;
        __syncthreads();
        if (tid < NP) {
            double tot = 0.0;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) tot += sd[kk * 16 + tid];
            handoff::publish(a.results + (long)b * NP + tid, tot);
        }
        if (!handoff::arrive([&] { return a.counter; }, [&] { return a.B; }, a.fences, a.fences, s_last)) return;
    }
    // last sample: the sums -> LDS (one round trip for the whole workgroup), one thread does the scalar arithmetic
    const int n = a.B * NP;
    if (n <= sd_elems) {
        __syncthreads();
        for (int i = tid; i < n; i += 256) sd[i] = handoff::read(a.results + i);
        __syncthreads();
        if (tid == 0) finalize(a, LdsView{sd});
    } else if (tid == 0) {
        finalize(a, MemView{a.results});
    }
}

template <bool BOX>
__global__ __launch_bounds__(256) void edge_kind_fwd_kernel(KindArgs a) {
    __shared__ __attribute__((aligned(16))) float sd[(TH + 2) * LS];
    __shared__ float slab[BOX ? Box<0>::ROWS * Box<0>::COLS : 1];
    __shared__ float shs[BOX ? Box<0>::ROWS * Box<0>::ACOLS : 1];
    __shared__ float sred[4][NP];
    __shared__ int s_last;
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int x0 = (t % a.tiles_x) * TW, y0 = (t / a.tiles_x) * TH;
    const int tid = threadIdx.x;
    const int c = (tid & 15) * 4, r0 = tid >> 4;                   // this thread's 4 pixels: columns c..c+3 of rows r0 and r0 + 16
    const long img = (long)b * a.H;
    const bool has_mask = a.mask != nullptr, has_normal = a.normal != nullptr, is_grad = a.is_grad != 0;

    DepthTile<1> tile;
    if (is_grad) tile.issue(a, a.vec, b, x0, y0);
    f32x4_t e4[2], n4[2], m4[2], i4[2];
    const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int gy = y0 + r0 + 16 * ps;
        const bool ok = gy < a.H;
        e4[ps] = ok ? load4(a.edge, img + gy, x0 + c, a.W, a.vec) : z;
        n4[ps] = (ok && has_normal && is_grad) ? load4(a.normal, img + gy, x0 + c, a.W, a.vec) : z;
        m4[ps] = (ok && has_mask) ? load4(a.mask, img + gy, x0 + c, a.W, a.vec) : z;
        i4[ps] = (ok && !is_grad) ? load4(a.pred, img + gy, x0 + c, a.W, a.vec) : z;
    }
    if (is_grad) tile.commit(a, a.from_inv, x0, y0, sd);
    if (BOX) box_alpha<0>(a, b, x0, y0, slab, shs);
    __syncthreads();

    float acc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) acc[i] = 0.f;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int ly = r0 + 16 * ps, gy = y0 + ly;
        if (gy >= a.H) continue;
        float w[3][6];
        if (is_grad) window(sd, ly + 1, c, w);
        f32x4_t g4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (x0 + c + k >= a.W) { g4[k] = 0.f; continue; }
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
            const float e = e4[ps][k], m = has_mask ? m4[ps][k] : 1.f;
            float p;
            if (a.kind == 0) {
                float omp;
                prob_ce(a, g, p, omp);
                const float pos = -e * fast_log(p + 0.001f), neg = -(1.f - e) * fast_log(omp + 0.001f);
                acc[2] += pos; acc[3] += neg;
                if (has_mask) {
                    const float keep = m != 0.f ? 1.f : 0.f;
                    acc[0] += e * m; acc[1] += (1.f - e) * m;
                    acc[4] += pos * keep; acc[5] += neg * keep;
                    acc[6] += m == 0.f ? 1.f : 0.f; acc[7] += m == 1.f ? 1.f : 0.f; acc[8] += (m != 0.f && m != 1.f) ? 1.f : 0.f; acc[9] += m;
                } else {
                    acc[0] += e; acc[1] += 1.f - e;
                }
            } else {
                p = prob_att(a, g);
                float f1, f0;
                focal(p, f1, f0);
                const float bce = (e - 1.f) * fmaxf(log1pf(-p), -100.f) - e * fmaxf(logf(p), -100.f);
                if (a.kind == 1) {
                    acc[0] += m * e * f1 * bce; acc[1] += m * (1.f - e) * f0 * bce;
                    acc[2] += e == 1.f ? 1.f : 0.f; acc[3] += e == 0.f ? 1.f : 0.f;
                } else {
                    const float al = slab[ly * Box<0>::ACOLS + c + k];
                    float wt = e * al * f1 + (1.f - e) * (1.f - al) * f0;
                    if (has_mask) wt *= m;
                    acc[0] += wt * bce;
                }
            }
            if (a.dice) { acc[10] += p * p; acc[11] += e * e; acc[12] += p * e; }
        }
        if (a.gmap) store4(a.gmap, img + gy, x0 + c, a.W, a.vec, g4);
    }
    forward_tail(a, b, acc, (double*)sd, (TH + 2) * LS / 2, sred, &s_last);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
// Transposed Sobel as in edge_loss.hip: per-pixel planes A (X coefficient) and B (Y coefficient) of G = d loss / d s on the tile + 1-pixel halo,
// then d loss / d depth(q) = sum_t A(q - t) X[t] + B(q - t) Y[t] + C(q - t) Xc[t] + D(q - t) Yc[t] with C = A where B = 0, D = B where A = 0.
template <bool BOX>
__global__ __launch_bounds__(256) void edge_kind_bwd_kernel(KindArgs a) {
    __shared__ __attribute__((aligned(16))) float sd[(TH + 4) * LS];
    __shared__ __attribute__((aligned(16))) float sga[(TH + 2) * LS], sgb[(TH + 2) * LS];
    __shared__ float slab[BOX ? Box<1>::ROWS * Box<1>::COLS : 1];
    __shared__ float shs[BOX ? Box<1>::ROWS * Box<1>::ACOLS : 1];
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int x0 = (t % a.tiles_x) * TW, y0 = (t / a.tiles_x) * TH;
    const int tid = threadIdx.x;
    const int c = (tid & 15) * 4, r0 = tid >> 4;
    const long img = (long)b * a.H;
    const float go = a.gout ? a.gout[0] : 1.f;
    BwdCoef k;
    k.alpha = a.coef[0]; k.gw = a.coef[1] * go; k.c1 = a.coef[2] * go; k.c2 = a.coef[3] * go;
    k.cpos = k.cneg = 0.f; k.use_keep = false;
    if (a.kind == 0) {
        k.cpos = a.coef[NC + 2 * b] * go; k.cneg = a.coef[NC + 2 * b + 1] * go;
        k.use_keep = a.coef[NC + 2 * a.B] != 0.f && a.mask != nullptr;
    }
    const bool magnitude = a.normal == nullptr, is_grad = a.is_grad != 0, has_mask = a.mask != nullptr;

    constexpr int GITEMS = (TH + 2) * (TW / 4 + 2), NG = (GITEMS + 255) / 256;     // G region: interior groups of 4 + two halo columns per row
    DepthTile<2> tile;
    f32x4_t ge[NG], gn[NG], gm[NG];
    f32x4_t inv4[2], oe4[2], om4[2];
    if (is_grad) {
        tile.issue(a, a.vec, b, x0, y0);
#pragma unroll
        for (int q4 = 0; q4 < NG; ++q4) {
            const int i = tid + q4 * 256;
            const int ly = i / (TW / 4 + 2), q = i % (TW / 4 + 2);               // q < 16: interior group, 16 / 17: left / right halo column
            const int gy = y0 + ly - 1;
            const bool group = q < TW / 4;
            const int j0 = group ? q * 4 : (q == TW / 4 ? -1 : TW);
            ge[q4] = f32x4_t{0.f, 0.f, 0.f, 0.f}; gn[q4] = ge[q4]; gm[q4] = f32x4_t{1.f, 1.f, 1.f, 1.f};
            if (i < GITEMS && (unsigned)gy < (unsigned)a.H) {
                if (group) {
                    ge[q4] = load4(a.edge, img + gy, x0 + j0, a.W, a.vec);
                    if (!magnitude) gn[q4] = load4(a.normal, img + gy, x0 + j0, a.W, a.vec);
                    if (has_mask) gm[q4] = load4(a.mask, img + gy, x0 + j0, a.W, a.vec);
                } else if ((unsigned)(x0 + j0) < (unsigned)a.W) {
                    const long idx = (img + gy) * a.W + x0 + j0;
                    ge[q4][0] = a.edge[idx];
                    if (!magnitude) gn[q4][0] = a.normal[idx];
                    if (has_mask) gm[q4][0] = a.mask[idx];
                }
            }
        }
    }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int gy = y0 + r0 + 16 * ps;
        const bool ok = gy < a.H && x0 + c < a.W;
        const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
        inv4[ps] = ok ? load4(a.pred, img + gy, x0 + c, a.W, a.vec) : z;
        if (!is_grad) {
            oe4[ps] = ok ? load4(a.edge, img + gy, x0 + c, a.W, a.vec) : z;
            om4[ps] = (ok && has_mask) ? load4(a.mask, img + gy, x0 + c, a.W, a.vec) : f32x4_t{1.f, 1.f, 1.f, 1.f};
        }
    }
    if (BOX) box_alpha<1>(a, b, x0, y0, slab, shs);               // alpha at tile (ly, j): slab[(ly + 1) * (TW + 2) + j + 1]
    constexpr int AC = Box<1>::ACOLS;
    if (is_grad) {
        tile.commit(a, a.from_inv, x0, y0, sd);
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
            const bool rowok = (unsigned)gy < (unsigned)a.H;
            float w[3][6];
            if (group) window(sd, ly + 1, j0, w);
            else {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int kk = 0; kk < 3; ++kk) w[r][kk] = sd[(ly + r) * LS + 4 + j0 - 1 + kk];
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (kk >= np) break;
                const int gx = x0 + j0 + kk;
                float ga = 0.f, gb = 0.f;
                if (rowok && (unsigned)gx < (unsigned)a.W) {
                    float sh, sv, srl, slr;
                    sobel4(w, kk, sh, sv, srl, slr);
                    float g, da, db = 0.f;
                    int code = 0;
                    if (!magnitude) {
                        code = direction_code(n4[kk]);
                        const float s = code == 0 ? sh : (code == 1 ? sv : (code == 2 ? srl : slr));
                        g = fabsf(s);
                        da = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
                    } else {
                        g = sqrtf(sv * sv + sh * sh + 1e-6f);
                        da = sv / g; db = sh / g;
                    }
                    const float al = BOX ? slab[ly * AC + j0 + kk + 1] : 0.f;
                    const float dg = dloss_dg(a, k, g, e4[kk], m4[kk], al);
                    if (magnitude) { ga = dg * db; gb = dg * da; }
                    else {
                        const float G = dg * da;
                        ga = code != 1 ? G : 0.f;
                        gb = code == 1 ? G : (code == 2 ? -G : (code == 3 ? G : 0.f));
                    }
                }
                const int o = ly * LS + 4 + j0 + kk;
                sga[o] = ga; sgb[o] = gb;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int ly = r0 + 16 * ps, gy = y0 + ly;
        if (gy >= a.H || x0 + c >= a.W) continue;
        f32x4_t out = {0.f, 0.f, 0.f, 0.f};
        if (is_grad) {
            float wa[3][6], wb[3][6];
            window(sga, ly + 1, c, wa);
            window(sgb, ly + 1, c, wb);
            float ca[6], eb[6], cc1[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                ca[j] = (wa[0][j] + wa[1][j]) + wa[2][j];
                eb[j] = wb[0][j] - wb[2][j];
                cc1[j] = magnitude ? wa[1][j] : (wb[1][j] == 0.f ? wa[1][j] : 0.f);
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float d0 = magnitude ? wb[0][kk + 1] : (wa[0][kk + 1] == 0.f ? wb[0][kk + 1] : 0.f);
                const float d2 = magnitude ? wb[2][kk + 1] : (wa[2][kk + 1] == 0.f ? wb[2][kk + 1] : 0.f);
                float dd = (ca[kk] - ca[kk + 2]) + ((eb[kk] + eb[kk + 1]) + eb[kk + 2]) + (cc1[kk] - cc1[kk + 2]) + (d0 - d2);
                if (a.from_inv) {
                    const float inv = inv4[ps][kk];
                    const float d = rcpf(fmaxf(inv, 1e-6f));
                    dd = inv >= 1e-6f ? -dd * d * d : 0.f;
                }
                out[kk] = dd;
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float al = BOX ? slab[(ly + 1) * AC + c + kk + 1] : 0.f;
                out[kk] = dloss_dg(a, k, inv4[ps][kk], oe4[ps][kk], om4[ps][kk], al);
            }
        }
        store4(a.dpred, img + gy, x0 + c, a.W, a.vec, out);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int setup(KindArgs& a, const float* pred, const float* edge, const float* normal, const float* mask, int B, int H, int W, int kind, int dice,
          int from_inv, int is_grad, int is_sigmoid, float thresh) {
    if (!pred || !edge || B < 1 || H < 1 || W < 1 || kind < 0 || kind > 2) return -1;
    a.pred = pred; a.edge = edge; a.normal = normal; a.mask = mask;
    a.B = B; a.H = H; a.W = W;
    a.tiles_x = (W + TW - 1) / TW; a.tiles_y = (H + TH - 1) / TH;
    a.vec = W % 4 == 0 && aligned16(pred) && aligned16(edge) && aligned16(normal) && aligned16(mask);
    a.kind = kind; a.dice = dice != 0; a.from_inv = from_inv; a.is_grad = is_grad; a.is_sigmoid = is_sigmoid; a.thresh = thresh;
    a.fences = g_mte_handoff_fences;
    return B * a.tiles_x * a.tiles_y;
}
long results_elems(int B) { return ((long)B * NP + 1) & ~1L; }
long counter_elems(int B) { return (((long)B + 1) * 4 + 15) / 16 * 2; }      // doubles holding the tickets (16-byte multiple)

}  // namespace

extern "C" {

// doubles of workspace for one forward launch: [B][13] sums + the arrival tickets + one 16-double record per 64 x 32 tile
long mte_edge_loss_kind_work_elems(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return -1;
    const long tiles = (long)((W + TW - 1) / TW) * ((H + TH - 1) / TH);
    return results_elems(B) + counter_elems(B) + (long)B * tiles * REC;
}

// Forward of one scale.  *loss <- weight * (base loss of `kind` + dice term when `dice`); coef [2B + 5] <- backward coefficients.
int mte_edge_loss_kind_fwd(const float* pred, const float* edge, const float* normal, const float* mask, float* gmap, int B, int H, int W,
                           int kind, int dice, int from_inv, int is_grad, int is_sigmoid, float thresh, float weight, float pos_to_neg,
                           double* work, float* loss, float* coef, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    KindArgs a{};
    const int blocks = setup(a, pred, edge, normal, mask, B, H, W, kind, dice, from_inv, is_grad, is_sigmoid, thresh);
    if (blocks < 0 || !work || !loss || !coef) return MTE_ERR_ARG;
    if (gmap && !aligned16(gmap)) a.vec = 0;
    a.gmap = gmap; a.weight = weight; a.pos_to_neg = pos_to_neg; a.loss = loss; a.coef = coef;
    const long r = results_elems(B), cn = counter_elems(B);
    a.results = work; a.counter = (unsigned*)(work + r); a.records = work + r + cn;
    if (mte_memset_async(work, 0, sizeof(double) * (r + cn), stream) != hipSuccess) return MTE_ERR_LAUNCH;     // sums + tickets (records are overwritten)
    if (kind == 2) hipLaunchKernelGGL(edge_kind_fwd_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(edge_kind_fwd_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}

// Backward of the same: dpred <- gout * d loss / d pred  (gout: device scalar, nullable = 1)
int mte_edge_loss_kind_bwd(const float* pred, const float* edge, const float* normal, const float* mask, const float* coef, const float* gout,
                           float* dpred, int B, int H, int W, int kind, int dice, int from_inv, int is_grad, int is_sigmoid, float thresh,
                           hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    KindArgs a{};
    const int blocks = setup(a, pred, edge, normal, mask, B, H, W, kind, dice, from_inv, is_grad, is_sigmoid, thresh);
    if (blocks < 0 || !coef || !dpred) return MTE_ERR_ARG;
    if (!aligned16(dpred)) a.vec = 0;
    a.coef = (float*)coef; a.gout = gout; a.dpred = dpred;
    if (kind == 2) hipLaunchKernelGGL(edge_kind_bwd_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(edge_kind_bwd_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}

}  // extern "C"
