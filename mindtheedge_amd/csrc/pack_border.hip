// The exact border of the folded pack layers from a one-pixel ring -- gfx950 helpers (index arithmetic: pack_border_plan.hpp).
//
// pack_fold.hip folds conv3d(1->4) into the k x k convolution; the folded form is exact except within pad = k/2 pixels of the border, where it sees
// conv3d's values OUTSIDE the image (the reference, layers01.py:241-247, zero-pads between the two ops).  Those values depend on the data only on the
// ring at distance 1 (conv3d reaches one pixel) and equal b3[f] everywhere else, so
//     y_ref(p) = y_fold(p) - sum_{t : p+t on the ring} W[t] . U(p+t) - sum_{t : p+t outside} S[t]
//     U = conv3d's data part on the ring [16C channels],   S[co][t] = sum_f b3[f] sum_d W[co][f*D+d][t].
// A pixel j < pad away from an edge meets that edge's ring line with ONE tap row (column): the ring term is a zero-padded 1 x k convolution along the
// top / bottom ring rows plus a k x 1 convolution along the left / right ring columns, with the (edge, j) pairs stacked in the output channels -- two
// small GEMMs per pass through mte_conv2d_igemm / mte_conv2d_wgrad (KH = 1 or KW = 1).  The bias term is a table over the (2 pad + 1)^2 pixel classes.
//
// This file: the ring stencil U (forward, data gradient, conv3d weight gradient), the negated ring weights + class table, the in-place border
// correction of y, the gather of dy into the GEMMs' gradient operand with the class sums, and the scatter of the ring-weight gradients into dW.
// Every sum has a fixed order (per-workgroup partials, added in index order): the results are bit-reproducible.
#include "common.hpp"
#include "pack_border_plan.hpp"

namespace {

inline int bgrid(long n, int cap = 4096) { long g = (n + 255) / 256; return (int)(g > cap ? cap : (g < 1 ? 1 : g)); }

// v[0 .. 33] = p[d0 - 1 .. d0 + 32] of one D-channel block (zero beyond the block): the depth window of 32 outputs of a 3-tap stencil along d
template <typename T>
__device__ __forceinline__ void load_span(const T* __restrict__ p, int d0, int D, float* v) {
    constexpr int P = Elem<T>::PER16;
    v[0] = d0 > 0 ? Elem<T>::ld(p + d0 - 1) : 0.f;
    v[33] = d0 + 32 < D ? Elem<T>::ld(p + d0 + 32) : 0.f;
#pragma unroll
    for (int c = 0; c < 32 / P; ++c) unpack16<T>(*(const u32x4_t*)(p + d0 + c * P), v + 1 + c * P);
}
template <typename T>
__device__ __forceinline__ void store32(T* __restrict__ p, const float* v) {
    constexpr int P = Elem<T>::PER16;
#pragma unroll
    for (int c = 0; c < 32 / P; ++c) *(u32x4_t*)(p + c * P) = pack16<T>(v + c * P);
}

// item -> (edge, sample, ring position, 32-depth block); rows first (edges 0, 1), then columns (2, 3)
__device__ __forceinline__ void ring_item(long it, int B, int H2, int W2, int nb, int* e, int* b, int* i, int* jb) {
    const long per_row = (long)B * (W2 + 2) * nb, per_col = (long)B * H2 * nb;
    int ee = 0;
    if (it >= 2 * per_row) { it -= 2 * per_row; ee = 2; if (it >= per_col) { it -= per_col; ee = 3; } }
    else if (it >= per_row) { it -= per_row; ee = 1; }
    *e = ee;
    *jb = (int)(it % nb); it /= nb;
    const int len = pb_edge_len(ee, H2, W2);
    *i = (int)(it % len); *b = (int)(it / len);
}

// R_rows [2B][W2+2][4D], R_cols [2B][H2][4D] <- P [B][H2][W2][D]: U on the ring (no bias), fp32 sums rounded once
template <typename T>
__global__ __launch_bounds__(256) void ring_fwd_kernel(const T* __restrict__ P, long ldp, const float* __restrict__ K3, T* __restrict__ Rr, T* __restrict__ Rc,
                                                       int B, int H2, int W2, int D) {
    __shared__ float s3[108];
    if (threadIdx.x < 108) s3[threadIdx.x] = K3[threadIdx.x];
    __syncthreads();
    const int nb = D / 32;
    const long total = 2L * B * (W2 + 2 + H2) * nb;
    for (long it = blockIdx.x * (long)blockDim.x + threadIdx.x; it < total; it += (long)gridDim.x * blockDim.x) {
        int e, b, i, jb;
        ring_item(it, B, H2, W2, nb, &e, &b, &i, &jb);
        const int d0 = 32 * jb, len = pb_edge_len(e, H2, W2);
        float in[3][34];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int h, w;
            if (pb_edge_src(e, i, a, H2, W2, &h, &w)) load_span<T>(P + (((long)b * H2 + h) * W2 + w) * ldp, d0, D, in[a]);
            else {
#pragma unroll
                for (int q = 0; q < 34; ++q) in[a][q] = 0.f;
            }
        }
        T* out = (e < 2 ? Rr : Rc) + (((long)(e & 1) * B + b) * len + i) * 4 * D + d0;
        for (int f = 0; f < 4; ++f) {
            float acc[32];
#pragma unroll
            for (int q = 0; q < 32; ++q) acc[q] = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int kd = 0; kd < 3; ++kd) {
                    const float kv = s3[pb_k3_index(e, f, kd, a)];
#pragma unroll
                    for (int q = 0; q < 32; ++q) acc[q] = fmaf(kv, in[a][q + kd], acc[q]);
                }
            store32<T>(out + (long)f * D, acc);
        }
    }
}

// dx [B][2 H2][2 W2][C] (un-shuffled, d = 4c + s) += transpose of the ring stencil applied to dR; only pixels of the outermost packed rows / columns.
// Four neighbouring lanes share an item (sample, pixel, 32 depths): lane f sums the terms of conv3d filter f (the item's loads are one dependent chain,
// and a layer has under a thousand waves of items), the four partial sums meet by two lane exchanges in a fixed order, lane f then adds sub-pixel s = f
template <typename T>
__global__ __launch_bounds__(256) void ring_bwd_data_kernel(const T* __restrict__ dRr, const T* __restrict__ dRc, const float* __restrict__ K3,
                                                            T* __restrict__ dx, long lddx, int B, int H2, int W2, int D) {
    constexpr int P = Elem<T>::PER16;
    __shared__ float s3[108];
    if (threadIdx.x < 108) s3[threadIdx.x] = K3[threadIdx.x];
    __syncthreads();
    const int nb = D / 32;
    const long npix = pb_border_count(H2, W2, 1);
    const long total = (long)B * npix * nb * 4;
    for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < total; i4 += (long)gridDim.x * blockDim.x) {
        const int f = (int)(i4 & 3); const long it = i4 >> 2;
        const int jb = (int)(it % nb); long t = it / nb;
        const long pix = t % npix; const int b = (int)(t / npix);
        int h, w;
        pb_border_pixel(pix, H2, W2, 1, &h, &w);
        const int d0 = 32 * jb;
        float acc[32];
#pragma unroll
        for (int q = 0; q < 32; ++q) acc[q] = 0.f;
        for (int e = 0; e < 4; ++e) {
            int along, off;
            if (!pb_edge_of_pixel(e, h, w, H2, W2, &along, &off)) continue;
            const int len = pb_edge_len(e, H2, W2);
            const T* base = (e < 2 ? dRr : dRc) + ((long)(e & 1) * B + b) * len * 4 * D + (long)f * D;
            for (int a = 0; a < 3; ++a) {
                const int i = along + off - a;
                if (i < 0 || i >= len) continue;
                float v[34];
                load_span<T>(base + (long)i * 4 * D, d0, D, v);
#pragma unroll
                for (int kd = 0; kd < 3; ++kd) {
                    const float kv = s3[pb_k3_index(e, f, kd, a)];
#pragma unroll
                    for (int q = 0; q < 32; ++q) acc[q] = fmaf(kv, v[q - kd + 2], acc[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 32; ++q) {          // (f0 + f1) + (f2 + f3) on every lane of the group
            acc[q] += __shfl_xor(acc[q], 1, 64);
            acc[q] += __shfl_xor(acc[q], 2, 64);
        }
        const int s = f;
        T* p = dx + (((long)b * 2 * H2 + 2 * h + (s >> 1)) * 2 * W2 + 2 * w + (s & 1)) * lddx + 8 * jb;
        float cur[8];
        unpack16<T>(*(const u32x4_t*)p, cur);
        if constexpr (P == 4) unpack16<T>(*(const u32x4_t*)(p + 4), cur + 4);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float a_ = 0.f;
#pragma unroll
            for (int ss = 0; ss < 4; ++ss) a_ = ss == s ? acc[4 * c + ss] : a_;
            cur[c] += a_;
        }
        *(u32x4_t*)p = pack16<T>(cur);
        if constexpr (P == 4) *(u32x4_t*)(p + 4) = pack16<T>(cur + 4);
    }
}

// part [4 edges][PB_RING_BLOCKS][36 = f, kd, a] = sum over the edge's ring positions of dR[f*D+d] * P[src(a)][d+kd-1]; blockIdx.y = edge
template <typename T>
__global__ __launch_bounds__(256) void ring_bwd_weight_kernel(const T* __restrict__ dRr, const T* __restrict__ dRc, const T* __restrict__ P, long ldp,
                                                              float* __restrict__ part, int B, int H2, int W2, int D) {
    constexpr int PE = Elem<T>::PER16;
    __shared__ float sred[4][36];
    const int e = blockIdx.y, nb = D / 32, len = pb_edge_len(e, H2, W2);
    const T* dR = e < 2 ? dRr : dRc;
    float acc[36];
#pragma unroll
    for (int q = 0; q < 36; ++q) acc[q] = 0.f;
    const long total = (long)B * len * nb;
    for (long it = blockIdx.x * (long)blockDim.x + threadIdx.x; it < total; it += (long)gridDim.x * blockDim.x) {
        const int jb = (int)(it % nb); long t = it / nb;
        const int i = (int)(t % len), b = (int)(t / len), d0 = 32 * jb;
        float in[3][34];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int h, w;
            if (pb_edge_src(e, i, a, H2, W2, &h, &w)) load_span<T>(P + (((long)b * H2 + h) * W2 + w) * ldp, d0, D, in[a]);
            else {
#pragma unroll
                for (int q = 0; q < 34; ++q) in[a][q] = 0.f;
            }
        }
        const T* g = dR + (((long)(e & 1) * B + b) * len + i) * 4 * D + d0;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            float gv[32];
#pragma unroll
            for (int c = 0; c < 32 / PE; ++c) unpack16<T>(*(const u32x4_t*)(g + (long)f * D + c * PE), gv + c * PE);
#pragma unroll
            for (int kd = 0; kd < 3; ++kd)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float s = acc[(f * 3 + kd) * 3 + a];
#pragma unroll
                    for (int q = 0; q < 32; ++q) s = fmaf(gv[q], in[a][q + kd], s);
                    acc[(f * 3 + kd) * 3 + a] = s;
                }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 36; ++q) {
        const float s = wave_sum(acc[q]);
        if (lane == 0) sred[wave][q] = s;
    }
    __syncthreads();
    if (threadIdx.x < 36)
        part[((long)e * gridDim.x + blockIdx.x) * 36 + threadIdx.x] = (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
}

// dk3[f][kd][dh][dw] += the partials of the edges whose fixed tap it is: one wave per output, lane = workgroup of the partials, butterfly sum (fixed order)
static_assert(PB_RING_BLOCKS == 64, "ring_bwd_weight_finish_kernel: one lane per workgroup of partials");
__global__ __launch_bounds__(64) void ring_bwd_weight_finish_kernel(const float* __restrict__ part, float* __restrict__ dk3) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const int dw = t % 3, dh = (t / 3) % 3, fk = t / 9;          // fk = f * 3 + kd
    float sum = 0.f;
    for (int e = 0; e < 4; ++e) {
        const int fix = (e == 0 || e == 2) ? 2 : 0;
        int a;
        if (e < 2) { if (dh != fix) continue; a = dw; }
        else { if (dw != fix) continue; a = dh; }
        sum += part[((long)e * PB_RING_BLOCKS + lane) * 36 + fk * 3 + a];
    }
    sum = wave_sum(sum);
    if (lane == 0) dk3[t] += sum;
}

// Wr [2 pad Co][CT][1][k], Wc [2 pad Co][CT][k][1] (OIHW fp32, NEGATED) and Dt [(2 pad + 1)^2][Co] from W [Co][CT = 4D][k][k], b3 [4]
__global__ __launch_bounds__(256) void border_weights_kernel(const float* __restrict__ W, const float* __restrict__ b3, float* __restrict__ Wr,
                                                             float* __restrict__ Wc, float* __restrict__ Dt, int Co, int D, int k) {
    const int pad = k >> 1, CT = 4 * D, kk = k * k;
    const long half = 2L * pad * Co * CT * k;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < 2 * half; idx += (long)gridDim.x * blockDim.x) {
        const bool cols = idx >= half;
        long r = cols ? idx - half : idx;
        const int t = (int)(r % k); r /= k;
        const int ch = (int)(r % CT); r /= CT;
        const int co = (int)(r % Co); const int fj = (int)(r / Co);
        const int tap = pb_tap(fj / pad, fj % pad, pad);
        const float* wp = W + ((long)co * CT + ch) * kk;
        if (cols) Wc[idx - half] = -wp[t * k + tap];
        else Wr[idx] = -wp[tap * k + t];
    }
    __shared__ float sS[32], sw[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nc = 2 * pad + 1;
    for (int co = blockIdx.x; co < Co; co += gridDim.x) {
        for (int t = 0; t < kk; ++t) {
            float a = 0.f;
            for (int ch = threadIdx.x; ch < CT; ch += 256) a = fmaf(b3[ch / D], W[((long)co * CT + ch) * kk + t], a);
            a = wave_sum(a);
            __syncthreads();
            if (lane == 0) sw[wave] = a;
            __syncthreads();
            if (threadIdx.x == 0) sS[t] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
        }
        __syncthreads();
        if ((int)threadIdx.x < nc * nc) {
            const int cy = threadIdx.x / nc, cx = threadIdx.x % nc;
            float s = 0.f;
            for (int t = 0; t < kk; ++t)
                if (pb_tap_outside(cy, t / k, pad) || pb_tap_outside(cx, t % k, pad)) s += sS[t];
            Dt[(long)threadIdx.x * Co + co] = -s;
        }
        __syncthreads();
    }
}

// y [B][H2][W2][Co] += corr_rows [2B][W2+2][N] / corr_cols [2B][H2][N] (fp32, N = 2 pad Co) + Dt[class] on the border pixels; fp32 sum, rounded once.
// splits > 1: the ring terms arrive as `splits` slabs of partial sums (mte_pack_border_gemm_fwd), slab_r / slab_c elements apart; each term is the sum of its
// slabs in slab order, formed here -- no finish launch, the summed terms are never written
template <typename T>
__global__ __launch_bounds__(256) void border_apply_kernel(T* __restrict__ y, long ldy, const float* __restrict__ cr, const float* __restrict__ cc,
                                                           const float* __restrict__ Dt, int B, int H2, int W2, int Co, int pad,
                                                           int splits, long slab_r, long slab_c) {
    constexpr int P = Elem<T>::PER16;
    const int cpr = Co / P, N = 2 * pad * Co, nc = 2 * pad + 1;
    const long npix = pb_border_count(H2, W2, pad), total = (long)B * npix * cpr;
    for (long it = blockIdx.x * (long)blockDim.x + threadIdx.x; it < total; it += (long)gridDim.x * blockDim.x) {
        const int c0 = (int)(it % cpr) * P; long t = it / cpr;
        const long pix = t % npix; const int b = (int)(t / npix);
        int r, x;
        pb_border_pixel(pix, H2, W2, pad, &r, &x);
        T* p = y + (((long)b * H2 + r) * W2 + x) * ldy + c0;
        float v[P], add[P];
        unpack16<T>(*(const u32x4_t*)p, v);
#pragma unroll
        for (int c = 0; c < P; ++c) add[c] = 0.f;
        const float* src[4] = {nullptr, nullptr, nullptr, nullptr};
        if (r < pad) src[0] = cr + (((long)b * (W2 + 2)) + x + 1) * N + pb_col(0, r, c0, pad, Co);
        if (H2 - 1 - r < pad) src[1] = cr + (((long)(B + b) * (W2 + 2)) + x + 1) * N + pb_col(1, H2 - 1 - r, c0, pad, Co);
        if (x < pad) src[2] = cc + (((long)b * H2) + r) * N + pb_col(0, x, c0, pad, Co);
        if (W2 - 1 - x < pad) src[3] = cc + (((long)(B + b) * H2) + r) * N + pb_col(1, W2 - 1 - x, c0, pad, Co);
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (src[s]) {
#pragma unroll
                for (int c = 0; c < P; c += 4) {
                    f32x4_t q = *(const f32x4_t*)(src[s] + c);
                    const long slab = s < 2 ? slab_r : slab_c;
                    for (int sp = 1; sp < splits; ++sp) q += *(const f32x4_t*)(src[s] + sp * slab + c);
                    add[c] += q[0]; add[c + 1] += q[1]; add[c + 2] += q[2]; add[c + 3] += q[3];
                }
            }
        const float* dt = Dt + (long)(pb_class(r, H2, pad) * nc + pb_class(x, W2, pad)) * Co + c0;
#pragma unroll
        for (int c = 0; c < P; ++c) v[c] += add[c] + dt[c];
        *(u32x4_t*)p = pack16<T>(v);
    }
}

// G_rows [2B][W2+2][N], G_cols [2B][H2][N] <- dy [B][H2][W2][Co]: column (far, j, co) of line-batch (far', b) holds dy of the pixel j away from that
// edge where far == far' (zero in the cross blocks and, for the rows, at the two end positions)
template <typename T>
__global__ __launch_bounds__(256) void border_gather_kernel(const T* __restrict__ dy, long lddy, T* __restrict__ Gr, T* __restrict__ Gc,
                                                            int B, int H2, int W2, int Co, int pad) {
    constexpr int P = Elem<T>::PER16;
    const int N = 2 * pad * Co, npr = N / P;
    const long rows = 2L * B * (W2 + 2) * npr, total = rows + 2L * B * H2 * npr;
    for (long it = blockIdx.x * (long)blockDim.x + threadIdx.x; it < total; it += (long)gridDim.x * blockDim.x) {
        const bool cols = it >= rows;
        long t = cols ? it - rows : it;
        const int n0 = (int)(t % npr) * P; t /= npr;
        const int len = cols ? H2 : W2 + 2;
        const int i = (int)(t % len), fb = (int)(t / len), far = fb / B, b = fb % B;
        const int fj = n0 / Co, co = n0 % Co, j = fj % pad;
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (fj / pad == far) {
            if (cols) v = *(const u32x4_t*)(dy + (((long)b * H2 + i) * W2 + (far ? W2 - 1 - j : j)) * lddy + co);
            else if (i >= 1 && i <= W2) v = *(const u32x4_t*)(dy + (((long)b * H2 + (far ? H2 - 1 - j : j)) * W2 + i - 1) * lddy + co);
        }
        *(u32x4_t*)((cols ? Gc : Gr) + ((long)fb * len + i) * N + n0) = v;
    }
}

// part [(2 pad + 1)^2][PB_CLASS_SPLITS][Co]: sums of dy over the pixels of each class; grid (split, class), the four waves of a block reduced in order
template <typename T>
__global__ __launch_bounds__(256) void border_class_sums_kernel(const T* __restrict__ dy, long lddy, float* __restrict__ part,
                                                                int B, int H2, int W2, int Co, int pad) {
    __shared__ float sred[4][64];
    const int nc = 2 * pad + 1, cls = blockIdx.y, cy = cls / nc, cx = cls % nc, split = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool centre = cy == pad && cx == pad;
    const int ny = pb_class_count(cy, H2, pad), nx = pb_class_count(cx, W2, pad), y0 = pb_class_first(cy, H2, pad), x0 = pb_class_first(cx, W2, pad);
    const long np = centre ? 0 : (long)B * ny * nx;
    for (int c0 = 0; c0 < Co; c0 += 64) {
        const int c = c0 + lane;
        float a = 0.f;
        if (c < Co)
#pragma unroll 4
            for (long p = split * 4 + wave; p < np; p += 4 * PB_CLASS_SPLITS) {
                const int x = (int)(p % nx); long t = p / nx;
                const int yy = (int)(t % ny), b = (int)(t / ny);
                a += Elem<T>::ld(dy + (((long)b * H2 + y0 + yy) * W2 + x0 + x) * lddy + c);
            }
        __syncthreads();
        sred[wave][lane] = a;
        __syncthreads();
        if (wave == 0 && c < Co) part[((long)cls * PB_CLASS_SPLITS + split) * Co + c] = (sred[0][lane] + sred[1][lane]) + (sred[2][lane] + sred[3][lane]);
    }
}

// dS [Co][k*k] = - sum over the classes for which the tap is outside of dD[class][co]; one wave per (co, tap), the lanes walk the (class, split) partials
// in a fixed assignment and meet in the butterfly
__global__ __launch_bounds__(256) void border_ds_kernel(const float* __restrict__ part, float* __restrict__ dS, int Co, int k) {
    const int pad = k >> 1, nc = 2 * pad + 1, kk = k * k;
    const int lane = threadIdx.x & 63, idx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= Co * kk) return;
    const int t = idx % kk, co = idx / kk;
    float s = 0.f;
    for (int q = lane; q < nc * nc * PB_CLASS_SPLITS; q += 64) {
        const int cls = q / PB_CLASS_SPLITS;
        if (pb_tap_outside(cls / nc, t / k, pad) || pb_tap_outside(cls % nc, t % k, pad)) s += part[(long)q * Co + co];
    }
    s = wave_sum(s);
    if (lane == 0) dS[idx] = -s;
}

// dW [Co][CT][k][k] = - dWr[(far, j)(ty), co][ch][tx] - dWc[(far, j)(tx), co][ch][ty] + b3[f] dS[co][t]   (overwritten);
// part3 [blocks][4] = per-workgroup sums of dS[co][t] * W[co][f*D+d][t] per f (db3)
__global__ __launch_bounds__(256) void border_scatter_kernel(const float* __restrict__ dWr, const float* __restrict__ dWc, const float* __restrict__ dS,
                                                             const float* __restrict__ W, const float* __restrict__ b3, float* __restrict__ dW,
                                                             float* __restrict__ part3, int Co, int D, int k) {
    __shared__ float sred[4][4];
    const int pad = k >> 1, CT = 4 * D, kk = k * k;
    const long total = (long)Co * CT * kk;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int t = (int)(idx % kk); long r = idx / kk;
        const int ch = (int)(r % CT), co = (int)(r / CT), ty = t / k, tx = t - ty * k, f = ch / D;
        const float ds = dS[co * kk + t];
        float v = 0.f;
        int far, j;
        if (pb_tap_owner(ty, pad, &far, &j)) v -= dWr[((long)pb_col(far, j, co, pad, Co) * CT + ch) * k + tx];
        if (pb_tap_owner(tx, pad, &far, &j)) v -= dWc[((long)pb_col(far, j, co, pad, Co) * CT + ch) * k + ty];
        dW[idx] = fmaf(b3[f], ds, v);
        const float c = ds * W[idx];
        a0 += f == 0 ? c : 0.f; a1 += f == 1 ? c : 0.f; a2 += f == 2 ? c : 0.f; a3 += f == 3 ? c : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
    if (lane == 0) { sred[wave][0] = a0; sred[wave][1] = a1; sred[wave][2] = a2; sred[wave][3] = a3; }
    __syncthreads();
    if (threadIdx.x < 4) part3[(long)blockIdx.x * 4 + threadIdx.x] = (sred[0][threadIdx.x] + sred[1][threadIdx.x]) + (sred[2][threadIdx.x] + sred[3][threadIdx.x]);
}

constexpr int SCATTER_BLOCKS = 256;

// db3[f] += the workgroups' partials: one wave per f, lane l adds partials l, l + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void border_scatter_finish_kernel(const float* __restrict__ part3, float* __restrict__ db3) {
    const int f = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int blk = lane; blk < SCATTER_BLOCKS; blk += 64) s += part3[(long)blk * 4 + f];
    s = wave_sum(s);
    if (lane == 0) db3[f] += s;
}

inline bool ring_ok(int B, int H2, int W2, int D, int dtype) {
    return B > 0 && H2 >= 2 && W2 >= 2 && D > 0 && D % 32 == 0 && (dtype == MTE_DT_BF16 || dtype == MTE_DT_F32);
}
inline bool border_ok(int B, int H2, int W2, int Co, int k, int dtype) {
    return B > 0 && Co > 0 && Co % 8 == 0 && k <= 5 && pb_shape_ok(H2, W2, k) && (dtype == MTE_DT_BF16 || dtype == MTE_DT_F32);
}

}  // namespace

extern "C" {

// fp32 elements of the `work` buffers below: ring weight gradient [4][PB_RING_BLOCKS][36]; scatter: dS [Co][k*k] + [SCATTER_BLOCKS][4]
long mte_pack_ring_work_elems(void) { return 4L * PB_RING_BLOCKS * 36; }
long mte_pack_border_scatter_work_elems(int Co, int k) { return (long)Co * k * k + 4L * SCATTER_BLOCKS; }
long mte_pack_border_class_sums_elems(int Co, int k) { return (long)k * k * PB_CLASS_SPLITS * Co; }

int mte_pack_ring_fwd(const void* P, long ldp, const float* K3, void* R_rows, void* R_cols, int B, int H2, int W2, int D, int dtype, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!P || !K3 || !R_rows || !R_cols || !ring_ok(B, H2, W2, D, dtype) || ldp < D || ldp % (dtype == MTE_DT_BF16 ? 8 : 4) != 0) return MTE_ERR_ARG;
    const int grid = bgrid(2L * B * (W2 + 2 + H2) * (D / 32));
    if (dtype == MTE_DT_BF16) hipLaunchKernelGGL(ring_fwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)P, ldp, K3, (bf16_t*)R_rows, (bf16_t*)R_cols, B, H2, W2, D);
    else hipLaunchKernelGGL(ring_fwd_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)P, ldp, K3, (float*)R_rows, (float*)R_cols, B, H2, W2, D);
    return mte_check_launch();
}

// dx [B][2 H2][2 W2][D/4] (the layer's un-shuffled input gradient) += ring stencil^T (dR_rows, dR_cols)
int mte_pack_ring_bwd_data(const void* dR_rows, const void* dR_cols, const float* K3, void* dx, long lddx, int B, int H2, int W2, int D, int dtype,
                           hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!dR_rows || !dR_cols || !K3 || !dx || !ring_ok(B, H2, W2, D, dtype) || lddx < D / 4 || lddx % (dtype == MTE_DT_BF16 ? 8 : 4) != 0) return MTE_ERR_ARG;
    const int grid = bgrid((long)B * pb_border_count(H2, W2, 1) * (D / 32) * 4);
    if (dtype == MTE_DT_BF16) hipLaunchKernelGGL(ring_bwd_data_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)dR_rows, (const bf16_t*)dR_cols, K3, (bf16_t*)dx, lddx, B, H2, W2, D);
    else hipLaunchKernelGGL(ring_bwd_data_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)dR_rows, (const float*)dR_cols, K3, (float*)dx, lddx, B, H2, W2, D);
    return mte_check_launch();
}

// dk3 [108] += sum dR (x) P through the ring stencil; work: mte_pack_ring_work_elems() floats (overwritten)
int mte_pack_ring_bwd_weight(const void* dR_rows, const void* dR_cols, const void* P, long ldp, float* dk3, float* work, int B, int H2, int W2, int D,
                             int dtype, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!dR_rows || !dR_cols || !P || !dk3 || !work || !ring_ok(B, H2, W2, D, dtype) || ldp < D || ldp % (dtype == MTE_DT_BF16 ? 8 : 4) != 0) return MTE_ERR_ARG;
    const dim3 grid(PB_RING_BLOCKS, 4);
    if (dtype == MTE_DT_BF16) hipLaunchKernelGGL(ring_bwd_weight_kernel<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)dR_rows, (const bf16_t*)dR_cols, (const bf16_t*)P, ldp, work, B, H2, W2, D);
    else hipLaunchKernelGGL(ring_bwd_weight_kernel<float>, grid, dim3(256), 0, stream, (const float*)dR_rows, (const float*)dR_cols, (const float*)P, ldp, work, B, H2, W2, D);
    hipLaunchKernelGGL(ring_bwd_weight_finish_kernel, dim3(108), dim3(64), 0, stream, (const float*)work, dk3);
    return mte_check_launch();
}

// Wr [2 pad Co][4D][1][k], Wc [2 pad Co][4D][k][1] (fp32 OIHW, negated), Dt [(2 pad + 1)^2][Co]  <-  W [Co][4D][k][k], b3 [4]
int mte_pack_border_weights(const float* W, const float* b3, float* Wr, float* Wc, float* Dt, int Co, int D, int k, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!W || !b3 || !Wr || !Wc || !Dt || Co <= 0 || D <= 0 || (k & 1) == 0 || k < 3 || k > 5) return MTE_ERR_ARG;
    int grid = bgrid(4L * (k / 2) * Co * 4 * D * k);
    if (grid < Co) grid = Co < 4096 ? Co : 4096;
    hipLaunchKernelGGL(border_weights_kernel, dim3(grid), dim3(256), 0, stream, W, b3, Wr, Wc, Dt, Co, D, k);
    return mte_check_launch();
}

int mte_pack_border_apply(void* y, long ldy, const float* corr_rows, const float* corr_cols, const float* Dt, int B, int H2, int W2, int Co, int k,
                          int dtype, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!y || !corr_rows || !corr_cols || !Dt || !border_ok(B, H2, W2, Co, k, dtype) || ldy < Co || ldy % (dtype == MTE_DT_BF16 ? 8 : 4) != 0) return MTE_ERR_ARG;
    const int pad = k / 2, per16 = dtype == MTE_DT_BF16 ? 8 : 4;
    const int grid = bgrid((long)B * pb_border_count(H2, W2, pad) * (Co / per16));
    if (dtype == MTE_DT_BF16) hipLaunchKernelGGL(border_apply_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (bf16_t*)y, ldy, corr_rows, corr_cols, Dt, B, H2, W2, Co, pad, 1, 0L, 0L);
    else hipLaunchKernelGGL(border_apply_kernel<float>, dim3(grid), dim3(256), 0, stream, (float*)y, ldy, corr_rows, corr_cols, Dt, B, H2, W2, Co, pad, 1, 0L, 0L);
    return mte_check_launch();
}

// mte_pack_border_apply on the workspace of mte_pack_border_gemm_fwd: `splits` slabs per ring-line family (rows first), added in slab order inside the apply loop
int mte_pack_border_apply_slabs(void* y, long ldy, const float* ws, int splits, const float* Dt, int B, int H2, int W2, int Co, int k, int dtype,
                                hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!y || !ws || splits < 1 || splits > PBG_MAX_SPLITS || !Dt || !border_ok(B, H2, W2, Co, k, dtype) || ldy < Co || ldy % (dtype == MTE_DT_BF16 ? 8 : 4) != 0)
        return MTE_ERR_ARG;
    const int pad = k / 2, per16 = dtype == MTE_DT_BF16 ? 8 : 4;
    const long slab_r = pb_gemm_slab_elems(0, B, H2, W2, Co, k), slab_c = pb_gemm_slab_elems(1, B, H2, W2, Co, k);
    const float* cr = ws;
    const float* cc = ws + splits * slab_r;
    const int grid = bgrid((long)B * pb_border_count(H2, W2, pad) * (Co / per16));
    if (dtype == MTE_DT_BF16) hipLaunchKernelGGL(border_apply_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (bf16_t*)y, ldy, cr, cc, Dt, B, H2, W2, Co, pad, splits, slab_r, slab_c);
    else hipLaunchKernelGGL(border_apply_kernel<float>, dim3(grid), dim3(256), 0, stream, (float*)y, ldy, cr, cc, Dt, B, H2, W2, Co, pad, splits, slab_r, slab_c);
    return mte_check_launch();
}

int mte_pack_border_gather(const void* dy, long lddy, void* G_rows, void* G_cols, int B, int H2, int W2, int Co, int k, int dtype, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!dy || !G_rows || !G_cols || !border_ok(B, H2, W2, Co, k, dtype) || lddy < Co || lddy % (dtype == MTE_DT_BF16 ? 8 : 4) != 0) return MTE_ERR_ARG;
    const int pad = k / 2, per16 = dtype == MTE_DT_BF16 ? 8 : 4;
    const int grid = bgrid(2L * B * (W2 + 2 + H2) * (2 * pad * Co / per16));
    if (dtype == MTE_DT_BF16) hipLaunchKernelGGL(border_gather_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, (const bf16_t*)dy, lddy, (bf16_t*)G_rows, (bf16_t*)G_cols, B, H2, W2, Co, pad);
    else hipLaunchKernelGGL(border_gather_kernel<float>, dim3(grid), dim3(256), 0, stream, (const float*)dy, lddy, (float*)G_rows, (float*)G_cols, B, H2, W2, Co, pad);
    return mte_check_launch();
}

// part [(2 pad + 1)^2][PB_CLASS_SPLITS][Co] (mte_pack_border_class_sums_elems floats, overwritten) <- dy
int mte_pack_border_class_sums(const void* dy, long lddy, float* part, int B, int H2, int W2, int Co, int k, int dtype, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!dy || !part || !border_ok(B, H2, W2, Co, k, dtype) || lddy < Co) return MTE_ERR_ARG;
    const dim3 grid(PB_CLASS_SPLITS, k * k);
    if (dtype == MTE_DT_BF16) hipLaunchKernelGGL(border_class_sums_kernel<bf16_t>, grid, dim3(256), 0, stream, (const bf16_t*)dy, lddy, part, B, H2, W2, Co, k / 2);
    else hipLaunchKernelGGL(border_class_sums_kernel<float>, grid, dim3(256), 0, stream, (const float*)dy, lddy, part, B, H2, W2, Co, k / 2);
    return mte_check_launch();
}

// dW [Co][4D][k][k] (overwritten: the dw_band argument of mte_unfold_pack_wgrad), dk3b[108 .. 112) += db3 of the class-bias path
// dWr / dWc: fp32 OIHW gradients of the (negated) ring weights; part: the class sums; work: mte_pack_border_scatter_work_elems floats
int mte_pack_border_scatter(const float* dWr, const float* dWc, const float* part, const float* W, const float* b3, float* dW, float* dk3b, float* work,
                            int Co, int D, int k, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!dWr || !dWc || !part || !W || !b3 || !dW || !dk3b || !work || Co <= 0 || D <= 0 || (k & 1) == 0 || k < 3 || k > 5) return MTE_ERR_ARG;
    float* dS = work;
    float* part3 = work + (long)Co * k * k;
    hipLaunchKernelGGL(border_ds_kernel, dim3((Co * k * k + 3) / 4), dim3(256), 0, stream, part, dS, Co, k);
    hipLaunchKernelGGL(border_scatter_kernel, dim3(SCATTER_BLOCKS), dim3(256), 0, stream, dWr, dWc, (const float*)dS, W, b3, dW, part3, Co, D, k);
    hipLaunchKernelGGL(border_scatter_finish_kernel, dim3(4), dim3(64), 0, stream, (const float*)part3, dk3b + 108);
    return mte_check_launch();
}

}  // extern "C"
