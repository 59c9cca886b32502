// Per-frame visualisation and ordinal-error work of the inference side on device for gfx950:
//   mte_order_stats_f32   the exact k-th and (k+1)-th smallest of n float32 values per image (np.percentile's two neighbours, min / max)
//   mte_colormap_u8       float32 [B,H,W] -> uint8 [B,H,W,3] through a 256-entry colour table (viz_inv_depth, the log colouring of infer_edges.py)
//   mte_d3r_count         the number of point pairs whose ordinal relation agrees between ground truth and prediction (utils/d3r.py)
// Every result is an integer or a copy of an input value: there is no floating-point sum anywhere, so results are bit-equal run to run.
//
// Order statistics: radix select over the order-preserving 32-bit key of a float (sign bit flipped for x >= 0, all bits for x < 0), four
// passes of 8 bits from the top.  A pass is two launches: os_hist_kernel counts, per image, the digit of every value whose upper bits equal
// the prefix chosen so far (a histogram per workgroup in LDS with integer atomics, merged into the image's histogram with integer global
// atomics), os_select_kernel (one workgroup per image) scans the 256 counts, picks the digit that holds the wanted rank, subtracts the counts
// in front of it and clears the histogram for the next pass.  The two ranks k and k + 1 may part ways at any digit, so each keeps a prefix
// and a histogram of its own.  No workgroup waits for another: what a pass needs from the one before arrives with the launch order.
#include "common.hpp"
#include "lidar_work.hpp"

namespace {

constexpr int DV_THREADS = 256;
constexpr int OS_BINS = 256;
constexpr int OS_STATE = 8;                               // uints per image in front of its histograms: [r] prefix, [2 + r] rank, [4] count
constexpr int OS_PER_IMAGE = OS_STATE + 2 * OS_BINS;      // uints of workspace per image

__device__ __forceinline__ unsigned os_key(float x) {
    const unsigned u = __float_as_uint(x + 0.f);          // -0 -> +0: one key for the two zeros
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float os_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

// shift = 24, 16, 8, 0.  grid (x, B).  Values that fail positive_only's test are in no histogram.
__global__ __launch_bounds__(DV_THREADS) void os_hist_kernel(const float* __restrict__ x, long stride, int n, int positive_only, int shift,
                                                             unsigned* __restrict__ work) {
    __shared__ unsigned s_hist[2][OS_BINS];
    unsigned* const st = work + (long)blockIdx.y * OS_PER_IMAGE;
    s_hist[0][threadIdx.x] = 0;
    s_hist[1][threadIdx.x] = 0;
    const unsigned upper = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    const unsigned p0 = st[0], p1 = st[1];                // written by the select launch in front (zero before the first pass)
    __syncthreads();
    const float* const src = x + (long)blockIdx.y * stride;
    for (int i = blockIdx.x * DV_THREADS + threadIdx.x; i < n; i += gridDim.x * DV_THREADS) {
        const float v = src[i];
        if (positive_only && !(v > 0.f)) continue;
        const unsigned key = os_key(v), digit = (key >> shift) & 255u;
        if ((key & upper) == p0) atomicAdd(&s_hist[0][digit], 1u);
        if ((key & upper) == p1) atomicAdd(&s_hist[1][digit], 1u);
    }
    __syncthreads();
    unsigned* const hist = st + OS_STATE;
    const unsigned c0 = s_hist[0][threadIdx.x], c1 = s_hist[1][threadIdx.x];
    if (c0) atomicAdd(&hist[threadIdx.x], c0);
    if (c1) atomicAdd(&hist[OS_BINS + threadIdx.x], c1);
}

// one workgroup per image, thread t owns digit t
__global__ __launch_bounds__(OS_BINS) void os_select_kernel(const int* __restrict__ k, int shift, unsigned* __restrict__ work, float* __restrict__ out,
                                                            int* __restrict__ count_out) {
    __shared__ unsigned s_wave[2][OS_BINS / 64];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned* const st = work + (long)b * OS_PER_IMAGE;
    unsigned* const hist = st + OS_STATE;
    unsigned c[2] = {hist[t], hist[OS_BINS + t]}, incl[2] = {c[0], c[1]};
    hist[t] = 0;
    hist[OS_BINS + t] = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_up(incl[r], o, 64);
            if (lane >= o) incl[r] += v;
        }
        if (lane == 63) s_wave[r][wave] = incl[r];
    }
    const unsigned prefix[2] = {st[0], st[1]};
    unsigned rank[2] = {st[2], st[3]};
    __syncthreads();                                      // the state words are read by every thread before any is rewritten below
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < OS_BINS / 64; ++w) {
            const unsigned v = s_wave[r][w];
            if (w < wave) before += v;
            total += v;
        }
        if (shift == 24) {                                // first pass: total = the number of values that take part
            const long want = (long)k[b] + r;
            rank[r] = total == 0 ? 0u : (unsigned)(want < 0 ? 0 : (want > (long)total - 1 ? (long)total - 1 : want));
            if (t == 0 && r == 0) {
                st[4] = total;
                if (count_out) count_out[b] = (int)total;
                if (total == 0) { out[2 * b] = 0.f; out[2 * b + 1] = 0.f; }
            }
        }
        const unsigned excl = before + incl[r] - c[r];
        if (rank[r] >= excl && rank[r] < excl + c[r]) {    // exactly one thread when the image has a value at all
            const unsigned key = prefix[r] | ((unsigned)t << shift);
            st[r] = key;
            st[2 + r] = rank[r] - excl;
            if (shift == 0) out[2 * b + r] = os_value(key);
        }
    }
}

// ---- colour look-up: a thread owns 4 consecutive pixels of the flat [B*H*W] range = 12 output bytes, stored as three words
constexpr int CM_PIX = 4;

__device__ __forceinline__ unsigned cm_lookup(float v, float d, int log_mode, float lo, float hi, const unsigned* s_table) {
    float x;
    if (log_mode) x = ((float)log((double)v) - lo) / hi;  // the log in double, rounded to float32 once
    else x = v / d;
    if (x != x) return 0u;                                // matplotlib's "bad" colour (0, 0, 0, 0) -> black
    x = fminf(fmaxf(x, 0.f), 1.f);
    int idx = (int)(x * 256.f);
    idx = idx > 255 ? 255 : idx;
    return s_table[idx];
}

__global__ __launch_bounds__(DV_THREADS) void colormap_kernel(const float* __restrict__ x, long total, int hw, const float* __restrict__ divisor,
                                                              const float* __restrict__ lo_hi, const unsigned char* __restrict__ table,
                                                              int vec_in, unsigned char* __restrict__ out) {
    __shared__ unsigned s_table[256];
    s_table[threadIdx.x] = (unsigned)table[3 * threadIdx.x] | ((unsigned)table[3 * threadIdx.x + 1] << 8) | ((unsigned)table[3 * threadIdx.x + 2] << 16);
    __syncthreads();
    const int log_mode = lo_hi != nullptr;
    const long groups = (total + CM_PIX - 1) / CM_PIX;
    for (long g = (long)blockIdx.x * DV_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * DV_THREADS) {
        const long p = g * CM_PIX;
        float v[CM_PIX];
        if (vec_in && p + CM_PIX <= total) {
            const f32x4_t q = *reinterpret_cast<const f32x4_t*>(x + p);
#pragma unroll
            for (int e = 0; e < CM_PIX; ++e) v[e] = q[e];
        } else {
#pragma unroll
            for (int e = 0; e < CM_PIX; ++e) v[e] = p + e < total ? x[p + e] : 0.f;
        }
        long b = p / hw;
        long next = (b + 1) * hw;                         // first pixel of the next image
        unsigned c[CM_PIX];
#pragma unroll
        for (int e = 0; e < CM_PIX; ++e) {
            if (p + e >= next) { ++b; next += hw; }
            c[e] = 0;
            if (p + e < total) c[e] = log_mode ? cm_lookup(v[e], 1.f, 1, lo_hi[2 * b], lo_hi[2 * b + 1], s_table)
                                               : cm_lookup(v[e], divisor[b], 0, 0.f, 0.f, s_table);
        }
        unsigned char* const o = out + 3 * p;             // 12 g bytes in: word aligned when `out` is
        if (p + CM_PIX <= total) {
            unsigned* const ow = reinterpret_cast<unsigned*>(o);
            ow[0] = c[0] | (c[1] << 24);
            ow[1] = (c[1] >> 8) | (c[2] << 16);
            ow[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
            for (int e = 0; e < CM_PIX && p + e < total; ++e) {
                o[3 * e] = (unsigned char)(c[e] & 255u);
                o[3 * e + 1] = (unsigned char)((c[e] >> 8) & 255u);
                o[3 * e + 2] = (unsigned char)(c[e] >> 16);
            }
        }
    }
}

// ---- D3R: the ordinal relation of a pair is +1 / -1 / 0 by the ratio of its two values against 1 +- 0.03; a pair agrees when ground truth and
// prediction both say +1 or both say -1 (utils/d3r.py).  The ground-truth ratio is a double (upstream divides a float64 map), the prediction's
// a float32 compared with the float32 roundings of the two bounds (numpy >= 2 compares a float32 array with a Python float in float32).
__global__ __launch_bounds__(DV_THREADS) void d3r_count_kernel(const float* __restrict__ gt, const float* __restrict__ pred, int hw, const int* __restrict__ pts,
                                                               int n, const int* __restrict__ n_dev, const int* __restrict__ pairs, int P,
                                                               int* __restrict__ count) {
    if (*n_dev < n) n = *n_dev;                            // never past the list the index stage wrote
    const double tol = 0.03, g_hi = 1 + tol, g_lo = 1 - tol;
    const float p_hi = (float)g_hi, p_lo = (float)g_lo;
    int agree = 0;
    for (int i = blockIdx.x * DV_THREADS + threadIdx.x; i < P; i += gridDim.x * DV_THREADS) {
        const int o1 = pairs[2 * i], o2 = pairs[2 * i + 1];
        if ((unsigned)o1 >= (unsigned)n || (unsigned)o2 >= (unsigned)n) continue;
        const int q1 = pts[o1], q2 = pts[o2];
        if ((unsigned)q1 >= (unsigned)hw || (unsigned)q2 >= (unsigned)hw) continue;
        const double gr = (double)gt[q1] / (double)gt[q2];
        const float pr = pred[q1] / pred[q2];
        agree += ((gr > g_hi) && (pr > p_hi)) || ((gr < g_lo) && (pr < p_lo));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) agree += __shfl_xor(agree, o, 64);
    if ((threadIdx.x & 63) == 0 && agree) atomicAdd(count, agree);
}

inline unsigned dv_grid(long items, long cap) { long g = (items + DV_THREADS - 1) / DV_THREADS; if (g > cap) g = cap; if (g < 1) g = 1; return (unsigned)g; }

}  // namespace

extern "C" {

long mte_order_stats_work_bytes(int B) { return B > 0 && B <= 65535 ? 4L * B * OS_PER_IMAGE : 0; }

int mte_order_stats_f32(const float* x, long stride, int B, long n, const int* k, int positive_only, float* out, int* count_out, void* work,
                        hipStream_t stream) {
    if (!x || !k || !out || !work || B <= 0 || B > 65535 || n <= 0 || stride < 0 || ((uintptr_t)work & 3)) return MTE_ERR_ARG;
    if (n >= (1L << 30)) return MTE_ERR_UNSUPPORTED;
    if (mte_memset_async(work, 0, (size_t)mte_order_stats_work_bytes(B), stream) != hipSuccess) return MTE_ERR_LAUNCH;
    const dim3 grid(dv_grid((n + 3) / 4, 1024), B);        // about four values per thread
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(os_hist_kernel, grid, dim3(DV_THREADS), 0, stream, x, stride, (int)n, positive_only, shift, (unsigned*)work);
        hipLaunchKernelGGL(os_select_kernel, dim3(B), dim3(OS_BINS), 0, stream, k, shift, (unsigned*)work, out, count_out);
    }
    return mte_check_launch();
}

int mte_colormap_u8(const float* x, int B, int H, int W, const float* divisor, const float* lo_hi, const unsigned char* table, unsigned char* out,
                    hipStream_t stream) {
    if (!x || !table || !out || B <= 0 || H <= 0 || W <= 0 || (!divisor && !lo_hi) || ((uintptr_t)out & 3) || ((uintptr_t)x & 3)) return MTE_ERR_ARG;
    if ((long)H * W >= (1L << 30) || (long)B * H * W >= (1L << 30)) return MTE_ERR_UNSUPPORTED;
    const long total = (long)B * H * W;
    hipLaunchKernelGGL(colormap_kernel, dim3(dv_grid((total + CM_PIX - 1) / CM_PIX, 2048)), dim3(DV_THREADS), 0, stream, x, total, H * W, divisor, lo_hi,
                       table, (int)(((uintptr_t)x & 15) == 0), out);
    return mte_check_launch();
}

int mte_d3r_count(const float* gt, const float* pred, int H, int W, const void* index_work, int n, const int* pairs, int P, int* count,
                  hipStream_t stream) {
    if (!gt || !pred || !index_work || !pairs || !count || H <= 0 || W <= 0 || ((uintptr_t)index_work & 7) || n <= 0 || P <= 0) return MTE_ERR_ARG;
    if ((long)H * W >= (1L << 30) || P >= (1 << 30)) return MTE_ERR_UNSUPPORTED;
    if (n > H * W) return MTE_ERR_ARG;
    const LpWork w = lp_carve(const_cast<void*>(index_work), (long)H * W);
    if (mte_memset_async(count, 0, sizeof(int), stream) != hipSuccess) return MTE_ERR_LAUNCH;
    hipLaunchKernelGGL(d3r_count_kernel, dim3(dv_grid(P, 1024)), dim3(DV_THREADS), 0, stream, gt, pred, H * W, (const int*)w.pts, n, (const int*)w.head, pairs,
                       P, count);
    return mte_check_launch();
}

}  // extern "C"
