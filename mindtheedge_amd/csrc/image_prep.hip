// Training-image preparation on device for gfx950: the 8-bit image half of the reference's train_transforms
// (datasets/transforms.py:17-50), bit for bit as PIL / torchvision-on-PIL compute it on the host.
//   resample   Image.crop(borders) + Image.resize((W, H), LANCZOS) = PIL's ImagingResample for 8-bit RGB: a horizontal pass whose result
//              is clipped and stored as uint8, then a vertical pass.  The 22-bit fixed-point coefficient tables come from the host
//              (datasets/image_prep.py::lanczos_coeffs, double precision like precompute_coeffs + normalize_coeffs_8bpc); a pass whose
//              input and output length agree gets the identity table (one tap of 1 << 22), which reproduces the byte.
//              One launch: a workgroup owns a 16 x 64 output tile, stages the source rows it needs into LDS with dword loads, filters
//              them horizontally into a uint8 LDS image and runs the vertical pass out of that.  When the tap span of a tile does not
//              fit (heavy down-scaling): two launches with a uint8 intermediate in a caller-provided workspace, same arithmetic.
//   jitter     torchvision's adjust_brightness / adjust_contrast / adjust_saturation (ImageEnhance = Image.blend in float32) and
//              adjust_hue (Convert.c rgb2hsv / hsv2rgb) in a per-sample order, each rounding to uint8, then ToTensor:
//              float32(u8) / 255 as CHW.  Contrast needs the mean luma of the whole image as it is at that point of the order:
//              launch A re-applies the operations in front of contrast and adds the luma up with 64-bit integer atomics (exact,
//              order-independent), launch B applies everything and writes the outputs.
// Integer / IEEE float and double arithmetic only, no fast-math intrinsics; this file relies on -ffp-contract=off (_build.FLAGS).
#include "common.hpp"

namespace {

constexpr int PREC = 22;                        // PIL PRECISION_BITS
constexpr int TW = 64, TH = 16;                 // output tile of the fused kernel
constexpr int RAW_BYTES = 16384;                // staged source rows (one chunk)
constexpr int MID_BYTES = 32768;                // horizontally filtered rows of the tile, uint8 [R][TW][3]
constexpr int MID_PITCH = TW * 3;

// The empty asm keeps the clipped byte opaque.  Without it hipcc (ROCm 7.2) fuses two clips and the byte packing of the vertical pass
// into v_ashr_pk_u8_i32 and treats the upper half of its destination as zero; on the MI355X bytes 2 and 3 of the packed word then came out
// OR-ed with the previous contents of that register (deterministic, only positive errors, only in those two bytes).
// tests/test_image_prep_cpu.py checks that the instruction is absent from this file's code.
__device__ __forceinline__ unsigned clip8(int acc) {
    const int v = acc >> PREC;
    unsigned r = (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
    asm volatile("" : "+v"(r));
    return r;
}

__global__ __launch_bounds__(256) void resample_fused_kernel(const unsigned char* __restrict__ src, long stride, int in_h, int in_w,
                                                             unsigned char* __restrict__ dst, int out_h, int out_w,
                                                             const int* __restrict__ kkh, const int* __restrict__ bh, int ksh,
                                                             const int* __restrict__ kkv, const int* __restrict__ bv, int ksv,
                                                             unsigned* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[RAW_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char mid[MID_BYTES];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int tw = min(TW, out_w - x0), th = min(TH, out_h - y0);
    if (tw <= 0 || th <= 0) return;
    // source window of the tile: the bounds are non-decreasing in the output index
    const int xs = max(bh[2 * x0], 0), xe = min(bh[2 * (x0 + tw - 1)] + bh[2 * (x0 + tw - 1) + 1], in_w);
    const int ys = max(bv[2 * y0], 0), ye = min(bv[2 * (y0 + th - 1)] + bv[2 * (y0 + th - 1) + 1], in_h);
    const int segb = (xe - xs) * 3, R = ye - ys;
    const int rpitch = (segb + 6) & ~3;         // staged row: up to 3 bytes of lead-in so that LDS and global dwords line up
    if (segb <= 0 || R <= 0 || rpitch > RAW_BYTES || R * MID_PITCH > MID_BYTES) {
        // cannot happen with the LANCZOS tables of exactly (in, out): the host checked a bound of the tap span (fused_fits).  Tables of
        // another filter leave this tile unwritten -- say so through the device error word instead of returning quietly.
        if (tid == 0) mte_report_device_error(err, MTE_DEVERR_IMAGE_RESAMPLE);
        return;
    }
    const int ndw = rpitch >> 2;
    const int rows_per_chunk = RAW_BYTES / rpitch;
    for (int r0 = 0; r0 < R; r0 += rows_per_chunk) {
        const int nr = min(rows_per_chunk, R - r0);
        for (int i = tid; i < nr * ndw; i += 256) {
            const int r = i / ndw, d = i - r * ndw;
            const unsigned char* g0 = src + (long)(ys + r0 + r) * stride + (long)xs * 3;
            const int b0 = 4 * d - (int)((uintptr_t)g0 & 3);                  // first segment byte of this (global-aligned) dword
            unsigned v = 0;
            if (b0 >= 0 && b0 + 4 <= segb) {
                v = *(const unsigned*)(g0 + b0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (b0 + j >= 0 && b0 + j < segb) v |= (unsigned)g0[b0 + j] << (8 * j);
            }
            ((unsigned*)raw)[r * ndw + d] = v;
        }
        __syncthreads();
        for (int i = tid; i < nr * tw; i += 256) {
            const int r = i / tw, x = i - r * tw;
            const int mis = (int)((uintptr_t)(src + (long)(ys + r0 + r) * stride + (long)xs * 3) & 3);
            const int xmin = max(bh[2 * (x0 + x)], xs);
            const int cnt = min(min(bh[2 * (x0 + x) + 1], ksh), xe - xmin);
            const unsigned char* p = raw + r * rpitch + mis + (xmin - xs) * 3;
            const int* k = kkh + (long)(x0 + x) * ksh;
            int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < cnt; ++t, p += 3) {
                const int c = k[t];
                a0 += (int)p[0] * c;
                a1 += (int)p[1] * c;
                a2 += (int)p[2] * c;
            }
            unsigned char* m = mid + (r0 + r) * MID_PITCH + x * 3;
            m[0] = (unsigned char)clip8(a0);
            m[1] = (unsigned char)clip8(a1);
            m[2] = (unsigned char)clip8(a2);
            if (x == tw - 1)                                 // ragged tile: the vertical pass reads whole dwords, give the row's last one defined bytes
                for (int j = 3; ((x * 3 + j) & 3) != 0; ++j) m[j] = 0;
        }
        __syncthreads();
    }
    // vertical pass: every byte column is independent, a thread owns four of them
    const int nb = tw * 3, ndq = (nb + 3) >> 2;
    for (int i = tid; i < th * ndq; i += 256) {
        const int y = i / ndq, d = i - y * ndq;
        const int ymin = max(bv[2 * (y0 + y)], ys);
        const int cnt = min(min(bv[2 * (y0 + y) + 1], ksv), ye - ymin);
        const int* k = kkv + (long)(y0 + y) * ksv;
        const unsigned* m = (const unsigned*)(mid + (ymin - ys) * MID_PITCH) + d;
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int t = 0; t < cnt; ++t, m += MID_PITCH / 4) {
            const unsigned v = *m;
            const int c = k[t];
            a0 += (int)(v & 255u) * c;
            a1 += (int)((v >> 8) & 255u) * c;
            a2 += (int)((v >> 16) & 255u) * c;
            a3 += (int)(v >> 24) * c;
        }
        const unsigned packed = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (clip8(a3) << 24);
        unsigned char* o = dst + ((long)(y0 + y) * out_w + x0) * 3 + 4 * d;
        const int nvalid = min(4, nb - 4 * d);
        if (nvalid == 4 && ((uintptr_t)o & 3) == 0) {
            *(unsigned*)o = packed;
        } else {
            for (int j = 0; j < nvalid; ++j) o[j] = (unsigned char)(packed >> (8 * j));
        }
    }
}

// two-launch form: src window -> mid uint8 [in_h][out_w][3] -> dst
__global__ __launch_bounds__(256) void resample_h_kernel(const unsigned char* __restrict__ src, long stride, int in_h, int in_w,
                                                         unsigned char* __restrict__ mid, int out_w, const int* __restrict__ kkh,
                                                         const int* __restrict__ bh, int ksh) {
    const long n = (long)in_h * out_w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int y = (int)(i / out_w), x = (int)(i - (long)y * out_w);
        const int xmin = max(bh[2 * x], 0);
        const int cnt = min(min(bh[2 * x + 1], ksh), in_w - xmin);
        const unsigned char* p = src + (long)y * stride + (long)xmin * 3;
        const int* k = kkh + (long)x * ksh;
        int a0 = 1 << (PREC - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < cnt; ++t, p += 3) {
            const int c = k[t];
            a0 += (int)p[0] * c;
            a1 += (int)p[1] * c;
            a2 += (int)p[2] * c;
        }
        unsigned char* m = mid + i * 3;
        m[0] = (unsigned char)clip8(a0);
        m[1] = (unsigned char)clip8(a1);
        m[2] = (unsigned char)clip8(a2);
    }
}

__global__ __launch_bounds__(256) void resample_v_kernel(const unsigned char* __restrict__ mid, int in_h, int out_w,
                                                         unsigned char* __restrict__ dst, int out_h, const int* __restrict__ kkv,
                                                         const int* __restrict__ bv, int ksv) {
    const long nb = (long)out_w * 3, n = (long)out_h * nb;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int y = (int)(i / nb);
        const long j = i - (long)y * nb;
        const int ymin = max(bv[2 * y], 0);
        const int cnt = min(min(bv[2 * y + 1], ksv), in_h - ymin);
        const unsigned char* p = mid + (long)ymin * nb + j;
        const int* k = kkv + (long)y * ksv;
        int a = 1 << (PREC - 1);
        for (int t = 0; t < cnt; ++t, p += nb) a += (int)p[0] * k[t];
        dst[i] = (unsigned char)clip8(a);
    }
}

// conservative bound of a tile's tap span: xe - xs <= (n - 1) * scale + 2 * support + 1
inline bool fused_fits(int in_h, int in_w, int out_h, int out_w) {
    const double sx = (double)in_w / out_w, sy = (double)in_h / out_h;
    const double fx = sx > 1.0 ? sx : 1.0, fy = sy > 1.0 ? sy : 1.0;
    long segw = (long)((TW - 1) * sx + 6.0 * fx) + 3, rows = (long)((TH - 1) * sy + 6.0 * fy) + 3;
    if (segw > in_w) segw = in_w;
    if (rows > in_h) rows = in_h;
    return ((segw * 3 + 6) & ~3L) <= RAW_BYTES && rows * MID_PITCH <= MID_BYTES;
}

// ---- colour jitter + ToTensor ---------------------------------------------------------------------------------------------------------

#define OP_BRIGHTNESS 0
#define OP_CONTRAST 1
#define OP_SATURATION 2
#define OP_HUE 3

struct Jitter {
    float f[4];          // brightness, contrast, saturation factor; f[3] = the uint8 added to H (0..255)
    int order[4];        // operation ids in the order they are applied, -1 = none
};

__device__ __forceinline__ Jitter load_jitter(const float* __restrict__ factors, const int* __restrict__ order, int b) {
    Jitter P;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        P.f[i] = order ? factors[4 * b + i] : 0.f;
        P.order[i] = order ? order[4 * b + i] : -1;
    }
    return P;
}

__device__ __forceinline__ bool has_contrast(const Jitter& P) {
    return P.order[0] == OP_CONTRAST || P.order[1] == OP_CONTRAST || P.order[2] == OP_CONTRAST || P.order[3] == OP_CONTRAST;
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate, image, f): float32, truncation; clipping only when f is outside [0, 1]
__device__ __forceinline__ int blend1(int d, int i, float f) {
    const float t = (float)d + f * (float)(i - d);
    if (f >= 0.f && f <= 1.f) return (int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ void rgb2hsv(int r, int g, int b, int& H, int& S, int& V) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    V = maxc;
    if (minc == maxc) { H = 0; S = 0; return; }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    double hd = (double)h / 6.0 + 1.0;                   // in [5/6, 2): fmod(hd, 1.0) is one exact subtraction
    if (hd >= 1.0) hd -= 1.0;
    h = (float)hd;
    H = clip255((int)((double)h * 255.0));
    S = clip255((int)((double)s * 255.0));
}

__device__ __forceinline__ int round_away(double x) { return (int)(x >= 0.0 ? floor(x + 0.5) : ceil(x - 0.5)); }

__device__ __forceinline__ void hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
    if (s == 0) { r = g = b = v; return; }
    const double hf = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)(float)i);
    const float fs = (float)((double)(float)s / 255.0);
    const double vd = (double)v;
    const float fsf = fs * f;
    const int p = clip255(round_away(vd * (1.0 - (double)fs)));
    const int q = clip255(round_away(vd * (1.0 - (double)fsf)));
    const int t = clip255(round_away(vd * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// applies the operations in order; stop_at_contrast: only those in front of contrast (launch A)
__device__ __forceinline__ void jitter_pixel(int& r, int& g, int& b, const Jitter& P, bool stop_at_contrast, int mean) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = P.order[k];
        if (op == OP_BRIGHTNESS) {
            r = blend1(0, r, P.f[0]); g = blend1(0, g, P.f[0]); b = blend1(0, b, P.f[0]);
        } else if (op == OP_CONTRAST) {
            if (stop_at_contrast) return;
            r = blend1(mean, r, P.f[1]); g = blend1(mean, g, P.f[1]); b = blend1(mean, b, P.f[1]);
        } else if (op == OP_SATURATION) {
            const int L = luma(r, g, b);
            r = blend1(L, r, P.f[2]); g = blend1(L, g, P.f[2]); b = blend1(L, b, P.f[2]);
        } else if (op == OP_HUE) {
            int H, S, V;
            rgb2hsv(r, g, b, H, S, V);
            H = (H + (int)P.f[3]) & 255;
            hsv2rgb(H, S, V, r, g, b);
        }
    }
}

// VEC pixels of sample b starting at pixel VEC * g: 4 = three aligned dword loads, 1 = bytes
template <int VEC>
__device__ __forceinline__ void load_px(const unsigned char* __restrict__ in, long pix, int* r, int* g, int* b) {
    if (VEC == 4) {
        const unsigned* p = (const unsigned*)(in + pix * 3);
        const unsigned w0 = p[0], w1 = p[1], w2 = p[2];
        r[0] = w0 & 255; g[0] = (w0 >> 8) & 255; b[0] = (w0 >> 16) & 255;
        r[1] = w0 >> 24; g[1] = w1 & 255; b[1] = (w1 >> 8) & 255;
        r[2] = (w1 >> 16) & 255; g[2] = w1 >> 24; b[2] = w2 & 255;
        r[3] = (w2 >> 8) & 255; g[3] = (w2 >> 16) & 255; b[3] = w2 >> 24;
    } else {
        const unsigned char* p = in + pix * 3;
        r[0] = p[0]; g[0] = p[1]; b[0] = p[2];
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void jitter_luma_sum_kernel(const unsigned char* __restrict__ in, const float* __restrict__ factors,
                                                              const int* __restrict__ order, unsigned long long* __restrict__ sums, int HW) {
    __shared__ unsigned long long part[256];
    const int smp = blockIdx.y;
    const Jitter P = load_jitter(factors, order, smp);
    if (!has_contrast(P)) return;                          // uniform per workgroup
    unsigned long long acc = 0;
    const int ngroups = HW / VEC;
    for (int gi = blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += gridDim.x * 256) {
        int r[VEC], g[VEC], b[VEC];
        load_px<VEC>(in, (long)smp * HW + (long)gi * VEC, r, g, b);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            jitter_pixel(r[v], g[v], b[v], P, true, 0);
            acc += (unsigned long long)luma(r[v], g[v], b[v]);
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(&sums[smp], part[0]);
}

template <int VEC>
__global__ __launch_bounds__(256) void jitter_apply_kernel(const unsigned char* __restrict__ in, const float* __restrict__ factors,
                                                           const int* __restrict__ order, const unsigned long long* __restrict__ sums,
                                                           float* __restrict__ out, float* __restrict__ out_orig, int HW) {
    const int smp = blockIdx.y;
    const Jitter P = load_jitter(factors, order, smp);
    int mean = 0;
    if (has_contrast(P) && sums) mean = (int)((double)sums[smp] / (double)HW + 0.5);       // int(ImageStat.Stat(L).mean[0] + 0.5)
    const int ngroups = HW / VEC;
    float* o = out + (long)smp * 3 * HW;
    float* oo = out_orig ? out_orig + (long)smp * 3 * HW : nullptr;
    for (int gi = blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += gridDim.x * 256) {
        int r[VEC], g[VEC], b[VEC];
        load_px<VEC>(in, (long)smp * HW + (long)gi * VEC, r, g, b);
        if (oo) {
            if (VEC == 4) {
                *(f32x4_t*)(oo + (long)gi * 4) = f32x4_t{(float)r[0] / 255.0f, (float)r[1] / 255.0f, (float)r[2] / 255.0f, (float)r[3] / 255.0f};
                *(f32x4_t*)(oo + HW + (long)gi * 4) = f32x4_t{(float)g[0] / 255.0f, (float)g[1] / 255.0f, (float)g[2] / 255.0f, (float)g[3] / 255.0f};
                *(f32x4_t*)(oo + 2L * HW + (long)gi * 4) = f32x4_t{(float)b[0] / 255.0f, (float)b[1] / 255.0f, (float)b[2] / 255.0f, (float)b[3] / 255.0f};
            } else {
                oo[gi] = (float)r[0] / 255.0f; oo[HW + gi] = (float)g[0] / 255.0f; oo[2L * HW + gi] = (float)b[0] / 255.0f;
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) jitter_pixel(r[v], g[v], b[v], P, false, mean);
        if (VEC == 4) {
            *(f32x4_t*)(o + (long)gi * 4) = f32x4_t{(float)r[0] / 255.0f, (float)r[1] / 255.0f, (float)r[2] / 255.0f, (float)r[3] / 255.0f};
            *(f32x4_t*)(o + HW + (long)gi * 4) = f32x4_t{(float)g[0] / 255.0f, (float)g[1] / 255.0f, (float)g[2] / 255.0f, (float)g[3] / 255.0f};
            *(f32x4_t*)(o + 2L * HW + (long)gi * 4) = f32x4_t{(float)b[0] / 255.0f, (float)b[1] / 255.0f, (float)b[2] / 255.0f, (float)b[3] / 255.0f};
        } else {
            o[gi] = (float)r[0] / 255.0f; o[HW + gi] = (float)g[0] / 255.0f; o[2L * HW + gi] = (float)b[0] / 255.0f;
        }
    }
}

inline unsigned blocks_for(long items, long cap) { long g = (items + 255) / 256; if (g > cap) g = cap; if (g < 1) g = 1; return (unsigned)g; }

}  // namespace

extern "C" {

long mte_image_resample_work_bytes(int in_h, int in_w, int out_h, int out_w, int two_pass) {
    if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return 0;
    return (!two_pass && fused_fits(in_h, in_w, out_h, out_w)) ? 0 : (long)in_h * out_w * 3;
}

int mte_image_resample_u8(const unsigned char* src, long src_stride, int crop_x, int crop_y, int in_h, int in_w, unsigned char* dst,
                          int out_h, int out_w, const int* kk_h, const int* bounds_h, int ksize_h, const int* kk_v, const int* bounds_v,
                          int ksize_v, unsigned char* workspace, int two_pass, hipStream_t stream) {
    if (!src || !dst || !kk_h || !bounds_h || !kk_v || !bounds_v || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 || ksize_h <= 0 ||
        ksize_v <= 0 || crop_x < 0 || crop_y < 0 || src_stride < ((long)crop_x + in_w) * 3 || out_h > 65535 * TH ||
        (long)in_h * out_w * 3 >= (1L << 40) || (long)out_h * out_w * 3 >= (1L << 40))
        return MTE_ERR_ARG;
    const unsigned char* win = src + (long)crop_y * src_stride + (long)crop_x * 3;
    if (!two_pass && fused_fits(in_h, in_w, out_h, out_w)) {
        hipLaunchKernelGGL(resample_fused_kernel, dim3(cdiv(out_w, TW), cdiv(out_h, TH)), dim3(256), 0, stream, win, src_stride, in_h, in_w, dst,
                           out_h, out_w, kk_h, bounds_h, ksize_h, kk_v, bounds_v, ksize_v, g_mte_err_dev);
        return mte_check_launch();
    }
    if (!workspace) return MTE_ERR_ARG;
    hipLaunchKernelGGL(resample_h_kernel, dim3(blocks_for((long)in_h * out_w, 8192)), dim3(256), 0, stream, win, src_stride, in_h, in_w, workspace,
                       out_w, kk_h, bounds_h, ksize_h);
    hipLaunchKernelGGL(resample_v_kernel, dim3(blocks_for((long)out_h * out_w * 3, 8192)), dim3(256), 0, stream, workspace, in_h, out_w, dst, out_h,
                       kk_v, bounds_v, ksize_v);
    return mte_check_launch();
}

int mte_color_jitter_u8_to_f32(const unsigned char* in, int B, int H, int W, const float* factors, const int* order, int any_contrast,
                               unsigned long long* luma_sums, float* out, float* out_original, hipStream_t stream) {
    if (!in || !out || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long)H * W >= (1L << 30) || (order && !factors) ||
        (any_contrast && (!order || !luma_sums)))
        return MTE_ERR_ARG;
    const int HW = H * W;
    const bool vec = HW % 4 == 0 && ((uintptr_t)in & 3) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)out_original & 15) == 0;
    const dim3 grid(blocks_for(vec ? HW / 4 : HW, 2048), B);
    if (any_contrast) {
        if (vec) hipLaunchKernelGGL(jitter_luma_sum_kernel<4>, grid, dim3(256), 0, stream, in, factors, order, luma_sums, HW);
        else hipLaunchKernelGGL(jitter_luma_sum_kernel<1>, grid, dim3(256), 0, stream, in, factors, order, luma_sums, HW);
    }
    if (vec) hipLaunchKernelGGL(jitter_apply_kernel<4>, grid, dim3(256), 0, stream, in, factors, order, luma_sums, out, out_original, HW);
    else hipLaunchKernelGGL(jitter_apply_kernel<1>, grid, dim3(256), 0, stream, in, factors, order, luma_sums, out, out_original, HW);
    return mte_check_launch();
}

}  // extern "C"
