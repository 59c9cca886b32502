// Evaluation-sample preparation on device for gfx950: the two OpenCV resizes the reference's validation_transforms / test_transforms apply
// on the host (datasets/transforms.py:53-125, augmentations.py:37-55).
//   resize_linear_u8    cv2.resize(uint8 map, (W,H)) with the default INTER_LINEAR: OpenCV's fixed-point bilinear (11-bit coefficients,
//                       horizontal pass in int32, vertical pass with the >>4 / >>16 / +2 >>2 rounding), and the 2x2 area average OpenCV
//                       switches to when the source is EXACTLY twice the target in both axes.
//   resize_nearest_f32  cv2.resize(float map, (W,H), INTER_NEAREST): sx = min(floor(dx * (1 / (W / w))), w - 1), rows alike.
// PARITY UNPINNED: both restate OpenCV's published algorithms without OpenCV at hand, like mte_resize_linear and the Canny step; they are
// pinned bit for bit to an independent NumPy statement of the same rules (tests/eval_prep_ref.py).
// One thread per output pixel; the horizontal intermediate is never stored: each thread recomputes its two row taps (4 byte loads).
#include "common.hpp"

namespace {

constexpr int COEF_BITS = 11;                 // INTER_RESIZE_COEF_BITS
constexpr int COEF_ONE = 1 << COEF_BITS;

// source index and the two 16-bit coefficients of output coordinate d along an axis of `n` source and `N` target pixels
__device__ __forceinline__ void linear_tap(int d, int n, double scale, int& s, int& c0, int& c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n - 1) { s = n - 1; f = 0.f; }
    c1 = (int)(short)rintf(f * (float)COEF_ONE);                 // round half to even, float products
    c0 = (int)(short)rintf((1.f - f) * (float)COEF_ONE);
}

__global__ __launch_bounds__(256) void resize_linear_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                               int h, int w, int H, int W, double scale_y, double scale_x, int area) {
    const int b = blockIdx.y;
    const unsigned char* S = src + (long)b * h * w;
    unsigned char* D = dst + (long)b * H * W;
    const int HW = H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const int dy = i / W, dx = i - dy * W;
        if (area) {                                              // h == 2H and w == 2W: every index below is inside the source
            const unsigned char* r0 = S + (long)(2 * dy) * w + 2 * dx;
            D[i] = (unsigned char)(((int)r0[0] + (int)r0[1] + (int)r0[w] + (int)r0[w + 1] + 2) >> 2);
            continue;
        }
        int sx, a0, a1, sy, b0, b1;
        linear_tap(dx, w, scale_x, sx, a0, a1);
        linear_tap(dy, h, scale_y, sy, b0, b1);
        const int sx1 = min(sx + 1, w - 1), sy1 = min(sy + 1, h - 1);
        const unsigned char* r0 = S + (long)sy * w;
        const unsigned char* r1 = S + (long)sy1 * w;
        const int R0 = (int)r0[sx] * a0 + (int)r0[sx1] * a1;
        const int R1 = (int)r1[sx] * a0 + (int)r1[sx1] * a1;
        D[i] = (unsigned char)((((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2);
    }
}

__global__ __launch_bounds__(256) void resize_nearest_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int h, int w, int H, int W,
                                                                 double ify, double ifx) {
    const int b = blockIdx.y;
    const float* S = src + (long)b * h * w;
    float* D = dst + (long)b * H * W;
    const int HW = H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const int dy = i / W, dx = i - dy * W;
        const int sy = min((int)floor((double)dy * ify), h - 1);
        const int sx = min((int)floor((double)dx * ifx), w - 1);
        D[i] = S[(long)sy * w + sx];
    }
}

inline unsigned grid_for(long total) { long g = (total + 255) / 256; if (g > 4096) g = 4096; if (g < 1) g = 1; return (unsigned)g; }

inline bool bad_shape(const void* src, const void* dst, int B, int h, int w, int H, int W) {
    return !src || !dst || B <= 0 || B > 65535 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || (long)h * w >= (1L << 30) || (long)H * W >= (1L << 30);
}

}  // namespace

extern "C" {

int mte_resize_linear_u8(const unsigned char* src, int B, int h, int w, unsigned char* dst, int H, int W, hipStream_t stream) {
    if (bad_shape(src, dst, B, h, w, H, W)) return MTE_ERR_ARG;
    const int area = (w == 2 * W && h == 2 * H) ? 1 : 0;
    hipLaunchKernelGGL(resize_linear_u8_kernel, dim3(grid_for((long)H * W), B), dim3(256), 0, stream, src, dst, h, w, H, W,
                       (double)h / (double)H, (double)w / (double)W, area);
    return mte_check_launch();
}

int mte_resize_nearest_f32(const float* src, int B, int h, int w, float* dst, int H, int W, hipStream_t stream) {
    if (bad_shape(src, dst, B, h, w, H, W)) return MTE_ERR_ARG;
    hipLaunchKernelGGL(resize_nearest_f32_kernel, dim3(grid_for((long)H * W), B), dim3(256), 0, stream, src, dst, h, w, H, W,
                       1.0 / ((double)H / (double)h), 1.0 / ((double)W / (double)w));
    return mte_check_launch();
}

}  // extern "C"
