// Tile geometry and per-pixel helpers shared by the edge-loss kernels (edge_loss.hip: the generic four-scale kernels; edge_fast.hpp: the training
// configuration's, for one or two predictions per label set; edge_loss_kinds.hip: the other loss kinds, one scale per launch).  A workgroup of 256 threads is one 64 x 32-pixel tile of one sample; a thread owns 4 consecutive
// pixels of rows r0 and r0 + 16, so every global access is a 16-byte load / store; the prediction tile + halo is staged in LDS as DEPTH.
#pragma once
#include "common.hpp"

constexpr int TW = 64, TH = 32;         // output tile (256 threads x 2 passes x 4 pixels)
constexpr int LS = 72;                  // LDS row stride in floats: image column j of the tile sits at index 4 + j (16-byte aligned interior)
constexpr int REC = 16;                 // doubles per workgroup record (one 128-byte line)

// 1 / x as v_rcp_f32 (1 ulp) + one Newton step: r' = r + r (1 - x r), the two fmas of the IEEE division sequence without its scaling and
// fix-up instructions (3 instructions instead of ~10).  x is in [1e-6, ~1e3] here -- no denormals, overflow or division by zero to fix up -- and
// the result is within 1 ulp of the correctly rounded quotient (almost always equal to it).
__device__ __forceinline__ float rcp_newton(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(r, __builtin_fmaf(-x, r, 1.f), r);
}
#if defined(MTE_EDGE_ABLATE) && (MTE_EDGE_ABLATE & 4)
__device__ __forceinline__ float to_depth(int from_inv, float v) { return from_inv ? 1.f / fmaxf(v, 1e-6f) : v; }   // diagnostic: the IEEE division of rounds 1-3
#else
__device__ __forceinline__ float to_depth(int from_inv, float v) { return from_inv ? rcp_newton(fmaxf(v, 1e-6f)) : v; }
#endif

// 4 consecutive floats of row `row` starting at column x (x % 4 == 0); zero beyond the image
__device__ __forceinline__ f32x4_t load4(const float* base, long row, int x, int W, int vec) {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (vec) { if (x < W) v = *(const f32x4_t*)(base + row * W + x); }
    else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (x + k < W) v[k] = base[row * W + x + k];
    }
    return v;
}
__device__ __forceinline__ void store4(float* base, long row, int x, int W, int vec, const f32x4_t& v) {
    if (vec) { if (x < W) *(f32x4_t*)(base + row * W + x) = v; }
    else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (x + k < W) base[row * W + x + k] = v[k];
    }
}

// Depth tile: rows y0-R .. y0+TH+R-1, columns x0-R .. x0+TW+R-1 of sample b of a [B,H,W] map, staged as DEPTH into sd (row stride LS,
// column j at 4 + j).  Two steps so that the loads are in flight together with the workgroup's other loads: issue -> registers, commit
// -> reciprocal (from_inv: the map is inverse depth) + LDS store.  vec: 16-byte accesses are legal (W % 4 == 0, aligned base).
// Map: the caller's description of the map, any struct with members pred, H and W (EdgeScale, KindArgs); vec and from_inv by reference.
//
// The plain signature would be issue(pred, H, W, vec, ...) / commit(H, W, from_inv, ...) with values.  This one departs from it for code
// generation only; the result is the same either way.  The kernels pass (members of) their kernel-argument struct, and through the
// references the argument reads stay where the values are used, as when this code stood in each kernel.  Copied into by-value parameters
// they are read at the call and stay live across the kernel, which costs the edge-loss kernels SGPRs, and with pred / H / W as three
// separate references edge_loss_fwd_kernel<false> still gets another instruction order (compile either form with
// -Rpass-analysis=kernel-resource-usage to see it).  A caller that passes locals is correct and loses just that.
template <int R> struct DepthTile {
    static constexpr int ROWS = TH + 2 * R;
    static constexpr int NI = (ROWS * (TW / 4) + 255) / 256;      // interior float4 groups per thread
    static_assert(ROWS * 2 * R <= 256, "one halo pixel per thread");
    f32x4_t v[NI];
    float hv;
    template <class Map> __device__ __forceinline__ void issue(const Map& sc, const int& vec, int b, int x0, int y0) {
        const float* img = sc.pred + (long)b * sc.H * sc.W;
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const int i = threadIdx.x + k * 256;
            const int ly = i >> 4, c4 = (i & 15) * 4;
            const int gy = y0 + ly - R;
            v[k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if (i < ROWS * (TW / 4) && (unsigned)gy < (unsigned)sc.H) v[k] = load4(img, gy, x0 + c4, sc.W, vec);
        }
        hv = 0.f;
        const int i = threadIdx.x;
        if (i < ROWS * 2 * R) {
            const int ly = i / (2 * R), k = i % (2 * R);
            const int j = k < R ? k - R : TW + (k - R);
            const int gy = y0 + ly - R, gx = x0 + j;
            if ((unsigned)gy < (unsigned)sc.H && (unsigned)gx < (unsigned)sc.W) hv = img[(long)gy * sc.W + gx];
        }
    }
    template <class Map> __device__ __forceinline__ void commit(const Map& sc, const int& from_inv, int x0, int y0, float* sd) const {
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i >= ROWS * (TW / 4)) break;
            const int ly = i >> 4, c4 = (i & 15) * 4;
            const bool rowok = (unsigned)(y0 + ly - R) < (unsigned)sc.H;
            f32x4_t d;
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = (rowok && x0 + c4 + e < sc.W) ? to_depth(from_inv, v[k][e]) : 0.f;
            *(f32x4_t*)(sd + ly * LS + 4 + c4) = d;
        }
        const int i = threadIdx.x;
        if (i < ROWS * 2 * R) {
            const int ly = i / (2 * R), k = i % (2 * R);
            const int j = k < R ? k - R : TW + (k - R);
            const int gy = y0 + ly - R, gx = x0 + j;
            sd[ly * LS + 4 + j] = ((unsigned)gy < (unsigned)sc.H && (unsigned)gx < (unsigned)sc.W) ? to_depth(from_inv, hv) : 0.f;
        }
    }
};

// the 3 x 6 window around 4 consecutive pixels: w[r][0..5] = columns c-1 .. c+4 of LDS rows (ly-1, ly, ly+1); c % 4 == 0
__device__ __forceinline__ void window(const float* sd, int ly, int c, float w[3][6]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float* row = sd + (ly - 1 + r) * LS + 4 + c;
        const f32x4_t m = *(const f32x4_t*)row;
        w[r][0] = row[-1]; w[r][1] = m[0]; w[r][2] = m[1]; w[r][3] = m[2]; w[r][4] = m[3]; w[r][5] = row[4];
    }
}
// Sobel responses of pixel k (0..3) of the window -- kernels of grad_loss.py:20-31
__device__ __forceinline__ void sobel4(const float w[3][6], int k, float& sh, float& sv, float& srl, float& slr) {
    const float n0 = w[0][k], n1 = w[0][k + 1], n2 = w[0][k + 2], n3 = w[1][k], n5 = w[1][k + 2], n6 = w[2][k], n7 = w[2][k + 1], n8 = w[2][k + 2];
    sh = (n2 - n0) + 2.f * (n5 - n3) + (n8 - n6);
    sv = (n6 - n0) + 2.f * (n7 - n1) + (n8 - n2);
    srl = (n1 - n3) + 2.f * (n2 - n6) + (n5 - n7);
    slr = (n5 - n1) + 2.f * (n8 - n0) + (n7 - n3);
}
// 1-ulp reciprocal (v_rcp_f32): enough wherever the result is not differenced against a neighbour (the depth tile takes the Newton step above)
__device__ __forceinline__ float rcpf(float x) { return __builtin_amdgcn_rcpf(x); }
// natural log / exp on the transcendental unit without the denormal-range scaling of __logf / __expf (5 extra instructions each): every
// argument here is >= 1e-4 (p + 0.001, 10 (inv + 1e-5), 10 / depth), and an exp that underflows may flush to zero (1 + t follows)
__device__ __forceinline__ float fast_log(float x) { return __builtin_amdgcn_logf(x) * 0.693147180559945309f; }
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
