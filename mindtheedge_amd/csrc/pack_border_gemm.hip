// The forward ring GEMMs of a folded pack layer as ONE grouped split-K launch -- gfx950, bf16 (launch plan: pack_border_plan.hpp, plan_pack_border_gemm).
//
// pack_border.hip's ring terms are a zero-padded 1 x k convolution along the ring rows and a k x 1 convolution along the ring columns.  Through
// mte_conv2d_igemm's fp32-output form they were two launches of 12-81 workgroups with 80-192 K-steps each, one memory round trip per K-step, back to back on
// the main queue, and half of their columns (far != far') were never read.  Here the four (family, far) sub-problems share one grid, each K range is cut
// into slices so that the chip is full, and every slice leaves its partial tile in an fp32 slab; mte_pack_border_apply_slabs adds the slabs in slice order
// where it consumes the terms.  Every sum has a fixed order: the result is bit-reproducible.
//
// Tile 128 x 64, four waves as 2 x 2, each wave 64 x 32 outputs as 4 x 2 blocks of v_mfma_f32_16x16x32_bf16 (operands swapped as in conv_igemm.hip: a lane holds
// four consecutive output channels of one ring position, so a slab store is 16 bytes).  A K-step is 32 channels of one tap = 64 bytes of a row; LDS images have
// 64-byte rows with 16-byte chunk c of row r at slot c ^ ((r >> 1) & 3) (conv_igemm.hip's layout: conflict-free fragment reads), filled by LDS-DMA with the
// swizzle on the per-lane SOURCE chunk.  A ring of PBG_RING slots of PBG_STAGE K-steps, two stages (48 KiB) in flight per workgroup; 72 KiB of LDS, so two
// workgroups fit a CU.  Taps that leave the line, rows beyond M, columns beyond Ng and K-steps beyond the slice load zeros.
#include "common.hpp"
#include "pack_border_plan.hpp"

namespace {

struct PbGemmArgs {
    const bf16_t* x[2];        // ring lines of the two families: Rr [2B][W2+2][Cin], Rc [2B][H2][Cin]
    const bf16_t* w[2];        // forward weight packs [N][k][Cin] of Wr, Wc
    float* ws;                 // the slabs
    PbGemmPlan p;
};

__device__ u32x4_t g_pbg_zero16 = {0u, 0u, 0u, 0u};      // source of zero chunks for the LDS-DMA loader

__device__ __forceinline__ int pbg_swz(int row) { return (row >> 1) & 3; }
__device__ __forceinline__ int pbg_chunk_off(int row, int kc) { return row * 64 + ((kc ^ pbg_swz(row)) << 4); }

__global__ __launch_bounds__(256) void pack_border_gemm_kernel(PbGemmArgs a) {
    constexpr int BM = PBG_BM, BN = PBG_BN, NTHR = 256, ST = PBG_STAGE, RING = PBG_RING;
    constexpr int A_CH = BM * 4 / NTHR, B_CH = BN * 4 / NTHR;          // 16-byte chunks per thread and K-step
    static_assert(A_CH * NTHR == BM * 4 && B_CH * NTHR == BN * 4, "the tiles must split evenly over the threads");
    static_assert((NTHR / 4) % 8 == 0, "the rows a thread fills must share their swizzle");
    constexpr int IMG = (BM + BN) * 64;                                // LDS bytes of one K-step: A image, then B image
    extern __shared__ __attribute__((aligned(16))) char smem[];        // [RING slots][ST][IMG]
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;

    const PbGemmPlan& p = a.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    // ---- which sub-problem, slice and tile (all wave-uniform)
    int g, split, tile_m, tile_n;
    pb_gemm_block(p, (int)blockIdx.x, &g, &split, &tile_m, &tile_n);
    const int fam = g >> 1, far = g & 1;
    const int M = p.M[g], n = p.n[g], Cin = p.Cin, pad = p.pad;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    int s_begin, s_end;
    pb_gemm_slice(p.ksteps, p.per_split, split, &s_begin, &s_end);
    const bf16_t* __restrict__ xg = a.x[fam] + (long)far * M * Cin;
    const long Kp = (long)p.taps * Cin;
    const bf16_t* __restrict__ wg = a.w[fam] + (long)far * p.Ng * Kp;
    const int cps = Cin / PBG_KSTEP;                                   // K-steps per tap

    // ---- loader state: LDS slot (tid & 3) of every row this thread fills holds source chunk kc
    const int kc = (tid & 3) ^ pbg_swz(tid >> 2);
    int a_m[A_CH], a_pos[A_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        const int m = m0 + (tid >> 2) + i * (NTHR / 4);
        a_m[i] = m < M ? m : -1;
        a_pos[i] = m < M ? m % n : 0;
    }
    const int b_n = n0 + (tid >> 2);                                   // (B_CH == 1)
    static_assert(B_CH == 1, "one weight row per thread");
    int ks = s_begin, tap = s_begin / cps, cb = s_begin - tap * cps;   // the next K-step to stage: its tap and its 32-channel block inside the tap
    auto stage = [&](int buf) {
#pragma unroll
        for (int u = 0; u < ST; ++u) {
            char* img = smem + (buf * ST + u) * IMG;
            const bool live = ks < s_end;
            const int d = tap - pad, c0 = cb * PBG_KSTEP + kc * 8;
#pragma unroll
            for (int i = 0; i < A_CH; ++i) {
                const int j = a_pos[i] + d;
                const bool ok = live && a_m[i] >= 0 && j >= 0 && j < n;
                const void* src = ok ? (const void*)(xg + (long)(a_m[i] + d) * Cin + c0) : (const void*)&g_pbg_zero16;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(img + (wv * 16 + i * (NTHR / 4)) * 64), 16, 0, 0);
            }
            {
                const bool ok = live && b_n < p.Ng;
                const void* src = ok ? (const void*)(wg + (long)b_n * Kp + (long)ks * PBG_KSTEP + kc * 8) : (const void*)&g_pbg_zero16;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(img + BM * 64 + (wv * 16) * 64), 16, 0, 0);
            }
            ++ks;
            if (++cb == cps) { cb = 0; ++tap; }
        }
    };

    // ---- a wave's 64 x 32 sub-tile as 4 x 2 blocks of 16 x 16
    constexpr int AM = 4, AN = 2;
    const int wm = wave >> 1, wn = wave & 1;
    const int r16 = lane & 15, q16 = lane >> 4;
    f32x4_t acc[AM][AN];
#pragma unroll
    for (int i = 0; i < AM; ++i)
#pragma unroll
        for (int j = 0; j < AN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int buf) {
#pragma unroll
        for (int u = 0; u < ST; ++u) {
            const char* pA = smem + (buf * ST + u) * IMG;
            const char* pB = pA + BM * 64;
            u32x4_t fa[AM], fb[AN];
#pragma unroll
            for (int i = 0; i < AM; ++i) fa[i] = *(const u32x4_t*)(pA + pbg_chunk_off((wm * AM + i) * 16 + r16, q16));
#pragma unroll
            for (int j = 0; j < AN; ++j) fb[j] = *(const u32x4_t*)(pB + pbg_chunk_off((wn * AN + j) * 16 + r16, q16));
#pragma unroll
            for (int i = 0; i < AM; ++i)
#pragma unroll
                for (int j = 0; j < AN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fb[j]), __builtin_bit_cast(bf16x8_t, fa[i]), acc[i][j], 0, 0, 0);
        }
    };

    // ---- main loop: a ring of RING slots, RING - 1 stages in flight.  Per stage every wave waits for its own DMA of THAT stage (counted vmcnt: the younger
    // stage stays in flight across the barrier, which is why the barrier is the raw instruction -- __syncthreads() would drain it) and for its fragment reads of
    // the previous stage (lgkmcnt) BEFORE the barrier; behind the barrier the stage is complete for every reader, and the slot read one stage ago is free for
    // the DMA of stage st + RING - 1.  The first form of this loop had two slots and waited for each stage right after issuing the next: 31.2 / 23.8 / 19.3 us
    // for pack3 / pack2 / pack1 against 29.6 / 22.3 / 17.4 us with this ring (profiles/pack_border_gemm_ab.txt) -- the memory round trip was NOT most of a
    // stage's ~1.5 us.  With 270-318 workgroups on 256 CUs a SIMD holds one wave, so the stage's own chain is exposed: the loader's per-K-step address
    // arithmetic and the selects of the zero chunk, the fragment reads, 16 MFMAs.  A buffer-descriptor loader (out-of-range offsets read zeros, the K advance
    // is a scalar offset, as conv_igemm.hip's LD = 2) and eight waves per workgroup are the next steps.
    constexpr int AHEAD = RING - 1, LPS = ST * (A_CH + B_CH);             // DMA instructions per wave and stage
    static_assert(RING == 3, "the wait below is written for two stages in flight");
    const int nstages = (s_end - s_begin + ST - 1) / ST;
#pragma unroll
    for (int q = 0; q < AHEAD; ++q)
        if (q < nstages) stage(q);
    for (int st = 0; st < nstages; ++st) {
        if (st + 1 < nstages) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPS) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (st + AHEAD < nstages) stage((st + AHEAD) % RING);
        compute(st % RING);
    }

    // ---- partial tile -> slab `split`: lane (r16, q16) holds channels 4 q16 .. + 3 of ring position r16 of every block
#pragma unroll
    for (int i = 0; i < AM; ++i) {
        const int m = m0 + (wm * AM + i) * 16 + r16;
#pragma unroll
        for (int j = 0; j < AN; ++j) {
            const int c = n0 + (wn * AN + j) * 16 + 4 * q16;
            if (m < M && c < p.Ng) *(f32x4_t*)(a.ws + pb_gemm_ws_index(p, g, split, m, c)) = acc[i][j];      // (Ng % 8 == 0: a group of four is inside or outside)
        }
    }
}

int pbg_cus() {
    static const int cus = [] {
        int dev = 0, v = 0;
        return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0 ? v : 256;
    }();
    return cus;
}

}  // namespace

extern "C" {

// fp32 elements of the workspace of mte_pack_border_gemm_fwd, *splits = the slices it writes (what mte_pack_border_apply_slabs is told); MTE_ERR_UNSUPPORTED (< 0)
// for a shape or type the grouped launch does not take (the caller then runs the two mte_conv2d_igemm launches).  force_splits: 0, or (tests) that many slices
long mte_pack_border_gemm_ws_elems(int B, int H2, int W2, int C16, int Co, int k, int dtype, int force_splits, int* splits) {
    const PbGemmPlan p = plan_pack_border_gemm(B, H2, W2, C16, Co, k, dtype == MTE_DT_BF16, pbg_cus(), force_splits);
    if (p.rc != MTE_OK) return p.rc;
    if (splits) *splits = p.splits[0];
    return p.ws_elems;
}

// ws <- the ring terms of a folded pack layer's forward pass as slabs of partial sums: R_rows [2B][W2+2][C16], R_cols [2B][H2][C16] (the output of
// mte_pack_ring_fwd), Wr_pack / Wc_pack the forward packs [2 pad Co][k][C16] of the ring weights.  One launch; only the columns with far == far' are written.
int mte_pack_border_gemm_fwd(const void* R_rows, const void* R_cols, const void* Wr_pack, const void* Wc_pack, float* ws, long ws_elems, int B, int H2, int W2,
                             int C16, int Co, int k, int dtype, int force_splits, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!R_rows || !R_cols || !Wr_pack || !Wc_pack || !ws) return MTE_ERR_ARG;
    PbGemmArgs a;
    a.p = plan_pack_border_gemm(B, H2, W2, C16, Co, k, dtype == MTE_DT_BF16, pbg_cus(), force_splits);
    if (a.p.rc != MTE_OK) return a.p.rc;
    if (ws_elems < a.p.ws_elems) return MTE_ERR_ARG;
    a.x[0] = (const bf16_t*)R_rows; a.x[1] = (const bf16_t*)R_cols;
    a.w[0] = (const bf16_t*)Wr_pack; a.w[1] = (const bf16_t*)Wc_pack;
    a.ws = ws;
    if (mte_allow_lds<pack_border_gemm_kernel>(a.p.lds_bytes) != MTE_OK) return MTE_ERR_LAUNCH;       // (72 KiB: beyond what a kernel may use unasked)
    hipLaunchKernelGGL(pack_border_gemm_kernel, dim3(a.p.grid), dim3(a.p.threads), a.p.lds_bytes, stream, a);
    return mte_check_launch();
}

}  // extern "C"
