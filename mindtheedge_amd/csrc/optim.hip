// The optimizer family beside mte_adam_step (heads_misc.hip): torch.optim.Adam with L2 weight decay, torch.optim.AdamW and torch.optim.SGD
// (momentum, dampening, Nesterov, weight decay) as ONE streaming launch over the flat fp32 master buffers (gfx950; reference
// models/model_wrapper.py:142-180 builds getattr(torch.optim, config.model.optimizer.name) with config.model.optimizer.depth's keys).
//
// HBM-bound: Adam / AdamW move 28 B per parameter (read p, g, m, v; write p, m, v), SGD with momentum 20 B (p, g, buf; p, buf), plain SGD
// 12 B (p, g; p).  The launch shape is adam_kernel's: 256 threads, one 16-byte vector of each buffer per thread and trip, a grid-stride
// loop under the 8192-workgroup cap, the n & 3 tail in workgroup 0.  The weight decay adds no memory traffic, so every variant should run
// at its bytes over the rate of the plain Adam launch.
//
// Every algorithm has two entry points: scalars from the host, and the per-step scalars read from DEVICE memory (`hyper`, three floats),
// so that nothing in the launch changes from step to step and a captured HIP graph of the training step stays valid.  Both forms run the
// same template on the same float32 scalars and give bit-equal results.  The arithmetic is fp32 with -ffp-contract=off, the operations in
// the order written below (tests/optim_ref.py states them in float64).
//
// Gradient-norm clipping and the non-finite step guard: mte_grad_norm_clip (one read-only launch over the gradient, fixed order) leaves
// ctl = {clip coefficient, skip flag, norm, skipped steps} in device memory, and the device-scalar steps' CTL form (mte_adamw_step_ctl_dev,
// mte_sgd_step_ctl_dev) multiplies gscale by ctl[0] or, with ctl[1] set, returns before its first load.  Without CTL the kernels are the
// instruction streams they were (profiles/grad_clip.txt).
//
// Gradient accumulation: mte_grad_accumulate adds (or copies) one flat buffer into another in the same launch shape -- the micro-batch
// sum of FusedFlatOptimizer(accumulate_grad_batches > 1).  It is a kernel of its own: nothing is added to the step kernels.
//
// Weight EMA: mte_ema_update / mte_ema_update_dev (ema = d * ema + omd * p, 12 B per element, after the step launch) and mte_flat_swap
// (weights <-> average, bit for bit) in the same launch shape -- FusedFlatOptimizer(ema_decay > 0).  Kernels of their own as well.
#include "common.hpp"
#include "handoff.hpp"
#include <cstdint>
#include <type_traits>

namespace {

constexpr int OPT_THREADS = 256;
inline int opt_grid(long n4) { long g = (n4 + OPT_THREADS - 1) / OPT_THREADS; return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }

enum { WD_NONE = 0, WD_L2 = 1, WD_DECOUPLED = 2 };
enum { MOM_NONE = 0, MOM_PLAIN = 1, MOM_NESTEROV = 2 };

// The CTL form of a step kernel takes its `ctl` pointer INSIDE the by-value scalars: the plain instances keep the kernel arguments (and the
// offsets of the hidden ones behind them) they had before the form existed, and with them their instruction streams.
template <class S> struct WithCtl : S { const float* ctl; };
template <class S, bool CTL> using StepScalars = std::conditional_t<CTL, WithCtl<S>, S>;
template <bool CTL, class S>
inline StepScalars<S, CTL> step_scalars(const S& s, const float* ctl) {
    StepScalars<S, CTL> o;
    static_cast<S&>(o) = s;
    if constexpr (CTL) o.ctl = ctl;
    return o;
}

// ---- Adam ------------------------------------------------------------------------------------------------------------------------
// WD_NONE:      adam_kernel's update, operation for operation
// WD_L2:        g' = g * gscale + wd * p                                   (torch.optim.Adam(weight_decay=wd))
// WD_DECOUPLED: p - ((lr * wd) * p + step) = p * (1 - lr * wd) - step      (torch.optim.AdamW; p meets ONE rounding instead of two, and the
//               decay is held relative to lr * wd * p, not to p)
struct AdamScalars { float lr, bc1, bc2s, b1, b2, eps, gscale, wd; };

template <int WD>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s, float lrwd) {
    float gk = g * s.gscale;
    if (WD == WD_L2) gk = gk + s.wd * p;
    m = s.b1 * m + (1.f - s.b1) * gk;
    v = s.b2 * v + (1.f - s.b2) * gk * gk;
    const float denom = sqrtf(v) / s.bc2s + s.eps;
    if (WD == WD_DECOUPLED) p -= lrwd * p + (s.lr / s.bc1) * (m / denom);
    else p -= (s.lr / s.bc1) * (m / denom);
}

template <int WD, bool DEV, bool CTL>
__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, long n, const float* __restrict__ hyper,
                                                            StepScalars<AdamScalars, CTL> s) {
    if constexpr (CTL) {                                   // ctl = {clip coefficient, skip flag, ...} left by grad_norm_kernel (below)
        if (s.ctl[1] != 0.f) return;                       // a non-finite gradient: p, m, v keep their bits
        s.gscale = s.gscale * s.ctl[0];
    }
    if (DEV) { s.lr = hyper[0]; s.bc1 = hyper[1]; s.bc2s = hyper[2]; }
    const float lrwd = s.lr * s.wd;                        // from the step's own learning rate: a scheduler's change reaches the decay
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], mm = ((f32x4_t*)m)[i], vv = ((f32x4_t*)v)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pp[k], mk = mm[k], vk = vv[k];
            adam_elem<WD>(pk, gg[k], mk, vk, s, lrwd);
            pp[k] = pk; mm[k] = mk; vv[k] = vk;
        }
        ((f32x4_t*)p)[i] = pp; ((f32x4_t*)m)[i] = mm; ((f32x4_t*)v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        float pk = p[i], mk = m[i], vk = v[i];
        adam_elem<WD>(pk, g[i], mk, vk, s, lrwd);
        p[i] = pk; m[i] = mk; v[i] = vk;
    }
}

template <bool DEV, bool CTL = false>
int adamw_launch(float* p, const float* g, float* m, float* v, long n, const float* hyper, const AdamScalars& s, int decoupled, const float* ctl,
                 hipStream_t stream) {
    const dim3 grid(opt_grid(n >> 2)), block(OPT_THREADS);
    const auto sc = step_scalars<CTL>(s, ctl);
    if (s.wd == 0.f) hipLaunchKernelGGL((adamw_kernel<WD_NONE, DEV, CTL>), grid, block, 0, stream, p, g, m, v, n, hyper, sc);
    else if (decoupled) hipLaunchKernelGGL((adamw_kernel<WD_DECOUPLED, DEV, CTL>), grid, block, 0, stream, p, g, m, v, n, hyper, sc);
    else hipLaunchKernelGGL((adamw_kernel<WD_L2, DEV, CTL>), grid, block, 0, stream, p, g, m, v, n, hyper, sc);
    return mte_check_launch();
}

// ---- SGD -------------------------------------------------------------------------------------------------------------------------
// g' = g * gscale (+ wd * p);  buf = mu_eff * buf + omd_eff * g';  g'' = buf, or g' + mu * buf under Nesterov;  p -= lr * g''.
// {mu_eff, omd_eff} = {0, 1} at step 1 and {momentum, 1 - dampening} afterwards: torch's "buf = g' on the first step" from a
// zero-initialised (finite) buffer, without a launch that differs between the first step and the rest.  Nesterov's look-ahead takes
// the real momentum, a launch constant.  MOM_NONE neither reads nor writes buf.
struct SgdScalars { float lr, mu_eff, omd_eff, mu, gscale, wd; };

template <int MOM, bool WD>
__device__ __forceinline__ void sgd_elem(float& p, float g, float& buf, const SgdScalars& s) {
    float gk = g * s.gscale;
    if (WD) gk = gk + s.wd * p;
    if (MOM != MOM_NONE) {
        buf = s.mu_eff * buf + s.omd_eff * gk;
        gk = MOM == MOM_NESTEROV ? gk + s.mu * buf : buf;
    }
    p -= s.lr * gk;
}

template <int MOM, bool WD, bool DEV, bool CTL>
__global__ __launch_bounds__(OPT_THREADS) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                          const float* __restrict__ hyper, StepScalars<SgdScalars, CTL> s) {
    if constexpr (CTL) {                                   // as adamw_kernel
        if (s.ctl[1] != 0.f) return;
        s.gscale = s.gscale * s.ctl[0];
    }
    if (DEV) { s.lr = hyper[0]; s.mu_eff = hyper[1]; s.omd_eff = hyper[2]; }
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], bb = {0.f, 0.f, 0.f, 0.f};
        if (MOM != MOM_NONE) bb = ((f32x4_t*)buf)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pp[k], bk = bb[k];
            sgd_elem<MOM, WD>(pk, gg[k], bk, s);
            pp[k] = pk; bb[k] = bk;
        }
        ((f32x4_t*)p)[i] = pp;
        if (MOM != MOM_NONE) ((f32x4_t*)buf)[i] = bb;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        float pk = p[i], bk = MOM != MOM_NONE ? buf[i] : 0.f;
        sgd_elem<MOM, WD>(pk, g[i], bk, s);
        p[i] = pk;
        if (MOM != MOM_NONE) buf[i] = bk;
    }
}

template <int MOM, bool DEV, bool CTL>
void sgd_launch_wd(float* p, const float* g, float* buf, long n, const float* hyper, const SgdScalars& s, const float* ctl, hipStream_t stream) {
    const dim3 grid(opt_grid(n >> 2)), block(OPT_THREADS);
    const auto sc = step_scalars<CTL>(s, ctl);
    if (s.wd != 0.f) hipLaunchKernelGGL((sgd_kernel<MOM, true, DEV, CTL>), grid, block, 0, stream, p, g, buf, n, hyper, sc);
    else hipLaunchKernelGGL((sgd_kernel<MOM, false, DEV, CTL>), grid, block, 0, stream, p, g, buf, n, hyper, sc);
}

template <bool DEV, bool CTL = false>
int sgd_launch(float* p, const float* g, float* buf, long n, const float* hyper, const SgdScalars& s, int nesterov, const float* ctl,
               hipStream_t stream) {
    if (s.mu == 0.f) sgd_launch_wd<MOM_NONE, DEV, CTL>(p, g, buf, n, hyper, s, ctl, stream);
    else if (nesterov) sgd_launch_wd<MOM_NESTEROV, DEV, CTL>(p, g, buf, n, hyper, s, ctl, stream);
    else sgd_launch_wd<MOM_PLAIN, DEV, CTL>(p, g, buf, n, hyper, s, ctl, stream);
    return mte_check_launch();
}

// ---- global gradient norm, clip coefficient and non-finite guard -----------------------------------------------------------------------
// One read-only pass over the flat gradient (4 B per parameter against the step's 28) that leaves, in device memory, what the step kernels'
// CTL form reads: ctl = {clip coefficient, skip flag, norm, skipped-step count}.  Every thread adds (double)g * (double)g in fp64 -- the
// square of an fp32 value is exact there, only the additions round -- over the vectors i = thread, thread + grid * 256, ... in that
// order (NORM_UNROLL loads are issued ahead of their additions; the order of the additions is the one-vector-per-trip order), workgroup 0
// the n & 3 tail.  A workgroup folds its 256 partials in a fixed tree and leaves ONE fp64 record; the workgroup that draws the last ticket
// (handoff.hpp) adds the records in index order.  The grid is a function of n alone, so the sum has one order: bit-equal run to run and
// under HIP-graph replay; the ticket goes back to zero.  work = {S (fp64), ticket, pad, records[grid]}, zeroed once by the caller.
constexpr int NORM_CAP = 256;                              // workgroups: one of 256 threads per CU.  Measured at 77.0 M elements (profiles/grad_clip.txt):
constexpr int NORM_UNROLL = 8;                             // 0.051 ms; 512 x 4: 0.054, 1024 x 4: 0.063, 2048 x 4: 0.073 -- the last arriver's sum grows with the cap
constexpr long NORM_HEAD_BYTES = 16;
inline int norm_grid(long n4) { long g = (n4 + OPT_THREADS - 1) / OPT_THREADS; return (int)(g > NORM_CAP ? NORM_CAP : (g < 1 ? 1 : g)); }

struct NormArgs {
    const float* g; long n;
    float gscale, max_norm; int skip_nonfinite, fences;
    double* sum; unsigned* ticket; double* records; float* ctl;
};

__device__ __forceinline__ void norm_add(double& acc, const f32x4_t& x) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc += (double)x[k] * (double)x[k];
}

__global__ __launch_bounds__(OPT_THREADS) void grad_norm_kernel(NormArgs a) {
    __shared__ double sd[NORM_CAP];                        // the workgroup's 256 partials, then the last arriver's copy of the records
    __shared__ int s_last;
    static_assert(NORM_CAP >= OPT_THREADS, "sd holds a workgroup's partials");
    const int tid = threadIdx.x;
    const long n4 = a.n >> 2, stride = (long)gridDim.x * OPT_THREADS;
    const f32x4_t* g4 = (const f32x4_t*)a.g;
    double acc = 0.0;
    long i = blockIdx.x * (long)OPT_THREADS + tid;
    for (; i + (NORM_UNROLL - 1) * stride < n4; i += NORM_UNROLL * stride) {
        f32x4_t x[NORM_UNROLL];
#pragma unroll
        for (int u = 0; u < NORM_UNROLL; ++u) x[u] = g4[i + u * stride];
#pragma unroll
        for (int u = 0; u < NORM_UNROLL; ++u) norm_add(acc, x[u]);
    }
    for (; i < n4; i += stride) norm_add(acc, g4[i]);
    if (blockIdx.x == 0 && tid < (a.n & 3)) {
        const float x = a.g[(n4 << 2) + tid];
        acc += (double)x * (double)x;
    }
    sd[tid] = acc;
    __syncthreads();
    for (int st = OPT_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) sd[tid] += sd[tid + st];
        __syncthreads();
    }
    if (tid == 0) handoff::publish(a.records + blockIdx.x, sd[0]);
    if (!handoff::arrive<true>([&] { return a.ticket; }, [] { return gridDim.x; }, a.fences, a.fences, &s_last)) return;

    // last workgroup: the records into LDS, then one thread adds them in index order (<= NORM_CAP fp64 additions)
    for (int j = tid; j < (int)gridDim.x; j += OPT_THREADS) sd[j] = handoff::read(a.records + j);
    __syncthreads();
    if (tid != 0) return;
    double S = 0.0;
    for (int j = 0; j < (int)gridDim.x; ++j) S += sd[j];
    const double norm = fabs((double)a.gscale) * sqrt(S);
    double c = (double)a.max_norm / (norm + 1e-6);         // torch's clamp(max_norm / (total_norm + 1e-6), max=1): a NaN stays a NaN
    if (c > 1.0) c = 1.0;
    // S is non-finite exactly when some element is: fp64 cannot overflow on 2^38 squared fp32 values
    const bool skip = a.skip_nonfinite && !(fabs(S) <= 1.7976931348623157e308);
    *a.sum = S;
    a.ctl[0] = (float)c;
    a.ctl[1] = skip ? 1.f : 0.f;
    a.ctl[2] = (float)norm;
    if (skip) a.ctl[3] = a.ctl[3] + 1.f;
}

// ---- gradient accumulation over micro-batches --------------------------------------------------------------------------------------------
// dst[i] = dst[i] + src[i] (one fp32 rounding), or with ASSIGN dst[i] = src[i] (a bit copy: dst is not read), in the step kernels' launch
// shape.  12 B per element without ASSIGN (read, read, write): the plain SGD launch's count and read:write mix.  No atomics, no state.
template <bool ASSIGN>
__global__ __launch_bounds__(OPT_THREADS) void grad_accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, long n) {
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4_t s = ((const f32x4_t*)src)[i];
        if (!ASSIGN) {
            const f32x4_t d = ((const f32x4_t*)dst)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = d[k] + s[k];
        }
        ((f32x4_t*)dst)[i] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        dst[i] = ASSIGN ? src[i] : dst[i] + src[i];
    }
}

// ---- exponential moving average of the weights -------------------------------------------------------------------------------------------
// e[i] = d * e[i] + omd * p[i]: two fp32 multiplications and one fp32 addition, each rounded once, in that order (-ffp-contract=off), in
// grad_accumulate_kernel's launch shape and with its 12 B per element (read e, read p, write e).  p is read-only.  DEV: {d, omd} come from
// `scal` in device memory, and a non-null `ctl` (mte_grad_norm_clip's word) with ctl[1] set ends the kernel before its first load of e or
// p -- the average keeps its bits over a skipped step, as p, m and v do.  ctl[0], the clip coefficient, is not the average's business.
template <bool DEV>
__global__ __launch_bounds__(OPT_THREADS) void ema_update_kernel(float* __restrict__ e, const float* __restrict__ p, long n, float d, float omd,
                                                                 const float* __restrict__ scal, const float* __restrict__ ctl) {
    if (DEV) {
        if (ctl != nullptr && ctl[1] != 0.f) return;
        d = scal[0]; omd = scal[1];
    }
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4_t ee = ((const f32x4_t*)e)[i];
        const f32x4_t pp = ((const f32x4_t*)p)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) ee[k] = d * ee[k] + omd * pp[k];
        ((f32x4_t*)e)[i] = ee;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        e[i] = d * e[i] + omd * p[i];
    }
}

// ---- exchange of two flat buffers -------------------------------------------------------------------------------------------------------
// a[i] <-> b[i] as 32-bit words (16 B per element: read both, write both): no arithmetic touches the values, so NaN payloads survive.
__global__ __launch_bounds__(OPT_THREADS) void flat_swap_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, long n) {
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const u32x4_t x = ((const u32x4_t*)a)[i], y = ((const u32x4_t*)b)[i];
        ((u32x4_t*)a)[i] = y;
        ((u32x4_t*)b)[i] = x;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        const uint32_t x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

// mte_grad_accumulate's argument rules for two flat ranges of n floats: -> MTE_ERR_ARG, 0 with nothing to launch (n = 0), or 1
inline int flat_pair_check(const void* a, const void* b, long n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    if (!a || !b || n < 0 || ((x | y) & 15) || x == y) return MTE_ERR_ARG;
    if (n == 0) return 0;
    const uintptr_t bytes = (uintptr_t)n * sizeof(float);
    if (x < y + bytes && y < x + bytes) return MTE_ERR_ARG;
    return 1;
}

}  // namespace

extern "C" {

// Exponential moving average over flat fp32 buffers (16-byte aligned, disjoint): ema[i] = d * ema[i] + omd * p[i], three fp32 roundings in
// that order; p is only read.  n = 0 launches nothing.  n < 0, a null or misaligned pointer and overlapping ranges (equal pointers
// included) are MTE_ERR_ARG.
int mte_ema_update(float* ema, const float* p, long n, float d, float omd, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    const int ok = flat_pair_check(ema, p, n);
    if (ok <= 0) return ok;
    hipLaunchKernelGGL(ema_update_kernel<false>, dim3(opt_grid(n >> 2)), dim3(OPT_THREADS), 0, stream, ema, p, n, d, omd, (const float*)nullptr,
                       (const float*)nullptr);
    return mte_check_launch();
}

// The same update with scal = {d, omd} in DEVICE memory (the launch is identical every step: it replays from a captured graph).  ctl may be
// null; otherwise it is mte_grad_norm_clip's word, and with ctl[1] != 0 nothing is loaded or stored.  A null scal is MTE_ERR_ARG.
int mte_ema_update_dev(float* ema, const float* p, long n, const float* scal, const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!scal) return MTE_ERR_ARG;
    const int ok = flat_pair_check(ema, p, n);
    if (ok <= 0) return ok;
    hipLaunchKernelGGL(ema_update_kernel<true>, dim3(opt_grid(n >> 2)), dim3(OPT_THREADS), 0, stream, ema, p, n, 0.f, 0.f, scal, ctl);
    return mte_check_launch();
}

// Exchange two flat fp32 buffers (16-byte aligned, disjoint) bit for bit in one launch; the argument rules of mte_ema_update.
int mte_flat_swap(float* a, float* b, long n, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    const int ok = flat_pair_check(a, b, n);
    if (ok <= 0) return ok;
    hipLaunchKernelGGL(flat_swap_kernel, dim3(opt_grid(n >> 2)), dim3(OPT_THREADS), 0, stream, (uint32_t*)a, (uint32_t*)b, n);
    return mte_check_launch();
}

// Gradient accumulation over flat fp32 buffers (16-byte aligned, disjoint): assign = 0 adds src into dst, dst[i] = dst[i] + src[i] with one
// fp32 rounding; assign = 1 copies src's bits.  n = 0 launches nothing.  n < 0, a null or misaligned pointer and overlapping ranges
// (equal pointers included) are MTE_ERR_ARG.
int mte_grad_accumulate(float* dst, const float* src, long n, int assign, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    const uintptr_t d = (uintptr_t)dst, s = (uintptr_t)src;
    if (!dst || !src || n < 0 || ((d | s) & 15) || d == s) return MTE_ERR_ARG;
    if (n == 0) return 0;
    const uintptr_t bytes = (uintptr_t)n * sizeof(float);
    if (d < s + bytes && s < d + bytes) return MTE_ERR_ARG;
    const dim3 grid(opt_grid(n >> 2)), block(OPT_THREADS);
    if (assign) hipLaunchKernelGGL(grad_accumulate_kernel<true>, grid, block, 0, stream, dst, src, n);
    else hipLaunchKernelGGL(grad_accumulate_kernel<false>, grid, block, 0, stream, dst, src, n);
    return mte_check_launch();
}

// Bytes of `work` for mte_grad_norm_clip over n elements (16-byte aligned, zeroed ONCE by the caller): {S, ticket, pad, one record per workgroup}.
long mte_grad_norm_work_bytes(long n) { return n <= 0 ? 0 : NORM_HEAD_BYTES + 8L * norm_grid(n >> 2); }

// Global L2 norm of the flat gradient g[0..n) (16-byte aligned) in one launch and a fixed order, and what a clipped / guarded step needs:
//   S = sum g^2 in fp64 (also in the first 8 bytes of `work`), norm = |gscale| * sqrt(S)
//   ctl[0] = min(max_norm / (norm + 1e-6), 1) as torch.nn.utils.clip_grad_norm_ forms it (max_norm = +inf gives exactly 1; NaN stays NaN)
//   ctl[1] = 1 if skip_nonfinite and S is not finite, else 0;   ctl[2] = norm;   ctl[3] += 1 when ctl[1] is set (never reset here)
// The launch is identical every step and leaves the ticket at zero: it replays from a captured graph.
int mte_grad_norm_clip(const float* g, long n, float gscale, float max_norm, int skip_nonfinite, void* work, float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!g || !work || !ctl || n <= 0 || !(max_norm > 0.f)) return MTE_ERR_ARG;
    NormArgs a;
    a.g = g; a.n = n; a.gscale = gscale; a.max_norm = max_norm; a.skip_nonfinite = skip_nonfinite != 0; a.fences = g_mte_handoff_fences;
    a.sum = (double*)work; a.ticket = (unsigned*)((char*)work + 8); a.records = (double*)((char*)work + NORM_HEAD_BYTES); a.ctl = ctl;
    hipLaunchKernelGGL(grad_norm_kernel, dim3(norm_grid(n >> 2)), dim3(OPT_THREADS), 0, stream, a);
    return mte_check_launch();
}

// In-place Adam with weight decay over flat fp32 buffers (16-byte aligned).  decoupled = 0: torch.optim.Adam(weight_decay) (L2, added to
// the gradient), decoupled = 1: torch.optim.AdamW.  weight_decay = 0 is mte_adam_step's update bit for bit.  step >= 1; gscale multiplies
// the gradient first.
int mte_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int decoupled, int step, float gscale, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !m || !v || n <= 0 || step < 1 || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const AdamScalars s = {lr, (float)bc1, (float)sqrt(bc2), beta1, beta2, eps, gscale, weight_decay};
    return adamw_launch<false>(p, g, m, v, n, nullptr, s, decoupled, nullptr, stream);
}

// The same step with hyper = {lr, 1 - beta1^t, sqrt(1 - beta2^t)} in DEVICE memory, as mte_adam_step_dev: lr * weight_decay is formed in
// the kernel from hyper[0].
int mte_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                       float weight_decay, int decoupled, float gscale, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !m || !v || !hyper || n <= 0 || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    const AdamScalars s = {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay};
    return adamw_launch<true>(p, g, m, v, n, hyper, s, decoupled, nullptr, stream);
}

// In-place torch.optim.SGD over flat fp32 buffers (16-byte aligned).  momentum = 0: `buf` is neither read nor written and may be null.
// With momentum, `buf` is zero-initialised by the caller before step 1.  Nesterov needs momentum > 0 and dampening = 0, as torch.
int mte_sgd_step(float* p, const float* g, float* buf, long n, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                 int step, float gscale, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || n <= 0 || step < 1 || !(momentum >= 0.f) || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    if ((momentum > 0.f && !buf) || (nesterov && (momentum <= 0.f || dampening != 0.f))) return MTE_ERR_ARG;
    const SgdScalars s = {lr, step == 1 ? 0.f : momentum, step == 1 ? 1.f : (float)(1.0 - (double)dampening), momentum, gscale, weight_decay};
    return sgd_launch<false>(p, g, buf, n, nullptr, s, nesterov, nullptr, stream);
}

// The same step with hyper = {lr, mu_eff, (1 - dampening)_eff} in DEVICE memory: {lr, 0, 1} at step 1, {lr, momentum, 1 - dampening}
// afterwards.  `momentum` is the launch constant that selects the kernel and feeds Nesterov's look-ahead.
int mte_sgd_step_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                     float gscale, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !hyper || n <= 0 || !(momentum >= 0.f) || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    if ((momentum > 0.f && !buf) || (nesterov && momentum <= 0.f)) return MTE_ERR_ARG;
    const SgdScalars s = {0.f, 0.f, 0.f, momentum, gscale, weight_decay};
    return sgd_launch<true>(p, g, buf, n, hyper, s, nesterov, nullptr, stream);
}

// mte_adamw_step_dev / mte_sgd_step_dev with ctl = {clip coefficient, skip flag, ...} in DEVICE memory (mte_grad_norm_clip writes it):
// the gradient scale is float32(gscale * ctl[0]); with ctl[1] != 0 nothing is loaded or stored.  weight_decay = 0 is the Adam step.
int mte_adamw_step_ctl_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                           float weight_decay, int decoupled, float gscale, const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !m || !v || !hyper || !ctl || n <= 0 || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    const AdamScalars s = {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay};
    return adamw_launch<true, true>(p, g, m, v, n, hyper, s, decoupled, ctl, stream);
}

int mte_sgd_step_ctl_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                         float gscale, const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !hyper || !ctl || n <= 0 || !(momentum >= 0.f) || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    if ((momentum > 0.f && !buf) || (nesterov && momentum <= 0.f)) return MTE_ERR_ARG;
    const SgdScalars s = {0.f, 0.f, 0.f, momentum, gscale, weight_decay};
    return sgd_launch<true, true>(p, g, buf, n, hyper, s, nesterov, ctl, stream);
}

}  // extern "C"
