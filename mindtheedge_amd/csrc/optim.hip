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
//
// Per-tensor learning-rate and weight-decay multipliers: the SEG form of the device-scalar steps (mte_adamw_step_seg_dev,
// mte_sgd_step_seg_dev) reads one class byte per aligned 64-element block of the flat buffers and {lr_mult, wd_mult} per class --
// FusedFlatOptimizer(tensor_scales=...).  Kernels of their own: adamw_kernel / sgd_kernel and their instances are what they were.
// Per-tensor gradient statistics: mte_tensor_stats, one read-only launch over the gradient (and the weights) with the tensor table in
// device memory, fp64 sums in an order fixed by that table.
// LAMB: mte_lamb_moments + mte_lamb_apply (24 + 16 B per parameter), the decoupled AdamW arithmetic with the per-tensor delta rescaled by
// ||p|| / ||update|| -- FusedLAMB.  The pair walks the statistics launch's tensor table and chunks; the step kernels above are untouched.
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

// The element update in its two halves -- the moments, then the delta that leaves p -- so that the LAMB launches (below), which need the
// delta before p moves, run these very operations: adam_elem is the two in a row, operation for operation what it always was.
template <int WD>
__device__ __forceinline__ void adam_moments(float p, float g, float& m, float& v, const AdamScalars& s) {
    float gk = g * s.gscale;
    if (WD == WD_L2) gk = gk + s.wd * p;
    m = s.b1 * m + (1.f - s.b1) * gk;
    v = s.b2 * v + (1.f - s.b2) * gk * gk;
}

template <int WD>
__device__ __forceinline__ float adam_delta(float p, float m, float v, const AdamScalars& s, float lrwd) {
    const float denom = sqrtf(v) / s.bc2s + s.eps;
    if (WD == WD_DECOUPLED) return lrwd * p + (s.lr / s.bc1) * (m / denom);
    return (s.lr / s.bc1) * (m / denom);
}

template <int WD>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s, float lrwd) {
    adam_moments<WD>(p, g, m, v, s);
    p -= adam_delta<WD>(p, m, v, s, lrwd);
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

// ---- the SEG form: per-tensor learning-rate and weight-decay multipliers --------------------------------------------------------------------
// FlatParameters aligns every tensor to 64 elements, so an aligned 64-element block of the flat buffers belongs to ONE tensor.  cls[b] is
// the class of elements 64 b .. 64 b + 63 (n / 64 bytes), scales = {lr_mult, wd_mult} per class (2 * n_classes floats); both are launch
// constants in device memory.  For class c: lr_c = lr * lr_mult_c and wd_c = wd * wd_mult_c, ONE fp32 multiplication each, lr the step's
// own hyper[0]; the element update is adam_elem / sgd_elem above with lr_c for lr and wd_c for wd (AdamW's lrwd = lr_c * wd_c).  A class
// whose wd_c is exactly 0 takes the no-decay instance of the element update (never `+ 0 * p`), as the plain launchers do for
// weight_decay = 0: a SEG launch equals, slice by slice and bit for bit, the plain launch on that slice with {lr_c, wd_c}.
// The table {lr_c, wd_c} is staged in LDS by the first n_classes threads (<= 16 entries: no by-value array, no scratch); a thread reads
// its vector's class byte (16 consecutive threads share it: a vector never straddles a block, and n % 64 == 0 leaves no tail) and then
// the pair, a broadcast or a few-way LDS read.  A byte >= n_classes is clamped to the last class.  ctl may be null (a uniform branch).
constexpr int SEG_MAX_CLASSES = 16;
struct SegArgs { const uint8_t* cls; const float* scales; const float* ctl; int n_classes; };

template <int WD>
__global__ __launch_bounds__(OPT_THREADS) void adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, long n, const float* __restrict__ hyper, AdamScalars s,
                                                                SegArgs t) {
    __shared__ float s_lr[SEG_MAX_CLASSES], s_wd[SEG_MAX_CLASSES];
    if (t.ctl != nullptr) {                                // as adamw_kernel's CTL form: the skip flag first, before any load
        if (t.ctl[1] != 0.f) return;
        s.gscale = s.gscale * t.ctl[0];
    }
    s.lr = hyper[0]; s.bc1 = hyper[1]; s.bc2s = hyper[2];
    if ((int)threadIdx.x < t.n_classes) {
        s_lr[threadIdx.x] = s.lr * t.scales[2 * threadIdx.x];
        s_wd[threadIdx.x] = s.wd * t.scales[2 * threadIdx.x + 1];
    }
    __syncthreads();
    const int last = t.n_classes - 1;
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        int c = t.cls[i >> 4];
        c = c > last ? last : c;
        AdamScalars sc = s;
        sc.lr = s_lr[c]; sc.wd = s_wd[c];
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], mm = ((f32x4_t*)m)[i], vv = ((f32x4_t*)v)[i];
        if (WD != WD_NONE && sc.wd != 0.f) {
            const float lrwd = sc.lr * sc.wd;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pp[k], mk = mm[k], vk = vv[k];
                adam_elem<WD>(pk, gg[k], mk, vk, sc, lrwd);
                pp[k] = pk; mm[k] = mk; vv[k] = vk;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pp[k], mk = mm[k], vk = vv[k];
                adam_elem<WD_NONE>(pk, gg[k], mk, vk, sc, 0.f);
                pp[k] = pk; mm[k] = mk; vv[k] = vk;
            }
        }
        ((f32x4_t*)p)[i] = pp; ((f32x4_t*)m)[i] = mm; ((f32x4_t*)v)[i] = vv;
    }
}

template <int MOM, bool WD>
__global__ __launch_bounds__(OPT_THREADS) void sgd_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                              const float* __restrict__ hyper, SgdScalars s, SegArgs t) {
    __shared__ float s_lr[SEG_MAX_CLASSES], s_wd[SEG_MAX_CLASSES];
    if (t.ctl != nullptr) {                                // as sgd_kernel's CTL form
        if (t.ctl[1] != 0.f) return;
        s.gscale = s.gscale * t.ctl[0];
    }
    s.lr = hyper[0]; s.mu_eff = hyper[1]; s.omd_eff = hyper[2];
    if ((int)threadIdx.x < t.n_classes) {
        s_lr[threadIdx.x] = s.lr * t.scales[2 * threadIdx.x];
        s_wd[threadIdx.x] = s.wd * t.scales[2 * threadIdx.x + 1];
    }
    __syncthreads();
    const int last = t.n_classes - 1;
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        int c = t.cls[i >> 4];
        c = c > last ? last : c;
        SgdScalars sc = s;
        sc.lr = s_lr[c]; sc.wd = s_wd[c];
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], bb = {0.f, 0.f, 0.f, 0.f};
        if (MOM != MOM_NONE) bb = ((f32x4_t*)buf)[i];
        if (WD && sc.wd != 0.f) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pp[k], bk = bb[k];
                sgd_elem<MOM, true>(pk, gg[k], bk, sc);
                pp[k] = pk; bb[k] = bk;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pp[k], bk = bb[k];
                sgd_elem<MOM, false>(pk, gg[k], bk, sc);
                pp[k] = pk; bb[k] = bk;
            }
        }
        ((f32x4_t*)p)[i] = pp;
        if (MOM != MOM_NONE) ((f32x4_t*)buf)[i] = bb;
    }
}

template <int MOM>
void sgd_seg_launch_wd(float* p, const float* g, float* buf, long n, const float* hyper, const SgdScalars& s, const SegArgs& t, hipStream_t stream) {
    const dim3 grid(opt_grid(n >> 2)), block(OPT_THREADS);
    if (s.wd != 0.f) hipLaunchKernelGGL((sgd_seg_kernel<MOM, true>), grid, block, 0, stream, p, g, buf, n, hyper, s, t);
    else hipLaunchKernelGGL((sgd_seg_kernel<MOM, false>), grid, block, 0, stream, p, g, buf, n, hyper, s, t);
}

// ---- per-tensor statistics of the flat gradient (and weights) ------------------------------------------------------------------------------
// One read-only launch.  Tensor t is elements [begin_t, begin_t + numel_t) of the flat buffers (begin_t a multiple of 64; the padding
// behind numel_t is never read).  out[4 t ..] = {S_g = sum g^2, amax_g = max |g| over the finite elements (0 without one), the count of
// non-finite elements of g, S_p = sum p^2 (0 without p)}, all fp64; the squares are exact there, only the additions round, and an inf
// or a NaN reaches S_g (inf^2 = inf).
// Order of the additions, a function of the tensor table alone -- not of the grid, not of arrival:
//   * a tensor is cut from its start into chunks of STAT_CHUNK elements (the last one ragged; an empty tensor has one empty chunk);
//     chunk k of tensor t has the global index first_t + k, first_t the running sum of the chunk counts (every workgroup forms that
//     table in LDS: T <= STAT_MAX_T);
//   * a chunk is read by ONE workgroup: thread j adds the vectors j, j + 256, ... of the chunk in that order (loads are issued ahead of
//     their additions), then thread j < (numel & 3) of the last chunk the tensor's j-th trailing element; the 256 partials fold in
//     a fixed tree (down each 64-lane wave by halving strides, then the four waves in index order) into ONE record of four fp64 values;
//   * a tensor of one chunk is finished there.  Otherwise the workgroup draws the TENSOR's ticket (handoff.hpp, as grad_norm_kernel),
//     and the one that draws the last of its chunk_count tickets adds the records: thread j the records j, j + 256, ... in that order,
//     then the same tree.  Workgroups take chunks c = workgroup, workgroup + grid, ...: every loop is bounded and nobody waits.
// Tickets go back to zero, so the launch replays from a captured graph and is bit-equal call to call.
// work = {tickets[T] (unsigned, padded to 16 B), records[n / STAT_CHUNK + T][4] fp64}, zeroed once by the caller.
constexpr long STAT_CHUNK = 32768;                          // elements: 128 KB of gradient per record (77.0 M elements: 2350 + 218 chunks)
constexpr int STAT_CAP = 1024;                              // workgroups
constexpr int STAT_MAX_T = 4096;
constexpr int STAT_UNROLL = 4;
inline long stat_max_chunks(long n, long T) { return n / STAT_CHUNK + T; }
inline long stat_ticket_bytes(long T) { return (4 * T + 15) / 16 * 16; }

struct StatArgs {
    const float* g; const float* p; long n;
    const long* begin; const long* numel; int T; int fences;
    long max_chunks;
    unsigned* tickets; double* records; double* out;
};

struct StatAcc { double sg, amax, nf, sp; };

__device__ __forceinline__ void stat_add_g(StatAcc& a, float x) {
    a.sg += (double)x * (double)x;
    const float ax = fabsf(x);
    if (ax <= 3.402823466e+38f) a.amax = fmax(a.amax, (double)ax);
    else a.nf += 1.0;                                      // inf or NaN (the comparison is false for a NaN)
}

// the workgroup's 256 partials -> thread 0's `a`, in a fixed tree; sh: 4 waves x 4 values.  Every thread calls it.
__device__ __forceinline__ void stat_fold(StatAcc& a, double (*sh)[4]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.sg += __shfl_down(a.sg, off, 64);
        a.amax = fmax(a.amax, __shfl_down(a.amax, off, 64));
        a.nf += __shfl_down(a.nf, off, 64);
        a.sp += __shfl_down(a.sp, off, 64);
    }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { sh[tid >> 6][0] = a.sg; sh[tid >> 6][1] = a.amax; sh[tid >> 6][2] = a.nf; sh[tid >> 6][3] = a.sp; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < OPT_THREADS / 64; ++w) {
            a.sg += sh[w][0]; a.amax = fmax(a.amax, sh[w][1]); a.nf += sh[w][2]; a.sp += sh[w][3];
        }
    }
    __syncthreads();                                       // sh may be written again
}

// The chunk walk of the per-tensor kernels (tensor_stats_kernel here, the LAMB pair below): ONE statement of how the tensor table is cut
// into chunks, so that every kernel that walks it gives a chunk the same elements and the same global index.
// A range that leaves [0, n) counts as empty: nothing outside the buffers is touched.
__device__ __forceinline__ bool chunk_range_ok(long b, long m, long n) { return b >= 0 && m > 0 && (b & 3) == 0 && b <= n && m <= n - b; }

// Every thread of the workgroup calls it.  s_first[t] <- the global index of tensor t's first chunk (the running sum of the chunk counts,
// an empty tensor counting one empty chunk), s_first[T] <- all chunks, which it returns.  s_first: STAT_MAX_T + 1 ints, s_part: 256 ints.
__device__ __forceinline__ long chunk_table(const long* begin, const long* numel, int T, long n, int* s_first, int* s_part) {
    const int tid = threadIdx.x;
    constexpr int PER = STAT_MAX_T / OPT_THREADS;          // consecutive tensors per thread in the scan
    int cnt[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int t = tid * PER + k;
        int c = 0;
        if (t < T) {
            const long b = begin[t], m = numel[t];
            c = chunk_range_ok(b, m, n) ? (int)((m + STAT_CHUNK - 1) / STAT_CHUNK) : 1;
        }
        cnt[k] = c;
        mine += c;
    }
    s_part[tid] = mine;
    __syncthreads();
    for (int st = 1; st < OPT_THREADS; st <<= 1) {         // inclusive scan of the 256 partials
        const int add = tid >= st ? s_part[tid - st] : 0;
        __syncthreads();
        s_part[tid] += add;
        __syncthreads();
    }
    int run = s_part[tid] - mine;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int t = tid * PER + k;
        if (t <= T) s_first[t] = run;
        run += cnt[k];
    }
    if (tid == OPT_THREADS - 1) s_first[STAT_MAX_T] = run; // T = STAT_MAX_T: no thread owns index T
    __syncthreads();
    return s_first[T];
}

// Chunk c of the table: tensor t (the last one with s_first[t] <= c) of `chunks` chunks, at elements [b + e0, b + e1) of the flat buffers
// -- nvec whole vectors, and in the tensor's last chunk (e1 == m) its m & 3 trailing elements.  An empty chunk has b = m = e0 = e1 = 0.
struct Chunk { int t, chunks; long b, m, e0, e1, nvec; };

__device__ __forceinline__ Chunk chunk_at(long c, const int* s_first, const long* begin, const long* numel, int T, long n) {
    int lo = 0, hi = T - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_first[mid] <= c) lo = mid; else hi = mid - 1;
    }
    Chunk ch;
    ch.t = lo;
    ch.chunks = s_first[lo + 1] - s_first[lo];
    const long k = c - s_first[lo];
    ch.b = begin[lo]; ch.m = numel[lo];
    if (!chunk_range_ok(ch.b, ch.m, n) || k < 0 || k * STAT_CHUNK > ch.m) { ch.b = 0; ch.m = 0; }
    ch.e0 = ch.m ? k * STAT_CHUNK : 0;
    ch.e1 = ch.e0 + STAT_CHUNK < ch.m ? ch.e0 + STAT_CHUNK : ch.m;
    ch.nvec = ch.e1 > ch.e0 ? (ch.e1 - ch.e0) >> 2 : 0;
    return ch;
}

template <bool WITH_P>
__global__ __launch_bounds__(OPT_THREADS) void tensor_stats_kernel(StatArgs a) {
    __shared__ int s_first[STAT_MAX_T + 1];                // s_first[t]: global index of tensor t's first chunk; s_first[T]: all chunks
    __shared__ int s_part[OPT_THREADS];
    __shared__ double s_fold[OPT_THREADS / 64][4];
    __shared__ int s_last;
    const int tid = threadIdx.x, T = a.T;

    long total = chunk_table(a.begin, a.numel, T, a.n, s_first, s_part);
    if (total > a.max_chunks) total = a.max_chunks;        // a table that overlaps itself: the records hold max_chunks, nothing is written past them

    for (long c = blockIdx.x; c < total; c += gridDim.x) {
        const Chunk ch = chunk_at(c, s_first, a.begin, a.numel, T, a.n);
        const int t = ch.t, chunks = ch.chunks;
        const long b = ch.b, m = ch.m, e0 = ch.e0, e1 = ch.e1, nvec = ch.nvec;
        const f32x4_t* g4 = (const f32x4_t*)(a.g + b + e0);
        const f32x4_t* p4 = WITH_P ? (const f32x4_t*)(a.p + b + e0) : nullptr;
        StatAcc acc = {0.0, 0.0, 0.0, 0.0};
        long i = tid;
        for (; i + (STAT_UNROLL - 1) * OPT_THREADS < nvec; i += STAT_UNROLL * OPT_THREADS) {
            f32x4_t x[STAT_UNROLL], y[STAT_UNROLL];
#pragma unroll
            for (int u = 0; u < STAT_UNROLL; ++u) {
                x[u] = g4[i + u * OPT_THREADS];
                if (WITH_P) y[u] = p4[i + u * OPT_THREADS];
            }
#pragma unroll
            for (int u = 0; u < STAT_UNROLL; ++u) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    stat_add_g(acc, x[u][q]);
                    if (WITH_P) acc.sp += (double)y[u][q] * (double)y[u][q];
                }
            }
        }
        for (; i < nvec; i += OPT_THREADS) {
            const f32x4_t x = g4[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) stat_add_g(acc, x[q]);
            if (WITH_P) {
                const f32x4_t y = p4[i];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc.sp += (double)y[q] * (double)y[q];
            }
        }
        if (e1 == m && e1 > e0 && tid < (int)(m & 3)) {    // the tensor's trailing elements, in its last chunk
            const long j = b + (m & ~3L) + tid;
            stat_add_g(acc, a.g[j]);
            if (WITH_P) acc.sp += (double)a.p[j] * (double)a.p[j];
        }
        stat_fold(acc, s_fold);
        if (chunks == 1) {                                 // finished here: no record, no ticket
            if (tid == 0) { double* o = a.out + 4L * t; o[0] = acc.sg; o[1] = acc.amax; o[2] = acc.nf; o[3] = acc.sp; }
            continue;
        }
        if (tid == 0) {
            double* r = a.records + 4 * c;
            handoff::publish(r, acc.sg); handoff::publish(r + 1, acc.amax); handoff::publish(r + 2, acc.nf); handoff::publish(r + 3, acc.sp);
        }
        if (!handoff::arrive<true>([&] { return a.tickets + t; }, [&] { return chunks; }, a.fences, a.fences, &s_last)) continue;
        // the last of this tensor's workgroups: its records in index order
        const double* r0 = a.records + 4L * s_first[t];
        StatAcc tot = {0.0, 0.0, 0.0, 0.0};
        for (int j = tid; j < chunks; j += OPT_THREADS) {
            tot.sg += handoff::read(r0 + 4L * j);
            tot.amax = fmax(tot.amax, handoff::read(r0 + 4L * j + 1));
            tot.nf += handoff::read(r0 + 4L * j + 2);
            tot.sp += handoff::read(r0 + 4L * j + 3);
        }
        stat_fold(tot, s_fold);
        if (tid == 0) { double* o = a.out + 4L * t; o[0] = tot.sg; o[1] = tot.amax; o[2] = tot.nf; o[3] = tot.sp; }
    }
}

// ---- LAMB: AdamW whose per-tensor delta is rescaled by a trust ratio, as two launches ----------------------------------------------------------
// (You et al., "Large Batch Optimization for Deep Learning").  Per element the arithmetic is the decoupled AdamW step's -- adam_moments,
// then adam_delta, on the tensor's own lr_t = float32(hyper[0] * lr_mult) and wd_t = float32(weight_decay * wd_mult), lrwd = lr_t * wd_t,
// wd_t == 0 taking the no-decay form -- and per tensor the delta d is rescaled before it leaves p:
//     S_p = sum (double)p^2,  S_d = sum (double)d^2   over the tensor's numel elements (the padding behind them is never read)
//     r_t = adapt && S_p > 0 && S_d > 0 ? lr_t * sqrt(S_p) / sqrt(S_d) (fp64) : 1;   max_trust > 0: r_t = min(r_t, max_trust)
//     q_t = float32(r_t);   p = p - q_t * d
// d = lr_t * u with u the paper's update direction, so q_t = |p| / |u| is the paper's trust ratio and p -= lr_t * r * u.  q_t = 1 is the
// AdamW step bit for bit (1 * d is exact).  Non-finite sums get no special case: a NaN fails both comparisons (r = 1) and reaches p
// through d, as it does in Adam; the guard is the remedy.
// lamb_moments_kernel (24 B per parameter: read p, g, m, v; write m, v) walks the tensor table chunk by chunk exactly as
//   tensor_stats_kernel does (chunk_table / chunk_at), forms d in registers and adds S_p and S_d in that kernel's fixed order: thread j the
//   vectors j, j + 256, ... of the chunk, then the tensor's trailing elements, the fixed tree, one record {S_p, S_d} per chunk, the
//   tensor's ticket, the last arrival adding the records in index order.  Whoever finishes a tensor writes trust[t] = q_t and
//   sums[2 t ..] = {S_p, S_d}.  work = {tickets[T] (padded to 16 B), records[n / STAT_CHUNK + T][2] fp64}, zeroed once by the caller;
//   the tickets go back to zero.
// lamb_apply_kernel (16 B per parameter: read p, m, v; write p) walks the same chunks, reads trust[t] once per workgroup and chunk,
//   forms d again from the stored m and v -- the same device function on the same inputs: the same bits -- and writes p.
// Both read `hyper` and `ctl` (which may be null) from device memory; with ctl[1] != 0 both return before their first load.  Nothing in
// either launch changes from step to step: the pair replays from a captured graph and is bit-equal call to call.
constexpr int LAMB_UNROLL = 2;                             // moments: 121 VGPRs, 4 workgroups per CU (4: 161 VGPRs, 3 per CU -- the 1024-workgroup grid no longer fits)
constexpr int LAMB_APPLY_UNROLL = 4;                       // apply: 109 VGPRs, 4 per CU

struct LambArgs {
    float* p; const float* g; float* m; float* v; long n;
    const float* hyper; const float* ctl;
    AdamScalars s;                                         // lr, bc1, bc2s come from `hyper` on the device
    float max_trust;
    const long* begin; const long* numel; const float* table;      // table: {lr_mult, wd_mult, adapt} per tensor
    int T, fences;
    long max_chunks;
    unsigned* tickets; double* records; float* trust; double* sums;
};

// the launch's scalars, or false when the step is skipped: before any load of the buffers
__device__ __forceinline__ bool lamb_scalars(const LambArgs& a, AdamScalars& s) {
    s = a.s;
    if (a.ctl != nullptr) {                                // as adamw_kernel's CTL form
        if (a.ctl[1] != 0.f) return false;
        s.gscale = s.gscale * a.ctl[0];
    }
    s.lr = a.hyper[0]; s.bc1 = a.hyper[1]; s.bc2s = a.hyper[2];
    return true;
}

// tensor t's own scalars from the launch's, ONE fp32 multiplication each (as the SEG form's classes)
__device__ __forceinline__ AdamScalars lamb_tensor_scalars(const AdamScalars& s, const float* table, int t, float& lrwd) {
    AdamScalars sc = s;
    sc.lr = s.lr * table[3 * t];
    sc.wd = s.wd * table[3 * t + 1];
    lrwd = sc.lr * sc.wd;
    return sc;
}

template <int WD>
__device__ __forceinline__ void lamb_moments_elem(float p, float g, float& m, float& v, const AdamScalars& sc, float lrwd, double& sp, double& sd) {
    adam_moments<WD>(p, g, m, v, sc);
    const float d = adam_delta<WD>(p, m, v, sc, lrwd);
    sp += (double)p * (double)p;
    sd += (double)d * (double)d;
}

template <int WD>
__device__ __forceinline__ void lamb_moments_chunk(const LambArgs& a, const Chunk& ch, const AdamScalars& sc, float lrwd, double& sp, double& sd) {
    const int tid = threadIdx.x;
    const long o = ch.b + ch.e0;
    const f32x4_t* p4 = (const f32x4_t*)(a.p + o);
    const f32x4_t* g4 = (const f32x4_t*)(a.g + o);
    f32x4_t* m4 = (f32x4_t*)(a.m + o);
    f32x4_t* v4 = (f32x4_t*)(a.v + o);
    long i = tid;
    for (; i + (LAMB_UNROLL - 1) * OPT_THREADS < ch.nvec; i += LAMB_UNROLL * OPT_THREADS) {
        f32x4_t pp[LAMB_UNROLL], gg[LAMB_UNROLL], mm[LAMB_UNROLL], vv[LAMB_UNROLL];
#pragma unroll
        for (int u = 0; u < LAMB_UNROLL; ++u) {
            pp[u] = p4[i + u * OPT_THREADS]; gg[u] = g4[i + u * OPT_THREADS]; mm[u] = m4[i + u * OPT_THREADS]; vv[u] = v4[i + u * OPT_THREADS];
        }
#pragma unroll
        for (int u = 0; u < LAMB_UNROLL; ++u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float mk = mm[u][k], vk = vv[u][k];
                lamb_moments_elem<WD>(pp[u][k], gg[u][k], mk, vk, sc, lrwd, sp, sd);
                mm[u][k] = mk; vv[u][k] = vk;
            }
            m4[i + u * OPT_THREADS] = mm[u]; v4[i + u * OPT_THREADS] = vv[u];
        }
    }
    for (; i < ch.nvec; i += OPT_THREADS) {
        const f32x4_t pp = p4[i], gg = g4[i];
        f32x4_t mm = m4[i], vv = v4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float mk = mm[k], vk = vv[k];
            lamb_moments_elem<WD>(pp[k], gg[k], mk, vk, sc, lrwd, sp, sd);
            mm[k] = mk; vv[k] = vk;
        }
        m4[i] = mm; v4[i] = vv;
    }
    if (ch.e1 == ch.m && ch.e1 > ch.e0 && tid < (int)(ch.m & 3)) {   // the tensor's trailing elements, in its last chunk
        const long j = ch.b + (ch.m & ~3L) + tid;
        float mk = a.m[j], vk = a.v[j];
        lamb_moments_elem<WD>(a.p[j], a.g[j], mk, vk, sc, lrwd, sp, sd);
        a.m[j] = mk; a.v[j] = vk;
    }
}

// the workgroup's 256 pairs -> thread 0's, in stat_fold's tree: down each 64-lane wave by halving strides, then the four waves in index
// order.  sh: 4 waves x 2 values.  Every thread calls it.
__device__ __forceinline__ void lamb_fold(double& sp, double& sd, double (*sh)[2]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sp += __shfl_down(sp, off, 64);
        sd += __shfl_down(sd, off, 64);
    }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { sh[tid >> 6][0] = sp; sh[tid >> 6][1] = sd; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < OPT_THREADS / 64; ++w) { sp += sh[w][0]; sd += sh[w][1]; }
    }
    __syncthreads();                                       // sh may be written again
}

// thread 0 of the workgroup that holds tensor t's finished sums
__device__ __forceinline__ void lamb_finish(const LambArgs& a, int t, float lr_t, double sp, double sd) {
    double r = 1.0;
    if (a.table[3 * t + 2] != 0.f && sp > 0.0 && sd > 0.0) r = (double)lr_t * sqrt(sp) / sqrt(sd);
    if (a.max_trust > 0.f && r > (double)a.max_trust) r = (double)a.max_trust;
    a.trust[t] = (float)r;
    a.sums[2L * t] = sp;
    a.sums[2L * t + 1] = sd;
}

__global__ __launch_bounds__(OPT_THREADS) void lamb_moments_kernel(LambArgs a) {
    __shared__ int s_first[STAT_MAX_T + 1];
    __shared__ int s_part[OPT_THREADS];
    __shared__ double s_fold[OPT_THREADS / 64][2];
    __shared__ int s_last;
    AdamScalars s;
    if (!lamb_scalars(a, s)) return;                       // a skipped step: m, v, trust, sums, tickets and records keep their bits
    const int tid = threadIdx.x, T = a.T;
    long total = chunk_table(a.begin, a.numel, T, a.n, s_first, s_part);
    if (total > a.max_chunks) total = a.max_chunks;        // as tensor_stats_kernel: nothing is written past the records

    for (long c = blockIdx.x; c < total; c += gridDim.x) {
        const Chunk ch = chunk_at(c, s_first, a.begin, a.numel, T, a.n);
        const int t = ch.t, chunks = ch.chunks;
        float lrwd;
        const AdamScalars sc = lamb_tensor_scalars(s, a.table, t, lrwd);
        double sp = 0.0, sd = 0.0;
        if (sc.wd != 0.f) lamb_moments_chunk<WD_DECOUPLED>(a, ch, sc, lrwd, sp, sd);
        else lamb_moments_chunk<WD_NONE>(a, ch, sc, 0.f, sp, sd);
        lamb_fold(sp, sd, s_fold);
        if (chunks == 1) {                                 // finished here: no record, no ticket
            if (tid == 0) lamb_finish(a, t, sc.lr, sp, sd);
            continue;
        }
        if (tid == 0) {
            double* r = a.records + 2 * c;
            handoff::publish(r, sp); handoff::publish(r + 1, sd);
        }
        if (!handoff::arrive<true>([&] { return a.tickets + t; }, [&] { return chunks; }, a.fences, a.fences, &s_last)) continue;
        // the last of this tensor's workgroups: its records in index order
        const double* r0 = a.records + 2L * s_first[t];
        double tp = 0.0, td = 0.0;
        for (int j = tid; j < chunks; j += OPT_THREADS) {
            tp += handoff::read(r0 + 2L * j);
            td += handoff::read(r0 + 2L * j + 1);
        }
        lamb_fold(tp, td, s_fold);
        if (tid == 0) lamb_finish(a, t, sc.lr, tp, td);
    }
}

template <int WD>
__device__ __forceinline__ void lamb_apply_chunk(const LambArgs& a, const Chunk& ch, const AdamScalars& sc, float lrwd, float q) {
    const int tid = threadIdx.x;
    const long o = ch.b + ch.e0;
    f32x4_t* p4 = (f32x4_t*)(a.p + o);
    const f32x4_t* m4 = (const f32x4_t*)(a.m + o);
    const f32x4_t* v4 = (const f32x4_t*)(a.v + o);
    long i = tid;
    for (; i + (LAMB_APPLY_UNROLL - 1) * OPT_THREADS < ch.nvec; i += LAMB_APPLY_UNROLL * OPT_THREADS) {
        f32x4_t pp[LAMB_APPLY_UNROLL], mm[LAMB_APPLY_UNROLL], vv[LAMB_APPLY_UNROLL];
#pragma unroll
        for (int u = 0; u < LAMB_APPLY_UNROLL; ++u) {
            pp[u] = p4[i + u * OPT_THREADS]; mm[u] = m4[i + u * OPT_THREADS]; vv[u] = v4[i + u * OPT_THREADS];
        }
#pragma unroll
        for (int u = 0; u < LAMB_APPLY_UNROLL; ++u) {
#pragma unroll
            for (int k = 0; k < 4; ++k) pp[u][k] = pp[u][k] - q * adam_delta<WD>(pp[u][k], mm[u][k], vv[u][k], sc, lrwd);
            p4[i + u * OPT_THREADS] = pp[u];
        }
    }
    for (; i < ch.nvec; i += OPT_THREADS) {
        f32x4_t pp = p4[i];
        const f32x4_t mm = m4[i], vv = v4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) pp[k] = pp[k] - q * adam_delta<WD>(pp[k], mm[k], vv[k], sc, lrwd);
        p4[i] = pp;
    }
    if (ch.e1 == ch.m && ch.e1 > ch.e0 && tid < (int)(ch.m & 3)) {
        const long j = ch.b + (ch.m & ~3L) + tid;
        const float pk = a.p[j];
        a.p[j] = pk - q * adam_delta<WD>(pk, a.m[j], a.v[j], sc, lrwd);
    }
}

__global__ __launch_bounds__(OPT_THREADS) void lamb_apply_kernel(LambArgs a) {
    __shared__ int s_first[STAT_MAX_T + 1];
    __shared__ int s_part[OPT_THREADS];
    AdamScalars s;
    if (!lamb_scalars(a, s)) return;                       // a skipped step: p keeps its bits
    const int T = a.T;
    long total = chunk_table(a.begin, a.numel, T, a.n, s_first, s_part);
    if (total > a.max_chunks) total = a.max_chunks;
    for (long c = blockIdx.x; c < total; c += gridDim.x) {
        const Chunk ch = chunk_at(c, s_first, a.begin, a.numel, T, a.n);
        float lrwd;
        const AdamScalars sc = lamb_tensor_scalars(s, a.table, ch.t, lrwd);
        const float q = a.trust[ch.t];                     // one load per workgroup and chunk (uniform)
        if (sc.wd != 0.f) lamb_apply_chunk<WD_DECOUPLED>(a, ch, sc, lrwd, q);
        else lamb_apply_chunk<WD_NONE>(a, ch, sc, 0.f, q);
    }
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

// The SEG form of mte_adamw_step_dev / mte_sgd_step_dev: per-class multipliers of the learning rate and the weight decay.  block_class[b]
// (DEVICE memory, n / 64 bytes) is the class of elements 64 b .. 64 b + 63 and class_scales (DEVICE memory, 2 * n_classes floats) holds
// {lr_mult, wd_mult} per class: lr_c = float32(hyper[0] * lr_mult_c), wd_c = float32(weight_decay * wd_mult_c), then the plain step's
// arithmetic on every block with its class's pair (wd_c == 0: the no-decay arithmetic).  ctl may be null; otherwise it is
// mte_grad_norm_clip's word with the meaning it has in the _ctl_dev forms.  n % 64 != 0, a null table, n_classes outside 1..16 and the
// plain forms' argument errors are MTE_ERR_ARG.  A class byte >= n_classes is read as n_classes - 1.
int mte_adamw_step_seg_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                           float weight_decay, int decoupled, float gscale, const uint8_t* block_class, const float* class_scales, int n_classes,
                           const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !m || !v || !hyper || n <= 0 || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    if ((n & 63) || !block_class || !class_scales || n_classes < 1 || n_classes > SEG_MAX_CLASSES) return MTE_ERR_ARG;
    const AdamScalars s = {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay};
    const SegArgs t = {block_class, class_scales, ctl, n_classes};
    const dim3 grid(opt_grid(n >> 2)), block(OPT_THREADS);
    if (s.wd == 0.f) hipLaunchKernelGGL((adamw_seg_kernel<WD_NONE>), grid, block, 0, stream, p, g, m, v, n, hyper, s, t);
    else if (decoupled) hipLaunchKernelGGL((adamw_seg_kernel<WD_DECOUPLED>), grid, block, 0, stream, p, g, m, v, n, hyper, s, t);
    else hipLaunchKernelGGL((adamw_seg_kernel<WD_L2>), grid, block, 0, stream, p, g, m, v, n, hyper, s, t);
    return mte_check_launch();
}

int mte_sgd_step_seg_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                         float gscale, const uint8_t* block_class, const float* class_scales, int n_classes, const float* ctl,
                         hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !hyper || n <= 0 || !(momentum >= 0.f) || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    if ((momentum > 0.f && !buf) || (nesterov && momentum <= 0.f)) return MTE_ERR_ARG;
    if ((n & 63) || !block_class || !class_scales || n_classes < 1 || n_classes > SEG_MAX_CLASSES) return MTE_ERR_ARG;
    const SgdScalars s = {0.f, 0.f, 0.f, momentum, gscale, weight_decay};
    const SegArgs t = {block_class, class_scales, ctl, n_classes};
    if (s.mu == 0.f) sgd_seg_launch_wd<MOM_NONE>(p, g, buf, n, hyper, s, t, stream);
    else if (nesterov) sgd_seg_launch_wd<MOM_NESTEROV>(p, g, buf, n, hyper, s, t, stream);
    else sgd_seg_launch_wd<MOM_PLAIN>(p, g, buf, n, hyper, s, t, stream);
    return mte_check_launch();
}

// Bytes of `work` for mte_tensor_stats over T tensors inside n flat elements (16-byte aligned, zeroed ONCE by the caller): one ticket per
// tensor, then one record of four fp64 values per chunk.  0 for n <= 0 or T outside 1..4096.
long mte_tensor_stats_work_bytes(long n, int T) {
    return (n <= 0 || T < 1 || T > STAT_MAX_T) ? 0 : stat_ticket_bytes(T) + 32L * stat_max_chunks(n, T);
}

// Per-tensor statistics of the flat gradient g[0..n) and, with p non-null, of the weights p[0..n) (both 16-byte aligned; read-only) in ONE
// launch: tensor t is elements seg_begin[t] .. seg_begin[t] + seg_numel[t] - 1 (`long` arrays in DEVICE memory; begins are multiples of
// 64, ranges disjoint and inside [0, n)), out[4 t ..] = {sum g^2, max |g| over the finite elements, count of non-finite elements,
// sum p^2 (0 without p)} as fp64 in DEVICE memory.  The order of every addition is fixed by the table (see the kernel): bit-equal call
// to call and under graph replay; the tickets in `work` go back to zero.  A range that leaves [0, n) reads nothing and reports zeros.
int mte_tensor_stats(const float* g, const float* p, long n, const long* seg_begin, const long* seg_numel, int T, void* work, double* out,
                     hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!g || !seg_begin || !seg_numel || !work || !out || n <= 0 || T < 1 || T > STAT_MAX_T) return MTE_ERR_ARG;
    if ((((uintptr_t)g | (uintptr_t)p | (uintptr_t)work) & 15) || stat_max_chunks(n, T) > 0x7fffffffL) return MTE_ERR_ARG;
    StatArgs a;
    a.g = g; a.p = p; a.n = n; a.begin = seg_begin; a.numel = seg_numel; a.T = T; a.fences = g_mte_handoff_fences;
    a.max_chunks = stat_max_chunks(n, T);
    a.tickets = (unsigned*)work; a.records = (double*)((char*)work + stat_ticket_bytes(T)); a.out = out;
    const long want = a.max_chunks;
    const dim3 grid((unsigned)(want > STAT_CAP ? STAT_CAP : want)), block(OPT_THREADS);
    if (p) hipLaunchKernelGGL(tensor_stats_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(tensor_stats_kernel<false>, grid, block, 0, stream, a);
    return mte_check_launch();
}

// Bytes of `work` for mte_lamb_moments over T tensors inside n flat elements (16-byte aligned, zeroed ONCE by the caller): one ticket per
// tensor, then one record {S_p, S_d} of two fp64 values per chunk.  0 for n <= 0 or T outside 1..4096.
long mte_lamb_work_bytes(long n, int T) {
    return (n <= 0 || T < 1 || T > STAT_MAX_T) ? 0 : stat_ticket_bytes(T) + 16L * stat_max_chunks(n, T);
}

// The first launch of the LAMB step (see lamb_moments_kernel): m and v move as in mte_adamw_step_dev (decoupled), p is only read, and
// trust[t] = q_t, sums[2 t ..] = {S_p, S_d} are left for every tensor of the table {seg_begin, seg_numel, tensor_table} (DEVICE memory).
// p, g, m, v and work are 16-byte aligned.  ctl may be null.  A range that leaves [0, n) reads and writes nothing in the flat buffers
// (its trust is 1, its sums are 0).
int mte_lamb_moments(const float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                     float weight_decay, float gscale, float max_trust, const long* seg_begin, const long* seg_numel, const float* tensor_table,
                     int T, void* work, float* trust, double* sums, const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !m || !v || !hyper || !seg_begin || !seg_numel || !tensor_table || !work || !trust || !sums) return MTE_ERR_ARG;
    if (n <= 0 || T < 1 || T > STAT_MAX_T || !(weight_decay >= 0.f) || !(max_trust >= 0.f)) return MTE_ERR_ARG;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)work) & 15) || ((uintptr_t)sums & 7)) return MTE_ERR_ARG;
    if (stat_max_chunks(n, T) > 0x7fffffffL) return MTE_ERR_ARG;
    LambArgs a;
    a.p = const_cast<float*>(p); a.g = g; a.m = m; a.v = v; a.n = n; a.hyper = hyper; a.ctl = ctl;
    a.s = {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay};
    a.max_trust = max_trust;
    a.begin = seg_begin; a.numel = seg_numel; a.table = tensor_table; a.T = T; a.fences = g_mte_handoff_fences;
    a.max_chunks = stat_max_chunks(n, T);
    a.tickets = (unsigned*)work; a.records = (double*)((char*)work + stat_ticket_bytes(T)); a.trust = trust; a.sums = sums;
    const long want = a.max_chunks;
    hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)(want > STAT_CAP ? STAT_CAP : want)), dim3(OPT_THREADS), 0, stream, a);
    return mte_check_launch();
}

// The second launch (see lamb_apply_kernel): p = p - trust[t] * d with d formed again from the stored m and v; m, v and trust are only
// read.  The same table, hyper, eps, weight_decay and ctl as the mte_lamb_moments launch in front of it.
int mte_lamb_apply(float* p, const float* m, const float* v, long n, const float* hyper, float eps, float weight_decay, const long* seg_begin,
                   const long* seg_numel, const float* tensor_table, int T, const float* trust, const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !m || !v || !hyper || !seg_begin || !seg_numel || !tensor_table || !trust) return MTE_ERR_ARG;
    if (n <= 0 || T < 1 || T > STAT_MAX_T || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    if ((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) || stat_max_chunks(n, T) > 0x7fffffffL) return MTE_ERR_ARG;
    LambArgs a;
    a.p = p; a.g = nullptr; a.m = const_cast<float*>(m); a.v = const_cast<float*>(v); a.n = n; a.hyper = hyper; a.ctl = ctl;
    a.s = {0.f, 0.f, 0.f, 0.f, 0.f, eps, 1.f, weight_decay};
    a.max_trust = 0.f;
    a.begin = seg_begin; a.numel = seg_numel; a.table = tensor_table; a.T = T; a.fences = 0;
    a.max_chunks = stat_max_chunks(n, T);
    a.tickets = nullptr; a.records = nullptr; a.trust = const_cast<float*>(trust); a.sums = nullptr;
    const long want = a.max_chunks;
    hipLaunchKernelGGL(lamb_apply_kernel, dim3((unsigned)(want > STAT_CAP ? STAT_CAP : want)), dim3(OPT_THREADS), 0, stream, a);
    return mte_check_launch();
}

}  // extern "C"
