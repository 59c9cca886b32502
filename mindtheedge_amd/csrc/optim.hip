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
#include "common.hpp"

namespace {

constexpr int OPT_THREADS = 256;
inline int opt_grid(long n4) { long g = (n4 + OPT_THREADS - 1) / OPT_THREADS; return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }

enum { WD_NONE = 0, WD_L2 = 1, WD_DECOUPLED = 2 };
enum { MOM_NONE = 0, MOM_PLAIN = 1, MOM_NESTEROV = 2 };

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

template <int WD, bool DEV>
__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, long n, const float* __restrict__ hyper, AdamScalars s) {
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

template <bool DEV>
int adamw_launch(float* p, const float* g, float* m, float* v, long n, const float* hyper, const AdamScalars& s, int decoupled, hipStream_t stream) {
    const dim3 grid(opt_grid(n >> 2)), block(OPT_THREADS);
    if (s.wd == 0.f) hipLaunchKernelGGL((adamw_kernel<WD_NONE, DEV>), grid, block, 0, stream, p, g, m, v, n, hyper, s);
    else if (decoupled) hipLaunchKernelGGL((adamw_kernel<WD_DECOUPLED, DEV>), grid, block, 0, stream, p, g, m, v, n, hyper, s);
    else hipLaunchKernelGGL((adamw_kernel<WD_L2, DEV>), grid, block, 0, stream, p, g, m, v, n, hyper, s);
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

template <int MOM, bool WD, bool DEV>
__global__ __launch_bounds__(OPT_THREADS) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                          const float* __restrict__ hyper, SgdScalars s) {
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

template <int MOM, bool DEV>
void sgd_launch_wd(float* p, const float* g, float* buf, long n, const float* hyper, const SgdScalars& s, hipStream_t stream) {
    const dim3 grid(opt_grid(n >> 2)), block(OPT_THREADS);
    if (s.wd != 0.f) hipLaunchKernelGGL((sgd_kernel<MOM, true, DEV>), grid, block, 0, stream, p, g, buf, n, hyper, s);
    else hipLaunchKernelGGL((sgd_kernel<MOM, false, DEV>), grid, block, 0, stream, p, g, buf, n, hyper, s);
}

template <bool DEV>
int sgd_launch(float* p, const float* g, float* buf, long n, const float* hyper, const SgdScalars& s, int nesterov, hipStream_t stream) {
    if (s.mu == 0.f) sgd_launch_wd<MOM_NONE, DEV>(p, g, buf, n, hyper, s, stream);
    else if (nesterov) sgd_launch_wd<MOM_NESTEROV, DEV>(p, g, buf, n, hyper, s, stream);
    else sgd_launch_wd<MOM_PLAIN, DEV>(p, g, buf, n, hyper, s, stream);
    return mte_check_launch();
}

}  // namespace

extern "C" {

// In-place Adam with weight decay over flat fp32 buffers (16-byte aligned).  decoupled = 0: torch.optim.Adam(weight_decay) (L2, added to
// the gradient), decoupled = 1: torch.optim.AdamW.  weight_decay = 0 is mte_adam_step's update bit for bit.  step >= 1; gscale multiplies
// the gradient first.
int mte_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int decoupled, int step, float gscale, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !m || !v || n <= 0 || step < 1 || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const AdamScalars s = {lr, (float)bc1, (float)sqrt(bc2), beta1, beta2, eps, gscale, weight_decay};
    return adamw_launch<false>(p, g, m, v, n, nullptr, s, decoupled, stream);
}

// The same step with hyper = {lr, 1 - beta1^t, sqrt(1 - beta2^t)} in DEVICE memory, as mte_adam_step_dev: lr * weight_decay is formed in
// the kernel from hyper[0].
int mte_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                       float weight_decay, int decoupled, float gscale, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !m || !v || !hyper || n <= 0 || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    const AdamScalars s = {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay};
    return adamw_launch<true>(p, g, m, v, n, hyper, s, decoupled, stream);
}

// In-place torch.optim.SGD over flat fp32 buffers (16-byte aligned).  momentum = 0: `buf` is neither read nor written and may be null.
// With momentum, `buf` is zero-initialised by the caller before step 1.  Nesterov needs momentum > 0 and dampening = 0, as torch.
int mte_sgd_step(float* p, const float* g, float* buf, long n, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                 int step, float gscale, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || n <= 0 || step < 1 || !(momentum >= 0.f) || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    if ((momentum > 0.f && !buf) || (nesterov && (momentum <= 0.f || dampening != 0.f))) return MTE_ERR_ARG;
    const SgdScalars s = {lr, step == 1 ? 0.f : momentum, step == 1 ? 1.f : (float)(1.0 - (double)dampening), momentum, gscale, weight_decay};
    return sgd_launch<false>(p, g, buf, n, nullptr, s, nesterov, stream);
}

// The same step with hyper = {lr, mu_eff, (1 - dampening)_eff} in DEVICE memory: {lr, 0, 1} at step 1, {lr, momentum, 1 - dampening}
// afterwards.  `momentum` is the launch constant that selects the kernel and feeds Nesterov's look-ahead.
int mte_sgd_step_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                     float gscale, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    if (!p || !g || !hyper || n <= 0 || !(momentum >= 0.f) || !(weight_decay >= 0.f)) return MTE_ERR_ARG;
    if ((momentum > 0.f && !buf) || (nesterov && momentum <= 0.f)) return MTE_ERR_ARG;
    const SgdScalars s = {0.f, 0.f, 0.f, momentum, gscale, weight_decay};
    return sgd_launch<true>(p, g, buf, n, hyper, s, nesterov, stream);
}

}  // extern "C"
