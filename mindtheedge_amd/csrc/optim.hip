// The optimizer family beside mte_adam_step (heads_misc.hip): Adam with L2 weight decay, AdamW, SGD (momentum, dampening, Nesterov, weight
// decay) and LAMB as streaming launches over the flat fp32 master buffers (gfx950), with what goes around a step: the gradient norm / clip
// coefficient / non-finite guard (ctl), gradient accumulation, the weight EMA and swap, per-tensor multipliers (the SEG form) and
// per-tensor statistics.  This file holds the kernels, the comments that state their arithmetic and order of additions, and thin extern "C"
// wrappers.  What the host decides -- argument rules, instance, grid, work-buffer layout, the chunk cut of a tensor table -- is
// optim_plan.hpp (no HIP; tests/test_optim_launch_table_cpu.py checks it without a GPU).
//
// HBM-bound: Adam / AdamW move 28 B per parameter (read p, g, m, v; write p, m, v), SGD with momentum 20 B, plain SGD 12 B.  The step
// kernels' launch shape is adam_kernel's: 256 threads, one 16-byte vector of each buffer per thread and trip, a grid-stride loop under the
// 8192-workgroup cap, the n & 3 tail in workgroup 0.  Every step has a form with scalars from the host and forms that read the per-step
// scalars from DEVICE memory (`hyper`, three floats), so that nothing in the launch changes from step to step and a captured HIP graph
// stays valid; all forms run the same template on the same float32 scalars and give bit-equal results.  The arithmetic is fp32 with
// -ffp-contract=off, the operations in the order written below (tests/optim_ref.py states them in float64). A feature is a kernel (or
// instance) of its own: the instances that existed before it keep their instruction streams (profiles/optim_refactor.txt).
#include "common.hpp"
#include "handoff.hpp"
#include "optim_plan.hpp"
#include <cstdint>
#include <type_traits>

namespace {
using namespace optim_plan;

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

// ctl = {clip coefficient, skip flag, norm, skipped steps} left by grad_norm_kernel (below).  -> false: a non-finite gradient, the step is
// skipped before its first load (p and the state keep their bits); otherwise the gradient scale takes the clip coefficient.
__device__ __forceinline__ bool ctl_gate(const float* ctl, float& gscale) {
    if (ctl[1] != 0.f) return false;
    gscale = gscale * ctl[0];
    return true;
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
    if constexpr (CTL) {
        if (!ctl_gate(s.ctl, s.gscale)) return;
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

template <int MOM, bool WD>
__device__ __forceinline__ void sgd_vec(f32x4_t& pp, const f32x4_t& gg, f32x4_t& bb, const SgdScalars& s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float pk = pp[k], bk = bb[k];
        sgd_elem<MOM, WD>(pk, gg[k], bk, s);
        pp[k] = pk; bb[k] = bk;
    }
}

template <int MOM, bool WD, bool DEV, bool CTL>
__global__ __launch_bounds__(OPT_THREADS) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n,
                                                          const float* __restrict__ hyper, StepScalars<SgdScalars, CTL> s) {
    if constexpr (CTL) {
        if (!ctl_gate(s.ctl, s.gscale)) return;
    }
    if (DEV) { s.lr = hyper[0]; s.mu_eff = hyper[1]; s.omd_eff = hyper[2]; }
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], bb = {0.f, 0.f, 0.f, 0.f};
        if (MOM != MOM_NONE) bb = ((f32x4_t*)buf)[i];
        sgd_vec<MOM, WD>(pp, gg, bb, s);
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

// ---- global gradient norm, clip coefficient and non-finite guard -----------------------------------------------------------------------
// One read-only pass over the flat gradient (4 B per parameter against the step's 28) that leaves, in device memory, what the step kernels'
// CTL form reads: ctl = {clip coefficient, skip flag, norm, skipped-step count}.  Every thread adds (double)g * (double)g in fp64 -- the
// square of an fp32 value is exact there, only the additions round -- over the vectors i = thread, thread + grid * 256, ... in that
// order (NORM_UNROLL loads are issued ahead of their additions; the order of the additions is the one-vector-per-trip order), workgroup 0
// the n & 3 tail.  A workgroup folds its 256 partials in a fixed tree and leaves ONE fp64 record; the workgroup that draws the last ticket
// (handoff.hpp) adds the records in index order.  The grid is a function of n alone, so the sum has one order: bit-equal run to run and
// under HIP-graph replay; the ticket goes back to zero.  work: norm_layout (optim_plan.hpp).
// measured at 77.0 M elements with NORM_CAP = 256 workgroups (profiles/grad_clip.txt): 0.051 ms; 512 x 4: 0.054, 1024 x 4: 0.063,
// 2048 x 4: 0.073 -- the last arriver's sum grows with the cap
constexpr int NORM_UNROLL = 8;

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
struct SegArgs { const uint8_t* cls; const float* scales; const float* ctl; int n_classes; };

// Every thread of the workgroup calls it: {lr_c, wd_c} of every class into LDS (SEG_MAX_CLASSES floats each).
__device__ __forceinline__ void seg_stage(const SegArgs& t, float lr, float wd, float* s_lr, float* s_wd) {
    if ((int)threadIdx.x < t.n_classes) {
        s_lr[threadIdx.x] = lr * t.scales[2 * threadIdx.x];
        s_wd[threadIdx.x] = wd * t.scales[2 * threadIdx.x + 1];
    }
    __syncthreads();
}
// the class of vector i, clamped to the last class
__device__ __forceinline__ int seg_class(const SegArgs& t, long i) {
    const int c = t.cls[i >> 4], last = t.n_classes - 1;
    return c > last ? last : c;
}

template <int WD>
__global__ __launch_bounds__(OPT_THREADS) void adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, long n, const float* __restrict__ hyper, AdamScalars s,
                                                                SegArgs t) {
    __shared__ float s_lr[SEG_MAX_CLASSES], s_wd[SEG_MAX_CLASSES];
    if (t.ctl != nullptr) {                                // as adamw_kernel's CTL form: the skip flag first, before any load
        if (!ctl_gate(t.ctl, s.gscale)) return;
    }
    s.lr = hyper[0]; s.bc1 = hyper[1]; s.bc2s = hyper[2];
    seg_stage(t, s.lr, s.wd, s_lr, s_wd);
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int c = seg_class(t, i);
        AdamScalars sc = s;
        sc.lr = s_lr[c]; sc.wd = s_wd[c];
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], mm = ((f32x4_t*)m)[i], vv = ((f32x4_t*)v)[i];
        // (the four lanes stay written out here and in adamw_kernel: as a shared adam_vec the decaying instances took 2 to 4 VGPRs more)
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
    if (t.ctl != nullptr && !ctl_gate(t.ctl, s.gscale)) return;        // as sgd_kernel's CTL form
    s.lr = hyper[0]; s.mu_eff = hyper[1]; s.omd_eff = hyper[2];
    seg_stage(t, s.lr, s.wd, s_lr, s_wd);
    const long n4 = n >> 2;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const int c = seg_class(t, i);
        SgdScalars sc = s;
        sc.lr = s_lr[c]; sc.wd = s_wd[c];
        f32x4_t pp = ((f32x4_t*)p)[i], gg = ((const f32x4_t*)g)[i], bb = {0.f, 0.f, 0.f, 0.f};
        if (MOM != MOM_NONE) bb = ((f32x4_t*)buf)[i];
        if (WD && sc.wd != 0.f) sgd_vec<MOM, true>(pp, gg, bb, sc);
        else sgd_vec<MOM, false>(pp, gg, bb, sc);
        ((f32x4_t*)p)[i] = pp;
        if (MOM != MOM_NONE) ((f32x4_t*)buf)[i] = bb;
    }
}

// ---- the chunk walk of the per-tensor kernels (tensor_stats_kernel, the LAMB pair) ---------------------------------------------------------------------
// The cut itself -- chunk_range_ok, chunk_count, Chunk, chunk_at -- is optim_plan.hpp's.  Order of the additions of a per-tensor sum, a
// function of the tensor table alone -- not of the grid, not of arrival:
//   * chunk k of tensor t has the global index first_t + k, first_t the running sum of the chunk counts (every workgroup forms that
//     table in LDS: T <= STAT_MAX_T);
//   * a chunk is read by ONE workgroup: thread j takes the vectors j, j + 256, ... of the chunk in that order (loads are issued ahead of
//     their use), then thread j < (numel & 3) of the tensor's last chunk the tensor's j-th trailing element; the 256 partials fold in a
//     fixed tree (down each 64-lane wave by halving strides, then the four waves in index order) into ONE record of fp64 values;
//   * a tensor of one chunk is finished there.  Otherwise the workgroup draws the TENSOR's ticket (handoff.hpp, as grad_norm_kernel), and
//     the one that draws the last of its chunk_count tickets adds the records: thread j the records j, j + 256, ... in that order, then
//     the same tree.  Workgroups take chunks c = workgroup, workgroup + grid, ...: every loop is bounded and nobody waits.
// Tickets go back to zero, so a launch replays from a captured graph and is bit-equal call to call.  work: chunk_layout (optim_plan.hpp).

// Every thread of the workgroup calls it.  s_first[t] <- the global index of tensor t's first chunk (the running sum of chunk_count, as
// chunk_table_host), s_first[T] <- all chunks, which it returns.  s_first: STAT_MAX_T + 1 ints, s_part: 256 ints.
__device__ __forceinline__ long chunk_table(const long* begin, const long* numel, int T, long n, int* s_first, int* s_part) {
    const int tid = threadIdx.x;
    constexpr int PER = STAT_MAX_T / OPT_THREADS;          // consecutive tensors per thread in the scan
    int cnt[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int t = tid * PER + k;
        cnt[k] = t < T ? chunk_count(begin[t], numel[t], n) : 0;
        mine += cnt[k];
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

// The workgroup's 256 partials -> thread 0's `a`, in the fixed tree; sh: 4 waves x A::N values.  Every thread calls it.  An accumulator A
// has N fp64 members, each(f) calling f(index, member) for every one, and add(f) combining every member with f(index, member) -- a sum, or
// a maximum.
template <class A>
__device__ __forceinline__ void fold_sums(A& a, double (*sh)[A::N]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a.add([&](int, double x) { return __shfl_down(x, off, 64); });
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) a.each([&](int i, double x) { sh[tid >> 6][i] = x; });
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < OPT_THREADS / 64; ++w) a.add([&](int i, double) { return sh[w][i]; });
    }
    __syncthreads();                                       // sh may be written again
}

// Every thread of the workgroup calls it with its partial of chunk c (of tensor ch.t, whose first chunk is s_first[ch.t]): the fold; for a
// tensor of one chunk finish(sums) on thread 0 (no record, no ticket); otherwise the record, the tensor's ticket, and in the last arrival
// the records in index order, the fold and finish(sums) on thread 0.
template <class A, class Finish>
__device__ __forceinline__ void chunk_reduce(A acc, const Chunk& ch, long c, const int* s_first, unsigned* tickets, double* records, int fences,
                                             double (*s_fold)[A::N], int* s_last, Finish finish) {
    const int tid = threadIdx.x;
    fold_sums(acc, s_fold);
    if (ch.chunks == 1) {
        if (tid == 0) finish(acc);
        return;
    }
    if (tid == 0) acc.each([&](int i, double x) { handoff::publish(records + A::N * c + i, x); });
    if (!handoff::arrive<true>([&] { return tickets + ch.t; }, [&] { return ch.chunks; }, fences, fences, s_last)) return;
    const double* r0 = records + (long)A::N * s_first[ch.t];
    A tot;
    for (int j = tid; j < ch.chunks; j += OPT_THREADS) tot.add([&](int i, double) { return handoff::read(r0 + (long)A::N * j + i); });
    fold_sums(tot, s_fold);
    if (tid == 0) finish(tot);
}

// ---- per-tensor statistics of the flat gradient (and weights) ------------------------------------------------------------------------------
// One read-only launch.  Tensor t is elements [begin_t, begin_t + numel_t) of the flat buffers (begin_t a multiple of 64; the padding
// behind numel_t is never read).  out[4 t ..] = {S_g = sum g^2, amax_g = max |g| over the finite elements (0 without one), the count of
// non-finite elements of g, S_p = sum p^2 (0 without p)}, all fp64; the squares are exact there, only the additions round, and an inf
// or a NaN reaches S_g (inf^2 = inf).  The order of the additions is the chunk walk's (above).
constexpr int STAT_UNROLL = 4;

struct StatArgs {
    const float* g; const float* p; long n;
    const long* begin; const long* numel; int T; int fences;
    long max_chunks;
    unsigned* tickets; double* records; double* out;
};

struct StatAcc {
    static constexpr int N = STAT_VALUES;
    double sg = 0.0, amax = 0.0, nf = 0.0, sp = 0.0;          // (zeroed here: a zero() returning the struct cost tensor_stats_kernel<true> 8 SGPRs)
    template <class F> __device__ __forceinline__ void each(F f) const { f(0, sg); f(1, amax); f(2, nf); f(3, sp); }
    // f(i, x): what member i (now x) is combined with -- fold_sums passes `__shfl_down(x, off, 64)`, then `sh[w][i]`; chunk_reduce the records' word i
    template <class F> __device__ __forceinline__ void add(F f) { sg += f(0, sg); amax = fmax(amax, f(1, amax)); nf += f(2, nf); sp += f(3, sp); }
};

__device__ __forceinline__ void stat_add_g(StatAcc& a, float x) {
    a.sg += (double)x * (double)x;
    const float ax = fabsf(x);
    if (ax <= 3.402823466e+38f) a.amax = fmax(a.amax, (double)ax);
    else a.nf += 1.0;                                      // inf or NaN (the comparison is false for a NaN)
}

template <bool WITH_P>
__global__ __launch_bounds__(OPT_THREADS) void tensor_stats_kernel(StatArgs a) {
    __shared__ int s_first[STAT_MAX_T + 1];                // s_first[t]: global index of tensor t's first chunk; s_first[T]: all chunks
    __shared__ int s_part[OPT_THREADS];
    __shared__ double s_fold[OPT_THREADS / 64][StatAcc::N];
    __shared__ int s_last;
    const int T = a.T;

    long total = chunk_table(a.begin, a.numel, T, a.n, s_first, s_part);
    if (total > a.max_chunks) total = a.max_chunks;        // a table that overlaps itself: the records hold max_chunks, nothing is written past them

    for (long c = blockIdx.x; c < total; c += gridDim.x) {
        const Chunk ch = chunk_at(c, s_first, a.begin, a.numel, T, a.n);
        const int tid = threadIdx.x;
        const long b = ch.b, m = ch.m, e0 = ch.e0, nvec = ch.nvec;
        const f32x4_t* g4 = (const f32x4_t*)(a.g + b + e0);
        const f32x4_t* p4 = WITH_P ? (const f32x4_t*)(a.p + b + e0) : nullptr;
        StatAcc acc;
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
        if (ch.has_tail() && tid < (int)(m & 3)) {    // the tensor's trailing elements, in its last chunk
            const long j = b + (m & ~3L) + tid;
            stat_add_g(acc, a.g[j]);
            if (WITH_P) acc.sp += (double)a.p[j] * (double)a.p[j];
        }
        chunk_reduce(acc, ch, c, s_first, a.tickets, a.records, a.fences, s_fold, &s_last, [&](const StatAcc& tot) {
            double* o = a.out + 4L * ch.t;
            o[0] = tot.sg; o[1] = tot.amax; o[2] = tot.nf; o[3] = tot.sp;
        });
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
//   tensor_stats_kernel does, forms d in registers and adds S_p and S_d in the chunk walk's fixed order (one record {S_p, S_d} per chunk).
//   Whoever finishes a tensor writes trust[t] = q_t and sums[2 t ..] = {S_p, S_d}.
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
    if (a.ctl != nullptr && !ctl_gate(a.ctl, s.gscale)) return false;  // as adamw_kernel's CTL form
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

struct LambAcc {
    static constexpr int N = LAMB_VALUES;
    double sp = 0.0, sd = 0.0;
    template <class F> __device__ __forceinline__ void each(F f) const { f(0, sp); f(1, sd); }
    template <class F> __device__ __forceinline__ void add(F f) { sp += f(0, sp); sd += f(1, sd); }
};

template <int WD>
__device__ __forceinline__ void lamb_moments_elem(float p, float g, float& m, float& v, const AdamScalars& sc, float lrwd, double& sp, double& sd) {
    adam_moments<WD>(p, g, m, v, sc);
    const float d = adam_delta<WD>(p, m, v, sc, lrwd);
    sp += (double)p * (double)p;
    sd += (double)d * (double)d;
}

template <int WD>
__device__ __forceinline__ void lamb_moments_chunk(const LambArgs& a, const Chunk& ch, const AdamScalars& sc, float lrwd, LambAcc& acc) {
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
                lamb_moments_elem<WD>(pp[u][k], gg[u][k], mk, vk, sc, lrwd, acc.sp, acc.sd);
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
            lamb_moments_elem<WD>(pp[k], gg[k], mk, vk, sc, lrwd, acc.sp, acc.sd);
            mm[k] = mk; vv[k] = vk;
        }
        m4[i] = mm; v4[i] = vv;
    }
    if (ch.has_tail() && tid < (int)(ch.m & 3)) {   // the tensor's trailing elements, in its last chunk
        const long j = ch.b + (ch.m & ~3L) + tid;
        float mk = a.m[j], vk = a.v[j];
        lamb_moments_elem<WD>(a.p[j], a.g[j], mk, vk, sc, lrwd, acc.sp, acc.sd);
        a.m[j] = mk; a.v[j] = vk;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void lamb_moments_kernel(LambArgs a) {
    __shared__ int s_first[STAT_MAX_T + 1];
    __shared__ int s_part[OPT_THREADS];
    __shared__ double s_fold[OPT_THREADS / 64][LambAcc::N];
    __shared__ int s_last;
    AdamScalars s;
    if (!lamb_scalars(a, s)) return;                       // a skipped step: m, v, trust, sums, tickets and records keep their bits
    const int T = a.T;
    long total = chunk_table(a.begin, a.numel, T, a.n, s_first, s_part);
    if (total > a.max_chunks) total = a.max_chunks;        // as tensor_stats_kernel: nothing is written past the records

    for (long c = blockIdx.x; c < total; c += gridDim.x) {
        const Chunk ch = chunk_at(c, s_first, a.begin, a.numel, T, a.n);
        float lrwd;
        const AdamScalars sc = lamb_tensor_scalars(s, a.table, ch.t, lrwd);
        LambAcc acc;
        if (sc.wd != 0.f) lamb_moments_chunk<WD_DECOUPLED>(a, ch, sc, lrwd, acc);
        else lamb_moments_chunk<WD_NONE>(a, ch, sc, 0.f, acc);
        chunk_reduce(acc, ch, c, s_first, a.tickets, a.records, a.fences, s_fold, &s_last, [&](const LambAcc& tot) {
            double r = 1.0;                                // thread 0 of the workgroup that holds tensor t's finished sums
            if (a.table[3 * ch.t + 2] != 0.f && tot.sp > 0.0 && tot.sd > 0.0) r = (double)sc.lr * sqrt(tot.sp) / sqrt(tot.sd);
            if (a.max_trust > 0.f && r > (double)a.max_trust) r = (double)a.max_trust;
            a.trust[ch.t] = (float)r;
            a.sums[2L * ch.t] = tot.sp;
            a.sums[2L * ch.t + 1] = tot.sd;
        });
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
    if (ch.has_tail() && tid < (int)(ch.m & 3)) {
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

// ---- launches: one switch per family from the plan's instance to the template ----------------------------------------------------------------------
template <StepForm FORM, int WD>
void adam_launch(const StepPlan& pl, const StepCall& c, const AdamScalars& s, const SegArgs& t, hipStream_t stream) {
    const dim3 grid(pl.grid), block(pl.block);
    float* const p = (float*)c.p; const float* const g = (const float*)c.g; float* const m = (float*)c.state[0]; float* const v = (float*)c.state[1];
    const float* const hyper = (const float*)c.hyper;
    if constexpr (FORM == STEP_SEG) hipLaunchKernelGGL((adamw_seg_kernel<WD>), grid, block, 0, stream, p, g, m, v, c.n, hyper, s, t);
    else hipLaunchKernelGGL((adamw_kernel<WD, FORM != STEP_HOST, FORM == STEP_CTL>), grid, block, 0, stream, p, g, m, v, c.n, hyper,
                            step_scalars<FORM == STEP_CTL>(s, t.ctl));
}
template <StepForm FORM>
int adam_step(const StepCall& c, const AdamScalars& s, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    const StepPlan pl = plan_adam(c, FORM);
    if (pl.rc != MTE_OK) return pl.rc;
    const SegArgs t = {(const uint8_t*)c.cls, (const float*)c.scales, (const float*)c.ctl, c.n_classes};
    switch (pl.wd) {
    case WD_NONE: adam_launch<FORM, WD_NONE>(pl, c, s, t, stream); break;
    case WD_L2: adam_launch<FORM, WD_L2>(pl, c, s, t, stream); break;
    default: adam_launch<FORM, WD_DECOUPLED>(pl, c, s, t, stream); break;
    }
    return mte_check_launch();
}

template <StepForm FORM, int MOM, bool WD>
void sgd_launch(const StepPlan& pl, const StepCall& c, const SgdScalars& s, const SegArgs& t, hipStream_t stream) {
    const dim3 grid(pl.grid), block(pl.block);
    float* const p = (float*)c.p; const float* const g = (const float*)c.g; float* const buf = (float*)c.state[0];
    const float* const hyper = (const float*)c.hyper;
    if constexpr (FORM == STEP_SEG) hipLaunchKernelGGL((sgd_seg_kernel<MOM, WD>), grid, block, 0, stream, p, g, buf, c.n, hyper, s, t);
    else hipLaunchKernelGGL((sgd_kernel<MOM, WD, FORM != STEP_HOST, FORM == STEP_CTL>), grid, block, 0, stream, p, g, buf, c.n, hyper,
                            step_scalars<FORM == STEP_CTL>(s, t.ctl));
}
template <StepForm FORM>
int sgd_step(const StepCall& c, const SgdScalars& s, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    const StepPlan pl = plan_sgd(c, FORM);
    if (pl.rc != MTE_OK) return pl.rc;
    const SegArgs t = {(const uint8_t*)c.cls, (const float*)c.scales, (const float*)c.ctl, c.n_classes};
    switch (2 * pl.mom + (pl.wd != WD_NONE)) {
    case 2 * MOM_NONE: sgd_launch<FORM, MOM_NONE, false>(pl, c, s, t, stream); break;
    case 2 * MOM_NONE + 1: sgd_launch<FORM, MOM_NONE, true>(pl, c, s, t, stream); break;
    case 2 * MOM_PLAIN: sgd_launch<FORM, MOM_PLAIN, false>(pl, c, s, t, stream); break;
    case 2 * MOM_PLAIN + 1: sgd_launch<FORM, MOM_PLAIN, true>(pl, c, s, t, stream); break;
    case 2 * MOM_NESTEROV: sgd_launch<FORM, MOM_NESTEROV, false>(pl, c, s, t, stream); break;
    default: sgd_launch<FORM, MOM_NESTEROV, true>(pl, c, s, t, stream); break;
    }
    return mte_check_launch();
}

// what every form of a step passes; a form's own arguments (hyper, ctl, step, dampening, the class tables) are set by name at the entry point
inline StepCall adam_call(const void* p, const void* g, const void* m, const void* v, long n, float weight_decay, int decoupled) {
    StepCall c = {};
    c.p = p; c.g = g; c.state[0] = m; c.state[1] = v; c.n = n; c.weight_decay = weight_decay; c.decoupled = decoupled;
    return c;
}
inline StepCall sgd_call(const void* p, const void* g, const void* buf, long n, float momentum, float weight_decay, int nesterov) {
    StepCall c = {};
    c.p = p; c.g = g; c.state[0] = buf; c.n = n; c.momentum = momentum; c.weight_decay = weight_decay; c.nesterov = nesterov;
    return c;
}
inline ChunkCall chunk_call(const void* p, long n, const void* seg_begin, const void* seg_numel, int T) {
    ChunkCall c = {};
    c.p = p; c.n = n; c.begin = seg_begin; c.numel = seg_numel; c.T = T;
    return c;
}

// the flat-pair launches: `launch(grid, block)` with the plan's shape, unless the plan says error or nothing to do
template <class Launch>
int pair_step(const PairPlan& pl, Launch launch) {
    if (pl.rc != MTE_OK || !pl.launch) return pl.rc;
    launch(dim3(pl.grid), dim3(pl.block));
    return mte_check_launch();
}

}  // namespace

extern "C" {

// Exponential moving average over flat fp32 buffers (16-byte aligned, disjoint): ema[i] = d * ema[i] + omd * p[i], three fp32 roundings in
// that order; p is only read.  n = 0 launches nothing.  n < 0, a null or misaligned pointer and overlapping ranges (equal pointers
// included) are MTE_ERR_ARG.
int mte_ema_update(float* ema, const float* p, long n, float d, float omd, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    return pair_step(plan_pair(ema, p, n), [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(ema_update_kernel<false>, grid, block, 0, stream, ema, p, n, d, omd, (const float*)nullptr, (const float*)nullptr);
    });
}

// The same update with scal = {d, omd} in DEVICE memory (the launch is identical every step: it replays from a captured graph).  ctl may be
// null; otherwise it is mte_grad_norm_clip's word, and with ctl[1] != 0 nothing is loaded or stored.  A null scal is MTE_ERR_ARG.
int mte_ema_update_dev(float* ema, const float* p, long n, const float* scal, const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    return pair_step(plan_pair(ema, p, n, scal != nullptr), [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(ema_update_kernel<true>, grid, block, 0, stream, ema, p, n, 0.f, 0.f, scal, ctl);
    });
}

// Exchange two flat fp32 buffers (16-byte aligned, disjoint) bit for bit in one launch; the argument rules of mte_ema_update.
int mte_flat_swap(float* a, float* b, long n, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    return pair_step(plan_pair(a, b, n), [&](dim3 grid, dim3 block) {
        hipLaunchKernelGGL(flat_swap_kernel, grid, block, 0, stream, (uint32_t*)a, (uint32_t*)b, n);
    });
}

// Gradient accumulation over flat fp32 buffers (16-byte aligned, disjoint): assign = 0 adds src into dst, dst[i] = dst[i] + src[i] with one
// fp32 rounding; assign = 1 copies src's bits.  The argument rules of mte_ema_update.
int mte_grad_accumulate(float* dst, const float* src, long n, int assign, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    return pair_step(plan_pair(dst, src, n), [&](dim3 grid, dim3 block) {
        if (assign) hipLaunchKernelGGL(grad_accumulate_kernel<true>, grid, block, 0, stream, dst, src, n);
        else hipLaunchKernelGGL(grad_accumulate_kernel<false>, grid, block, 0, stream, dst, src, n);
    });
}

// Bytes of `work` for mte_grad_norm_clip over n elements (16-byte aligned, zeroed ONCE by the caller): norm_layout.
long mte_grad_norm_work_bytes(long n) { return grad_norm_work_bytes(n); }

// Global L2 norm of the flat gradient g[0..n) (16-byte aligned) in one launch and a fixed order, and what a clipped / guarded step needs:
//   S = sum g^2 in fp64 (also in the first 8 bytes of `work`), norm = |gscale| * sqrt(S)
//   ctl[0] = min(max_norm / (norm + 1e-6), 1) as torch.nn.utils.clip_grad_norm_ forms it (max_norm = +inf gives exactly 1; NaN stays NaN)
//   ctl[1] = 1 if skip_nonfinite and S is not finite, else 0;   ctl[2] = norm;   ctl[3] += 1 when ctl[1] is set (never reset here)
// The launch is identical every step and leaves the ticket at zero: it replays from a captured graph.
int mte_grad_norm_clip(const float* g, long n, float gscale, float max_norm, int skip_nonfinite, void* work, float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    const NormPlan pl = plan_norm(g, n, max_norm, work, ctl);
    if (pl.rc != MTE_OK) return pl.rc;
    char* const w = (char*)work;
    NormArgs a;
    a.g = g; a.n = n; a.gscale = gscale; a.max_norm = max_norm; a.skip_nonfinite = skip_nonfinite != 0; a.fences = g_mte_handoff_fences;
    a.sum = (double*)(w + pl.work.sum); a.ticket = (unsigned*)(w + pl.work.ticket); a.records = (double*)(w + pl.work.records); a.ctl = ctl;
    hipLaunchKernelGGL(grad_norm_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, a);
    return mte_check_launch();
}

// In-place Adam with weight decay over flat fp32 buffers (16-byte aligned).  decoupled = 0: torch.optim.Adam(weight_decay) (L2, added to
// the gradient), decoupled = 1: torch.optim.AdamW.  weight_decay = 0 is mte_adam_step's update bit for bit.  step >= 1; gscale multiplies
// the gradient first.
int mte_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int decoupled, int step, float gscale, hipStream_t stream) {
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    StepCall c = adam_call(p, g, m, v, n, weight_decay, decoupled);
    c.step = step;
    return adam_step<STEP_HOST>(c, {lr, (float)bc1, (float)sqrt(bc2), beta1, beta2, eps, gscale, weight_decay}, stream);
}

// The same step with hyper = {lr, 1 - beta1^t, sqrt(1 - beta2^t)} in DEVICE memory, as mte_adam_step_dev: lr * weight_decay is formed in
// the kernel from hyper[0].
int mte_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                       float weight_decay, int decoupled, float gscale, hipStream_t stream) {
    StepCall c = adam_call(p, g, m, v, n, weight_decay, decoupled);
    c.hyper = hyper;
    return adam_step<STEP_DEV>(c, {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay}, stream);
}

// In-place torch.optim.SGD over flat fp32 buffers (16-byte aligned).  momentum = 0: `buf` is neither read nor written and may be null.
// With momentum, `buf` is zero-initialised by the caller before step 1.  Nesterov needs momentum > 0 and dampening = 0, as torch.
int mte_sgd_step(float* p, const float* g, float* buf, long n, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                 int step, float gscale, hipStream_t stream) {
    StepCall c = sgd_call(p, g, buf, n, momentum, weight_decay, nesterov);
    c.step = step; c.dampening = dampening;
    const SgdScalars s = {lr, step == 1 ? 0.f : momentum, step == 1 ? 1.f : (float)(1.0 - (double)dampening), momentum, gscale, weight_decay};
    return sgd_step<STEP_HOST>(c, s, stream);
}

// The same step with hyper = {lr, mu_eff, (1 - dampening)_eff} in DEVICE memory: {lr, 0, 1} at step 1, {lr, momentum, 1 - dampening}
// afterwards.  `momentum` is the launch constant that selects the kernel and feeds Nesterov's look-ahead.
int mte_sgd_step_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                     float gscale, hipStream_t stream) {
    StepCall c = sgd_call(p, g, buf, n, momentum, weight_decay, nesterov);
    c.hyper = hyper;
    return sgd_step<STEP_DEV>(c, {0.f, 0.f, 0.f, momentum, gscale, weight_decay}, stream);
}

// mte_adamw_step_dev / mte_sgd_step_dev with ctl = {clip coefficient, skip flag, ...} in DEVICE memory (mte_grad_norm_clip writes it):
// the gradient scale is float32(gscale * ctl[0]); with ctl[1] != 0 nothing is loaded or stored.  weight_decay = 0 is the Adam step.
int mte_adamw_step_ctl_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                           float weight_decay, int decoupled, float gscale, const float* ctl, hipStream_t stream) {
    StepCall c = adam_call(p, g, m, v, n, weight_decay, decoupled);
    c.hyper = hyper; c.ctl = ctl;
    return adam_step<STEP_CTL>(c, {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay}, stream);
}

int mte_sgd_step_ctl_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                         float gscale, const float* ctl, hipStream_t stream) {
    StepCall c = sgd_call(p, g, buf, n, momentum, weight_decay, nesterov);
    c.hyper = hyper; c.ctl = ctl;
    return sgd_step<STEP_CTL>(c, {0.f, 0.f, 0.f, momentum, gscale, weight_decay}, stream);
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
    StepCall c = adam_call(p, g, m, v, n, weight_decay, decoupled);
    c.hyper = hyper; c.ctl = ctl; c.cls = block_class; c.scales = class_scales; c.n_classes = n_classes;
    return adam_step<STEP_SEG>(c, {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay}, stream);
}

int mte_sgd_step_seg_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                         float gscale, const uint8_t* block_class, const float* class_scales, int n_classes, const float* ctl,
                         hipStream_t stream) {
    StepCall c = sgd_call(p, g, buf, n, momentum, weight_decay, nesterov);
    c.hyper = hyper; c.ctl = ctl; c.cls = block_class; c.scales = class_scales; c.n_classes = n_classes;
    return sgd_step<STEP_SEG>(c, {0.f, 0.f, 0.f, momentum, gscale, weight_decay}, stream);
}

// Bytes of `work` for mte_tensor_stats over T tensors inside n flat elements (16-byte aligned, zeroed ONCE by the caller): chunk_layout with
// records of four fp64 values.  0 for n <= 0 or T outside 1..4096.
long mte_tensor_stats_work_bytes(long n, int T) { return tensor_stats_work_bytes(n, T); }

// Per-tensor statistics of the flat gradient g[0..n) and, with p non-null, of the weights p[0..n) (both 16-byte aligned; read-only) in ONE
// launch: tensor t is elements seg_begin[t] .. seg_begin[t] + seg_numel[t] - 1 (`long` arrays in DEVICE memory; begins are multiples of
// 64, ranges disjoint and inside [0, n)), out[4 t ..] = {sum g^2, max |g| over the finite elements, count of non-finite elements,
// sum p^2 (0 without p)} as fp64 in DEVICE memory.  The order of every addition is fixed by the table (see the kernel): bit-equal call
// to call and under graph replay; the tickets in `work` go back to zero.  A range that leaves [0, n) reads nothing and reports zeros.
int mte_tensor_stats(const float* g, const float* p, long n, const long* seg_begin, const long* seg_numel, int T, void* work, double* out,
                     hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    ChunkCall c = chunk_call(p, n, seg_begin, seg_numel, T);
    c.g = g; c.work = work; c.out = out;
    const ChunkPlan pl = plan_chunks(c, WITH_G | WITH_WORK | WITH_OUT, STAT_VALUES);
    if (pl.rc != MTE_OK) return pl.rc;
    StatArgs a;
    a.g = g; a.p = p; a.n = n; a.begin = seg_begin; a.numel = seg_numel; a.T = T; a.fences = g_mte_handoff_fences;
    a.max_chunks = pl.max_chunks;
    a.tickets = (unsigned*)((char*)work + pl.work.tickets); a.records = (double*)((char*)work + pl.work.records); a.out = out;
    const dim3 grid(pl.grid), block(pl.block);
    if (pl.has_p) hipLaunchKernelGGL(tensor_stats_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(tensor_stats_kernel<false>, grid, block, 0, stream, a);
    return mte_check_launch();
}

// Bytes of `work` for mte_lamb_moments over T tensors inside n flat elements (16-byte aligned, zeroed ONCE by the caller): chunk_layout with
// records {S_p, S_d} of two fp64 values.  0 for n <= 0 or T outside 1..4096.
long mte_lamb_work_bytes(long n, int T) { return lamb_work_bytes(n, T); }

// The first launch of the LAMB step (see lamb_moments_kernel): m and v move as in mte_adamw_step_dev (decoupled), p is only read, and
// trust[t] = q_t, sums[2 t ..] = {S_p, S_d} are left for every tensor of the table {seg_begin, seg_numel, tensor_table} (DEVICE memory).
// p, g, m, v and work are 16-byte aligned.  ctl may be null.  A range that leaves [0, n) reads and writes nothing in the flat buffers
// (its trust is 1, its sums are 0).
int mte_lamb_moments(const float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                     float weight_decay, float gscale, float max_trust, const long* seg_begin, const long* seg_numel, const float* tensor_table,
                     int T, void* work, float* trust, double* sums, const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    ChunkCall c = chunk_call(p, n, seg_begin, seg_numel, T);
    c.g = g; c.m = m; c.v = v; c.hyper = hyper; c.table = tensor_table; c.weight_decay = weight_decay;
    c.work = work; c.trust = trust; c.sums = sums; c.max_trust = max_trust;
    const ChunkPlan pl = plan_chunks(c, WITH_P | WITH_G | WITH_MV | WITH_HYPER | WITH_WORK | WITH_TRUST | WITH_SUMS, LAMB_VALUES);
    if (pl.rc != MTE_OK) return pl.rc;
    LambArgs a;
    a.p = const_cast<float*>(p); a.g = g; a.m = m; a.v = v; a.n = n; a.hyper = hyper; a.ctl = ctl;
    a.s = {0.f, 0.f, 0.f, beta1, beta2, eps, gscale, weight_decay};
    a.max_trust = max_trust;
    a.begin = seg_begin; a.numel = seg_numel; a.table = tensor_table; a.T = T; a.fences = g_mte_handoff_fences;
    a.max_chunks = pl.max_chunks;
    a.tickets = (unsigned*)((char*)work + pl.work.tickets); a.records = (double*)((char*)work + pl.work.records); a.trust = trust; a.sums = sums;
    hipLaunchKernelGGL(lamb_moments_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, a);
    return mte_check_launch();
}

// The second launch (see lamb_apply_kernel): p = p - trust[t] * d with d formed again from the stored m and v; m, v and trust are only
// read.  The same table, hyper, eps, weight_decay and ctl as the mte_lamb_moments launch in front of it.
int mte_lamb_apply(float* p, const float* m, const float* v, long n, const float* hyper, float eps, float weight_decay, const long* seg_begin,
                   const long* seg_numel, const float* tensor_table, int T, const float* trust, const float* ctl, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    ChunkCall c = chunk_call(p, n, seg_begin, seg_numel, T);
    c.m = m; c.v = v; c.hyper = hyper; c.table = tensor_table; c.weight_decay = weight_decay; c.trust = trust;
    const ChunkPlan pl = plan_chunks(c, WITH_P | WITH_MV | WITH_HYPER | WITH_TRUST, LAMB_VALUES);
    if (pl.rc != MTE_OK) return pl.rc;
    LambArgs a;
    a.p = p; a.g = nullptr; a.m = const_cast<float*>(m); a.v = const_cast<float*>(v); a.n = n; a.hyper = hyper; a.ctl = ctl;
    a.s = {0.f, 0.f, 0.f, 0.f, 0.f, eps, 1.f, weight_decay};
    a.max_trust = 0.f;
    a.begin = seg_begin; a.numel = seg_numel; a.table = tensor_table; a.T = T; a.fences = 0;
    a.max_chunks = pl.max_chunks;
    a.tickets = nullptr; a.records = nullptr; a.trust = const_cast<float*>(trust); a.sums = nullptr;
    hipLaunchKernelGGL(lamb_apply_kernel, dim3(pl.grid), dim3(pl.block), 0, stream, a);
    return mte_check_launch();
}

}  // extern "C"
