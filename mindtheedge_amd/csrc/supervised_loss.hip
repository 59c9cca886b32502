// Supervised losses of SupervisedLoss (packnet_sfm/losses/supervised_loss.py:13-216) over up to four scales, fp32 NCHW maps with C = 1,
// and the nearest upsample of SfmModel's upsample_depth_maps (SfmModel.py:92-94, model_utils.py:154-176).
//
//   x_s = pred_s + 1e-5,  y_s = depth2inv(depth) at the nearest source pixel of scale s (utils/image.py:122-220, match_scales 'nearest'):
//   y = d > 0 ? 1 / max(d, 1e-6) : 0 (correctly rounded division), src = min(floorf(dst * ((float)in / out)), in - 1), identity when the
//   sizes are equal.  Sparse methods keep the pixels with y > 0, dense ones keep every pixel.  loss = sum_s f(x_s, y_s) / n with, per scale,
//   a mean over the kept pixels:
//     method 0 l1       mean |x - y|
//     method 1 mse      mean (x - y)^2
//     method 2 berhu    c = 0.2f * max(x - y) (signed max, no gradient), D = |x - y|:  (sum D + sum_{D > c} D^2) / (N + N2)
//     method 3 silog    10 sqrt(mean l^2 - 0.85 (mean l)^2),  l = log(10 x) - log(10 y)
//     method 4 abs_rel  mean |x - y| / x
//   An empty sparse scale gives NaN (the mean of an empty tensor) and a zero gradient.  Method ids follow the order in which the
//   reference tests the suffixes (get_loss_func, supervised_loss.py:73-87).
//
// Layout: a workgroup is one (scale, CHUNK-pixel slice of the scale's [B,H,W] plane); a thread owns 4 consecutive pixels per pass
// (16-byte prediction loads when W % 4 == 0), PASSES passes.  The ground truth is gathered at the nearest source index.
//
// Sums: fp32 per thread and per wave, fp64 per workgroup record.  The last workgroup of the launch to arrive (handoff.hpp) reduces
// the records of each scale in a fixed order and writes the loss, the per-scale values and the backward coefficients.  No floating-point
// atomics and no host sync; each forward call clears its tickets with a fill kernel, so the launches can be captured in a graph and the
// results are bit-reproducible.  BerHu takes two launches: A gives N, sum D and max(x - y), its last workgroup writes c; B reads c from
// device memory and sums N2 and D^2 over D > c.
//
// The nearest upsample (integer ratios only) writes the full-resolution maps; its backward gathers each r x r block in row-major order, as
// torch's CPU backward accumulates it, with no atomics.  One launch covers every map.
#include "common.hpp"
#include "handoff.hpp"

namespace {

constexpr int NT = 256;                 // threads per workgroup
constexpr int PASSES = 4;               // 4-pixel groups per thread
constexpr int CHUNK = NT * 4 * PASSES;  // pixels per workgroup
constexpr int REC = 4;                  // doubles per workgroup record: count, sum 1, sum 2, max
constexpr int MAXS = 4;                 // scales per launch
constexpr int NCOEF = 4;                // floats of backward coefficients per scale: k0, k1, c, unused
constexpr int RES = 4;                  // doubles of per-scale results kept between the two BerHu launches: N, sum D

enum { M_L1 = 0, M_MSE = 1, M_BERHU = 2, M_SILOG = 3, M_ABSREL = 4 };

struct SupScale { const float* pred; float* dpred; int H; int W; };   // mte_sup_scale of include/mte_kernels.h
struct UpMap { const float* src; float* dst; int h; int w; };         // mte_upsample_map of include/mte_kernels.h

struct SupArgs {
    const float* pred[MAXS];
    float* dpred[MAXS];
    int H[MAXS], W[MAXS], vec[MAXS];
    float sy[MAXS], sx[MAXS];            // nearest scales (float)Hd / H, (float)Wd / W
    int first[MAXS + 1];                 // first workgroup of each scale
    const float* depth;                  // metric depth [B,1,Hd,Wd]
    int Hd, Wd, B, n, method, sparse;
    int pass;                            // 0: the loss (BerHu: launch A), 1: BerHu launch B
    int fences;                          // MTE_OPT_HANDOFF_FENCES (handoff.hpp)
    unsigned* ticket;                    // this launch's arrival ticket (zeroed by the launcher)
    double* res;                         // [MAXS][RES] BerHu: launch A -> launch B
    double* records;                     // [blocks][REC]
    float* loss;                         // forward out: the loss scalar
    float* scale_loss;                   // forward out (nullable): the per-scale values
    float* coef;                         // forward out / backward in: [MAXS][NCOEF]
    const float* gout;                   // backward: upstream gradient of the loss (device, nullable = 1)
};

__device__ __forceinline__ int nearest_src(int dst, int in, int out, float scale) {
    if (in == out) return dst;
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}
// depth2inv (utils/depth.py): 1 / clamp(d, 1e-6), 0 where d <= 0.  `/` is the correctly rounded division (hipcc's default for fp32).
__device__ __forceinline__ float depth2inv(float d) { return d > 0.f ? 1.f / fmaxf(d, 1e-6f) : 0.f; }
__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// flat index q of a [B,H,W] plane (< 2^31, checked by the launchers) -> (b, y, x) in 32-bit arithmetic
__device__ __forceinline__ void pixel_of(long q, int H, int W, int& b, int& y, int& x) {
    const unsigned u = (unsigned)q, plane = (unsigned)H * (unsigned)W;
    b = (int)(u / plane);
    const unsigned r = u - (unsigned)b * plane;
    y = (int)(r / (unsigned)W);
    x = (int)(r - (unsigned)y * (unsigned)W);
}

// workgroup -> (scale, first pixel of its slice)
__device__ __forceinline__ void locate(const SupArgs& a, int& s, long& q0) {
    s = 0;
#pragma unroll
    for (int k = 1; k < MAXS; ++k) if (k < a.n && (int)blockIdx.x >= a.first[k]) s = k;
    q0 = (long)(blockIdx.x - a.first[s]) * CHUNK;
}

// the 4-pixel group at flat index q of scale s: prediction, ground truth (inverse depth) and whether each pixel is in range
struct Group { f32x4_t p, y; int ok[4]; };
__device__ __forceinline__ void load_group(const SupArgs& a, int s, long q, Group& g) {
    const int H = a.H[s], W = a.W[s];
    const long total = (long)a.B * H * W;
    const float* pred = a.pred[s];
    if (a.vec[s]) {                                          // W % 4 == 0: the 4 pixels share a row
        const bool ok = q < total;
        g.p = ok ? *(const f32x4_t*)(pred + q) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        int b = 0, y = 0, x = 0;
        if (ok) pixel_of(q, H, W, b, y, x);
        const float* drow = a.depth + ((long)b * a.Hd + nearest_src(y, a.Hd, H, a.sy[s])) * a.Wd;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            g.ok[k] = ok;
            g.y[k] = ok ? depth2inv(drow[nearest_src(x + k, a.Wd, W, a.sx[s])]) : 0.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long qk = q + k;
            g.ok[k] = qk < total;
            g.p[k] = 0.f; g.y[k] = 0.f;
            if (g.ok[k]) {
                int b, y, x;
                pixel_of(qk, H, W, b, y, x);
                g.p[k] = pred[qk];
                g.y[k] = depth2inv(a.depth[((long)b * a.Hd + nearest_src(y, a.Hd, H, a.sy[s])) * a.Wd + nearest_src(x, a.Wd, W, a.sx[s])]);
            }
        }
    }
}

// ---- forward --------------------------------------------------------------------------------------------------------------------------
// per-pixel sums (slot 0 count, 1, 2, 3 max):
//   l1 |d|;  mse d^2;  abs_rel |d| / x;  silog l, l^2;  berhu A |d|, max d;  berhu B count(D > c), D^2 over D > c (slot 0 = N2)
__device__ __forceinline__ void per_pixel(const SupArgs& a, float c, float p, float yv, float acc[4]) {
    const float x = p + 1e-5f;
    const float d = x - yv;                                  // fp32, no contraction (-ffp-contract=off): the mask D > c matches torch
    const float D = fabsf(d);
    switch (a.method) {
        case M_L1: acc[0] += 1.f; acc[1] += D; break;
        case M_MSE: acc[0] += 1.f; acc[1] += d * d; break;
        case M_ABSREL: acc[0] += 1.f; acc[1] += D / x; break;
        case M_SILOG: {
            const float l = logf(x * 10.f) - logf(yv * 10.f);
            acc[0] += 1.f; acc[1] += l; acc[2] += l * l;
            break;
        }
        default:
            if (a.pass == 0) { acc[0] += 1.f; acc[1] += D; acc[3] = fmaxf(acc[3], d); }
            else if (D > c) { acc[0] += 1.f; acc[2] += D * D; }
            break;
    }
}

// scale s of the loss from its reduced sums T (count, sum 1, sum 2, max); writes the coefficients.  -> the scale's value
__device__ double finish_scale(const SupArgs& a, int s, const double T[REC]) {
    float* co = a.coef + s * NCOEF;
    const double n = a.n;
    switch (a.method) {
        case M_L1: case M_ABSREL: {
            const double N = T[0];
            co[0] = (float)(1.0 / (n * N)); co[1] = 0.f;
            return T[1] / N;
        }
        case M_MSE: {
            const double N = T[0];
            co[0] = (float)(2.0 / (n * N)); co[1] = 0.f;
            return T[1] / N;
        }
        case M_SILOG: {
            const double N = T[0], M = T[1] / N, S = T[2] / N - 0.85 * M * M;
            co[0] = (float)(10.0 / (sqrt(S) * N * n)); co[1] = (float)(0.85 * M);
            return 10.0 * sqrt(S);
        }
        default: {                                           // BerHu, launch B: T = (N2, -, sum D^2 over D > c, -)
            const double N = a.res[s * RES], SD = a.res[s * RES + 1];
            const double N2 = T[0];
            co[0] = (float)(1.0 / (n * (N + N2))); co[1] = 0.f;
            return (SD + T[2]) / (N + N2);
        }
    }
}

__global__ __launch_bounds__(NT) void sup_fwd_kernel(SupArgs a) {
    __shared__ float sred[NT / 64][REC];
    __shared__ double sd[REC][NT];
    __shared__ double stot[MAXS][REC];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int s; long q0;
    locate(a, s, q0);
    const float c = (a.method == M_BERHU && a.pass == 1) ? a.coef[s * NCOEF + 2] : 0.f;

    float acc[REC] = {0.f, 0.f, 0.f, -INFINITY};
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        Group g;
        load_group(a, s, q0 + (long)ps * NT * 4 + tid * 4, g);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (g.ok[k] && (!a.sparse || g.y[k] > 0.f)) per_pixel(a, c, g.p[k], g.y[k], acc);
    }
#pragma unroll
    for (int v = 0; v < REC; ++v) {
        const float r = v == 3 ? wave_max(acc[v]) : wave_sum(acc[v]);
        if (lane == 0) sred[wave][v] = r;
    }
    __syncthreads();
    if (tid < REC) {
        double v;
        if (tid == 3) v = (double)fmaxf(fmaxf(sred[0][3], sred[1][3]), fmaxf(sred[2][3], sred[3][3]));
        else v = (double)sred[0][tid] + (double)sred[1][tid] + (double)sred[2][tid] + (double)sred[3][tid];
        handoff::publish(a.records + (long)blockIdx.x * REC + tid, v);
    }
    if (!handoff::arrive([&] { return a.ticket; }, [&] { return a.first[a.n]; }, a.fences, a.fences, &s_last)) return;

    // last workgroup: per scale, thread t adds records t, t + 256, ... then a fixed-order tree over the 256 partials
    for (int sc = 0; sc < a.n; ++sc) {
        double part[REC] = {0.0, 0.0, 0.0, -INFINITY};
        for (int j = a.first[sc] + tid; j < a.first[sc + 1]; j += NT) {
            const double* rec = a.records + (long)j * REC;
#pragma unroll
            for (int v = 0; v < 3; ++v) part[v] += handoff::read(rec + v);
            part[3] = fmax(part[3], handoff::read(rec + 3));
        }
#pragma unroll
        for (int v = 0; v < REC; ++v) sd[v][tid] = part[v];
        __syncthreads();
        for (int st = NT / 2; st > 0; st >>= 1) {
            if (tid < st) {
#pragma unroll
                for (int v = 0; v < 3; ++v) sd[v][tid] += sd[v][tid + st];
                sd[3][tid] = fmax(sd[3][tid], sd[3][tid + st]);
            }
            __syncthreads();
        }
        if (tid < REC) stot[sc][tid] = sd[tid][0];
        __syncthreads();
    }
    if (tid != 0) return;
    if (a.method == M_BERHU && a.pass == 0) {                // launch A: keep N and sum D, publish c for launch B
        for (int sc = 0; sc < a.n; ++sc) {
            a.res[sc * RES] = stot[sc][0];
            a.res[sc * RES + 1] = stot[sc][1];
            a.coef[sc * NCOEF + 2] = 0.2f * (float)stot[sc][3];      // torch: max (fp32) * 0.2 in fp32
        }
        return;
    }
    double total = 0.0;
    for (int sc = 0; sc < a.n; ++sc) {
        const double v = finish_scale(a, sc, stot[sc]);
        if (a.scale_loss) a.scale_loss[sc] = (float)v;
        total += v;
    }
    *a.loss = (float)(total / a.n);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void sup_bwd_kernel(SupArgs a) {
    const int tid = threadIdx.x;
    int s; long q0;
    locate(a, s, q0);
    const float go = a.gout ? a.gout[0] : 1.f;
    const float* co = a.coef + s * NCOEF;
    const float k0 = co[0] * go, k1 = co[1], c = co[2];
    const int H = a.H[s], W = a.W[s];
    const long total = (long)a.B * H * W;
    float* dpred = a.dpred[s];
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const long q = q0 + (long)ps * NT * 4 + tid * 4;
        if (q >= total) break;
        Group g;
        load_group(a, s, q, g);
        f32x4_t out;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float r = 0.f;
            if (g.ok[k] && (!a.sparse || g.y[k] > 0.f)) {
                const float x = g.p[k] + 1e-5f, d = x - g.y[k], D = fabsf(d);
                switch (a.method) {
                    case M_L1: r = k0 * sgn(d); break;
                    case M_MSE: r = k0 * d; break;
                    case M_ABSREL: r = k0 / x * sgn(d) - k0 * (D / x / x); break;
                    case M_SILOG: r = k0 * (logf(x * 10.f) - logf(g.y[k] * 10.f) - k1) / x; break;
                    default: r = k0 * sgn(d) * (D > c ? 1.f + 2.f * D : 1.f); break;
                }
            }
            out[k] = r;
        }
        if (a.vec[s]) *(f32x4_t*)(dpred + q) = out;
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (g.ok[k]) dpred[q + k] = out[k];
        }
    }
}

// ---- nearest upsample -----------------------------------------------------------------------------------------------------------------
constexpr int MAXU = 4;
struct UpArgs {
    const float* src[MAXU];
    float* dst[MAXU];
    int h[MAXU], w[MAXU];
    float sy[MAXU], sx[MAXU];            // (float)h / H, (float)w / W
    int first[MAXU + 1];
    int n, B, H, W, vec;
};

// forward: dst [B,H,W] <- src [B,h,w] at the nearest source pixel; a thread writes 4 consecutive output pixels
__global__ __launch_bounds__(NT) void up_fwd_kernel(UpArgs a) {
    int m = 0;
#pragma unroll
    for (int k = 1; k < MAXU; ++k) if (k < a.n && (int)blockIdx.x >= a.first[k]) m = k;
    const long q = ((long)(blockIdx.x - a.first[m]) * NT + threadIdx.x) * 4;
    const long plane = (long)a.H * a.W, total = (long)a.B * plane;
    if (q >= total) return;
    const int h = a.h[m], w = a.w[m];
    const float* src = a.src[m];
    float* dst = a.dst[m];
    if (a.vec) {
        int b, y, x;
        pixel_of(q, a.H, a.W, b, y, x);
        const float* row = src + ((long)b * h + nearest_src(y, h, a.H, a.sy[m])) * w;
        f32x4_t v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = row[nearest_src(x + k, w, a.W, a.sx[m])];
        *(f32x4_t*)(dst + q) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long qk = q + k;
            if (qk >= total) break;
            int b, y, x;
            pixel_of(qk, a.H, a.W, b, y, x);
            dst[qk] = src[((long)b * h + nearest_src(y, h, a.H, a.sy[m])) * w + nearest_src(x, w, a.W, a.sx[m])];
        }
    }
}

// backward: dsrc [B,h,w] <- sum of ddst [B,H,W] over the output pixels whose nearest source it is.  Integer ratios rh = H / h, rw = W / w:
// the candidates of source row i are rows i rh - 1 .. i rh + rh (the float scale can move a boundary by one), tested with the forward's
// own index function, summed row-major.  One thread per source pixel.
__global__ __launch_bounds__(NT) void up_bwd_kernel(UpArgs a) {
    int m = 0;
#pragma unroll
    for (int k = 1; k < MAXU; ++k) if (k < a.n && (int)blockIdx.x >= a.first[k]) m = k;
    const long q = (long)(blockIdx.x - a.first[m]) * NT + threadIdx.x;
    const int h = a.h[m], w = a.w[m];
    if (q >= (long)a.B * h * w) return;
    int b, i, j;
    pixel_of(q, h, w, b, i, j);
    const int rh = a.H / h, rw = a.W / w;
    const float* g = a.src[m] + (long)b * a.H * a.W;
    float acc = 0.f;
    for (int y = i * rh - 1; y <= i * rh + rh; ++y) {
        if (y < 0 || y >= a.H || nearest_src(y, h, a.H, a.sy[m]) != i) continue;
        for (int x = j * rw - 1; x <= j * rw + rw; ++x) {
            if (x < 0 || x >= a.W || nearest_src(x, w, a.W, a.sx[m]) != j) continue;
            acc += g[(long)y * a.W + x];
        }
    }
    a.dst[m][q] = acc;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr long TICKET_ELEMS = 2;                               // doubles holding the two arrival tickets (16 bytes)
constexpr long RES_ELEMS = MAXS * RES;

// -> number of workgroups, or -1 for bad arguments
int setup(SupArgs& a, const void* scales, int n, int B, const float* depth, int Hd, int Wd, int method, int sparse) {
    if (!scales || !depth || n < 1 || n > MAXS || B < 1 || Hd < 1 || Wd < 1 || method < 0 || method > 4) return -1;
    if (method == M_BERHU && !sparse) return -1;               // dense BerHu fails in the reference (torch.cat of 4-D and 1-D)
    if ((long)B * Hd * Wd >= (1L << 31)) return -1;
    const SupScale* sc = (const SupScale*)scales;
    a.depth = depth; a.Hd = Hd; a.Wd = Wd; a.B = B; a.n = n; a.method = method; a.sparse = sparse != 0;
    a.fences = g_mte_handoff_fences;
    long blocks = 0;
    for (int s = 0; s < n; ++s) {
        const long px = (long)B * sc[s].H * sc[s].W;
        if (!sc[s].pred || sc[s].H < 1 || sc[s].W < 1 || px >= (1L << 31)) return -1;
        a.pred[s] = sc[s].pred; a.dpred[s] = sc[s].dpred; a.H[s] = sc[s].H; a.W[s] = sc[s].W;
        a.vec[s] = sc[s].W % 4 == 0 && aligned16(sc[s].pred) && aligned16(sc[s].dpred);
        a.sy[s] = (float)Hd / (float)sc[s].H;
        a.sx[s] = (float)Wd / (float)sc[s].W;
        a.first[s] = (int)blocks;
        blocks += (px + CHUNK - 1) / CHUNK;
    }
    for (int s = n; s <= MAXS; ++s) a.first[s] = (int)blocks;
    if (blocks >= (1L << 30)) return -1;
    return (int)blocks;
}

int setup_up(UpArgs& a, const void* maps, int n, int B, int H, int W) {
    if (!maps || n < 1 || n > MAXU || B < 1 || H < 1 || W < 1 || (long)B * H * W >= (1L << 31)) return -1;
    a.n = n; a.B = B; a.H = H; a.W = W;
    a.vec = W % 4 == 0;
    return 0;
}

}  // namespace

extern "C" {

// doubles of workspace of one forward call: two tickets, the BerHu hand-over and one record per workgroup
long mte_supervised_loss_work_elems(const void* scales, int nscales, int B) {
    if (!scales || nscales < 1 || nscales > MAXS || B < 1) return -1;
    const SupScale* sc = (const SupScale*)scales;
    long blocks = 0;
    for (int s = 0; s < nscales; ++s) {
        if (sc[s].H < 1 || sc[s].W < 1) return -1;
        blocks += ((long)B * sc[s].H * sc[s].W + CHUNK - 1) / CHUNK;
    }
    return TICKET_ELEMS + RES_ELEMS + blocks * REC;
}

// Forward of every scale.  *loss <- sum_s f(x_s, y_s) / n; scale_loss [n] (nullable) <- the per-scale values; coef [4 * NCOEF] <- backward
// coefficients.  BerHu (sparse only) runs two launches, every other method one.
int mte_supervised_loss_fwd(const void* scales, int nscales, int B, const float* depth, int Hd, int Wd, int method, int sparse,
                            double* work, float* loss, float* scale_loss, float* coef, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    SupArgs a{};
    const int blocks = setup(a, scales, nscales, B, depth, Hd, Wd, method, sparse);
    if (blocks < 0 || !work || !loss || !coef) return MTE_ERR_ARG;
    if (!aligned16(work)) return MTE_ERR_ARG;
    a.res = work + TICKET_ELEMS; a.records = work + TICKET_ELEMS + RES_ELEMS;
    a.loss = loss; a.scale_loss = scale_loss; a.coef = coef;
    if (mte_memset_async(work, 0, sizeof(double) * TICKET_ELEMS, stream) != hipSuccess) return MTE_ERR_LAUNCH;   // tickets (records are overwritten)
    a.ticket = (unsigned*)work;
    a.pass = 0;
    hipLaunchKernelGGL(sup_fwd_kernel, dim3(blocks), dim3(NT), 0, stream, a);
    if (method == M_BERHU) {
        a.ticket = (unsigned*)work + 1;
        a.pass = 1;
        hipLaunchKernelGGL(sup_fwd_kernel, dim3(blocks), dim3(NT), 0, stream, a);
    }
    return mte_check_launch();
}

// Backward of the same: every pixel of every dpred_s (scales[s].dpred) <- gout * d loss / d pred_s, exact zeros where the mask drops a pixel
int mte_supervised_loss_bwd(const void* scales, int nscales, int B, const float* depth, int Hd, int Wd, int method, int sparse,
                            const float* coef, const float* gout, hipStream_t stream) {
    (void)hipGetLastError();
    SupArgs a{};
    const int blocks = setup(a, scales, nscales, B, depth, Hd, Wd, method, sparse);
    if (blocks < 0 || !coef) return MTE_ERR_ARG;
    for (int s = 0; s < nscales; ++s) if (!a.dpred[s]) return MTE_ERR_ARG;
    a.coef = (float*)coef; a.gout = gout;
    hipLaunchKernelGGL(sup_bwd_kernel, dim3(blocks), dim3(NT), 0, stream, a);
    return mte_check_launch();
}

// maps[m].dst [B,H,W] <- nearest upsample of maps[m].src [B,h,w]; H % h == 0 and W % w == 0
int mte_upsample_nearest_fwd(const void* maps, int nmaps, int B, int H, int W, hipStream_t stream) {
    (void)hipGetLastError();
    UpArgs a{};
    if (setup_up(a, maps, nmaps, B, H, W) < 0) return MTE_ERR_ARG;
    const UpMap* mp = (const UpMap*)maps;
    long blocks = 0;
    const long per = ((long)B * H * W + NT * 4 - 1) / (NT * 4);
    for (int m = 0; m < nmaps; ++m) {
        if (!mp[m].src || !mp[m].dst || mp[m].h < 1 || mp[m].w < 1 || H % mp[m].h || W % mp[m].w) return MTE_ERR_ARG;
        a.src[m] = mp[m].src; a.dst[m] = mp[m].dst; a.h[m] = mp[m].h; a.w[m] = mp[m].w;
        a.sy[m] = (float)mp[m].h / (float)H; a.sx[m] = (float)mp[m].w / (float)W;
        if (!aligned16(mp[m].dst)) a.vec = 0;
        a.first[m] = (int)blocks;
        blocks += per;
    }
    for (int m = nmaps; m <= MAXU; ++m) a.first[m] = (int)blocks;
    hipLaunchKernelGGL(up_fwd_kernel, dim3((unsigned)blocks), dim3(NT), 0, stream, a);
    return mte_check_launch();
}

// maps[m].dst [B,h,w] <- adjoint of the upsample applied to maps[m].src [B,H,W] (the gradient of the full-resolution map)
int mte_upsample_nearest_bwd(const void* maps, int nmaps, int B, int H, int W, hipStream_t stream) {
    (void)hipGetLastError();
    UpArgs a{};
    if (setup_up(a, maps, nmaps, B, H, W) < 0) return MTE_ERR_ARG;
    const UpMap* mp = (const UpMap*)maps;
    long blocks = 0;
    for (int m = 0; m < nmaps; ++m) {
        if (!mp[m].src || !mp[m].dst || mp[m].h < 1 || mp[m].w < 1 || H % mp[m].h || W % mp[m].w) return MTE_ERR_ARG;
        a.src[m] = mp[m].src; a.dst[m] = mp[m].dst; a.h[m] = mp[m].h; a.w[m] = mp[m].w;
        a.sy[m] = (float)mp[m].h / (float)H; a.sx[m] = (float)mp[m].w / (float)W;
        a.first[m] = (int)blocks;
        blocks += ((long)B * mp[m].h * mp[m].w + NT - 1) / NT;
    }
    for (int m = nmaps; m <= MAXU; ++m) a.first[m] = (int)blocks;
    hipLaunchKernelGGL(up_bwd_kernel, dim3((unsigned)blocks), dim3(NT), 0, stream, a);
    return mte_check_launch();
}

}  // extern "C"
