// Two-branch fused depth-edge + silog loss for gfx950: the completion models (models/SemiSupEdgeCompletionModel.py) hold TWO predictions, the RGB
// one (branch 0) and the RGB+LiDAR one (branch 1), against the SAME labels.  This is the pair form of edge_fwd_fast_kernel / edge_bwd_fast_kernel of
// edge_loss.hip (read that file first: tile, Sobel, direction bins, transposed Sobel, record / ticket hand-off are described there):
//   * workgroup = one 64 x 32 tile of one (scale, sample); the labels (edge, normal, ground truth on scale 0) are loaded ONCE, into registers, and
//     serve both branches: forward 16 B/pixel (two single launches: 24), backward 16 B/pixel read + 8 written (two single launches: 24 + 8);
//   * forward: both predictions' tiles + halo are staged as depth in two LDS planes (2 x (TH + 2) x LS floats = 19,584 B);
//     backward: the two branches take turns on ONE set of planes (depth + A + B = 29,952 B, as the single kernel); every global load of both
//     branches is issued before the first plane is built, so the workgroup still pays one memory latency;
//   * a workgroup leaves one 128-byte record PER BRANCH (slot 2 * workgroup + branch); tickets are per (scale, sample) and per launch as in the
//     single kernel; the last arriver of an image adds both branches' records in the single kernel's order, the last of those finishes the
//     2 * nscales losses, both silog losses and the coefficients.  Last-arriver tickets only: no workgroup waits for another, no floating-point
//     atomics.  The tiling, the per-thread order, the record order and the finish arithmetic are those of the single launch, so a branch's numbers
//     do not depend on the other branch (tests/test_gpu_completion.py: coupling).
// Only the training configuration (`fast_config` of edge_loss.hip) is built; the entry points answer MTE_ERR_UNSUPPORTED for anything else and the
// caller makes two mte_edge_loss_multi_* calls.  The small per-pixel helpers below are copies of those next to the fast kernels in edge_loss.hip:
// that file's code objects stay as they are.
#include "common.hpp"
#include "edge_direction.hpp"
#include "edge_tile.hpp"
#include "handoff.hpp"

namespace {

constexpr int MAXS = 4;                 // scales per launch
constexpr int NP = 13;                  // sums per (branch, scale, sample), laid out as in edge_loss.hip: 0..3 edge sums, 10..12 silog sums (4..9: mask, unused)
constexpr int NBR = 2;                  // branches
constexpr int FWD_TILES_PER_WG = 3;     // as the single launch: the record count per image, and with it the order of every sum, is the same
constexpr int NRED = 11;                // wave sums of a workgroup: e, valid - e, silog count (label-only, shared) + per branch pos, neg, dl, dl^2

struct PairScale {
    const float* pred[NBR]; float* dpred[NBR];
    const float* edge; const float* normal;
    int H, W, tiles_x, tiles_y, first_block, groups;
};
struct PairArgs {
    PairScale s[MAXS];
    int nscales, B, nblocks, tiles_per_wg;
    float thresh, weight, pos_to_neg;
    double* results;                    // [NBR][nscales][B][NP]
    double* records;                    // [nblocks][NBR][REC]
    unsigned* counter;                  // [0] launch ticket, [1 + s*B + b] ticket of (scale, sample)
    float* losses;                      // [NBR][nscales]
    float* coef;                        // [NBR][nscales][2B + 1]
    const float* gout;                  // backward: [NBR][nscales], nullable = 1
    const float* gt_depth;
    float* silog_loss; float* silog_aux;          // [NBR], [NBR][2]
    const float* silog_gout;            // [NBR], nullable = 1
    int fences;
};

struct BlockId { int s, b, t0, t1; };
__device__ __forceinline__ BlockId decode_block(const PairArgs& a) {
    BlockId id;
    int s = 0;
#pragma unroll
    for (int k = 1; k < MAXS; ++k) if (k < a.nscales && (int)blockIdx.x >= a.s[k].first_block) s = k;
    const int r = blockIdx.x - a.s[s].first_block;
    const int g = r % a.s[s].groups, tiles = a.s[s].tiles_x * a.s[s].tiles_y;
    id.s = s; id.b = r / a.s[s].groups;
    id.t0 = g * a.tiles_per_wg; id.t1 = id.t0 + a.tiles_per_wg < tiles ? id.t0 + a.tiles_per_wg : tiles;
    return id;
}

struct OwnGroup { bool ok; long off; };                        // a thread's 4 pixels of one row: inside the image?  offset of the (clamped) group
__device__ __forceinline__ OwnGroup own_group(const PairScale& sc, int b, int gy, int gx) {
    OwnGroup g;
    g.ok = (unsigned)gy < (unsigned)sc.H && (unsigned)gx < (unsigned)sc.W;
    const int cy = min(max(gy, 0), sc.H - 1), cx = min(max(gx, 0), sc.W - 4);
    g.off = ((long)b * sc.H + cy) * sc.W + cx;
    return g;
}
__device__ __forceinline__ f32x4_t sel4(bool ok, const f32x4_t& v) { return f32x4_t{ok ? v[0] : 0.f, ok ? v[1] : 0.f, ok ? v[2] : 0.f, ok ? v[3] : 0.f}; }
__device__ __forceinline__ f32x4_t depth4(bool ok, const f32x4_t& inv) {
    return f32x4_t{ok ? rcp_newton(fmaxf(inv[0], 1e-6f)) : 0.f, ok ? rcp_newton(fmaxf(inv[1], 1e-6f)) : 0.f,
                   ok ? rcp_newton(fmaxf(inv[2], 1e-6f)) : 0.f, ok ? rcp_newton(fmaxf(inv[3], 1e-6f)) : 0.f};
}
__device__ __forceinline__ float directed_response(const float w[3][6], int k, const DirMasks& m) {
    float sh, sv, srl, slr;
    sobel4(w, k, sh, sv, srl, slr);
    float s = m.v ? sv : sh;
    s = m.k1 ? (m.neg ? slr : srl) : s;
    s = m.k3 ? (m.neg ? srl : slr) : s;
    return s;
}
constexpr float LOG2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;

// ---------------- forward -----------------------------------------------------------------------------------------

// the finish, in the last workgroup of the launch: the arithmetic of finalize_losses / sample_term / silog_finish of edge_loss.hip without a mask
// (nvalid = B H W), once per branch
template <typename V> __device__ __forceinline__ double wneg_total_of(const V& R0, long R, int B) {
    double t = 0.0;
    for (int b = 0; b < B; ++b) t += (double)(float)R0(R + b * NP + 1);
    return t;
}
template <typename V> __device__ __forceinline__ double sample_term(const PairArgs& a, const V& R0, long sums, double wneg_total, double nvalid, float* coef, int b) {
    const float wp = (float)R0(sums), wn = (float)R0(sums + 1);
    const float alpha = wneg_total == 0.0 ? 1.f : wn / (wp + wn);
    const double P = R0(sums + 2), N = R0(sums + 3);
    coef[2 * b] = (float)((double)a.weight * a.pos_to_neg * alpha / nvalid);
    coef[2 * b + 1] = (float)((double)a.weight * (1.f - alpha) / nvalid);
    return (double)a.pos_to_neg * alpha * P + (double)(1.f - alpha) * N;
}
template <typename V> __device__ __forceinline__ void silog_finish(const PairArgs& a, const V& R0, int br) {   // loss = 10 sqrt(E[d^2] - 0.85 E[d]^2);  aux = (mean, 10/sqrt(S)/n)
    const long R = (long)br * a.nscales * a.B * NP;             // scale 0 of the branch
    double ss[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < a.B; ++b)
        for (int k = 0; k < 3; ++k) ss[k] += R0(R + (long)b * NP + 10 + k);
    const double n1 = ss[2];
    const double m1 = ss[0] / n1, m2 = ss[1] / n1;
    const double S = m2 - 0.85 * m1 * m1;
    a.silog_loss[br] = (float)(sqrt(S) * 10.0);
    a.silog_aux[2 * br] = (float)m1; a.silog_aux[2 * br + 1] = (float)(10.0 / sqrt(S) / n1);
}
struct LdsView { const double* l; __device__ __forceinline__ double operator()(long i) const { return l[i]; } };
struct MemView { const double* g; __device__ __forceinline__ double operator()(long i) const { return handoff::read(g + i); } };

// stage: LDS for `stage_elems` doubles (the depth planes, dead by now).  images = NBR * nscales * B (64 at B = 8, twice the single launch's) fits
// up to B = 21; beyond that one thread works straight from memory.
__device__ void finalize_pair(const PairArgs& a, double* stage, int stage_elems) {
    const int tid = threadIdx.x;
    const int images = NBR * a.nscales * a.B, n = images * NP;
    if (n + images <= stage_elems) {
        __syncthreads();                                          // every wave is done with the planes
        for (int i = tid; i < n; i += 256) stage[i] = handoff::read(a.results + i);
        __syncthreads();
        const LdsView R0{stage};
        double* term = stage + n;
        for (int i = tid; i < images; i += 256) {                 // i = (br * nscales + s) * B + b
            const int q = i / a.B, b = i - q * a.B, s = q % a.nscales;
            const long R = (long)q * a.B * NP;
            const double nvalid = (double)a.B * a.s[s].H * a.s[s].W;
            float* coef = a.coef + (long)q * (2 * a.B + 1);
            term[i] = sample_term(a, R0, R + b * NP, wneg_total_of(R0, R, a.B), nvalid, coef, b);
            if (b == 0) coef[2 * a.B] = 0.f;                      // no mask: never the binary-mask form
        }
        if (a.gt_depth && tid >= 256 - NBR) silog_finish(a, R0, 255 - tid);     // another wave than the first threads
        __syncthreads();
        if (tid < NBR * a.nscales) {
            const int s = tid % a.nscales;
            const double nvalid = (double)a.B * a.s[s].H * a.s[s].W;
            double total = 0.0;
            for (int b = 0; b < a.B; ++b) total += term[tid * a.B + b];
            a.losses[tid] = (float)((double)a.weight * total / nvalid);
        }
        return;
    }
    if (tid != 0) return;                                         // very large batches: one thread, straight from memory
    const MemView R0{a.results};
    for (int q = 0; q < NBR * a.nscales; ++q) {
        const int s = q % a.nscales;
        const long R = (long)q * a.B * NP;
        const double nvalid = (double)a.B * a.s[s].H * a.s[s].W;
        const double wneg = wneg_total_of(R0, R, a.B);
        float* coef = a.coef + (long)q * (2 * a.B + 1);
        double total = 0.0;
        for (int b = 0; b < a.B; ++b) total += sample_term(a, R0, R + b * NP, wneg, nvalid, coef, b);
        coef[2 * a.B] = 0.f;
        a.losses[q] = (float)((double)a.weight * total / nvalid);
    }
    if (a.gt_depth)
        for (int br = 0; br < NBR; ++br) silog_finish(a, R0, br);
}

__global__ __launch_bounds__(256, 4) void edge_pair_fwd_kernel(PairArgs a) {
    __shared__ __attribute__((aligned(16))) float sd[NBR][(TH + 2) * LS];
    __shared__ float sred[4][NRED];
    __shared__ int s_last_store;
    const BlockId id = decode_block(a);
    const PairScale& sc = a.s[id.s];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = (tid & 15) * 4, r0 = tid >> 4;                   // this thread's 4 pixels: columns c..c+3 of rows r0 and r0 + 16
    const bool silog = a.gt_depth != nullptr && id.s == 0;
    const float tk = a.thresh * LOG2E;
    float acc_e = 0.f, acc_ne = 0.f, acc_cnt = 0.f;               // label-only sums: the same value goes into both branches' records
    float acc[NBR][4];                                            // pos, neg, silog dl, dl^2
#pragma unroll
    for (int br = 0; br < NBR; ++br)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[br][i] = 0.f;
    for (int t = id.t0; t < id.t1; ++t) {
        const int x0 = (t % sc.tiles_x) * TW, y0 = (t / sc.tiles_x) * TH;
        if (t != id.t0) __syncthreads();                          // the previous tile's window reads are done
        // ---- loads: own pixels (both inverse depths, label, normal, ground truth), then the halos of both depth tiles
        OwnGroup og[2];
        f32x4_t inv4[NBR][2], e4[2], n4[2], d4[2];
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            og[ps] = own_group(sc, id.b, y0 + r0 + 16 * ps, x0 + c);
#pragma unroll
            for (int br = 0; br < NBR; ++br) inv4[br][ps] = *(const f32x4_t*)(sc.pred[br] + og[ps].off);
            e4[ps] = *(const f32x4_t*)(sc.edge + og[ps].off);
            n4[ps] = *(const f32x4_t*)(sc.normal + og[ps].off);
            if (silog) d4[ps] = *(const f32x4_t*)(a.gt_depth + og[ps].off);
        }
        f32x4_t hrow[NBR]; bool hrow_ok = false;
        float hcol[NBR]; bool hcol_ok = false;
#pragma unroll
        for (int br = 0; br < NBR; ++br) { hrow[br] = f32x4_t{0.f, 0.f, 0.f, 0.f}; hcol[br] = 0.f; }
        if (tid < 32) {                                            // halo rows -1 and TH: 2 x 16 groups
            const OwnGroup g = own_group(sc, id.b, y0 + (tid >> 4 ? TH : -1), x0 + c);
#pragma unroll
            for (int br = 0; br < NBR; ++br) hrow[br] = *(const f32x4_t*)(sc.pred[br] + g.off);
            hrow_ok = g.ok;
        } else if (tid >= 64 && tid < 64 + 2 * (TH + 2)) {         // halo columns -1 and TW of rows -1 .. TH
            const int i = tid - 64, gy = y0 + (i >> 1) - 1, gx = x0 + (i & 1 ? TW : -1);
            hcol_ok = (unsigned)gy < (unsigned)sc.H && (unsigned)gx < (unsigned)sc.W;
            const long o = ((long)id.b * sc.H + min(max(gy, 0), sc.H - 1)) * sc.W + min(max(gx, 0), sc.W - 1);
#pragma unroll
            for (int br = 0; br < NBR; ++br) hcol[br] = sc.pred[br][o];
        }
        // ---- depth tiles
#pragma unroll
        for (int br = 0; br < NBR; ++br) {
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) *(f32x4_t*)(sd[br] + (r0 + 16 * ps + 1) * LS + 4 + c) = depth4(og[ps].ok, inv4[br][ps]);
            if (tid < 32) *(f32x4_t*)(sd[br] + (tid >> 4 ? TH + 1 : 0) * LS + 4 + c) = depth4(hrow_ok, hrow[br]);
            else if (tid >= 64 && tid < 64 + 2 * (TH + 2)) {
                const int i = tid - 64;
                sd[br][(i >> 1) * LS + (i & 1 ? 4 + TW : 3)] = hcol_ok ? rcp_newton(fmaxf(hcol[br], 1e-6f)) : 0.f;
            }
        }
        __syncthreads();
        // ---- the 8 pixels, both branches
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const float vm = og[ps].ok ? 1.f : 0.f;
            const f32x4_t e = sel4(og[ps].ok, e4[ps]);
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc_e += e[k]; acc_ne += vm - e[k]; }
#pragma unroll
            for (int br = 0; br < NBR; ++br) {
                float w[3][6];
                window(sd[br], r0 + 16 * ps + 1, c, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float g = fabsf(directed_response(w, k, direction_masks(n4[ps][k])));
                    // p = 1 / (1 + t), 1 - p = t p with t = exp(-(g - thresh)) (see the generic kernel of edge_loss.hip)
                    const float tt = __builtin_amdgcn_exp2f(__builtin_fmaf(g, -LOG2E, tk));
                    const float p = rcpf(1.f + tt), omp = tt * p;
                    const float ne = e[k] * -LN2, nf = (e[k] - vm) * LN2;            // -e ln 2, -(1 - e) ln 2 (0 outside the image)
                    acc[br][0] = __builtin_fmaf(ne, __builtin_amdgcn_logf(p + 0.001f), acc[br][0]);
                    acc[br][1] = __builtin_fmaf(nf, __builtin_amdgcn_logf(omp + 0.001f), acc[br][1]);
                }
            }
            if (silog) {
                const f32x4_t d = sel4(og[ps].ok, d4[ps]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float gt = rcpf(fmaxf(d[k], 1e-6f));
                    const float lg = __builtin_amdgcn_logf(gt * 10.f);
                    acc_cnt += d[k] > 0.f ? 1.f : 0.f;
#pragma unroll
                    for (int br = 0; br < NBR; ++br) {
                        const float dl = (__builtin_amdgcn_logf((inv4[br][ps][k] + 1e-5f) * 10.f) - lg) * LN2;
                        const float dlm = d[k] > 0.f ? dl : 0.f;                     // dl itself may be NaN where d = 0
                        acc[br][2] += dlm; acc[br][3] = __builtin_fmaf(dlm, dlm, acc[br][3]);
                    }
                }
            }
        }
    }
    // ---- sums: fp32 per thread and per wave, fp64 from there on; one record per branch (forward_tail of edge_loss.hip, twice)
    {
        float s;
        s = wave_sum_dpp(acc_e); if (lane == 0) sred[wave][0] = s;
        s = wave_sum_dpp(acc_ne); if (lane == 0) sred[wave][1] = s;
        if (silog) { s = wave_sum_dpp(acc_cnt); if (lane == 0) sred[wave][2] = s; }
#pragma unroll
        for (int br = 0; br < NBR; ++br)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i >= 2 && !silog) continue;
                s = wave_sum_dpp(acc[br][i]);
                if (lane == 0) sred[wave][3 + 4 * br + i] = s;
            }
    }
    __syncthreads();
    volatile int* s_last = &s_last_store;
    // thread (br, v): value v of branch br's record; v = 0..3 edge sums, 10..12 silog sums
    const int pbr = tid >> 4, pv = tid & 15;
    const bool live = tid < NBR * 16 && (pv < 4 || (silog && pv >= 10 && pv < NP));
    if (live) {
        const int j = pv < 2 ? pv : (pv < 4 ? 3 + 4 * pbr + (pv - 2) : (pv == 12 ? 2 : 3 + 4 * pbr + 2 + (pv - 10)));
        const double v = (double)sred[0][j] + (double)sred[1][j] + (double)sred[2][j] + (double)sred[3][j];
        handoff::publish(a.records + ((long)blockIdx.x * NBR + pbr) * REC + pv, v);
    }
    handoff::drain();
    const int per_image = sc.groups;                               // workgroups of this image
    if (!handoff::draw([&] { return a.counter + 1 + id.s * a.B + id.b; }, [&] { return per_image; }, a.fences, a.fences, s_last)) return;
    // ---- last workgroup of this (scale, sample): per branch, value v = tid % 16 of records k, k + 16, ... (k = tid / 16), then the 16 part sums in order
    {
        double* s_fin = (double*)&sd[0][0];                        // the planes are dead (barriers above); NBR x 256 doubles
        const int v = tid & 15, k = tid >> 4;
        const bool has = v < 4 || (silog && v >= 10 && v < NP);
#pragma unroll
        for (int br = 0; br < NBR; ++br) {
            const double* rec = a.records + (((long)sc.first_block + (long)id.b * per_image) * NBR + br) * REC + v;
            double part = 0.0;
            if (has) {
#pragma unroll 4
                for (int j = k; j < per_image; j += 16) part += handoff::read(rec + (long)j * NBR * REC);
            }
            s_fin[br * 256 + k * 16 + v] = part;
        }
        __syncthreads();
        if (live) {
            double tot = 0.0;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) tot += s_fin[pbr * 256 + kk * 16 + pv];
            handoff::publish(a.results + (((long)pbr * a.nscales + id.s) * a.B + id.b) * NP + pv, tot);
        }
        if (!handoff::arrive([&] { return a.counter; }, [&] { return a.nscales * a.B; }, a.fences, a.fences, s_last)) return;
    }
    finalize_pair(a, (double*)&sd[0][0], NBR * (TH + 2) * LS / 2);
}

// ---------------- backward ----------------------------------------------------------------------------------------

// one G evaluation: planes A and B of pixel k of a window ("Transposed Sobel" in edge_loss.hip); cp / cn = cpos e, cneg (1 - e) (0 outside the image)
__device__ __forceinline__ void g_planes(const float w[3][6], int k, float n, float cp, float cn, float tk, float& A, float& B) {
    const DirMasks m = direction_masks(n);
    const float s = directed_response(w, k, m);
    const float tt = __builtin_amdgcn_exp2f(__builtin_fmaf(fabsf(s), -LOG2E, tk));
    const float p = rcpf(1.f + tt), omp = tt * p;
    const float dg = (p * omp) * (cn * rcpf(omp + 0.001f) - cp * rcpf(p + 0.001f));
    const float G = s > 0.f ? dg : (s < 0.f ? -dg : 0.f);           // d |s| / d s
    const float Gn = m.neg ? G : -G;
    A = m.v ? 0.f : G;
    B = m.v ? G : 0.f;
    B = m.k1 ? Gn : B;                                              // rl above zero (-1), lr below (+1)
    B = m.k3 ? -Gn : B;
}

__global__ __launch_bounds__(256, 4) void edge_pair_bwd_kernel(PairArgs a) {
    // depth on the tile + 2-pixel halo; the planes A, B of G = d loss / d s(p) on the tile + 1-pixel halo.  The branches take turns on them.
    __shared__ __attribute__((aligned(16))) float sd[(TH + 4) * LS];
    __shared__ __attribute__((aligned(16))) float sga[(TH + 2) * LS], sgb[(TH + 2) * LS];
    const BlockId id = decode_block(a);                            // one tile per workgroup
    const PairScale& sc = a.s[id.s];
    const int x0 = (id.t0 % sc.tiles_x) * TW, y0 = (id.t0 / sc.tiles_x) * TH;
    const int tid = threadIdx.x;
    const int c = (tid & 15) * 4, r0 = tid >> 4;
    const bool silog = a.gt_depth != nullptr && id.s == 0;
    const float tk = a.thresh * LOG2E;
    const long img = (long)id.b * sc.H;
    // ---- loads of BOTH branches (see edge_bwd_fast_kernel for the thread -> halo assignment); labels, normals and ground truth once
    OwnGroup og[2];
    f32x4_t inv4[NBR][2], e4[2], n4[2], d4[2];
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        og[ps] = own_group(sc, id.b, y0 + r0 + 16 * ps, x0 + c);
#pragma unroll
        for (int br = 0; br < NBR; ++br) inv4[br][ps] = *(const f32x4_t*)(sc.pred[br] + og[ps].off);
        e4[ps] = *(const f32x4_t*)(sc.edge + og[ps].off);
        n4[ps] = *(const f32x4_t*)(sc.normal + og[ps].off);
        if (silog) d4[ps] = *(const f32x4_t*)(a.gt_depth + og[ps].off);
    }
    f32x4_t hrow[NBR]; bool hrow_ok = false;
    float hcol[NBR]; bool hcol_ok = false;
#pragma unroll
    for (int br = 0; br < NBR; ++br) { hrow[br] = f32x4_t{0.f, 0.f, 0.f, 0.f}; hcol[br] = 0.f; }
    int hrow_ly = 0, hcol_idx = 0;
    if (tid < 64) {
        const int hr = tid >> 4;                                   // 0, 1: rows -2, -1;  2, 3: rows TH, TH + 1
        hrow_ly = hr < 2 ? hr : TH + hr;                           // LDS row (tile row + 2)
        const OwnGroup g = own_group(sc, id.b, y0 + hrow_ly - 2, x0 + c);
#pragma unroll
        for (int br = 0; br < NBR; ++br) hrow[br] = *(const f32x4_t*)(sc.pred[br] + g.off);
        hrow_ok = g.ok;
    } else if (tid < 64 + 4 * (TH + 4)) {
        const int i = tid - 64, q = i & 3, j = q < 2 ? q - 2 : TW - 2 + q;       // columns -2, -1, TW, TW + 1
        const int gy = y0 + (i >> 2) - 2, gx = x0 + j;
        hcol_ok = (unsigned)gy < (unsigned)sc.H && (unsigned)gx < (unsigned)sc.W;
        const long o = (img + min(max(gy, 0), sc.H - 1)) * sc.W + min(max(gx, 0), sc.W - 1);
#pragma unroll
        for (int br = 0; br < NBR; ++br) hcol[br] = sc.pred[br][o];
        hcol_idx = (i >> 2) * LS + 4 + j;
    }
    // the single G pixel of this thread (threads 0..195): LDS position (row gl of the planes, column gj of the image tile) and its labels
    const bool gx_row = tid < 2 * TW;
    const int gl = gx_row ? (tid < TW ? 0 : TH + 1) : (tid - 2 * TW) >> 1;                    // plane row = tile row + 1
    const int gj = gx_row ? (tid & (TW - 1)) : ((tid - 2 * TW) & 1 ? TW : -1);
    const bool g_has = tid < 2 * TW + 2 * (TH + 2);
    float ge = 0.f, gn = 0.f; bool g_ok = false;
    if (g_has) {
        const int gy = y0 + gl - 1, gx = x0 + gj;
        g_ok = (unsigned)gy < (unsigned)sc.H && (unsigned)gx < (unsigned)sc.W;
        const long o = (img + min(max(gy, 0), sc.H - 1)) * sc.W + min(max(gx, 0), sc.W - 1);
        ge = sc.edge[o]; gn = sc.normal[o];
    }
#pragma unroll
    for (int br = 0; br < NBR; ++br) {
        const float go = a.gout ? a.gout[br * a.nscales + id.s] : 1.f;
        const float* coef = a.coef + ((long)br * a.nscales + id.s) * (2 * a.B + 1);
        const float cpos = coef[2 * id.b] * go, cneg = coef[2 * id.b + 1] * go;
        if (br) __syncthreads();                                  // the previous branch's plane reads are done
        // ---- depth tile (the own rows' depth stays in registers for the chain rule)
        f32x4_t dep[2];
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            dep[ps] = depth4(og[ps].ok, inv4[br][ps]);
            *(f32x4_t*)(sd + (r0 + 16 * ps + 2) * LS + 4 + c) = dep[ps];
        }
        if (tid < 64) *(f32x4_t*)(sd + hrow_ly * LS + 4 + c) = depth4(hrow_ok, hrow[br]);
        else if (tid < 64 + 4 * (TH + 4)) sd[hcol_idx] = hcol_ok ? rcp_newton(fmaxf(hcol[br], 1e-6f)) : 0.f;
        __syncthreads();
        // ---- planes of G: own pixels, then the halo pixel
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            float w[3][6];
            window(sd, r0 + 16 * ps + 2, c, w);
            const f32x4_t e = sel4(og[ps].ok, e4[ps]);
            const float vm = og[ps].ok ? 1.f : 0.f;
            f32x4_t A, B;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float Ak, Bk;
                g_planes(w, k, n4[ps][k], cpos * e[k], cneg * (vm - e[k]), tk, Ak, Bk);
                A[k] = Ak; B[k] = Bk;
            }
            *(f32x4_t*)(sga + (r0 + 16 * ps + 1) * LS + 4 + c) = A;
            *(f32x4_t*)(sgb + (r0 + 16 * ps + 1) * LS + 4 + c) = B;
        }
        if (g_has) {
            float w[3][6];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) w[r][k] = sd[(gl + r) * LS + 4 + gj - 1 + k];          // plane row gl = depth rows gl .. gl + 2
            float Ak, Bk;
            const float e = g_ok ? ge : 0.f;
            g_planes(w, 0, gn, cpos * e, cneg * ((g_ok ? 1.f : 0.f) - e), tk, Ak, Bk);
            sga[gl * LS + 4 + gj] = Ak; sgb[gl * LS + 4 + gj] = Bk;
        }
        __syncthreads();
        // ---- transposed Sobel, chain rule through 1 / max(inv, 1e-6), silog gradient
        const float m1 = silog ? a.silog_aux[2 * br] : 0.f, ksl = silog ? a.silog_aux[2 * br + 1] * (a.silog_gout ? a.silog_gout[br] : 1.f) : 0.f;
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            float wa[3][6], wb[3][6];
            window(sga, r0 + 16 * ps + 1, c, wa);
            window(sgb, r0 + 16 * ps + 1, c, wb);
            float ca[6], eb[6], cc1[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                ca[j] = (wa[0][j] + wa[1][j]) + wa[2][j];
                eb[j] = wb[0][j] - wb[2][j];
                cc1[j] = wb[1][j] == 0.f ? wa[1][j] : 0.f;
            }
            f32x4_t out;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d0 = wa[0][k + 1] == 0.f ? wb[0][k + 1] : 0.f, d2 = wa[2][k + 1] == 0.f ? wb[2][k + 1] : 0.f;
                const float dd = (ca[k] - ca[k + 2]) + ((eb[k] + eb[k + 1]) + eb[k + 2]) + (cc1[k] - cc1[k + 2]) + (d0 - d2);
                const float d = dep[ps][k];
                out[k] = inv4[br][ps][k] >= 1e-6f ? -dd * d * d : 0.f;
            }
            if (silog) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float dgt = d4[ps][k];
                    const float gt = rcpf(fmaxf(dgt, 1e-6f));
                    const float pi = inv4[br][ps][k] + 1e-5f;
                    const float dl = (__builtin_amdgcn_logf(pi * 10.f) - __builtin_amdgcn_logf(gt * 10.f)) * LN2;
                    out[k] += dgt > 0.f ? ksl * (dl - 0.85f * m1) * rcpf(pi) : 0.f;
                }
            }
            if (og[ps].ok) *(f32x4_t*)(sc.dpred[br] + og[ps].off) = out;
        }
    }
}

// public scale record of include/mte_kernels.h
struct mte_edge_pair_scale_t { const float* pred[2]; float* dpred[2]; const float* edge; const float* normal; int H, W; };

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// fills the grid geometry.  -> workgroups, MTE_ERR_ARG, or MTE_ERR_UNSUPPORTED where a scale is outside the training configuration
int setup_scales(PairArgs& a, const mte_edge_pair_scale_t* scales, int nscales, int B, bool backward, bool check_config) {
    const int T = backward ? 1 : FWD_TILES_PER_WG;
    if (!scales || nscales < 1 || nscales > MAXS || B < 1) return MTE_ERR_ARG;
    long blocks = 0;
    bool supported = true;
    for (int s = 0; s < nscales; ++s) {
        const mte_edge_pair_scale_t& in = scales[s];
        if (!in.pred[0] || !in.pred[1] || !in.edge || in.H < 1 || in.W < 1 || (backward && (!in.dpred[0] || !in.dpred[1]))) return MTE_ERR_ARG;
        if (!in.normal || in.W % 4 != 0 || !aligned16(in.pred[0]) || !aligned16(in.pred[1]) || !aligned16(in.edge) || !aligned16(in.normal) ||
            (backward && (!aligned16(in.dpred[0]) || !aligned16(in.dpred[1]))))
            supported = false;
        PairScale& o = a.s[s];
        for (int br = 0; br < NBR; ++br) { o.pred[br] = in.pred[br]; o.dpred[br] = in.dpred[br]; }
        o.edge = in.edge; o.normal = in.normal;
        o.H = in.H; o.W = in.W;
        o.tiles_x = (in.W + TW - 1) / TW; o.tiles_y = (in.H + TH - 1) / TH;
        o.first_block = (int)blocks;
        o.groups = (o.tiles_x * o.tiles_y + T - 1) / T;
        blocks += (long)o.groups * B;
        if (blocks > 0x7fffffffL / (NBR * REC)) return MTE_ERR_ARG;
    }
    if (check_config && !supported) return MTE_ERR_UNSUPPORTED;
    a.nscales = nscales; a.B = B; a.nblocks = (int)blocks; a.tiles_per_wg = T;
    return (int)blocks;
}
long results_elems(int nscales, int B) { return ((long)NBR * nscales * B * NP + 1) & ~1L; }
long counter_elems(int nscales, int B) { return (((long)nscales * B + 1) * 4 + 15) / 16 * 2; }      // doubles holding the tickets (16-byte multiple)

}  // namespace

extern "C" {

// doubles of workspace for a forward launch over these scales: [2][nscales][B][13] sums + the arrival tickets + two 16-double records per workgroup
long mte_edge_loss_pair_work_elems(const void* scales, int nscales, int B) {
    PairArgs a{};
    const int blocks = setup_scales(a, (const mte_edge_pair_scale_t*)scales, nscales, B, false, false);
    if (blocks < 0) return -1;
    return results_elems(nscales, B) + counter_elems(nscales, B) + (long)blocks * NBR * REC;
}

int mte_edge_loss_pair_fwd(const void* scales, int nscales, int B, float thresh, float weight, float pos_to_neg, const float* gt_depth,
                           double* work, float* losses, float* coef, float* silog_loss, float* silog_aux, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    PairArgs a{};
    a.fences = g_mte_handoff_fences;
    const int blocks = setup_scales(a, (const mte_edge_pair_scale_t*)scales, nscales, B, false, true);
    if (blocks == MTE_ERR_UNSUPPORTED) return MTE_ERR_UNSUPPORTED;
    if (blocks < 0 || !work || !losses || !coef || (gt_depth && (!silog_loss || !silog_aux))) return MTE_ERR_ARG;
    if (gt_depth && !aligned16(gt_depth)) return MTE_ERR_UNSUPPORTED;
    a.thresh = thresh; a.weight = weight; a.pos_to_neg = pos_to_neg; a.gt_depth = gt_depth; a.losses = losses; a.coef = coef;
    a.silog_loss = silog_loss; a.silog_aux = silog_aux;
    const long r = results_elems(nscales, B);
    a.results = work; a.counter = (unsigned*)(work + r); a.records = work + r + counter_elems(nscales, B);
    if (!g_mte_loss_prezeroed && mte_memset_async(work, 0, sizeof(double) * (r + counter_elems(nscales, B)), stream) != hipSuccess) return MTE_ERR_LAUNCH;     // sums + tickets (the records are overwritten)
    hipLaunchKernelGGL(edge_pair_fwd_kernel, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}

int mte_edge_loss_pair_bwd(const void* scales, int nscales, int B, float thresh, const float* coef, const float* gout, const float* gt_depth,
                           const float* silog_aux, const float* silog_gout, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other runtime users (e.g. event queries)
    PairArgs a{};
    a.fences = g_mte_handoff_fences;
    const int blocks = setup_scales(a, (const mte_edge_pair_scale_t*)scales, nscales, B, true, true);
    if (blocks == MTE_ERR_UNSUPPORTED) return MTE_ERR_UNSUPPORTED;
    if (blocks < 0 || !coef || (gt_depth && !silog_aux)) return MTE_ERR_ARG;
    if (gt_depth && !aligned16(gt_depth)) return MTE_ERR_UNSUPPORTED;
    a.thresh = thresh; a.coef = (float*)coef; a.gout = gout; a.gt_depth = gt_depth; a.silog_aux = (float*)silog_aux; a.silog_gout = silog_gout;
    hipLaunchKernelGGL(edge_pair_bwd_kernel, dim3(blocks), dim3(256), 0, stream, a);
    return mte_check_launch();
}

}  // extern "C"
