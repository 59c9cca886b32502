// Device code shared by every forward / backward kernel of edge_loss.hip, and the training configuration's kernels themselves:
//   * the launch description (TileGrid, LossLaunch) and the workgroup -> (scale, sample, tiles) decoding;
//   * forward_tail: sums of one workgroup -> record -> image sums -> finish, for the generic forward (mask sums live) and the fast family;
//   * finalize_losses: the finish of a launch (class balance, losses, backward coefficients, silog), and its pieces scale_stats / sample_term, which
//     the single-scale finalize kernel of edge_loss.hip uses too;
//   * the fast family, template <int NBR>: NBR predictions against ONE set of labels.  NBR = 1 is the four-scale training launch
//     (mte_edge_loss_multi_*), NBR = 2 the completion models' RGB and RGB+LiDAR predictions (mte_edge_loss_pair_*).
// Every sum has a fixed order that does not depend on NBR: the tiling, the per-thread order, the record order and the finish arithmetic are the same
// source expressions in each instantiation (-ffp-contract=off, no fast-math), so a branch of the pair launch is bit-equal to a single launch of it.
#pragma once
#include "common.hpp"
#include "edge_direction.hpp"
#include "edge_tile.hpp"
#include "handoff.hpp"

namespace {                             // one translation unit includes this: the kernels stay internal to it

constexpr int MAXS = 4;                 // scales per launch
constexpr int NP = 13;                  // sums per (prediction, scale, sample): 0..3 edge sums (e, 1 - e, pos, neg), 4..9 mask statistics, 10..12 silog sums (dl, dl^2, count)
#ifndef MTE_EDGE_FWD_TILES
#define MTE_EDGE_FWD_TILES 3
#endif
constexpr int FWD_TILES_PER_WG = MTE_EDGE_FWD_TILES;     // forward: consecutive tiles per workgroup (3: 856 workgroups at T8, one round of the 1024 slots)

struct TileGrid {                       // one scale's maps and its place in the launch
    int H, W, tiles_x, tiles_y, first_block;
    int groups;                         // workgroups per image: each takes `tiles_per_wg` consecutive tiles (row-major)
};
struct LossLaunch {                     // NBR = predictions per label set (1 in the generic kernels)
    int nscales, B, nblocks, tiles_per_wg;
    float thresh, weight, pos_to_neg;
    double* results;                    // [NBR][nscales][B][NP] sums of each (prediction, scale, sample) (zeroed by the launcher; written by the image's last workgroup)
    double* records;                    // [nblocks][NBR][REC]: one record of partial sums per (workgroup, prediction)
    unsigned* counter;                  // [0] launch ticket, [1 + s*B + b] ticket of (scale, sample) (zeroed by the launcher)
    float* losses;                      // forward out: [NBR][nscales]
    float* coef;                        // forward out / backward in: [NBR][nscales][2B + 1]
    const float* gout;                  // backward: upstream gradient per loss [NBR][nscales] (device, nullable = 1)
    const float* gt_depth;              // optional fused silog on scale 0: metric depth, 0 = invalid
    float* silog_loss; float* silog_aux;          // forward out: loss [NBR], (mean, 10/sqrt(S)/n) [NBR][2]
    const float* silog_gout;            // backward: upstream gradient of the silog losses [NBR] (device, nullable = 1)
    int fences;                         // MTE_OPT_HANDOFF_FENCES (handoff.hpp)
};
template <int NBR> struct FastScale : TileGrid {
    const float* pred[NBR]; float* dpred[NBR];
    const float* edge; const float* normal;
};
template <int NBR> struct FastArgs : LossLaunch { FastScale<NBR> s[MAXS]; };

struct BlockId { int s, b, t0, t1; };                            // tiles t0 .. t1 - 1 of sample b of scale s
template <typename A> __device__ __forceinline__ BlockId decode_block(const A& a) {
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

// ---------------- the finish ----------------------------------------------------------------------------------------
// Runs in the last workgroup: every accumulator is complete.  The scalar arithmetic of comp_cross_entropy (grad_loss.py:161-219) and
// SilogLoss (supervised_loss.py:57-69) is a few hundred dependent reads of the accumulators; straight from memory (agent-scope loads,
// one L2 round trip each, one thread) that serial tail was ~45 us of a 73 us launch (round 4: forward 73 -> see profiles/README.md).  So the
// whole workgroup first copies the sums into LDS (`stage`: the depth tiles' storage, free by now; one round trip); one thread per
// (prediction, scale, sample) does the divisions, one per (prediction, scale) the ordered sum (+ one per silog loss, in another wave).
struct PlainView { const double* p; __device__ __forceinline__ double operator()(long i) const { return p[i]; } };       // LDS copy, or memory of an earlier launch
struct MemView { const double* g; __device__ __forceinline__ double operator()(long i) const { return handoff::read(g + i); } };
// class-balance arithmetic of one scale from its image sums R0(R + b * NP + i) (comp_cross_entropy, grad_loss.py:161-219)
struct ScaleStats { bool binary; double nvalid, wneg_total; };
template <typename V> __device__ __forceinline__ ScaleStats scale_stats(const V& R0, long R, int B, bool has_mask, double numel) {
    double mi[4] = {0.0, 0.0, 0.0, 0.0};
    if (has_mask)
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < 4; ++k) mi[k] += R0(R + b * NP + 6 + k);
    ScaleStats st;
    st.binary = has_mask && mi[2] == 0.0 && mi[0] > 0.0 && mi[1] > 0.0;          // unique(mask) == {0, 1}
    st.nvalid = st.binary ? mi[3] : numel;
    st.wneg_total = 0.0;
    for (int b = 0; b < B; ++b) st.wneg_total += (double)(float)R0(R + b * NP + 1);
    return st;
}
// sample b of a scale (its sums at `sums`): backward coefficients -> coef[2b], coef[2b + 1]; returns its term of the loss sum
template <typename V> __device__ __forceinline__ double sample_term(float weight, float pos_to_neg, const V& R0, long sums, const ScaleStats& st, float* coef, int b) {
    const float wp = (float)R0(sums), wn = (float)R0(sums + 1);
    const float alpha = st.wneg_total == 0.0 ? 1.f : wn / (wp + wn);
    const double P = st.binary ? R0(sums + 4) : R0(sums + 2), N = st.binary ? R0(sums + 5) : R0(sums + 3);
    coef[2 * b] = (float)((double)weight * pos_to_neg * alpha / st.nvalid);
    coef[2 * b + 1] = (float)((double)weight * (1.f - alpha) / st.nvalid);
    return (double)pos_to_neg * alpha * P + (double)(1.f - alpha) * N;
}
// silog of prediction br (scale 0): loss = 10 sqrt(E[d^2] - 0.85 E[d]^2);  aux = (mean, 10/sqrt(S)/n)
template <typename V> __device__ __forceinline__ void silog_finish(const LossLaunch& a, const V& R0, int br) {
    const long R = (long)br * a.nscales * a.B * NP;
    double ss[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < a.B; ++b)
        for (int k = 0; k < 3; ++k) ss[k] += R0(R + (long)b * NP + 10 + k);
    const double n1 = ss[2];
    const double m1 = ss[0] / n1, m2 = ss[1] / n1;
    const double S = m2 - 0.85 * m1 * m1;
    a.silog_loss[br] = (float)(sqrt(S) * 10.0);
    a.silog_aux[2 * br] = (float)m1; a.silog_aux[2 * br + 1] = (float)(10.0 / sqrt(S) / n1);
}

// stage: LDS for `stage_elems` doubles.  The sums and the terms of every image fit up to B = 21 at four scales (the same B for every NBR: the
// fast forward has NBR depth planes); beyond that one thread works straight from memory.  q = br * nscales + s throughout.  MASKS: the scale
// records have a (nullable) `mask`, and a scale with one takes `binary` / `nvalid` from its mask statistics.
template <int NBR, bool MASKS, typename A> __device__ void finalize_losses(const A& a, double* stage, int stage_elems) {
    const int tid = threadIdx.x;
    const int heads = NBR * a.nscales, images = heads * a.B, n = images * NP;
    const auto stats = [&](const auto& R0, int q) {
        const auto& sc = a.s[q % a.nscales];
        bool has_mask = false;
        if constexpr (MASKS) has_mask = sc.mask != nullptr;
        return scale_stats(R0, (long)q * a.B * NP, a.B, has_mask, (double)a.B * sc.H * sc.W);
    };
    if (n + images <= stage_elems) {
        // the usual case.  (1) sums -> LDS; (2) one thread per image: alpha, the two coefficients (fp64 divisions -- done by one thread per
        // SCALE these were ~3 us of serial tail) and the sample's term of the loss; (3) one thread per q adds the terms in order
        __syncthreads();                                          // every wave is done with the tiles
        for (int i = tid; i < n; i += 256) stage[i] = handoff::read(a.results + i);
        __syncthreads();
        const PlainView R0{stage};
        double* term = stage + n;
        for (int i = tid; i < images; i += 256) {                 // i = q * B + b
            const int q = i / a.B, b = i - q * a.B;
            const ScaleStats st = stats(R0, q);
            float* coef = a.coef + (long)q * (2 * a.B + 1);
            term[i] = sample_term(a.weight, a.pos_to_neg, R0, (long)i * NP, st, coef, b);
            if (b == 0) coef[2 * a.B] = st.binary ? 1.f : 0.f;
        }
        if (a.gt_depth && tid >= 256 - NBR) silog_finish(a, R0, 255 - tid);       // another wave than the first threads
        __syncthreads();
        if (tid < heads) {
            const ScaleStats st = stats(R0, tid);
            double total = 0.0;
            for (int b = 0; b < a.B; ++b) total += term[tid * a.B + b];
            a.losses[tid] = (float)((double)a.weight * total / st.nvalid);
        }
        return;
    }
    if (tid != 0) return;                                         // very large batches: one thread, straight from memory
    const MemView R0{a.results};
    for (int q = 0; q < heads; ++q) {
        const ScaleStats st = stats(R0, q);
        float* coef = a.coef + (long)q * (2 * a.B + 1);
        double total = 0.0;
        for (int b = 0; b < a.B; ++b) total += sample_term(a.weight, a.pos_to_neg, R0, ((long)q * a.B + b) * NP, st, coef, b);
        coef[2 * a.B] = st.binary ? 1.f : 0.f;
        a.losses[q] = (float)((double)a.weight * total / st.nvalid);
    }
    if (a.gt_depth)
        for (int br = 0; br < NBR; ++br) silog_finish(a, R0, br);
}

// ---------------- record / ticket tail of a forward workgroup --------------------------------------------------------
// The per-thread sums a forward kernel hands to forward_tail.  MASKS (the generic forward, one prediction): the NP sums themselves, slot = value.
// Otherwise (the fast family): e, valid - e and the silog count depend on the labels only and are kept once for all branches, then pos, neg, dl,
// dl^2 per branch.
template <int NBR, bool MASKS> struct TailSums {
    static_assert(!MASKS || NBR == 1, "mask sums: one prediction");
    static constexpr int N = MASKS ? NP : 3 + 4 * NBR;
    static constexpr int E = 0, NE = 1, CNT = 2;                  // !MASKS: the shared slots
    __device__ static constexpr int branch(int br) { return 3 + 4 * br; }        // !MASKS: + 0 pos, 1 neg, 2 dl, 3 dl^2
    __device__ static constexpr int slot(int br, int v) {         // value v (0 .. NP - 1) of branch br
        return MASKS ? v : (v < 2 ? v : (v < 4 ? branch(br) + v - 2 : (v == 12 ? CNT : branch(br) + v - 8)));
    }
    __device__ static constexpr int value(int j) {                // the value that slot j holds
        return MASKS ? j : (j < 2 ? j : (j == CNT ? 12 : (((j - 3) & 3) < 2 ? 2 + ((j - 3) & 3) : 8 + ((j - 3) & 3))));
    }
};
__device__ __forceinline__ bool live_value(int v, bool has_mask, bool silog) { return v < 4 || (v < 10 ? has_mask : (v < NP && silog)); }

// Sums of one workgroup -> records -> image sums -> losses.  sd: the depth tiles' LDS storage (NBR * (TH + 2) * LS floats, dead by now), sred /
// s_last: LDS scratch of the kernel.  fp32 per thread and per wave (xor butterfly in DPP / lane-swap instructions), fp64 from there on, NO atomic
// adds.  The workgroup leaves ONE record per branch (its own 128-byte line, slot NBR * workgroup + branch); the last workgroup of a
// (scale, sample) to arrive adds that image's <= 240 records per branch in a FIXED order and writes the image's sums; the last of those finishes
// the losses (finish: the single-scale entry point leaves that to its own launch).  Every sum of the launch has a fixed order, so losses and
// coefficients are bit-reproducible.  (Before: one fp64 atomicAdd per value into the image's accumulators -- 7 x 240 adds on ONE cache line per
// full-resolution image, serialised at its L2 channel: 27 us of a 54 us launch.  A first fixed-order attempt in round 1 had ONE workgroup sweep
// all 2,568 records: ~120 us.)
template <int NBR, bool MASKS, typename A>
__device__ __forceinline__ void forward_tail(const A& a, const BlockId& id, const float (&acc)[TailSums<NBR, MASKS>::N], bool has_mask, bool silog,
                                             bool finish, float* sd, float (*sred)[TailSums<NBR, MASKS>::N], int* s_last_p) {
    using S = TailSums<NBR, MASKS>;
    const auto& sc = a.s[id.s];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    volatile int* s_last = s_last_p;                               // handoff::arrive broadcasts through it
    if (!MASKS) has_mask = false;
#pragma unroll
    for (int j = 0; j < S::N; ++j) {
        if (!live_value(S::value(j), has_mask, silog)) continue;
        const float s = wave_sum_dpp(acc[j]);
        if (lane == 0) sred[wave][j] = s;
    }
    __syncthreads();
    // thread (br, v) = (tid / 16, tid % 16): value v of branch br's record
    const int pbr = tid >> 4, pv = tid & 15;
    const bool live = tid < NBR * 16 && live_value(pv, has_mask, silog);
    if (live) {
        const int j = S::slot(pbr, pv);
        const double v = (double)sred[0][j] + (double)sred[1][j] + (double)sred[2][j] + (double)sred[3][j];
        handoff::publish(a.records + ((long)blockIdx.x * NBR + pbr) * REC + pv, v);
    }
    handoff::drain();
    const int per_image = sc.groups;                               // workgroups of this image
    if (!handoff::draw([&] { return a.counter + 1 + id.s * a.B + id.b; }, [&] { return per_image; }, a.fences, a.fences, s_last)) return;
    // ---- last workgroup of this (scale, sample): per branch, value v = tid % 16 of records k, k + 16, ... (k = tid / 16), then the 16 part sums in order
    {
        double* s_fin = (double*)sd;                               // the tiles are dead (barriers above); NBR x 256 doubles
        const int v = tid & 15, k = tid >> 4;
        const bool has = live_value(v, has_mask, silog);
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
    if (finish) finalize_losses<NBR, MASKS>(a, (double*)sd, NBR * (TH + 2) * LS / 2);
}

// ======================= the training configuration: branch-free kernels ============================================================
// Every scale: 16-byte accesses legal (W % 4 == 0), inverse depth in, Sobel + normals + sigmoid, no mask, no edge-map output (`fast_config` of
// edge_loss.hip).  Round 4.  The generic kernels spend a third of their instructions on control flow: per-pixel bounds tests compiled to exec-mask
// branches with their phi copies, divergent loop exits between 4-pixel and 1-pixel items, a load guard per access.  Here
//   * every global address is CLAMPED into the image and the loaded value selected to zero afterwards -- no guard around a load;
//   * a thread stages the depth of ITS OWN 8 pixels (the same load feeds the silog term and the chain rule), the halo rows / columns are
//     single extra loads of the first threads: no index arithmetic by division, no scalar / vector load variants;
//   * validity is one factor per 4-pixel group folded into the sums (1 - e becomes valid - e), the silog mask is a select;
//   * the direction bins are three range tests (edge_direction.hpp) that select the Sobel response and the backward planes directly;
//   * logs stay in base 2 until the sums (the ln 2 is folded into the label factors).
// Per 8 pixels of a thread and branch: ~1,000 instructions forward (generic: 2,450), ~1,500 backward (3,100).
// NBR branches: the labels (edge, normal, ground truth on scale 0) are loaded ONCE, into registers, and serve every branch -- at NBR = 2 forward
// 16 B/pixel (two single launches: 24), backward 16 B/pixel read + 8 written (24 + 8).  Forward: the NBR predictions' tiles + halo are staged as
// depth in NBR LDS planes; backward: the branches take turns on ONE set of planes (depth + A + B = 29,952 B).  Every global load of all branches
// is issued before the first plane is built, so a workgroup pays one memory latency.  Last-arriver tickets only: no workgroup waits for another.
struct OwnGroup { bool ok; long off; };                        // a thread's 4 pixels of one row: inside the image?  offset of the (clamped) group
__device__ __forceinline__ OwnGroup own_group(const TileGrid& sc, int b, int gy, int gx) {
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
// signed Sobel response of the direction the normal selects
__device__ __forceinline__ float directed_response(const float w[3][6], int k, const DirMasks& m) {
    float sh, sv, srl, slr;
    sobel4(w, k, sh, sv, srl, slr);
    float s = m.v ? sv : sh;
    s = m.k1 ? (m.neg ? slr : srl) : s;
    s = m.k3 ? (m.neg ? srl : slr) : s;
    return s;
}
constexpr float LOG2E = 1.44269504088896341f, LN2 = 0.693147180559945309f;

template <int NBR> __global__ __launch_bounds__(256, 4) void edge_fwd_fast_kernel(FastArgs<NBR> a) {
    using S = TailSums<NBR, false>;
    __shared__ __attribute__((aligned(16))) float sd[NBR][(TH + 2) * LS];
    __shared__ float sred[4][S::N];
    __shared__ int s_last;
    const BlockId id = decode_block(a);
    const FastScale<NBR>& sc = a.s[id.s];
    const int tid = threadIdx.x;
    const int c = (tid & 15) * 4, r0 = tid >> 4;                   // this thread's 4 pixels: columns c..c+3 of rows r0 and r0 + 16
    const bool silog = a.gt_depth != nullptr && id.s == 0;
    const float tk = a.thresh * LOG2E;
    float acc[S::N];
#pragma unroll
    for (int i = 0; i < S::N; ++i) acc[i] = 0.f;
    // a workgroup walks `tiles_per_wg` consecutive tiles of its image and keeps the sums in registers: the record / ticket round trips
    // at the end (two dependent trips to the memory side, ~5 us with the slot held) are paid once per 3 tiles instead of per tile
    for (int t = id.t0; t < id.t1; ++t) {
        const int x0 = (t % sc.tiles_x) * TW, y0 = (t / sc.tiles_x) * TH;
        if (t != id.t0) __syncthreads();                          // the previous tile's window reads are done
        // ---- loads: own pixels (every branch's inverse depth, label, normal, ground truth), then the halos of the depth tiles
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
        // ---- the 8 pixels, every branch
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const float vm = og[ps].ok ? 1.f : 0.f;
            const f32x4_t e = sel4(og[ps].ok, e4[ps]);
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc[S::E] += e[k]; acc[S::NE] += vm - e[k]; }
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
                    acc[S::branch(br)] = __builtin_fmaf(ne, __builtin_amdgcn_logf(p + 0.001f), acc[S::branch(br)]);
                    acc[S::branch(br) + 1] = __builtin_fmaf(nf, __builtin_amdgcn_logf(omp + 0.001f), acc[S::branch(br) + 1]);
                }
            }
            if (silog) {
                const f32x4_t d = sel4(og[ps].ok, d4[ps]);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float gt = rcpf(fmaxf(d[k], 1e-6f));
                    const float lg = __builtin_amdgcn_logf(gt * 10.f);
                    acc[S::CNT] += d[k] > 0.f ? 1.f : 0.f;
#pragma unroll
                    for (int br = 0; br < NBR; ++br) {
                        const float dl = (__builtin_amdgcn_logf((inv4[br][ps][k] + 1e-5f) * 10.f) - lg) * LN2;
                        const float dlm = d[k] > 0.f ? dl : 0.f;                     // dl itself may be NaN where d = 0
                        acc[S::branch(br) + 2] += dlm; acc[S::branch(br) + 3] = __builtin_fmaf(dlm, dlm, acc[S::branch(br) + 3]);
                    }
                }
            }
        }
    }
#if defined(MTE_EDGE_ABLATE) && (MTE_EDGE_ABLATE & 1)
    { float tt = 0.f; for (int i = 0; i < S::N; ++i) tt += acc[i]; if (tt == 123.456f) a.losses[0] = tt; return; }      // diagnostic: no sums / records / tickets
#endif
    forward_tail<NBR, false>(a, id, acc, false, silog, true, &sd[0][0], sred, &s_last);
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

template <int NBR> __global__ __launch_bounds__(256, 4) void edge_bwd_fast_kernel(FastArgs<NBR> a) {
    // depth on the tile + 2-pixel halo; the planes A, B of G = d loss / d s(p) on the tile + 1-pixel halo.  The branches take turns on them.
    __shared__ __attribute__((aligned(16))) float sd[(TH + 4) * LS];
    __shared__ __attribute__((aligned(16))) float sga[(TH + 2) * LS], sgb[(TH + 2) * LS];
    const BlockId id = decode_block(a);                            // one tile per workgroup
    const FastScale<NBR>& sc = a.s[id.s];
    const int x0 = (id.t0 % sc.tiles_x) * TW, y0 = (id.t0 / sc.tiles_x) * TH;
    const int tid = threadIdx.x;
    const int c = (tid & 15) * 4, r0 = tid >> 4;
    const bool silog = a.gt_depth != nullptr && id.s == 0;
    const float tk = a.thresh * LOG2E;
    const long img = (long)id.b * sc.H;
    // ---- loads of EVERY branch; labels, normals and ground truth once.  Own pixels: inverse depth, label, normal (+ ground truth); depth halo:
    //      rows -2, -1, TH, TH + 1 (threads 0..63) and columns -2, -1, TW, TW + 1 of rows -2 .. TH + 1 (threads 64..207); G halo (label + normal
    //      of ONE pixel): rows -1 and TH (threads 0..127), columns -1 and TW of rows -1 .. TH (threads 128..195)
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

}  // namespace
