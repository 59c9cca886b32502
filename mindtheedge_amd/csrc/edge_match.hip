// Pixel correspondence of the edge benchmark on device for gfx950: the SIZE OF A MAXIMUM MATCHING between the predicted
// and the annotated edge pixels of one image, where two pixels may be paired iff dx^2 + dy^2 <= r2.
//
// Stands in for correspond_pixels.correspond_pixels of py-bsds500 as the reference calls it (eval_depth_edges.py:119-145
// through _pred_eval :179-230: thresholds=1, apply_thinning=False, max_dist=0.002).  That matcher solves a min-cost assignment
// whose outlier cost is 200 x the dearest admissible edge, i.e. it matches as many pixels as can be matched, and the
// benchmark reads only the number of matched pixels.  The size of a maximum matching is unique, so the count here is an exact
// integer that every correct algorithm agrees on.  PARITY UNPINNED against py-bsds500 itself (not available); pinned against
// an independent exact solver in tests/edge_benchmark_ref.py.
//
// Shape of the kernel:
//   * ONE workgroup per instance; its mates, parents, roots and queues live in that instance's slice of the workspace.
//     No workgroup ever waits on another; __syncthreads() is the only barrier.  The many instances of a benchmark run
//     (12 thresholds x ~100 frames) are what fills the chip.
//   * greedy initialisation (claims by atomicCAS, nearest offset first), or a caller's matching that is CHECKED, then
//     phases of multi-source alternating breadth-first search from all free predicted pixels.  Trees are vertex-disjoint:
//     a ground-truth pixel is claimed by one parent (atomicCAS), a matched predicted pixel is reached only through its mate.
//     A phase ends with the first level that reaches a free ground-truth pixel; one thread per tree that did so flips its
//     path along the parent pointers.  A phase that reaches none ends the instance: exact by Berge's theorem.
//   * every loop is bounded by a number derived from the instance: phases <= n_pred + 1, levels per phase <=
//     2 min(n_pred, n_gt) + 2, a path walk <= the level bound.  Hitting a bound writes `status` and ends the instance.
#include "common.hpp"

namespace {

constexpr int NT = 1024;                 // threads per workgroup (= per instance)
constexpr int MAX_R2 = 64;               // window of 17 x 17 offsets
constexpr int RAD = 8, SIDE = 2 * RAD + 1, NOFF = SIDE * SIDE;
constexpr int ARRAYS = 7;                // mate_p, mate_g, parent, root, found, queue 0, queue 1

enum { ST_OK = 0, ST_BAD_INIT = 1, ST_PHASES = 2, ST_LEVELS = 3, ST_WALK = 4, ST_QUEUE = 5, ST_BAD_GT_INDEX = 6 };

struct MatchArgs {
    const float* pred;       // [B][H][W], 0..255
    const float* gt;         // [Bg][H][W]
    const int* gt_of;        // [B]
    const int* init_mate;    // nullable [B][H][W]
    int* ws;                 // [B][ARRAYS][H*W]
    int* result;             // [B][4]: matched, n_pred, n_gt, status
    int* mate_pred;          // nullable [B][H][W]
    int Bg, H, W, r2;
};

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// mate_p[i]: -2 not a predicted pixel, -1 free, else its ground-truth partner.  mate_g likewise.  parent[v]: -2 not a ground-truth
// pixel, -1 not reached in this phase, else the predicted pixel that claimed v.
__global__ __launch_bounds__(NT) void edge_match_kernel(MatchArgs a) {
    __shared__ int s_off[NOFF];          // admissible offsets, nearest first: (dy + RAD) << 8 | (dx + RAD)
    __shared__ int s_k, s_npred, s_ngt, s_cnt[2], s_found, s_status, s_matched;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int H = a.H, W = a.W, N = H * W, r2 = a.r2;
    int* mate_p = a.ws + (long)b * ARRAYS * N;
    int* mate_g = mate_p + N;
    int* parent = mate_g + N;
    int* root = parent + N;
    int* found = root + N;
    int* queue0 = found + N;                                      // queue c = queue0 + c * N
    int* mate_out = a.mate_pred ? a.mate_pred + (long)b * N : nullptr;
    int* res = a.result + 4 * (long)b;

    if (tid == 0) { s_k = 0; s_npred = 0; s_ngt = 0; s_status = ST_OK; s_matched = 0; }
    __syncthreads();
    const int gi = a.gt_of[b];
    if (gi < 0 || gi >= a.Bg) {                                   // uniform: every thread reads the same word
        for (int i = tid; mate_out && i < N; i += NT) mate_out[i] = -1;
        if (tid == 0) { res[0] = 0; res[1] = 0; res[2] = 0; res[3] = ST_BAD_GT_INDEX; }
        return;
    }
    if (tid < NOFF) {
        const int dx = tid % SIDE - RAD, dy = tid / SIDE - RAD, d2 = dx * dx + dy * dy;
        if (d2 <= r2) {
            int rank = 0;
            for (int t = 0; t < NOFF; ++t) {
                const int ex = t % SIDE - RAD, ey = t / SIDE - RAD, e2 = ex * ex + ey * ey;
                rank += (e2 < d2 || (e2 == d2 && t < tid)) ? 1 : 0;
            }
            s_off[rank] = ((dy + RAD) << 8) | (dx + RAD);
            atomicAdd(&s_k, 1);
        }
    }
    const float* pim = a.pred + (long)b * N;
    const float* gim = a.gt + (long)gi * N;
    {
        int np = 0, ng = 0;
        for (int i = tid; i < N; i += NT) {
            const bool p = pim[i] > 127.5f, g = gim[i] > 127.5f;                 // v/255 > 0.5, as mte_chamfer_distance
            mate_p[i] = p ? -1 : -2;
            mate_g[i] = g ? -1 : -2;
            np += p; ng += g;
        }
        if (np) atomicAdd(&s_npred, np);
        if (ng) atomicAdd(&s_ngt, ng);
    }
    __syncthreads();
    const int K = s_k, n_pred = s_npred, n_gt = s_ngt;
    const int level_bound = 2 * min(n_pred, n_gt) + 2;

    // ---- starting matching
    if (a.init_mate) {
        const int* im = a.init_mate + (long)b * N;
        for (int i = tid; i < N; i += NT) {
            const int m = im[i];
            if (m == -1) continue;
            bool ok = mate_p[i] == -1 && m >= 0 && m < N;
            if (ok) {
                const int dx = m % W - i % W, dy = m / W - i / W;
                ok = dx * dx + dy * dy <= r2 && ld_agent(&mate_g[m]) != -2 && atomicCAS(&mate_g[m], -1, i) == -1;
            }
            if (ok) mate_p[i] = m; else s_status = ST_BAD_INIT;
        }
    } else {
        for (int i = tid; i < N; i += NT) {
            if (mate_p[i] != -1) continue;
            const int x = i % W, y = i / W;
            for (int k = 0; k < K; ++k) {
                const int o = s_off[k], vx = x + (o & 255) - RAD, vy = y + (o >> 8) - RAD;
                if ((unsigned)vx >= (unsigned)W || (unsigned)vy >= (unsigned)H) continue;
                const int v = vy * W + vx;
                if (ld_agent(&mate_g[v]) == -1 && atomicCAS(&mate_g[v], -1, i) == -1) { mate_p[i] = v; break; }
            }
        }
    }
    __syncthreads();
    int status = s_status;
    if (status != ST_OK) {                                         // a matching that does not check out: report, touch nothing else
        for (int i = tid; mate_out && i < N; i += NT) mate_out[i] = -1;
        if (tid == 0) { res[0] = 0; res[1] = n_pred; res[2] = n_gt; res[3] = status; }
        return;
    }

    // ---- augmenting phases
    for (int phase = 0; K > 0 && n_pred > 0 && n_gt > 0; ++phase) {
        if (phase > n_pred) { status = ST_PHASES; break; }         // every phase but the last adds a pair: at most n_pred + 1 phases
        if (tid == 0) { s_cnt[0] = 0; s_cnt[1] = 0; s_found = 0; }
        __syncthreads();
        for (int i = tid; i < N; i += NT) {
            parent[i] = mate_g[i] == -2 ? -2 : -1;
            if (mate_p[i] == -1) {
                root[i] = i;
                found[i] = -1;
                queue0[atomicAdd(&s_cnt[0], 1)] = i;               // at most n_pred <= N entries
            }
        }
        __syncthreads();
        int cur = 0, nf = s_cnt[0], level = 0;
        bool augment = false;
        while (nf > 0) {
            if (level >= level_bound) { status = ST_LEVELS; break; }
            const int* q = queue0 + (long)cur * N;
            int* qn = queue0 + (long)(cur ^ 1) * N;
            const int chunk = 0x7fffffff / K;                      // keeps (frontier entries) x (offsets) inside 32 bits
            for (int base = 0; base < nf; base += chunk) {
                const unsigned items = (unsigned)min(chunk, nf - base) * (unsigned)K;
                for (unsigned it = tid; it < items; it += NT) {
                    const int u = q[base + (int)(it / (unsigned)K)], o = s_off[it % (unsigned)K];
                    const int vx = u % W + (o & 255) - RAD, vy = u / W + (o >> 8) - RAD;
                    if ((unsigned)vx >= (unsigned)W || (unsigned)vy >= (unsigned)H) continue;
                    const int v = vy * W + vx;
                    if (ld_agent(&parent[v]) != -1 || atomicCAS(&parent[v], -1, u) != -1) continue;
                    const int w = mate_g[v], r = root[u];
                    if (w == -1) {                                 // a free ground-truth pixel: the first one per tree is kept
                        atomicCAS(&found[r], -1, v);
                        s_found = 1;
                    } else {
                        root[w] = r;
                        const int slot = atomicAdd(&s_cnt[cur ^ 1], 1);
                        if (slot < N) qn[slot] = w; else s_status = ST_QUEUE;
                    }
                }
            }
            __syncthreads();
            const int f = s_found, nn = s_cnt[cur ^ 1], st = s_status;
            if (tid == 0) s_cnt[cur] = 0;                          // the queue just consumed is the one the next level fills
            __syncthreads();
            if (st != ST_OK) { status = st; break; }
            if (f) { augment = true; break; }
            cur ^= 1; nf = nn; ++level;
        }
        if (status != ST_OK || !augment) break;
        for (int i = tid; i < N; i += NT) {
            if (mate_p[i] != -1) continue;
            int v = found[i];
            if (v < 0) continue;
            for (int step = 0;; ++step) {                          // i is the root of its tree; the trees are vertex-disjoint
                if (step >= level_bound) { s_status = ST_WALK; break; }
                const int u = parent[v], prev = mate_p[u];
                mate_p[u] = v;
                mate_g[v] = u;
                if (prev < 0) break;
                v = prev;
            }
        }
        __syncthreads();
        status = s_status;
        if (status != ST_OK) break;
    }

    {
        int m = 0;
        for (int i = tid; i < N; i += NT) {
            const int v = mate_p[i];
            m += v >= 0;
            if (mate_out) mate_out[i] = v >= 0 ? v : -1;
        }
        if (m) atomicAdd(&s_matched, m);
    }
    __syncthreads();
    if (tid == 0) { res[0] = s_matched; res[1] = n_pred; res[2] = n_gt; res[3] = status; }
}

}  // namespace

extern "C" long mte_edge_match_workspace_bytes(int B, int H, int W, int r2) {
    (void)r2;
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (long)B * ARRAYS * (long)H * W * (long)sizeof(int);
}

extern "C" int mte_edge_match(const float* pred, const float* gt, const int* gt_of, int B, int Bg, int H, int W, int r2,
                              const int* init_mate, void* workspace, long workspace_bytes, int* result, int* mate_pred,
                              hipStream_t stream) {
    if (!pred || !gt || !gt_of || !workspace || !result || B <= 0 || Bg <= 0 || H <= 0 || W <= 0 || r2 < 0) return MTE_ERR_ARG;
    if (r2 > MAX_R2 || (long)H * W >= (1L << 30)) return MTE_ERR_UNSUPPORTED;
    if (workspace_bytes < mte_edge_match_workspace_bytes(B, H, W, r2)) return MTE_ERR_ARG;
    MatchArgs a;
    a.pred = pred; a.gt = gt; a.gt_of = gt_of; a.init_mate = init_mate; a.ws = (int*)workspace; a.result = result; a.mate_pred = mate_pred;
    a.Bg = Bg; a.H = H; a.W = W; a.r2 = r2;
    hipLaunchKernelGGL(edge_match_kernel, dim3((unsigned)B), dim3(NT), 0, stream, a);
    return mte_check_launch();
}
