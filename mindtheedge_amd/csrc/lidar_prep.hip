// Sparse LiDAR input on device for gfx950: the point perturbation of the reference's augment_depth_values (utils/depth.py:366-438)
// and the projection of a velodyne cloud into a sparse map (process_lidar, datasets/gta_dataset.py:85-104).
//
// Perturbation, three stages with one 4-byte host read after the first and after the second (the host draws per-point random
// numbers from numpy's stream and needs the counts to do so):
//   index    every pixel > 0 gets its ordinal k in raster order (np.where), n = their number          count -> scan -> compact
//   perturb  d' = add_d[k] + d * scale_d0;  i' = rint(i + add_i[k]), j' = rint(j + add_j[k]);  key = i' + rows * (j' - 1);
//            target cell ii = key mod rows (non-negative), jj = (key - ii) / rows + 1, only 0 <= jj < cols is tested;
//            every point whose key is the smallest key of the map is discarded (the reference's diff / +1 indexing never keeps
//            sorted position 0); among equal keys the lowest ordinal survives (= the reference under a stable argsort);
//            survivors with jj in range get the rank m = their order by ordinal, n' = their number
//                                                                                init -> keys -> count -> scan -> ranks
//   scatter  out[ii,jj] = float32(d') for survivors with keep[m] == 1, every other element of out = 0            one gather
// A key and a cell with jj in range determine each other, so "equal key" is "same cell" and the winner of a cell is found with an
// integer atomicMin on ordinals: bit-reproducible whatever the scheduling.  No kernel waits on another workgroup: where a pass
// needs the result of another it is a launch of its own.  All arithmetic is double; the one rounding to float32 is the final store.
#include "common.hpp"
#include "lidar_work.hpp"

namespace {

// Flags of this thread's LP_ITEMS elements (bit e = pred(first + e)) and the number of flagged elements of the workgroup in front of
// them; block_total = flagged elements of the whole workgroup.  Every thread of the workgroup calls it, once per kernel.
template <class Pred>
__device__ __forceinline__ int lp_block_exclusive(Pred pred, int base, int total, unsigned& bits, int& block_total) {
    __shared__ int s_wave[LP_THREADS / 64];
    bits = 0;
    const int first = base + (int)threadIdx.x * LP_ITEMS;
#pragma unroll
    for (int e = 0; e < LP_ITEMS; ++e)
        if (first + e < total && pred(first + e)) bits |= 1u << e;
    const int c = __popc(bits);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0;
    block_total = 0;
#pragma unroll
    for (int w = 0; w < LP_THREADS / 64; ++w) {
        const int v = s_wave[w];
        if (w < wave) before += v;
        block_total += v;
    }
    return before + incl - c;
}

struct ValidPixel {                                       // stage 1: sample > 0
    const float* src;
    __device__ bool operator()(int p) const { return src[p] > 0.f; }
};
struct Survivor {                                         // stage 2: owns its cell and does not carry the smallest key
    const int* cell; const int* winner; const long long* minkey; int rows, cols;
    __device__ bool operator()(int k) const {
        const int c = cell[k];
        if (c < 0 || winner[c] != k) return false;
        const int ii = c / cols, jj = c - ii * cols;
        return (long long)ii + (long long)rows * (jj - 1) != *minkey;
    }
};

// The bodies below are shared by the per-map kernels and by the batched ones (sample = blockIdx.y, further down): they index with
// blockIdx.x / gridDim.x only.
template <class Pred> __device__ __forceinline__ void lp_count_body(Pred pred, int total, int* __restrict__ blk) {
    unsigned bits;
    int block_total;
    lp_block_exclusive(pred, blockIdx.x * LP_CHUNK, total, bits, block_total);
    if (threadIdx.x == 0) blk[blockIdx.x] = block_total;
}

template <class Pred> __global__ __launch_bounds__(LP_THREADS) void lp_count_kernel(Pred pred, const int* __restrict__ limit, int total, int* __restrict__ blk) {
    if (limit && *limit < total) total = *limit;          // stage 2 never walks past the points stage 1 found
    lp_count_body(pred, total, blk);
}

// one workgroup: blk[b] = flagged elements in front of workgroup b; *total_out = their number
__device__ __forceinline__ void lp_scan_blocks_body(int* __restrict__ blk, int nblk, int* __restrict__ total_out) {
    __shared__ int s_wave[LP_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nblk; base += LP_THREADS) {
        const int i = base + (int)threadIdx.x;
        const int c = i < nblk ? blk[i] : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < LP_THREADS / 64; ++w) {
            const int v = s_wave[w];
            if (w < wave) before += v;
            all += v;
        }
        if (i < nblk) blk[i] = carry + before + incl - c;
        carry += all;
        __syncthreads();                                  // s_wave is rewritten by the next round
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(LP_THREADS) void lp_scan_blocks_kernel(int* __restrict__ blk, int nblk, int* __restrict__ total_out) {
    lp_scan_blocks_body(blk, nblk, total_out);
}

__device__ __forceinline__ void lp_compact_body(ValidPixel pred, int total, const int* __restrict__ blk, int* __restrict__ pts) {
    unsigned bits;
    int block_total;
    int k = blk[blockIdx.x] + lp_block_exclusive(pred, blockIdx.x * LP_CHUNK, total, bits, block_total);
    const int first = blockIdx.x * LP_CHUNK + (int)threadIdx.x * LP_ITEMS;
#pragma unroll
    for (int e = 0; e < LP_ITEMS; ++e)
        if (bits & (1u << e)) pts[k++] = first + e;       // k < number of valid pixels <= total: inside pts
}

__global__ __launch_bounds__(LP_THREADS) void lp_compact_kernel(ValidPixel pred, int total, const int* __restrict__ blk, int* __restrict__ pts) {
    lp_compact_body(pred, total, blk, pts);
}

__device__ __forceinline__ void lp_init_body(int* __restrict__ winner, int hw, long long* __restrict__ minkey) {
    for (int i = blockIdx.x * LP_THREADS + threadIdx.x; i < hw; i += gridDim.x * LP_THREADS) winner[i] = LP_NONE;
    if (blockIdx.x == 0 && threadIdx.x == 0) *minkey = 0x7fffffffffffffffLL;
}

__global__ __launch_bounds__(LP_THREADS) void lp_init_kernel(int* __restrict__ winner, int hw, long long* __restrict__ minkey) {
    lp_init_body(winner, hw, minkey);
}

// np.round(x).astype('int') for |x| far below 2^62 (a shift of 1e15 pixels is no LiDAR map; the clamp keeps the conversion defined)
__device__ __forceinline__ long long lp_round_index(double x) { return (long long)rint(fmin(fmax(x, -1e15), 1e15)); }

// n: already clamped to the device's own count
__device__ __forceinline__ void lp_keys_body(const float* __restrict__ src, int rows, int cols, int n, double scale_d0, const double* __restrict__ add_i,
                                             const double* __restrict__ add_j, const double* __restrict__ add_d, const int* __restrict__ pts,
                                             int* __restrict__ cell, double* __restrict__ dprime, int* __restrict__ winner, long long* __restrict__ minkey) {
    const int hw = rows * cols;
    long long lowest = 0x7fffffffffffffffLL;
    for (int k = blockIdx.x * LP_THREADS + threadIdx.x; k < n; k += gridDim.x * LP_THREADS) {
        const int p = pts[k];
        if ((unsigned)p >= (unsigned)hw) { cell[k] = -1; dprime[k] = 0.0; continue; }      // not an index stage 1 wrote
        const int i = p / cols, j = p - i * cols;
        dprime[k] = add_d[k] + (double)src[p] * scale_d0;
        const long long ip = lp_round_index((double)i + add_i[k]), jp = lp_round_index((double)j + add_j[k]);
        const long long key = ip + (long long)rows * (jp - 1);
        long long ii = key % rows;
        if (ii < 0) ii += rows;                           // Python's modulo
        const long long jj = (key - ii) / rows + 1;
        const int c = (jj >= 0 && jj < cols) ? (int)(ii * cols + jj) : -1;
        cell[k] = c;
        if (c >= 0) atomicMin(&winner[c], k);
        lowest = key < lowest ? key : lowest;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long v = __shfl_xor(lowest, o, 64);
        lowest = v < lowest ? v : lowest;
    }
    if ((threadIdx.x & 63) == 0 && lowest != 0x7fffffffffffffffLL) atomicMin(minkey, lowest);
}

__global__ __launch_bounds__(LP_THREADS) void lp_keys_kernel(const float* __restrict__ src, int rows, int cols, int n, const int* __restrict__ n_dev,
                                                             double scale_d0, const double* __restrict__ add_i, const double* __restrict__ add_j,
                                                             const double* __restrict__ add_d, const int* __restrict__ pts, int* __restrict__ cell,
                                                             double* __restrict__ dprime, int* __restrict__ winner, long long* __restrict__ minkey) {
    if (*n_dev < n) n = *n_dev;
    lp_keys_body(src, rows, cols, n, scale_d0, add_i, add_j, add_d, pts, cell, dprime, winner, minkey);
}

__device__ __forceinline__ void lp_rank_body(Survivor pred, int n, const int* __restrict__ blk, int* __restrict__ rank) {
    unsigned bits;
    int block_total;
    int m = blk[blockIdx.x] + lp_block_exclusive(pred, blockIdx.x * LP_CHUNK, n, bits, block_total);
    const int first = blockIdx.x * LP_CHUNK + (int)threadIdx.x * LP_ITEMS;
#pragma unroll
    for (int e = 0; e < LP_ITEMS; ++e)
        if (first + e < n) rank[first + e] = (bits & (1u << e)) ? m++ : -1;
}

__global__ __launch_bounds__(LP_THREADS) void lp_rank_kernel(Survivor pred, int n, const int* __restrict__ n_dev, const int* __restrict__ blk,
                                                             int* __restrict__ rank) {
    if (*n_dev < n) n = *n_dev;
    lp_rank_body(pred, n, blk, rank);
}

__device__ __forceinline__ void lp_gather_body(const int* __restrict__ winner, const int* __restrict__ rank, const double* __restrict__ dprime,
                                               const unsigned char* __restrict__ keep, int n_keep, int n, float* __restrict__ out, int hw) {
    for (int c = blockIdx.x * LP_THREADS + threadIdx.x; c < hw; c += gridDim.x * LP_THREADS) {
        float v = 0.f;
        const int k = winner[c];
        if (k >= 0 && k < n) {
            const int m = rank[k];
            if (m >= 0 && m < n_keep && keep[m] == 1) v = (float)dprime[k];
        }
        out[c] = v;
    }
}

__global__ __launch_bounds__(LP_THREADS) void lp_gather_kernel(const int* __restrict__ winner, const int* __restrict__ rank, const double* __restrict__ dprime,
                                                               const unsigned char* __restrict__ keep, int n_keep, int n, const int* __restrict__ n_dev,
                                                               float* __restrict__ out, int hw) {
    if (*n_dev < n) n = *n_dev;
    lp_gather_body(winner, rank, dprime, keep, n_keep, n, out, hw);
}

// ---- the batched form (mte_batch_lidar_perturb): index -> perturb -> scatter for every map of a [B,H,W] tensor, the sample in blockIdx.y.
// Everything per sample comes from a descriptor table in device memory; the host knows both counts beforehand (datasets/lidar_prep.py) and
// has sized and uploaded the draws with them, so nothing is read back between the stages.  Every loop runs to min(host count, device's
// own count): a wrong host count gives a wrong map, reported in `status`, never an access outside the draws or the workspace.
enum { LB_N = 0, LB_SURVIVORS, LB_SCALE_D0, LB_ADD_I, LB_ADD_J, LB_ADD_D, LB_KEEP, LB_RESERVED, LB_ROW_WORDS };

struct LbSample {
    int n, n_keep;                                        // the host's n and n'
    double scale_d0;
    const double *add_i, *add_j, *add_d;
    const unsigned char* keep;
};

__device__ __forceinline__ LbSample lb_load(const long* __restrict__ table, const unsigned char* __restrict__ arena, int b) {
    const long* r = table + (long)b * LB_ROW_WORDS;
    LbSample s;
    s.n = (int)r[LB_N]; s.n_keep = (int)r[LB_SURVIVORS];
    s.scale_d0 = __longlong_as_double((long long)r[LB_SCALE_D0]);
    s.add_i = (const double*)(arena + r[LB_ADD_I]); s.add_j = (const double*)(arena + r[LB_ADD_J]); s.add_d = (const double*)(arena + r[LB_ADD_D]);
    s.keep = arena + r[LB_KEEP];
    return s;
}
__device__ __forceinline__ LpWork lb_work(void* work, long stride, int hw) { return lp_carve((char*)work + (long)blockIdx.y * stride, hw); }
__device__ __forceinline__ int lb_points(const LbSample& s, const LpWork& w) { const int n_dev = w.head[0]; return n_dev < s.n ? n_dev : s.n; }

__global__ __launch_bounds__(LP_THREADS) void lb_count_valid_kernel(const float* __restrict__ lidar, int hw, void* work, long stride) {
    const LpWork w = lb_work(work, stride, hw);
    lp_count_body(ValidPixel{lidar + (long)blockIdx.y * hw}, hw, w.blk);
}
__global__ __launch_bounds__(LP_THREADS) void lb_scan_kernel(int hw, int nblk, int which, void* work, long stride) {
    const LpWork w = lb_work(work, stride, hw);
    lp_scan_blocks_body(w.blk, nblk, w.head + which);
}
__global__ __launch_bounds__(LP_THREADS) void lb_compact_kernel(const float* __restrict__ lidar, int hw, void* work, long stride) {
    const LpWork w = lb_work(work, stride, hw);
    lp_compact_body(ValidPixel{lidar + (long)blockIdx.y * hw}, hw, w.blk, w.pts);
}
__global__ __launch_bounds__(LP_THREADS) void lb_init_kernel(int hw, void* work, long stride) {
    const LpWork w = lb_work(work, stride, hw);
    lp_init_body(w.winner, hw, w.minkey);
}
__global__ __launch_bounds__(LP_THREADS) void lb_keys_kernel(const float* __restrict__ lidar, int rows, int cols, const long* __restrict__ table,
                                                             const unsigned char* __restrict__ arena, void* work, long stride) {
    const int hw = rows * cols;
    const LpWork w = lb_work(work, stride, hw);
    const LbSample s = lb_load(table, arena, blockIdx.y);
    lp_keys_body(lidar + (long)blockIdx.y * hw, rows, cols, lb_points(s, w), s.scale_d0, s.add_i, s.add_j, s.add_d, w.pts, w.cell, w.dprime, w.winner,
                 w.minkey);
}
__global__ __launch_bounds__(LP_THREADS) void lb_count_survivors_kernel(int rows, int cols, const long* __restrict__ table,
                                                                        const unsigned char* __restrict__ arena, void* work, long stride) {
    const LpWork w = lb_work(work, stride, rows * cols);
    const LbSample s = lb_load(table, arena, blockIdx.y);
    lp_count_body(Survivor{w.cell, w.winner, w.minkey, rows, cols}, lb_points(s, w), w.blk);
}
__global__ __launch_bounds__(LP_THREADS) void lb_rank_kernel(int rows, int cols, const long* __restrict__ table, const unsigned char* __restrict__ arena,
                                                             void* work, long stride) {
    const LpWork w = lb_work(work, stride, rows * cols);
    const LbSample s = lb_load(table, arena, blockIdx.y);
    lp_rank_body(Survivor{w.cell, w.winner, w.minkey, rows, cols}, lb_points(s, w), w.blk, w.rank);
}
__global__ __launch_bounds__(LP_THREADS) void lb_gather_kernel(int hw, const long* __restrict__ table, const unsigned char* __restrict__ arena,
                                                               void* work, long stride, float* __restrict__ out, int* __restrict__ status) {
    const LpWork w = lb_work(work, stride, hw);
    const LbSample s = lb_load(table, arena, blockIdx.y);
    lp_gather_body(w.winner, w.rank, w.dprime, s.keep, s.n_keep, lb_points(s, w), out + (long)blockIdx.y * hw, hw);
    if (blockIdx.x == 0 && threadIdx.x == 0) {            // the counts of both sides, for the host to compare later
        int* st = status + 4 * blockIdx.y;
        st[0] = s.n; st[1] = w.head[0]; st[2] = s.n_keep; st[3] = w.head[1];
    }
}

// ---- projection
__device__ __forceinline__ void lp_project(const double* __restrict__ pts, long N, long idx, const double* __restrict__ K, double& u, double& v, double& z) {
    const double X = pts[idx], Y = pts[N + idx], Z = pts[2 * N + idx];
    const double p0 = K[0] * X + K[1] * Y + K[2] * Z, p1 = K[3] * X + K[4] * Y + K[5] * Z;
    z = K[6] * X + K[7] * Y + K[8] * Z;
    u = p0 / z;
    v = p1 / z;
}

__global__ __launch_bounds__(LP_THREADS) void lp_project_scatter_kernel(const double* __restrict__ pts, int N, const double* __restrict__ K, int H, int W,
                                                                        int* __restrict__ winner) {
    for (int idx = blockIdx.x * LP_THREADS + threadIdx.x; idx < N; idx += gridDim.x * LP_THREADS) {
        double u, v, z;
        lp_project(pts, N, idx, K, u, v, z);
        if (u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H)                       // false for NaN: such points are dropped, as upstream
            atomicMax(&winner[(int)v * W + (int)u], idx);                                  // numpy's repeated-index assignment: the last point wins
    }
}

__global__ __launch_bounds__(LP_THREADS) void lp_project_gather_kernel(const double* __restrict__ pts, int N, const double* __restrict__ K,
                                                                       const int* __restrict__ winner, const float* __restrict__ depth_map,
                                                                       float* __restrict__ out, int hw) {
    for (int c = blockIdx.x * LP_THREADS + threadIdx.x; c < hw; c += gridDim.x * LP_THREADS) {
        const int idx = winner[c];
        double lidar = 0.0;
        if (idx >= 0 && idx < N) {
            double u, v;
            lp_project(pts, N, idx, K, u, v, lidar);
        }
        if (depth_map) {
            const double diff = lidar - (double)depth_map[c];
            if (sqrt(diff * diff) > 0.1 && lidar > 0.0) lidar = 0.0;
        }
        out[c] = (float)lidar;
    }
}

inline unsigned lp_grid(long total) { long g = (total + LP_THREADS - 1) / LP_THREADS; if (g > 4096) g = 4096; if (g < 1) g = 1; return (unsigned)g; }
inline bool lp_shape_ok(int H, int W) { return H > 0 && W > 0 && (long)H * W < (1L << 30); }
inline long lb_stride(long hw) { return (lp_work_bytes(hw) + 15) & ~15L; }      // one sample's workspace

}  // namespace

extern "C" {

long mte_lidar_perturb_work_bytes(int H, int W) { return lp_shape_ok(H, W) ? lp_work_bytes((long)H * W) : 0; }

int mte_lidar_index(const float* depth, int H, int W, void* work, hipStream_t stream) {
    if (!depth || !work || !lp_shape_ok(H, W) || ((uintptr_t)work & 7)) return MTE_ERR_ARG;
    const int hw = H * W, nblk = (int)lp_blocks(hw);
    const LpWork w = lp_carve(work, hw);
    const ValidPixel pred{depth};
    hipLaunchKernelGGL(lp_count_kernel<ValidPixel>, dim3(nblk), dim3(LP_THREADS), 0, stream, pred, (const int*)nullptr, hw, w.blk);
    hipLaunchKernelGGL(lp_scan_blocks_kernel, dim3(1), dim3(LP_THREADS), 0, stream, w.blk, nblk, w.head);
    hipLaunchKernelGGL(lp_compact_kernel, dim3(nblk), dim3(LP_THREADS), 0, stream, pred, hw, w.blk, w.pts);
    return mte_check_launch();
}

int mte_lidar_perturb(const float* depth, int H, int W, int n, double scale_d0, const double* add_i, const double* add_j, const double* add_d,
                      void* work, hipStream_t stream) {
    if (!depth || !work || !lp_shape_ok(H, W) || ((uintptr_t)work & 7) || n <= 0 || n > H * W || !add_i || !add_j || !add_d) return MTE_ERR_ARG;
    const int hw = H * W, nblk = (int)lp_blocks(n);
    const LpWork w = lp_carve(work, hw);
    hipLaunchKernelGGL(lp_init_kernel, dim3(lp_grid(hw)), dim3(LP_THREADS), 0, stream, w.winner, hw, w.minkey);
    hipLaunchKernelGGL(lp_keys_kernel, dim3(lp_grid(n)), dim3(LP_THREADS), 0, stream, depth, H, W, n, (const int*)w.head, scale_d0, add_i, add_j, add_d,
                       (const int*)w.pts, w.cell, w.dprime, w.winner, w.minkey);
    const Survivor pred{w.cell, w.winner, w.minkey, H, W};
    hipLaunchKernelGGL(lp_count_kernel<Survivor>, dim3(nblk), dim3(LP_THREADS), 0, stream, pred, (const int*)w.head, n, w.blk);
    hipLaunchKernelGGL(lp_scan_blocks_kernel, dim3(1), dim3(LP_THREADS), 0, stream, w.blk, nblk, w.head + 1);
    hipLaunchKernelGGL(lp_rank_kernel, dim3(nblk), dim3(LP_THREADS), 0, stream, pred, n, (const int*)w.head, (const int*)w.blk, w.rank);
    return mte_check_launch();
}

int mte_lidar_scatter(int H, int W, int n, const unsigned char* keep, int n_keep, float* out, const void* work, hipStream_t stream) {
    if (!out || !lp_shape_ok(H, W) || n < 0 || n > H * W || n_keep < 0 || n_keep > n || (n_keep > 0 && !keep)) return MTE_ERR_ARG;
    const int hw = H * W;
    if (n == 0 || n_keep == 0)                             // an empty map, or nothing survived / everything is dropped: zeros, the workspace is not read
        return mte_memset_async(out, 0, sizeof(float) * (size_t)hw, stream) == hipSuccess ? MTE_OK : MTE_ERR_LAUNCH;
    if (!work || ((uintptr_t)work & 7)) return MTE_ERR_ARG;
    const LpWork w = lp_carve(const_cast<void*>(work), hw);
    hipLaunchKernelGGL(lp_gather_kernel, dim3(lp_grid(hw)), dim3(LP_THREADS), 0, stream, (const int*)w.winner, (const int*)w.rank, (const double*)w.dprime, keep,
                       n_keep, n, (const int*)w.head, out, hw);
    return mte_check_launch();
}

long mte_batch_lidar_perturb_work_bytes(int B, int H, int W) { return (B > 0 && B <= 65535 && lp_shape_ok(H, W)) ? (long)B * lb_stride((long)H * W) : 0; }

int mte_batch_lidar_perturb(const float* lidar, int B, int H, int W, const unsigned char* arena, long arena_bytes, const long* table_host,
                            const long* table_dev, float* out, void* work, int* status, hipStream_t stream) {
    if (!lidar || !arena || !table_host || !table_dev || !out || !work || !status || B <= 0 || B > 65535 || !lp_shape_ok(H, W) || arena_bytes <= 0 ||
        ((uintptr_t)work & 7))
        return MTE_ERR_ARG;
    const int hw = H * W;
    long max_n = 0;
    for (int b = 0; b < B; ++b) {                          // every index a kernel forms from the table is bounded here
        const long* r = table_host + (long)b * LB_ROW_WORDS;
        const long n = r[LB_N], m = r[LB_SURVIVORS];
        if (n < 0 || n > hw || m < 0 || m > n) return MTE_ERR_ARG;
        for (int c = LB_ADD_I; c <= LB_ADD_D; ++c)
            if (r[c] < 0 || r[c] > arena_bytes || 8 * n > arena_bytes - r[c] || ((uintptr_t)(arena + r[c]) & 7)) return MTE_ERR_ARG;
        if (r[LB_KEEP] < 0 || r[LB_KEEP] > arena_bytes || m > arena_bytes - r[LB_KEEP]) return MTE_ERR_ARG;
        if (n > max_n) max_n = n;
    }
    const long stride = lb_stride(hw);
    const int nblk_hw = (int)lp_blocks(hw), nblk_n = max_n > 0 ? (int)lp_blocks(max_n) : 1;      // nblk_n <= nblk_hw: inside every sample's blk
    const dim3 th(LP_THREADS);
    hipLaunchKernelGGL(lb_count_valid_kernel, dim3(nblk_hw, B), th, 0, stream, lidar, hw, work, stride);
    hipLaunchKernelGGL(lb_scan_kernel, dim3(1, B), th, 0, stream, hw, nblk_hw, 0, work, stride);
    hipLaunchKernelGGL(lb_compact_kernel, dim3(nblk_hw, B), th, 0, stream, lidar, hw, work, stride);
    hipLaunchKernelGGL(lb_init_kernel, dim3(lp_grid(hw), B), th, 0, stream, hw, work, stride);
    hipLaunchKernelGGL(lb_keys_kernel, dim3(lp_grid(max_n), B), th, 0, stream, lidar, H, W, table_dev, arena, work, stride);
    hipLaunchKernelGGL(lb_count_survivors_kernel, dim3(nblk_n, B), th, 0, stream, H, W, table_dev, arena, work, stride);
    hipLaunchKernelGGL(lb_scan_kernel, dim3(1, B), th, 0, stream, hw, nblk_n, 1, work, stride);
    hipLaunchKernelGGL(lb_rank_kernel, dim3(nblk_n, B), th, 0, stream, H, W, table_dev, arena, work, stride);
    hipLaunchKernelGGL(lb_gather_kernel, dim3(lp_grid(hw), B), th, 0, stream, hw, table_dev, arena, work, stride, out, status);
    return mte_check_launch();
}

int mte_lidar_project(const double* points, int N, const double* K, const float* depth_map, float* out, int H, int W, int* winner_ws, hipStream_t stream) {
    if (!K || !out || !winner_ws || !lp_shape_ok(H, W) || N < 0 || (N > 0 && !points)) return MTE_ERR_ARG;
    const int hw = H * W;
    if (mte_memset_async(winner_ws, 0xff, sizeof(int) * (size_t)hw, stream) != hipSuccess) return MTE_ERR_LAUNCH;      // -1
    if (N > 0) hipLaunchKernelGGL(lp_project_scatter_kernel, dim3(lp_grid(N)), dim3(LP_THREADS), 0, stream, points, N, K, H, W, winner_ws);
    hipLaunchKernelGGL(lp_project_gather_kernel, dim3(lp_grid(hw)), dim3(LP_THREADS), 0, stream, points, N, K, (const int*)winner_ws, depth_map, out, hw);
    return mte_check_launch();
}

}  // extern "C"
