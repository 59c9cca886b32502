// Workspace layout of the LiDAR index / perturbation stages (lidar_prep.hip), shared with the kernels that read the raster-order list of
// valid pixels mte_lidar_index leaves there (depth_viz.hip: mte_d3r_count).
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_ITEMS = 8;                               // consecutive elements per thread: raster order inside a workgroup
constexpr int LP_CHUNK = LP_THREADS * LP_ITEMS;           // elements per workgroup of the scans
constexpr int LP_HEAD = 16;                               // ints in front of the workspace: [0] n, [1] n', [2..3] the smallest key (64 bit)
constexpr int LP_NONE = 0x7fffffff;                       // "no point landed here" in the winner map

struct LpWork {                                           // the caller's workspace, carved up; hw = H * W
    int* head; long long* minkey; int* blk; int* pts; int* winner; int* rank; int* cell; double* dprime;
};
__host__ __device__ inline long lp_blocks(long hw) { return (hw + LP_CHUNK - 1) / LP_CHUNK; }
__host__ __device__ inline long lp_round4(long v) { return (v + 3) & ~3L; }
inline long lp_work_bytes(long hw) { return 4 * (LP_HEAD + lp_round4(lp_blocks(hw)) + 4 * lp_round4(hw)) + 8 * hw; }
__host__ __device__ inline LpWork lp_carve(void* work, long hw) {
    LpWork w;
    w.head = (int*)work;
    w.minkey = (long long*)(w.head + 2);
    w.blk = w.head + LP_HEAD;
    w.pts = w.blk + lp_round4(lp_blocks(hw));
    w.winner = w.pts + lp_round4(hw);
    w.rank = w.winner + lp_round4(hw);
    w.cell = w.rank + lp_round4(hw);
    w.dprime = (double*)(w.cell + lp_round4(hw));         // 16 + 4 * (multiples of 4) ints in front: 8-byte aligned when `work` is
    return w;
}

}  // namespace
