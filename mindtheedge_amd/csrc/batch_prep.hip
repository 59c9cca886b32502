// Batched training-target preparation on device for gfx950: the per-sample work of data_prep.hip (edge / depth preserve-resize, the
// edge maps' conditional /255, the normals' de-quantisation) for every map of a batch at once, over a descriptor table, reading the
// raw file contents (uint8 / uint16 / float32) straight from the batch's upload arena and writing into the collated [B,1,H_s,W_s]
// float32 tensors.  The number of launches does not depend on the batch size or on the number of maps:
//   fill      winner words = -1 and the per-map maxima = -1                            (one fill kernel)
//   scatter   every valid source pixel of the crop window claims its target pixel, the largest raster index wins (atomicMax, int)
//   gather    every target pixel takes its winner's value (0 without one); EDGE_U8 maps also leave their maximum (atomicMax on the
//             float's bits: the values are >= 0, so the bits order like the values); NORMAL_U8 maps are converted pixel by pixel
//   scale     EDGE_U8 maps whose maximum, AFTER the resize, is > 1 are put on the 0..1 scale (x float32(1/255), see bp_scale_kernel); the others stay
// Integer atomics only: bit-reproducible.  Rules and arithmetic are those of rdp_scatter_kernel / rdp_gather_kernel /
// u8_to_target_kernel (data_prep.hip) and of datasets/kitti_edges.py::prepare_edge_sample, which decides the edge scale per map on
// the host; here the decision stays on the device.  Byte / index work, HBM- and launch-bound.
#include "common.hpp"

namespace {

enum { KIND_EDGE_U8 = 0, KIND_SPARSE_U16 = 1, KIND_SPARSE_F32 = 2, KIND_NORMAL_U8 = 3, KIND_COUNT = 4 };
enum { R_KIND = 0, R_SRC_OFF, R_SRC_H, R_SRC_W, R_CROP_X, R_CROP_Y, R_CROP_H, R_CROP_W, R_DST_OFF, R_DST_H, R_DST_W, R_RESERVED, ROW_WORDS };

struct Map {
    int kind, src_w, crop_x, crop_y, crop_h, crop_w, H, W;
    long src_off, dst_off;
};

__device__ __forceinline__ Map load_map(const long* __restrict__ table, int m) {
    const long* r = table + (long)m * ROW_WORDS;
    Map d;
    d.kind = (int)r[R_KIND]; d.src_off = r[R_SRC_OFF]; d.src_w = (int)r[R_SRC_W];
    d.crop_x = (int)r[R_CROP_X]; d.crop_y = (int)r[R_CROP_Y]; d.crop_h = (int)r[R_CROP_H]; d.crop_w = (int)r[R_CROP_W];
    d.dst_off = r[R_DST_OFF]; d.H = (int)r[R_DST_H]; d.W = (int)r[R_DST_W];
    return d;
}

// the value of pixel k (raster index inside the crop window) as the per-sample path hands it to resize_depth_preserve
__device__ __forceinline__ float load_value(const unsigned char* __restrict__ arena, const Map& d, int k) {
    const int y = k / d.crop_w, x = k - y * d.crop_w;
    const long p = (long)(d.crop_y + y) * d.src_w + d.crop_x + x;
    if (d.kind == KIND_SPARSE_U16) return (float)((const unsigned short*)(arena + d.src_off))[p] / 256.f;     // 0 stays 0: "no return"
    if (d.kind == KIND_SPARSE_F32) return ((const float*)(arena + d.src_off))[p];
    return (float)arena[d.src_off + p];
}

__global__ __launch_bounds__(256) void bp_scatter_kernel(const unsigned char* __restrict__ arena, const long* __restrict__ table,
                                                         int* __restrict__ winner) {
    const Map d = load_map(table, blockIdx.y);
    if (d.kind == KIND_NORMAL_U8) return;
    const int n = d.crop_h * d.crop_w;
    const double sy = (double)d.H / (double)d.crop_h, sx = (double)d.W / (double)d.crop_w;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (!(load_value(arena, d, i) > 0.f)) continue;
        const int y = i / d.crop_w, x = i - y * d.crop_w;
        const int ty = (int)((double)y * sy), tx = (int)((double)x * sx);
        if (ty < d.H && tx < d.W) atomicMax(&winner[d.dst_off + (long)ty * d.W + tx], i);      // raster order: the largest source index wins
    }
}

__global__ __launch_bounds__(256) void bp_gather_kernel(const unsigned char* __restrict__ arena, const long* __restrict__ table,
                                                        const int* __restrict__ winner, int* __restrict__ map_max, float* __restrict__ out) {
    const Map d = load_map(table, blockIdx.y);
    const int HW = d.H * d.W;
    // a normal is a function of one byte: the 256 values once per workgroup (u8_to_target_kernel's expression, in double) instead of a
    // double-precision division per pixel
    __shared__ float normal_of[256];
    if (d.kind == KIND_NORMAL_U8) {                                                            // (the whole workgroup: one map per blockIdx.y)
        normal_of[threadIdx.x] = (float)((360.0 * ((double)threadIdx.x / 255.0) + -180.0) * (3.141592653589793 / 180.0));
        __syncthreads();
    }
    int top = 0;                                                                               // bits of the largest value this thread wrote
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        float v;
        if (d.kind == KIND_NORMAL_U8) {
            v = normal_of[(int)load_value(arena, d, i)];                                       // crop window == target
        } else {
            const int k = winner[d.dst_off + i];
            v = k < 0 ? 0.f : load_value(arena, d, k);
            top = max(top, __float_as_int(v));                                                 // v >= 0 here
        }
        out[d.dst_off + i] = v;
    }
    if (d.kind != KIND_EDGE_U8) return;                                                        // (the whole workgroup: one map per blockIdx.y)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
    __shared__ int wave_top[4];
    if ((threadIdx.x & 63) == 0) wave_top[threadIdx.x >> 6] = top;
    __syncthreads();
    if (threadIdx.x != 0) return;
    top = max(max(wave_top[0], wave_top[1]), max(wave_top[2], wave_top[3]));
    // One word per map takes the maxima of up to 256 workgroups on all XCDs: look first, most find their value (255, usually) already there.
    // A stale look only costs an atomic more; the maximum itself is the atomics'.
    if (top > __hip_atomic_load(&map_max[blockIdx.y], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&map_max[blockIdx.y], top);
}

__global__ __launch_bounds__(256) void bp_scale_kernel(const long* __restrict__ table, const int* __restrict__ map_max, float* __restrict__ out) {
    const Map d = load_map(table, blockIdx.y);
    if (d.kind != KIND_EDGE_U8 || !(map_max[blockIdx.y] > __float_as_int(1.f))) return;       // resized.max() > 1, per map
    const int HW = d.H * d.W;
    // prepare_edge_sample computes `resized / 255.0` with the tensor library, whose division by a host scalar is a multiplication by the
    // scalar's float32 reciprocal (1 ulp off the true quotient for about half of the 255 values); the batches must equal its bit for bit
    const float inv = 1.f / 255.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) out[d.dst_off + i] = out[d.dst_off + i] * inv;
}

inline unsigned grid_for(long total) { long g = (total + 255) / 256; if (g > 256) g = 256; if (g < 1) g = 1; return (unsigned)g; }

}  // namespace

extern "C" {

int mte_batch_prep(const unsigned char* arena, long arena_bytes, const long* table_host, const long* table_dev, int n_maps, float* out,
                   long out_elems, int* work, long winner_elems, hipStream_t stream) {
    if (!arena || !table_host || !table_dev || !out || !work || n_maps <= 0 || n_maps > 65535 || arena_bytes <= 0 || out_elems <= 0 ||
        winner_elems < 0 || winner_elems > out_elems)
        return MTE_ERR_ARG;
    long max_src = 1, max_dst = 1;
    for (int m = 0; m < n_maps; ++m) {                                    // every index a kernel forms below is bounded here
        const long* r = table_host + (long)m * ROW_WORDS;
        const long kind = r[R_KIND], off = r[R_SRC_OFF], h = r[R_SRC_H], w = r[R_SRC_W], cx = r[R_CROP_X], cy = r[R_CROP_Y], ch = r[R_CROP_H],
                   cw = r[R_CROP_W], dst = r[R_DST_OFF], H = r[R_DST_H], W = r[R_DST_W];
        if (kind < 0 || kind >= KIND_COUNT) return MTE_ERR_ARG;
        const long esize = kind == KIND_SPARSE_U16 ? 2 : kind == KIND_SPARSE_F32 ? 4 : 1;
        if (h <= 0 || w <= 0 || H <= 0 || W <= 0 || h >= (1L << 30) || w >= (1L << 30) || H >= (1L << 30) || W >= (1L << 30) ||
            h * w >= (1L << 30) || H * W >= (1L << 30))
            return MTE_ERR_ARG;
        if (off < 0 || off > arena_bytes || h * w * esize > arena_bytes - off || ((uintptr_t)(arena + off)) % esize != 0) return MTE_ERR_ARG;
        if (cx < 0 || cy < 0 || ch <= 0 || cw <= 0 || cx > w - cw || cy > h - ch) return MTE_ERR_ARG;
        if (dst < 0 || dst > out_elems || H * W > out_elems - dst) return MTE_ERR_ARG;
        if (kind == KIND_NORMAL_U8) {
            if (ch != H || cw != W) return MTE_ERR_ARG;                   // a normal map of another size goes through mte_resize_linear
        } else if (H * W > winner_elems - dst) {
            return MTE_ERR_ARG;
        }
        if (ch * cw > max_src) max_src = ch * cw;
        if (H * W > max_dst) max_dst = H * W;
    }
    int* map_max = work + winner_elems;
    if (mte_memset_async(work, 0xff, sizeof(int) * (size_t)(winner_elems + n_maps), stream) != hipSuccess) return MTE_ERR_LAUNCH;      // -1
    hipLaunchKernelGGL(bp_scatter_kernel, dim3(grid_for(max_src), n_maps), dim3(256), 0, stream, arena, table_dev, work);
    hipLaunchKernelGGL(bp_gather_kernel, dim3(grid_for(max_dst), n_maps), dim3(256), 0, stream, arena, table_dev, work, map_max, out);
    hipLaunchKernelGGL(bp_scale_kernel, dim3(grid_for(max_dst), n_maps), dim3(256), 0, stream, table_dev, map_max, out);
    return mte_check_launch();
}

}  // extern "C"
