/* mte_kernels.h -- C ABI of libmte_hip.so, the gfx950 (MI355X) kernel library underneath mindtheedge_amd.
 *
 * The reference (liortalker/MindTheEdge) has no native code and no FFI: every op below replaces a PyTorch
 * module call of the reference's hot path.  Each entry cites the reference call site it stands in for
 * (paths relative to packnet_code/packnet_sfm/).  A maintainer binds these with ctypes.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless noted
 *   - caller owns and pre-allocates every buffer (including scratch); no hidden allocation, no host sync;
 *     kernels are enqueued on `stream` and are re-entrant
 *   - return value: 0 = MTE_OK, negative = error (never throws):
 *       -1 MTE_ERR_ARG  -2 MTE_ERR_LAUNCH  -3 MTE_ERR_UNSUPPORTED
 *   - activations are NHWC ("pixel-major"): element (b,y,x,c) at ((b*H + y)*W + x)*ld + c, where `ld`
 *     (elements per pixel) >= C lets a tensor be a channel slice of a wider buffer (decoder concat buffers)
 *   - dtype: 0 = bf16 (raw 16-bit), 1 = fp32.  Channel counts / ld / slice offsets are multiples of 8
 *   - loss maps are fp32 [B,H,W] (the reference's [B,1,H,W])
 */
#ifndef MTE_KERNELS_H
#define MTE_KERNELS_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mte_stream_t; /* hipStream_t */

#define MTE_OK 0
#define MTE_ERR_ARG (-1)
#define MTE_ERR_LAUNCH (-2)
#define MTE_ERR_UNSUPPORTED (-3)
#define MTE_DT_BF16 0
#define MTE_DT_F32 1

/* ---- convolution: nn.Conv2d(k, stride 1) + ConstantPad2d(k//2)  (networks/layers/packnet/layers01.py:29-31,61,116-117)
 * y = conv(x, wpack) + bias.  wpack = [N][KH*KW][Cin_p] in `dtype` (see mte_pack_conv_weights).
 * Also the data-gradient: call with the "backward" pack and x := dy.
 * workspace (nullable): fp32 scratch of >= 2*B*H*W*N elements; when given, shapes with few output tiles and a long
 * reduction (pack4/pack5.conv at low resolution) are split along K over up to min(8, workspace_elems / (B*H*W*N)) workgroups
 * per tile.  Every split STORES its partial tile into its own [M][N] slab and a finish kernel adds the slabs in split order:
 * no floating-point atomics, the result is bit-reproducible and the workspace needs no clearing.
 * accumulate = 1: y += conv(x) (conv + bias rounded to the activation type, added to the old value in fp32, rounded again -- every tile form
 * alike): the second data gradient of an activation with two consumers
 * lands in the first one's buffer instead of going through a separate add.  `accumulate` is a bit set: MTE_CONV_ACCUMULATE (1) and
 * MTE_CONV_SOLO (2) = no kernel of another stream is expected to run beside this launch (forward pass, inference), so the 256 x 128
 * tile may use its 3-slot-ring variant that puts two workgroups on a CU and claims 148 of the 160 KB of LDS: measured 15-20 % faster
 * on the short-reduction layers when alone, but slower for the step when the weight-gradient stream needs LDS on the same CUs. */
#define MTE_CONV_ACCUMULATE 1
#define MTE_CONV_SOLO 2
int mte_conv2d_igemm(const void* x, long ldx, const void* wpack, const float* bias, void* y, long ldy, int out_f32,
                     int B, int H, int W, int Cin_p, int N, int KH, int KW, int dtype,
                     float* workspace, long workspace_elems, int accumulate, mte_stream_t stream);
/* Round 6: the data gradient of a folded pack layer (reference: networks/layers/packnet/layers01.py:214-250, PackLayerConv3d backward) written WITHOUT the
 * mte_pixel_shuffle pass behind it.  The N = 4 C output channels are the packed depths d = 4 c + s of the [B][H][W] packed grid; y is the un-shuffled tensor
 * [B][2H][2W][C] (pixel stride ldy): GEMM row (b, h, w), column d goes to y[b][2h + s / 2][2w + s % 2][c].  accumulate as in mte_conv2d_igemm (bit 0).  bf16.
 * Returns MTE_ERR_UNSUPPORTED where the launch would not take a tile form that stages its result in LDS (no K split, no 8-phase kernel): the caller then runs
 * mte_conv2d_igemm + mte_pixel_shuffle -- the results are bit-identical. */
int mte_conv2d_igemm_unshuffle(const void* x, long ldx, const void* wpack, void* y, long ldy,
                               int B, int H, int W, int Cin_p, int N, int KH, int KW, int dtype, int accumulate, mte_stream_t stream);
/* Library options.  MTE_OPT_GN_PREZEROED (0): when 1, the GroupNorm statistics / reduction / bias-gradient buffers handed to
 * mte_gn_stats and mte_gn_elu_bwd -- and, since round 4, that call's dgamma / dbeta -- are already zero (the caller clears one arena
 * per step with a single fill; a zeroed flat gradient buffer qualifies) and the library skips its own per-call fills. */
#define MTE_OPT_GN_PREZEROED 0
/* MTE_OPT_LOSS_PREZEROED (1): when 1, `work` of mte_edge_loss_multi_fwd and `sums` of mte_edge_loss_fwd are zero on entry (first
 * mte_edge_loss_work_elems / _sums_elems doubles; same arena) and the launch's own fill is skipped. */
#define MTE_OPT_LOSS_PREZEROED 1
/* MTE_OPT_HANDOFF_FENCES (2), round 5: when 1, the last-arriver hand-offs of the read-only reduction kernels (mte_gn_stats, the fused loss
 * forward) draw their arrival ticket behind an agent-scope RELEASE fence and the last arriver issues an agent-scope ACQUIRE before it reads
 * the other workgroups' records.  Off, the protocol is the one MI355X_MICROARCH.md's visibility table lists as measured-valid: records by
 * returning atomic exchanges (performed at the memory side), a drained wait, a relaxed agent-scope ticket, agent-scope atomic loads. */
#define MTE_OPT_HANDOFF_FENCES 2
/* MTE_OPT_WGRAD_SHARES_CHIP (3), round 5: 1 = the caller queues the weight-gradient launches (mte_conv2d_wgrad, mte_conv2d_patch_wgrad) on a stream of their own
 * beside the data-gradient chain; those kernels then aim for half a chip of workgroups, which is faster for the STEP (same box 23.59 -> 23.1 ms) although each launch
 * is slower on its own.  0 (default): one workgroup (group) per CU, the right geometry when nothing runs beside them. */
#define MTE_OPT_WGRAD_SHARES_CHIP 3
int mte_set_option(int option, int value);
/* Device error word, round 5.  Kernels whose workgroups wait for each other inside a launch (the GroupNorm cluster kernels) bound that wait;
 * a wait that gives up sets a flag in one word of pinned host memory instead of going on silently with incomplete statistics.
 * mte_device_error_init: allocate the word (once, outside stream capture).  mte_device_error_poll: -> flags set since the last poll
 * (MTE_DEVERR_*; 0 = none) and clears them; no synchronisation -- the host polls once per training step and raises.
 * (No reference counterpart: the reference's GroupNorm is one cuDNN call, layers01.py:32.) */
#define MTE_DEVERR_GN_CLUSTER_FWD 1
#define MTE_DEVERR_GN_CLUSTER_BWD 2
#define MTE_DEVERR_IMAGE_RESAMPLE 4 /* mte_image_resample_u8 was handed tables whose tap span exceeds that of the LANCZOS tables of (in, out) */
int mte_device_error_init(void);
int mte_device_error_poll(void);
/* weight gradient of the same conv into dw_stage = `stage_parts` x [N][KH*KW][Cin_p] fp32 (overwritten).  The reduction over
 * pixels is split over at most stage_parts workgroup groups; each one stores its PARTIAL gradient in its own part (plain stores;
 * *parts_out = parts written, mte_unpack_conv_wgrad adds them in part order: round 4 -- no floating-point atomics on the conv weight
 * gradient's path, the result does not depend on the order in which workgroups finish).  mte_unpack_conv_wgrad with parts > 32 uses
 * up to 32 further slabs BEHIND the parts as scratch: a stage of more than 32 parts is allocated with parts + 32 slabs.
 * MTE_ERR_ARG also for B, H, W, N, Cin_p, KH or KW below 1 and for a launch whose grid or block counts do not fit 32 bits. */
int mte_conv2d_wgrad(const void* x, long ldx, const void* dy, long ldy, float* dw_stage, int stage_parts, int* parts_out,
                     int B, int H, int W, int Cin_p, int N, int KH, int KW, int dtype, mte_stream_t stream);
/* 1 when mte_conv2d_wgrad takes this 3x3 bf16 layer with its nine-tap kernel (conv_wgrad9.hip: N % 128 == 0, Cin_p % 64 == 0, W % 32 == 0 or W % 16 == 0
 * and H even).  Round 5: measured faster than the LDS-patch weight gradient on every 128-output layer both take (128 -> 128 @96x320: 100.5 -> 84.9 us,
 * 192 -> 128: 147 -> 115), so the host asks this first. */
int mte_conv2d_wgrad_nine_tap(int H, int W, int Cin_p, int N, int KH, int KW, int dtype);
/* OIHW fp32 master weights -> forward pack [Cout][taps][Cin_p] and (optional) dgrad pack [Cin_p][taps rot180][Cout_p] */
int mte_pack_conv_weights(const float* w_oihw, void* wfwd, void* wbwd, int Cout, int Cin, int KH, int KW,
                          int Cin_p, int Cout_p, int dtype, mte_stream_t stream);
/* Every kernel-ready weight copy of `njobs` conv layers in ceil(njobs / 48) launches (the ~100 layers of the network after an
 * optimizer step: ~400 launch-bound per-layer launches otherwise).  `jobs` is a HOST array; per job, from the OIHW fp32 master `w`
 * [Cout][Cin][taps]: wf = forward pack [Cout][taps][Cin_p]; wb (nullable) = data-gradient pack [Cin_p][taps rot180][Cout]; pf / pb
 * (nullable, bf16 only) = the fragment-block packs of mte_conv2d_patch_fwd for wf / wb (mte_conv2d_patch_pack_elems(Cin_p, Cout, ..)
 * / (Cout, Cin_p, ..) elements).  end_* are scratch the library fills.  Same values as mte_pack_conv_weights + _patch_repack. */
typedef struct { const float* w; void* wf; void* wb; void* pf; void* pb; int Cout, Cin, taps, Cin_p; int end_f, end_b, end_pf, end_pb; } mte_pack_job;
int mte_pack_conv_weights_multi(const void* jobs, int njobs, int dtype, mte_stream_t stream);
/* dgrad pack derived from an existing forward pack */
int mte_pack_conv_weights_bwd(const void* wfwd, void* wbwd, int Cout, int KH, int KW, int Cin_p, int dtype, mte_stream_t stream);
/* sum of the `parts` partial stages -> OIHW fp32 gradient (drops channel padding).  The stage is scratch: with more than 32 parts
 * (LDS-patch weight gradient: one slab per workgroup) a parallel first level adds parts 1.. into part 0 before the transpose. */
int mte_unpack_conv_wgrad(float* dw_stage, int parts, float* dw_oihw, int Cout, int Cin, int KH, int KW, int Cin_p, mte_stream_t stream);
/* out[N] (overwritten) = column sums of y[M][N] (conv bias gradient).  N % 8 == 0 and at most 256 16-byte chunks per row (2048 bf16 / 1024 fp32
 * columns): more is MTE_ERR_UNSUPPORTED and leaves `out` as it was */
int mte_colsum(const void* y, long ld, long M, int N, float* out, int dtype, mte_stream_t stream);

/* ---- LDS-patch convolution for the high-resolution, few-channel layers (bf16, C_out <= 64, W % 32 == 0, k in {1,3,5,7}):
 * same math as mte_conv2d_igemm / mte_conv2d_wgrad, different tiling (the 8x32-pixel tile's input patch is staged once
 * per 32-channel slice and reused by all k*k taps).  *_supported and *_pack_elems are queries (they return a value).
 * mte_conv2d_patch_fwd: y = bf16(conv(x) + bias), fp32 sums rounded to nearest even once; accumulate = 1: y = bf16(float(bf16(conv(x) + bias)) + y), the two
 * roundings of mte_conv2d_igemm -- the two families are bit-identical wherever the fp32 sum does not depend on its order.  Pixel strides ldx >= Cin_p and
 * ldy >= N: channel slices of wider buffers are read and written in place, nothing outside the N output channels of a pixel is touched. */
int mte_conv2d_patch_supported(int W, int Cin_p, int N, int KH, int KW, int dtype);
int mte_conv2d_patch_wgrad_supported(int W, int Cin_p, int N, int KH, int KW, int dtype);   /* + 3x3 layers with 65..128 output channels (weight gradient only) */
long mte_conv2d_patch_pack_elems(int Cin_p, int N, int KH, int KW);
int mte_conv2d_patch_repack(const void* wgeneric, void* wpatch, int Cin_p, int N, int KH, int KW, mte_stream_t stream);
int mte_conv2d_patch_fwd(const void* x, long ldx, const void* wpatch, const float* bias, void* y, long ldy,
                         int B, int H, int W, int Cin_p, int N, int KH, int KW, int accumulate, mte_stream_t stream);
int mte_conv2d_patch_wgrad(const void* x, long ldx, const void* dy, long lddy, float* dw_stage, int stage_parts, int* parts_out,
                           int B, int H, int W, int Cin_p, int N, int KH, int KW, mte_stream_t stream);
/* round 5 -- mte_conv2d_patch_fwd that also leaves the GroupNorm(16) statistics of what it stores (reference layers01.py:35-38: Conv2d -> GroupNorm(16) -> ELU;
 * the reference's GroupNorm is a cuDNN call that reads the conv output again): one record of 32 floats (sum, sum of squares per group, fp32 over the tile's
 * pixels) per output tile, written in the store loop from the bf16 values being stored -- with `accumulate` from the sums.  rec: at least
 * mte_conv2d_patch_fwd_gn_elems(B, H, W) floats; *tiles_per_sample_out records per sample were written (tile height depends on the kernel form).
 * mte_gn_stats_from_records (below) adds them in tile order into the buffer mte_gn_stats would have filled: the stand-alone statistics pass over y
 * (252 MB per full-resolution layer at B = 8) is not run.  N % 16 == 0, else MTE_ERR_UNSUPPORTED.  Bit-reproducible (no atomics). */
long mte_conv2d_patch_fwd_gn_elems(int B, int H, int W);
int mte_conv2d_patch_fwd_gn(const void* x, long ldx, const void* wpatch, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N, int KH, int KW,
                            int accumulate, float* rec, long rec_elems, int* tiles_per_sample_out, mte_stream_t stream);

/* ---- stem convolution: exactly 8 input channels (the zero-padded rgb image), C_out <= 32, k in {3,5,7}, W % 32 == 0, bf16
 * (encoder.pre_calc = Conv2D(3, 32, 5, 1): networks/depth/PackNetSAN01.py:27, layers01.py:29-31).  With 8 channels a pixel is one
 * 16-byte chunk, so the reduction runs over (tap, channel) and an MFMA covers two taps: a quarter of the MFMA work the 32-channel
 * slices of the LDS-patch kernels spend on it.  wf = the GENERIC forward pack [N][taps][8] of mte_pack_conv_weights (no special pack);
 * _wgrad fills dw_stage like mte_conv2d_patch_wgrad (one slab per workgroup, *parts_out slabs, summed by mte_unpack_conv_wgrad).
 * The image needs no data gradient. */
int mte_conv2d_stem_supported(int W, int Cin_p, int N, int KH, int KW, int dtype);
int mte_conv2d_stem_fwd(const void* x, long ldx, const void* wf, const float* bias, void* y, long ldy,
                        int B, int H, int W, int N, int KH, int KW, mte_stream_t stream);
int mte_conv2d_stem_wgrad(const void* x, long ldx, const void* dy, long lddy, float* dw_stage, int stage_parts, int* parts_out,
                          int B, int H, int W, int N, int KH, int KW, mte_stream_t stream);

/* ---- GroupNorm(16, C) + ELU, optionally over y1 + scale2[b,c]*y2 (residual tail with Dropout2d)
 *      (layers01.py:32-38 Conv2D; layers01.py:62-73 ResidualConv)
 * A statistics buffer is mte_gn_stats_elems(B) doubles: [B][16][2] (sum, sum of squares) -- what mte_gn_elu_fwd / _bwd read --
 * followed by the statistics pass's workspace (one arrival ticket per sample, which must be zero on entry -- cleared here unless
 * MTE_OPT_GN_PREZEROED -- and one record per workgroup).  The pass uses no floating-point atomics: per-thread sums, fixed wave
 * butterflies, waves in order, and the LAST workgroup of a sample adds the workgroup records in slot order, so the forward pass is
 * bit-reproducible run to run and under HIP-graph replay (round 3; the fp32 LDS / fp64 global atomics it replaces made two
 * forward passes of one frame differ by 1-2 % in inverse depth after ~60 bf16 layers). */
long mte_gn_stats_elems(int B);
int mte_gn_stats(const void* y1, long ld1, const void* y2, long ld2, const float* scale2, double* stats,
                 int B, int HW, int C, int dtype, mte_stream_t stream);
/* round 5: the same sums from the per-tile records a convolution left in its store loop (mte_conv2d_patch_fwd_gn): stats[b][group][2] = the
 * tiles_per_sample records of sample b added in tile order (fp64).  Only the first 32 B doubles of `stats` are written. */
int mte_gn_stats_from_records(const float* rec, int tiles_per_sample, double* stats, int B, mte_stream_t stream);
/* mte_gn_elu_fwd: stats_ready = 1: `stats` holds the sums of mte_gn_stats.  stats_ready = 0 (allowed where
 * mte_gn_fwd_is_single_pass(HW, C, y2 != NULL, dtype) returns 1: a (sample, group) slab fits one workgroup's registers): the
 * kernel loads each slab ONCE, computes its statistics on chip, normalises and stores `stats` in the same format as an
 * OUTPUT for the backward pass -- the forward is then one read + one write, and mte_gn_stats is not called.
 * mte_gn_elu_bwd takes the matching one-pass route by itself where the slab of (y, dz) fits (low-resolution layers).
 * (development knob 13 of the -DMTE_DEV build: 0 = streaming two-pass kernels everywhere.) */
int mte_gn_fwd_is_single_pass(int HW, int C, int has_y2, int dtype);
/* Round 4: the same route for slabs too large for one workgroup (512 channels at 24x80, 256 at 48x160, 128 at 96x320): a CLUSTER of
 * 2-8 workgroups holds the slab in registers and exchanges its partial sums through the record area of `stats` (fixed order:
 * bit-reproducible; the whole buffer must be zero at entry -- MTE_OPT_GN_PREZEROED callers guarantee it, otherwise the library clears it).
 * The cluster's size depends on the batch, so callers that know B ask mte_gn_fwd_is_single_pass_b; stats_ready = 0 is allowed wherever it
 * returns 1.  Replaces the same reference ops (nn.GroupNorm(16, C) + nn.ELU of Conv2D, layers01.py:32-38; residual tail :62-73).
 * (development knob 25 of the -DMTE_DEV build: 0 = no cluster kernels.) */
int mte_gn_fwd_is_single_pass_b(int B, int HW, int C, int has_y2, int dtype);
int mte_gn_elu_fwd(const void* y1, long ld1, const void* y2, long ld2, const float* scale2, double* stats, int stats_ready,
                   const float* gamma, const float* beta, void* z, long ldz,
                   int B, int HW, int C, float eps, int dtype, mte_stream_t stream);
/* mte_gn_elu_bwd: y2 = NULL with scale2 and d2 given (round 5, the backward of mte_gn_tail_fwd's outer norm): ONE input tensor, but the
 * gradient leaves twice -- d1 = dv and d2 = scale2[b,c] * dv -- and dbias, if asked, is the column sum of d2.  d2 without y2 AND without scale2 is
 * MTE_ERR_ARG (there is no factor to form it with). */
int mte_gn_elu_bwd(const void* dz, long lddz, const void* y1, long ld1, const void* y2, long ld2, const float* scale2,
                   const double* stats, const float* gamma, const float* beta, float* red,
                   void* d1, long ldd1, void* d2, long ldd2, float* dgamma, float* dbeta, float* dbias,
                   int B, int HW, int C, float eps, int dtype, mte_stream_t stream);
/* Round 5 -- the tail of a residual block in two launches: ResidualConv.forward's `self.activ(self.normalize(x_out + shortcut))` with
 * x_out = conv2's GroupNorm + ELU applied on the fly (layers01.py:35-38 and :69-73).
 *   y1 = conv2's CONVOLUTION output (+ bias), stats1 = its sums (mte_gn_stats), gamma1 / beta1 = conv2.normalize;
 *   y2 = the 1x1 shortcut's output, scale2 = Dropout2d's keep / (1 - p) per (sample, channel) or NULL;
 *   t  = ELU(GN(y1)) + scale2 * y2 -- an OUTPUT in the activation type, the tensor both backward norms need -- with its statistics in stats_t
 *        (a statistics buffer, tickets zero at entry; bit-reproducible like mte_gn_stats);  z = ELU(GN_t(t)) with gamma_t / beta_t = the block's normalize.
 * Against the four launches it replaces (mte_gn_elu_fwd of conv2, mte_gn_stats and mte_gn_elu_fwd over two tensors): 6 tensor passes instead of 8, and the
 * backward of the outer norm reads one tensor instead of two in both of its passes. */
int mte_gn_tail_fwd(const void* y1, long ld1, const double* stats1, const float* gamma1, const float* beta1,
                    const void* y2, long ld2, const float* scale2, void* t, long ldt, double* stats_t,
                    const float* gamma_t, const float* beta_t, void* z, long ldz,
                    int B, int HW, int C, float eps, int dtype, mte_stream_t stream);

/* ---- 3-D packing / unpacking stencils: packing + nn.Conv3d(1,4,3,pad 1) (+ view / PixelShuffle)
 *      (layers01.py:127-149, 214-248 PackLayerConv3d; 251-287 UnpackLayerConv3d).  H,W,C describe x.
 * Rounding contract, every kernel form alike: w3 and b3 are fp32 and enter as they are (the matrix-core forms multiply with bf16(w) and
 * bf16(w - bf16(w)), which together are w to 16 bits and exactly w for integers below 2^16); products and sums are fp32; out / dx are rounded
 * ONCE, to nearest even, to the activation type; dwb[112] = (dw3[108], db3[4]) is fp32, cleared by the call and summed with float atomics.
 * The one exception is not in the shipped library: the P3_ONE_BF16_WEIGHT forms of the development build (mte_debug_set(1, 300 + bits) with bit 4,
 * csrc/p3_plan.hpp) multiply with bf16(w) alone -- each weight rounded once, to nearest even -- and are otherwise as above: their result is the
 * operation on those rounded weights.  tests/test_gpu_conv3d_exact.py pins all of this bit for bit on integer operands. */
int mte_pack3d_fwd(const void* x, long ldx, const float* w3, const float* b3, void* out, long ldo,
                   int B, int H, int W, int C, int dtype, mte_stream_t stream);
int mte_pack3d_bwd_data(const void* dout, long ldo, const float* w3, void* dx, long lddx,
                        int B, int H, int W, int C, int dtype, mte_stream_t stream);
int mte_pack3d_bwd_weight(const void* x, long ldx, const void* dout, long ldo, float* dwb,
                          int B, int H, int W, int C, int dtype, mte_stream_t stream);
int mte_unpack3d_fwd(const void* x, long ldx, const float* w3, const float* b3, void* out, long ldo,
                     int B, int H, int W, int C, int dtype, mte_stream_t stream);
int mte_unpack3d_bwd_data(const void* dout, long ldo, const float* w3, void* dx, long lddx,
                          int B, int H, int W, int C, int dtype, mte_stream_t stream);
int mte_unpack3d_bwd_weight(const void* x, long ldx, const void* dout, long ldo, float* dwb,
                            int B, int H, int W, int C, int dtype, mte_stream_t stream);

/* ---- conv3d folded into the pack convolution (see csrc/pack_fold.hip): exact away from the border; kernels.PackFoldedConvFn
 *      recomputes the k/2-pixel border bands with the unfolded kernels.  (layers01.py:241-247) */
int mte_fold_pack_weights(const float* W, const float* K3, const float* b, const float* b3, float* Wf, float* bf,
                          int Co, int D, int k, mte_stream_t stream);
int mte_unfold_pack_wgrad(const float* dWf, const float* dbf, const float* W, const float* K3, const float* b3,
                          float* dW, float* dk3b, int Co, int D, int k, int accumulate, mte_stream_t stream);
int mte_pixel_shuffle(const void* src, long lds_, void* dst, long ldd, int B, int H, int W, int C, int dir, int dtype, mte_stream_t stream);
int mte_copy_rect(const void* src, long lds_, int Hs, int Ws, int sy, int sx, void* dst, long ldd, int Hd, int Wd, int dy, int dx,
                  int B, int h, int w, int C, int mode, int dtype, mte_stream_t stream);
/* the same for up to 8 rectangles in ONE launch; ops = HOST array of n records (device pointers inside) */
typedef struct { const void* src; long lds_; int Hs, Ws, sy, sx; void* dst; long ldd; int Hd, Wd, dy, dx, h, w, mode; } mte_rect_op;
int mte_copy_rects(const void* ops, int n, int B, int C, int dtype, mte_stream_t stream);

/* ---- the exact border of a folded pack layer from a one-pixel ring (csrc/pack_border.hip, index arithmetic csrc/pack_border_plan.hpp).
 *      The folded convolution runs over ALL pixels; within pad = k/2 pixels of the border it has seen conv3d's values outside the image, which the
 *      reference (layers01.py:241-247, zero padding between conv3d and the k x k conv) does not.  They depend on the data only on the ring at
 *      distance 1:  y_ref = y_fold - sum_{t: p+t on ring} W[t] . U(p+t) - sum_{t: p+t outside} S[t],  S[co][t] = sum_f b3[f] sum_d W[co][f*D+d][t].
 *   P [B][H2][W2][D = 4C] is the packed tensor (pixel stride ldp).  Ring lines: R_rows [2B][W2+2][4D] = top then bottom row over x' = -1 .. W2,
 *   R_cols [2B][H2][4D] = left then right column, contiguous, activation type; they hold U (conv3d's data part, no bias; fp32 sums rounded once).
 *   The ring terms are two GEMMs per pass through mte_conv2d_igemm / mte_conv2d_wgrad: KH = 1, KW = k over R_rows and KH = k, KW = 1 over R_cols,
 *   with N = 2 pad Co output columns (far edge, distance j, co) -> (far * pad + j) * Co + co and the NEGATED weights of mte_pack_border_weights
 *   (row j of the near edge uses tap row pad-1-j, of the far edge pad+1+j; columns alike), results corr_rows [2B][W2+2][N] / corr_cols [2B][H2][N] in fp32 (out_f32 = 1).
 *   mte_pack_border_apply adds them and the class table Dt [(2 pad + 1)^2][Co] to the border pixels of y in place, rounding once.
 *   Backward: mte_pack_border_gather forms the GEMMs' gradient operand G_rows [2B][W2+2][N] / G_cols [2B][H2][N] from dy (zeros in the cross
 *   blocks and at the rows' end positions); mte_pack_ring_bwd_data ACCUMULATES the ring stencil's transpose into the un-shuffled input gradient
 *   dx [B][2 H2][2 W2][C] (its two outermost rows / columns); mte_pack_ring_bwd_weight adds the conv3d weight gradient to dk3 [108];
 *   mte_pack_border_class_sums + mte_pack_border_scatter turn the ring-weight gradients and the class sums of dy into the dw_band argument of
 *   mte_unfold_pack_wgrad (overwritten) and add the class path's db3 to dk3b [108 .. 112).  All sums have a fixed order: bit-reproducible.
 *   Needs D % 32 == 0, Co % 8 == 0, k = 3 or 5, H2 and W2 >= 2 pad (smaller images and larger kernels: MTE_ERR_ARG; the host folds a layer only
 *   where kernels.pack_fold_applicable allows it and runs the un-folded layer otherwise).  The *_elems queries size the fp32 work buffers (overwritten by the calls). */
long mte_pack_ring_work_elems(void);
long mte_pack_border_scatter_work_elems(int Co, int k);
long mte_pack_border_class_sums_elems(int Co, int k);
int mte_pack_ring_fwd(const void* P, long ldp, const float* K3, void* R_rows, void* R_cols, int B, int H2, int W2, int D, int dtype, mte_stream_t stream);
int mte_pack_ring_bwd_data(const void* dR_rows, const void* dR_cols, const float* K3, void* dx, long lddx, int B, int H2, int W2, int D, int dtype,
                           mte_stream_t stream);
int mte_pack_ring_bwd_weight(const void* dR_rows, const void* dR_cols, const void* P, long ldp, float* dk3, float* work, int B, int H2, int W2, int D,
                             int dtype, mte_stream_t stream);
int mte_pack_border_weights(const float* W, const float* b3, float* Wr, float* Wc, float* Dt, int Co, int D, int k, mte_stream_t stream);
int mte_pack_border_apply(void* y, long ldy, const float* corr_rows, const float* corr_cols, const float* Dt, int B, int H2, int W2, int Co, int k,
                          int dtype, mte_stream_t stream);
int mte_pack_border_gather(const void* dy, long lddy, void* G_rows, void* G_cols, int B, int H2, int W2, int Co, int k, int dtype, mte_stream_t stream);
int mte_pack_border_class_sums(const void* dy, long lddy, float* part, int B, int H2, int W2, int Co, int k, int dtype, mte_stream_t stream);
int mte_pack_border_scatter(const float* dWr, const float* dWc, const float* part, const float* W, const float* b3, float* dW, float* dk3b, float* work,
                            int Co, int D, int k, mte_stream_t stream);
/* The forward ring terms in ONE grouped split-K launch (csrc/pack_border_gemm.hip, launch plan plan_pack_border_gemm in csrc/pack_border_plan.hpp), bf16:
 *   line-batch (far', b) only uses the columns (far, j, co) with far == far', so the two GEMMs are four of half the width (ring rows / columns x near / far
 *   edge); one grid covers their 128 x 64 tiles times `splits` slices of K = k * C16 (C16 = 4D = 16C channels of a ring line), chosen so that the launch
 *   fills the chip.  Slice s leaves its partial tile in slab s of its family: ws = fp32 [splits][2B][W2+2][N] then [splits][2B][H2][N], each slab in the
 *   layout of corr_rows / corr_cols (columns with far != far' are not written).  mte_pack_border_apply_slabs = mte_pack_border_apply reading that
 *   workspace: every term is the sum of its slabs in slab order, formed where it is added to y.  No atomics, fixed order: bit-reproducible.
 *   mte_pack_border_gemm_ws_elems returns the workspace's fp32 elements and stores the slice count in *splits, or MTE_ERR_UNSUPPORTED (as the launch does)
 *   for fp32 and for shapes outside C16 % 32 == 0, Co % 8 == 0, k = 3 or 5: the caller then takes the two mte_conv2d_igemm launches + mte_pack_border_apply.
 *   Wr_pack / Wc_pack: the forward packs [N][k][C16] of mte_pack_border_weights' Wr / Wc (mte_pack_conv_weights).  force_splits: 0; tests pass a slice count. */
long mte_pack_border_gemm_ws_elems(int B, int H2, int W2, int C16, int Co, int k, int dtype, int force_splits, int* splits);
int mte_pack_border_gemm_fwd(const void* R_rows, const void* R_cols, const void* Wr_pack, const void* Wc_pack, float* ws, long ws_elems, int B, int H2, int W2,
                             int C16, int Co, int k, int dtype, int force_splits, mte_stream_t stream);
int mte_pack_border_apply_slabs(void* y, long ldy, const float* ws, int splits, const float* Dt, int B, int H2, int W2, int Co, int k, int dtype,
                                mte_stream_t stream);

/* ---- InvDepth head: sigmoid(conv3x3(x) + b) / min_depth  (layers01.py:99-123) */
int mte_invdepth_fwd(const void* x, long ldx, const float* w, const float* bias, float* out,
                     int B, int H, int W, int C, float min_depth, int dtype, mte_stream_t stream);
/* backward, two independent halves: _data writes dlogit [B,H,W] (fp32 scratch, also the input of _weight) and dx;
 * _weight writes dwb [C*9 + 1] = (dW OIHW, db): every workgroup stores one record of its sums into `records`
 * (mte_invdepth_bwd_weight_workspace_elems(C) floats of scratch) and a second small launch adds the records in a fixed order
 * (no atomics: the C*9+1 contended adds per workgroup cost as much as the stream itself on the 256-channel head) */
int mte_invdepth_bwd_data(const float* w, const float* inv_out, const float* dout, float* dlogit,
                          void* dx, long lddx, int B, int H, int W, int C, float min_depth, int dtype, mte_stream_t stream);
long mte_invdepth_bwd_weight_workspace_elems(int C);
int mte_invdepth_bwd_weight(const void* x, long ldx, const float* dlogit, float* dwb, float* records,
                            int B, int H, int W, int C, int dtype, mte_stream_t stream);

/* The inverse-depth channel of the decoder's iconv inputs as a rank-1 term (round 4).  iconv3 / iconv2 / iconv1 see
 * torch.cat((unpack, skip, nearest_up2(inv_depth)), 1) (reference PackNetSAN01.py:118-143): conv(cat(x, u)) = conv(x) + conv_1(u).  The one-channel part is a
 * 3x3 stencil of the low-resolution map; the GEMM kernels run on the other C-1 = 64 / 96 / 192 channels and ACCUMULATE onto it.  w: channel C-1 of the OIHW
 * weight (element (n, tap) at w[n * w_stride + tap]).  _fwd overwrites y [B,2h,2w,N]; _bwd_data: dinv [B,h,w] (+)=; _bwd_weight below. */
int mte_rank1_conv_fwd(const float* inv, const float* w, long w_stride, void* y, long ldy, int B, int h, int wl, int N, int dtype, mte_stream_t stream);
int mte_rank1_conv_bwd_data(const void* dy, long lddy, const float* w, long w_stride, float* dinv, int B, int h, int wl, int N, int accumulate, int dtype,
                            mte_stream_t stream);
/* out [B,2h,2w] = nearest_up2(inv), fp32.  No host caller since the rank-1 weight gradient up-samples the map on its way into LDS (tap_wgrad.hip);
 * kept as part of the exported surface. */
int mte_upsample2_f32(const float* inv, float* out, int B, int h, int wl, mte_stream_t stream);
/* _fwd fused into the LDS-patch 3x3 forward (bf16, N <= 64): y = conv_3(x, wpatch) + bias + conv_1(nearest_up2(inv), w1) in ONE launch -- the store loop of a
 * tile adds the term from two small LDS tables (the map under the tile + halo, the 9 x N weights), so y is neither written first nor read back.  inv [B,H/2,W/2];
 * w1 / w1_stride as w / w_stride above.  _ok(...) = 1 when this form exists for the shape (otherwise: mte_rank1_conv_fwd, then the conv with accumulate = 1). */
int mte_conv2d_patch_fwd_rank1_ok(const float* bias, long ldx, int B, int H, int W, int Cin_p, int N);
int mte_conv2d_patch_fwd_rank1(const void* x, long ldx, const void* wpatch, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N,
                               const float* inv, const float* w1, long w1_stride, mte_stream_t stream);
/* y = conv_3x3(x, wpatch) + conv_1x1(x2, wpatch2) + bias in one launch of the LDS-patch kernel (bf16, N <= 64, W % 32 == 0): the second source's C2 channels are
 * further K-steps of every tile at the centre tap; wpatch2 = fragment-block pack of the 1x1 weights for the same N (mte_conv2d_patch_pack_elems(C2, N, 1, 1)).
 * The data gradient of a residual block's input (reference layers01.py:55-73: conv1 and the 1x1 shortcut read the same x): dx = conv3x3^T(dy1) + conv1x1^T(dy3)
 * without a stand-alone 1x1 launch and without an accumulating pass over dx. */
int mte_conv2d_patch_fwd_plus1x1(const void* x, long ldx, const void* wpatch, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N,
                                 const void* x2, long ldx2, const void* wpatch2, int C2, mte_stream_t stream);
/* its gradient with respect to the weight column: dw: element (n, tap) at dw[n * dw_stride + tap] (overwritten); records: mte_rank1_conv_bwd_records_elems(N)
 * floats of scratch.  Every record of dy is read once; no floating-point atomics (fixed-order sums: bit-reproducible). */
long mte_rank1_conv_bwd_records_elems(int N);
int mte_rank1_conv_bwd_weight(const void* dy, long lddy, const float* inv, float* dw, long dw_stride, float* records,
                              int B, int h, int wl, int N, int dtype, mte_stream_t stream);
/* ---- layout / wiring helpers (networks/depth/PackNetSAN01.py:92-143 cat + Upsample; models/model_utils.py:98-117 flip) */
int mte_nchw_to_nhwc(const float* src, void* dst, long ldd, int B, int C, int H, int W, int Cp, int flip_w, int dtype, mte_stream_t stream);
int mte_upsample_inv_fwd(const float* inv, void* dst, long ldd, int B, int h, int w, int dtype, mte_stream_t stream);
int mte_upsample_inv_bwd(const void* dsrc, long lds_, float* dinv, int B, int h, int w, int accumulate, int dtype, mte_stream_t stream);
int mte_copy_channels(const void* src, long lds_, void* dst, long ldd, long npix, int C, int dtype, mte_stream_t stream);
/* a [dW; db] record (conv3d weight gradients, the heads' weight gradients) into its two places of a flat gradient buffer in one launch:
 * dst0[0..n0) = src[0..n0), dst1[0..n1) = src[n0..n0+n1) */
int mte_split_record(const float* src, float* dst0, int n0, float* dst1, int n1, mte_stream_t stream);
/* out = a + b over NHWC channel-slice views: the summed gradient of an activation with two consumers (what autograd's
 * implicit accumulation does in the reference), one 16-byte-vectorised pass whatever the strides.  `out` may be `a` itself (same pointer and stride) */
int mte_add_channels(const void* a, long lda, const void* b, long ldb, void* out, long ldo, long npix, int C, int dtype, mte_stream_t stream);

/* ---- depth-edge loss: inv2depth + GradLayer + GradLoss('cross_entropy')
 *      (utils/depth.py:104-121; losses/grad_loss.py:20-31,65-95,122-219) */
/* All scales of SemiSupEdgeModel.compute_edge_loss_with_all_scales (models/SemiSupEdgeModel.py:164-198) in ONE forward and ONE
 * backward launch, optionally with the silog loss of scale 0 (models/SemiSupEdgeModel.py:144; losses/supervised_loss.py:57-69,
 * 155-216) fused in -- it reads the same full-resolution inverse depth.  Workgroup = 64x32-pixel tile of one (scale, sample); the
 * last workgroup to arrive adds the per-workgroup partial sums in a fixed order and computes alpha, the loss scalars and the
 * backward coefficients on the device (no reduce / finalize launches, no host sync, deterministic sums).
 *   scales : HOST array of nscales (<= 4) records; every map is fp32 [B,H,W]; normal / mask / gmap nullable; dpred = backward output
 *   work   : mte_edge_loss_work_elems() doubles (content on entry ignored; zero on entry under MTE_OPT_LOSS_PREZEROED)
 *   losses [nscales] <- weight * balanced BCE per scale;  coef [nscales][2B+1] <- backward coefficients
 *   gt_depth (nullable; metric depth, 0 = invalid, at the size of scale 0): fused silog -> silog_loss[1], silog_aux[2]
 *   backward: dpred_s <- gout[s] * d loss_s / d pred_s  (+ silog_gout[0] * d silog / d pred_0); gout / silog_gout: device, nullable = 1 */
typedef struct { const float* pred; const float* edge; const float* normal; const float* mask; float* gmap; float* dpred; int H; int W; } mte_edge_scale;
long mte_edge_loss_work_elems(const void* scales, int nscales, int B);
int mte_edge_loss_multi_fwd(const void* scales, int nscales, int B, int from_inv, int is_grad, int is_sigmoid, float thresh,
                            float weight, float pos_to_neg, const float* gt_depth, double* work, float* losses, float* coef,
                            float* silog_loss, float* silog_aux, mte_stream_t stream);
int mte_edge_loss_multi_bwd(const void* scales, int nscales, int B, int from_inv, int is_grad, int is_sigmoid, float thresh,
                            const float* coef, const float* gout, const float* gt_depth, const float* silog_aux, const float* silog_gout,
                            mte_stream_t stream);
/* The same for TWO predictions against one set of labels (models/SemiSupEdgeCompletionModel.py:128-165: branch 0 = the RGB prediction,
 * branch 1 = the RGB+LiDAR prediction) in ONE forward and ONE backward launch that read the labels once.  Only the training configuration
 * is built: inverse depth in, Sobel + normals + sigmoid, every scale with W % 4 == 0, 16-byte-aligned bases and normals, no mask, no
 * edge-map output.  Anything else answers MTE_ERR_UNSUPPORTED and launches nothing: the caller makes two mte_edge_loss_multi_* calls.
 *   work   : mte_edge_loss_pair_work_elems() doubles (content on entry ignored; zero on entry under MTE_OPT_LOSS_PREZEROED)
 *   losses [2][nscales], coef [2][nscales][2B+1], silog_loss [2], silog_aux [2][2]; gt_depth nullable
 *   backward: dpred[br]_s <- gout[br][s] * d loss / d pred[br]_s (+ silog_gout[br] * d silog / d pred[br]_0); gout / silog_gout: device, nullable = 1 */
typedef struct { const float* pred[2]; float* dpred[2]; const float* edge; const float* normal; int H; int W; } mte_edge_pair_scale;
long mte_edge_loss_pair_work_elems(const void* scales, int nscales, int B);
int mte_edge_loss_pair_fwd(const void* scales, int nscales, int B, float thresh, float weight, float pos_to_neg,
                           const float* gt_depth, double* work, float* losses, float* coef,
                           float* silog_loss, float* silog_aux, mte_stream_t stream);
int mte_edge_loss_pair_bwd(const void* scales, int nscales, int B, float thresh, const float* coef, const float* gout,
                           const float* gt_depth, const float* silog_aux, const float* silog_gout, mte_stream_t stream);
/* single-scale entry points (GradLoss / GradLayer called on their own): the same kernels with one scale */
long mte_edge_loss_sums_elems(int B, int H, int W);   /* doubles `sums` must hold: B*6 + 4 results, the arrival ticket, the per-workgroup partial sums */
int mte_edge_loss_fwd(const float* pred, const float* edge, const float* normal, const float* mask, double* sums, float* gmap,
                      int B, int H, int W, int from_inv, int is_grad, int is_sigmoid, float thresh, mte_stream_t stream);
int mte_edge_loss_finalize(const double* sums, int B, long numel, float weight, float pos_to_neg, int has_mask,
                           float out_scale, float* loss_acc, float* loss_this, float* coef, mte_stream_t stream);
int mte_edge_loss_bwd(const float* pred, const float* edge, const float* normal, const float* mask, const float* coef, const float* gout,
                      float* dpred, int B, int H, int W, int from_inv, int is_grad, int is_sigmoid, float thresh, mte_stream_t stream);

/* ---- the other edge-loss choices of GradLoss (losses/grad_loss.py:139-156), one scale per launch:
 *      kind 0 'cross_entropy' (comp_cross_entropy, grad_loss.py:161-219), kind 1 'attention_loss' (attention_loss2 with one alpha for the
 *      batch, losses/attention_loss.py:21-49), kind 2 'spatially_adaptive' (attention_loss2 with the per-pixel 15x15 box alpha,
 *      attention_loss.py:27-31); dice != 0 adds the dice term of grad_loss.py:151-156.  loss = weight * (base + dice).
 *   maps fp32 [B,H,W]; normal / mask / gmap nullable; from_inv / is_grad / is_sigmoid / thresh as mte_edge_loss_fwd
 *   work : mte_edge_loss_kind_work_elems(B, H, W) doubles (content on entry ignored: each forward launch clears what it needs)
 *   fwd  : loss[1] <- the loss scalar; coef [2B + 5] <- backward coefficients (computed on the device by the last workgroup; no host sync)
 *   bwd  : dpred <- gout * d loss / d pred (gout: device scalar, nullable = 1) */
long mte_edge_loss_kind_work_elems(int B, int H, int W);   /* attention_loss.py:21-49 / grad_loss.py:139-156: [B][13] sums, tickets, one record per 64x32 tile */
int mte_edge_loss_kind_fwd(const float* pred, const float* edge, const float* normal, const float* mask, float* gmap, int B, int H, int W,
                           int kind, int dice, int from_inv, int is_grad, int is_sigmoid, float thresh, float weight, float pos_to_neg,
                           double* work, float* loss, float* coef, mte_stream_t stream);    /* grad_loss.py:122-156, attention_loss.py:21-49 */
int mte_edge_loss_kind_bwd(const float* pred, const float* edge, const float* normal, const float* mask, const float* coef, const float* gout,
                           float* dpred, int B, int H, int W, int kind, int dice, int from_inv, int is_grad, int is_sigmoid, float thresh,
                           mte_stream_t stream);                                          /* autograd of grad_loss.py:122-156 */

/* ---- the supervised losses of SupervisedLoss (losses/supervised_loss.py:13-216) over up to four scales, all scales in one launch:
 *      method 0 'l1', 1 'mse', 2 'berhu' (sparse only), 3 'silog', 4 'abs_rel' (get_loss_func's suffix order); sparse != 0 keeps the
 *      pixels with a valid ground truth.  loss = sum_s f(pred_s + 1e-5, depth2inv(depth) at the nearest pixel of scale s) / nscales.
 *   scales: nscales (1..4) mte_sup_scale, fp32 [B,H,W] maps; dpred is read by the backward only.  depth: metric depth [B,Hd,Wd], 0 = invalid.
 *   work : mte_supervised_loss_work_elems(scales, nscales, B) doubles, 16-byte aligned (content on entry ignored: the forward clears its tickets)
 *   fwd  : loss[1] <- the loss scalar; scale_loss [nscales] (nullable) <- the per-scale values; coef [16] <- backward coefficients
 *          (computed on the device by the last workgroup; no host sync).  BerHu runs two launches.
 *   bwd  : every pixel of every dpred_s <- gout * d loss / d pred_s, exact zeros where the mask drops a pixel (gout: device scalar, nullable = 1) */
typedef struct { const float* pred; float* dpred; int H; int W; } mte_sup_scale;
long mte_supervised_loss_work_elems(const void* scales, int nscales, int B);   /* two tickets, the BerHu hand-over, one record per 4096 pixels */
int mte_supervised_loss_fwd(const void* scales, int nscales, int B, const float* depth, int Hd, int Wd, int method, int sparse,
                            double* work, float* loss, float* scale_loss, float* coef, mte_stream_t stream);   /* supervised_loss.py:155-216 */
int mte_supervised_loss_bwd(const void* scales, int nscales, int B, const float* depth, int Hd, int Wd, int method, int sparse,
                            const float* coef, const float* gout, mte_stream_t stream);                       /* autograd of the same */
/* F.interpolate(x, size = (H, W), mode = 'nearest') of upsample_output (model_utils.py:154-176) for up to four maps in one launch, integer
 * ratios only (H % h == 0, W % w == 0; anything else is MTE_ERR_ARG).  fwd: dst [B,H,W] <- src [B,h,w], bit-equal to torch;
 * bwd: dst [B,h,w] <- adjoint applied to src [B,H,W], each block summed row-major, no atomics */
typedef struct { const float* src; float* dst; int h; int w; } mte_upsample_map;
int mte_upsample_nearest_fwd(const void* maps, int nmaps, int B, int H, int W, mte_stream_t stream);
int mte_upsample_nearest_bwd(const void* maps, int nmaps, int B, int H, int W, mte_stream_t stream);

/* F.interpolate(pred, size = label size, mode = 'bilinear') of GradLoss.forward (grad_loss.py:127; identity on the multi-scale
 * training path, where every scale is compared at its own resolution) and its adjoint; fp32 [B,h,w] -> [B,H,W] */
int mte_resize_bilinear_fwd(const float* x, float* y, int B, int h, int w, int H, int W, mte_stream_t stream);
int mte_resize_bilinear_bwd(const float* dy, float* dx, int B, int h, int w, int H, int W, mte_stream_t stream);

/* ---- silog supervised loss: depth2inv + sparse mask + SilogLoss (utils/depth.py:124-144; losses/supervised_loss.py:57-69,155-216) */
int mte_silog_fwd(const float* inv, const float* depth, long n, double* sums, float out_scale, float* loss_acc, float* loss_this, float* aux, mte_stream_t stream);
int mte_silog_bwd(const float* inv, const float* depth, const float* aux, const float* gout, float* dinv, long n, int accumulate, mte_stream_t stream);

/* ---- optimizer: torch.optim.Adam step over a flat fp32 buffer (models/model_wrapper.py:142-180; trainers/common_trainer.py:125) */
int mte_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                  int step, float gscale, mte_stream_t stream);
/* the same update with hyper = {lr, 1 - beta1^t, sqrt(1 - beta2^t)} read from DEVICE memory: no per-step host scalar in the launch,
 * so the training step can be replayed from a HIP graph (utils/graph.py::GraphedTrainStep) */
int mte_adam_step_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                      float gscale, mte_stream_t stream);
/* ---- optimizer family (csrc/optim.hip): the other choices of config.model.optimizer, each one launch over the same flat buffers, each
 * with a host-scalar form and a device-scalar form (graph replay) that give bit-equal results.  weight_decay >= 0.
 * mte_adamw_step: decoupled = 0 is torch.optim.Adam(weight_decay) (g' = g * gscale + wd * p), decoupled = 1 torch.optim.AdamW
 *   (p * (1 - lr * wd), taken as p - ((lr * wd) * p + update), lr * wd formed in the kernel); weight_decay = 0 equals mte_adam_step bit
 *   for bit.  hyper as mte_adam_step_dev's.
 * mte_sgd_step: torch.optim.SGD(momentum, dampening, weight_decay, nesterov).  momentum = 0 reads and writes no `buf` (null accepted);
 *   with momentum, `buf` is zero before step 1.  The device form reads hyper = {lr, mu_eff, (1 - dampening)_eff}: {lr, 0, 1} at step 1
 *   ("buf = g' on the first step"), {lr, momentum, 1 - dampening} afterwards; its `momentum` argument is the launch constant of
 *   Nesterov's look-ahead.  nesterov needs momentum > 0 (and dampening = 0 in the host form), else MTE_ERR_ARG. */
int mte_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int decoupled, int step, float gscale, mte_stream_t stream);
int mte_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                       float weight_decay, int decoupled, float gscale, mte_stream_t stream);
int mte_sgd_step(float* p, const float* g, float* buf, long n, float lr, float momentum, float dampening, float weight_decay, int nesterov,
                 int step, float gscale, mte_stream_t stream);
int mte_sgd_step_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                     float gscale, mte_stream_t stream);
/* ---- gradient-norm clipping and the non-finite step guard (csrc/optim.hip): torch.nn.utils.clip_grad_norm_ (L2) over the flat gradient
 * without a pass that rescales it, and a step that is dropped on the device when a gradient is not finite.
 * mte_grad_norm_clip: ONE read-only launch over g[0..n) (16-byte aligned), fp64 sums in a fixed order (bit-equal run to run and under
 *   graph replay; no floating-point atomics).  With S = sum g^2 and norm = |gscale| * sqrt(S) it writes ctl (four floats, DEVICE memory):
 *     ctl[0] = max_norm / (norm + 1e-6), replaced by 1 where that is > 1 (max_norm = +inf gives exactly 1; a NaN stays a NaN)
 *     ctl[1] = 1 if skip_nonfinite and S is not finite, else 0
 *     ctl[2] = norm
 *     ctl[3] += 1 when ctl[1] is set: a running count of skipped steps that the kernel never resets
 *   `work`: mte_grad_norm_work_bytes(n) bytes, 16-byte aligned, zeroed ONCE by the caller; its first 8 bytes receive S (fp64).
 *   max_norm <= 0 or NaN, n <= 0 and null pointers are MTE_ERR_ARG.
 * mte_adamw_step_ctl_dev / mte_sgd_step_ctl_dev: mte_adamw_step_dev / mte_sgd_step_dev whose gradient scale is float32(gscale * ctl[0])
 *   and which, with ctl[1] != 0, return before their first load: p, m, v / buf keep their bits.  ctl = {1, 0} is the plain step bit for
 *   bit.  The host cannot know that a step was skipped: its step count (the bias corrections in `hyper`) advances all the same. */
long mte_grad_norm_work_bytes(long n);
int mte_grad_norm_clip(const float* g, long n, float gscale, float max_norm, int skip_nonfinite, void* work, float* ctl, mte_stream_t stream);
int mte_adamw_step_ctl_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                           float weight_decay, int decoupled, float gscale, const float* ctl, mte_stream_t stream);
int mte_sgd_step_ctl_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                         float gscale, const float* ctl, mte_stream_t stream);
/* ---- gradient accumulation over micro-batches (csrc/optim.hip): one streaming launch in the step kernels' shape, no atomics, no state.
 * assign = 0: dst[i] = dst[i] + src[i] in fp32, one rounding (12 B per element: read, read, write); assign != 0: dst[i] = src[i], a bit
 *   copy that does not read dst.  n = 0 returns 0 without a launch.  n < 0, a null pointer, a pointer that is not 16-byte aligned and
 *   overlapping ranges (equal pointers included) are MTE_ERR_ARG. */
int mte_grad_accumulate(float* dst, const float* src, long n, int assign, mte_stream_t stream);
/* ---- exponential moving average of the weights (csrc/optim.hip): streaming launches in mte_grad_accumulate's shape, no atomics, no state.
 * mte_ema_update: ema[i] = d * ema[i] + omd * p[i] in fp32 -- two multiplications and one addition, each rounded once, in that order
 *   (12 B per element: read, read, write); p is only read.
 * mte_ema_update_dev: the same template on scal = {d, omd} read from DEVICE memory, bit-equal to the host form.  ctl may be null; otherwise
 *   it is the word mte_grad_norm_clip leaves, and with ctl[1] != 0 the launch returns before its first load: the average keeps its bits
 *   over a skipped step.  ctl[0] (the clip coefficient) is not read.  A null scal is MTE_ERR_ARG.
 * mte_flat_swap: a[i] <-> b[i] bit for bit (16 B per element; NaN payloads survive: no arithmetic).
 * All three: n = 0 returns 0 without a launch.  n < 0, a null pointer, a pointer that is not 16-byte aligned and overlapping ranges (equal
 *   pointers included) are MTE_ERR_ARG. */
int mte_ema_update(float* ema, const float* p, long n, float d, float omd, mte_stream_t stream);
int mte_ema_update_dev(float* ema, const float* p, long n, const float* scal, const float* ctl, mte_stream_t stream);
int mte_flat_swap(float* a, float* b, long n, mte_stream_t stream);
/* ---- per-tensor learning-rate and weight-decay multipliers (csrc/optim.hip): the SEG form of the device-scalar steps.  The flat buffers
 * align every tensor to 64 elements, so an aligned 64-element block belongs to one tensor.
 *   block_class[b] (DEVICE memory, n / 64 bytes): the class of elements 64 b .. 64 b + 63; a byte >= n_classes is read as n_classes - 1.
 *   class_scales (DEVICE memory, 2 * n_classes floats): {lr_mult, wd_mult} per class, 1 <= n_classes <= 16.
 *   For class c: lr_c = float32(hyper[0] * lr_mult_c), wd_c = float32(weight_decay * wd_mult_c); every block is updated by the plain
 *   step's arithmetic with its class's pair, and wd_c == 0 takes the no-decay arithmetic (not `+ 0 * p`): the result equals, slice by
 *   slice and bit for bit, mte_adamw_step_dev / mte_sgd_step_dev on that slice with {lr_c, wd_c}.
 *   ctl may be null; non-null it is mte_grad_norm_clip's word with the meaning it has in the _ctl_dev forms.
 *   n % 64 != 0, a null table, n_classes out of range and the plain forms' argument errors are MTE_ERR_ARG. */
int mte_adamw_step_seg_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                           float weight_decay, int decoupled, float gscale, const unsigned char* block_class, const float* class_scales,
                           int n_classes, const float* ctl, mte_stream_t stream);
int mte_sgd_step_seg_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov,
                         float gscale, const unsigned char* block_class, const float* class_scales, int n_classes, const float* ctl,
                         mte_stream_t stream);
/* ---- per-tensor statistics of the flat gradient and weights (csrc/optim.hip): ONE read-only launch however many tensors there are.
 *   g, p: flat fp32 buffers of n elements, 16-byte aligned; p may be null.  Tensor t is elements seg_begin[t] .. seg_begin[t] +
 *   seg_numel[t] - 1 (`long` arrays of T entries in DEVICE memory; begins are multiples of 64, the padding behind a tensor is not read;
 *   1 <= T <= 4096).  out (DEVICE memory, 4 * T doubles): per tensor {sum g^2, max |g| over the finite elements (0 without one), the
 *   count of inf / NaN elements of g, sum p^2 (0 without p)}; the sums are fp64 (squares exact, additions rounded) in an order that the
 *   table alone fixes: bit-equal call to call and under graph replay.  A range that leaves [0, n) reads nothing and reports zeros.
 *   `work`: mte_tensor_stats_work_bytes(n, T) bytes, 16-byte aligned, zeroed ONCE by the caller (tickets that return to zero, records). */
long mte_tensor_stats_work_bytes(long n, int T);
int mte_tensor_stats(const float* g, const float* p, long n, const long* seg_begin, const long* seg_numel, int T, void* work, double* out,
                     mte_stream_t stream);
/* ---- LAMB (csrc/optim.hip): the decoupled AdamW step whose per-tensor delta is rescaled by a trust ratio, as TWO launches with no
 * scratch buffer.  The tensor table is mte_tensor_stats' (seg_begin / seg_numel: `long` arrays of T entries in DEVICE memory, begins
 * multiples of 64, ranges disjoint, 1 <= T <= 4096) plus tensor_table (DEVICE memory, 3 * T floats): {lr_mult, wd_mult, adapt} per tensor.
 * hyper = {lr, 1 - beta1^t, sqrt(1 - beta2^t)} in DEVICE memory, as mte_adamw_step_dev.  Per tensor t, in fp32 with contraction off:
 *     lr_t = float32(hyper[0] * lr_mult)    wd_t = float32(weight_decay * wd_mult)    lrwd = lr_t * wd_t
 *     g'   = g * gs                         (gs = gscale, or float32(gscale * ctl[0]) with a ctl)
 *     m    = b1 * m + (1 - b1) * g'         v = b2 * v + (1 - b2) * g' * g'
 *     den  = sqrtf(v) / hyper[2] + eps
 *     d    = lrwd * p + (lr_t / hyper[1]) * (m / den)          (wd_t == 0: the no-decay form, d = (lr_t / hyper[1]) * (m / den))
 *     S_p  = sum (double)p^2    S_d = sum (double)d^2          over the tensor's numel elements; the padding behind them is never read
 *     r_t  = adapt != 0 && S_p > 0 && S_d > 0 ? lr_t * sqrt(S_p) / sqrt(S_d) (fp64) : 1;   max_trust > 0: r_t = min(r_t, max_trust)
 *     q_t  = float32(r_t)                   p = p - q_t * d
 *   d = lr_t * u with u the LAMB paper's update, so q_t = ||p|| / ||u|| is its trust ratio.  With q_t = 1 the step is
 *   mte_adamw_step_dev (decoupled) bit for bit.  Non-finite sums get no special case: a NaN gives r_t = 1 and reaches p through d.
 * mte_lamb_moments (24 B per parameter): reads p, g, m, v, writes m, v, and leaves trust[t] = q_t (T floats) and sums[2 t ..] =
 *   {S_p, S_d} (2 * T doubles), both DEVICE memory.  The sums are fp64 in an order the table alone fixes (mte_tensor_stats' chunks, one
 *   record per chunk, a ticket per tensor; no floating-point atomics): bit-equal call to call and under graph replay.
 *   `work`: mte_lamb_work_bytes(n, T) bytes (0 for n <= 0 or T outside 1..4096), 16-byte aligned, zeroed ONCE by the caller; its
 *   tickets return to zero.
 * mte_lamb_apply (16 B per parameter): reads p, m, v and trust, forms d again from the stored m and v (the same operations on the same
 *   inputs: the same bits) and writes p.  It takes the hyper, eps, weight_decay, table and ctl of the mte_lamb_moments launch before it.
 * ctl may be null; otherwise it is mte_grad_norm_clip's word, and with ctl[1] != 0 BOTH launches return before their first load: p, m,
 *   v, trust, sums and work keep their bits.
 * MTE_ERR_ARG: a null pointer (except ctl); p, g, m, v or work not 16-byte aligned (sums: 8-byte); n <= 0; T outside 1..4096; a negative
 *   or NaN weight_decay or max_trust.  A table range that leaves [0, n) reads and writes nothing in the flat buffers for that tensor (its
 *   trust is 1 and its sums are 0), as in mte_tensor_stats. */
long mte_lamb_work_bytes(long n, int T);
int mte_lamb_moments(const float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps,
                     float weight_decay, float gscale, float max_trust, const long* seg_begin, const long* seg_numel,
                     const float* tensor_table, int T, void* work, float* trust, double* sums, const float* ctl, mte_stream_t stream);
int mte_lamb_apply(float* p, const float* m, const float* v, long n, const float* hyper, float eps, float weight_decay,
                   const long* seg_begin, const long* seg_numel, const float* tensor_table, int T, const float* trust,
                   const float* ctl, mte_stream_t stream);

/* ---- validation depth metrics: fp32 [B,1,H,W] maps, no host synchronisation
 * mte_post_process_inv_depth = post_process_inv_depth (utils/depth.py:230-256); method 0 'mean', 1 'max', 2 'min'
 *   (fuse_inv_depth, utils/depth.py:202-227).  `inv_depth_flipped` is the network output on the mirrored image.
 * mte_depth_metrics = compute_depth_metrics (utils/depth.py:259-325): `pred` [B,1,h,w] is brought to the ground-truth
 *   resolution by scale_mode 0 'resize' (bilinear, align_corners=True) or 1 'top-center' (utils/depth.py:328-361);
 *   valid = min_depth < gt < max_depth (and the garg crop window); with use_gt_scale the prediction is multiplied by
 *   median(gt)/median(pred) over the valid pixels (torch.median = element of rank (n-1)/2); out7 receives
 *   (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3) averaged over the B images (images without a valid pixel add 0).
 *   `workspace` needs mte_depth_metrics_workspace_bytes(B) bytes, 8-byte aligned; its content on entry is ignored. */
long mte_depth_metrics_workspace_bytes(int B);
int mte_depth_metrics(const float* gt, const float* pred, int B, int H, int W, int h, int w, int scale_mode, int garg_crop,
                      float min_depth, float max_depth, int use_gt_scale, void* workspace, long workspace_bytes,
                      float* out7, mte_stream_t stream);
int mte_post_process_inv_depth(const float* inv_depth, const float* inv_depth_flipped, float* out, int B, int H, int W,
                               int method, mte_stream_t stream);

/* ---- depth-edge annotation post-processing: fp32 [B,H,W] maps
 * mte_dee_sobel_nms: prob = pred*scale (the '/2' of infer_edge_estimation.py:192); 5x5 Sobel as cv2.Sobel(CV_64F, ksize=5);
 *   normals_u8 = uint8(((atan2(-sy,sx)*180/pi+180)/360)*255) (infer_edge_estimation.py:194-200) and/or
 *   nms = non_max_suppression(prob) (utils/tools.py:9-46; zero one-pixel frame).  Either output may be NULL.
 * hysteresis(img, t_low, t_high) (utils/tools.py:49-92) in three steps so that the host decides when to stop sweeping:
 *   mte_hysteresis_begin      classify into `state` (B*H*W bytes), reset `info` (B*4 ints)
 *   mte_hysteresis_propagate  run `sweeps` propagation sweeps; `flags` (sweeps+1 ints) is reset by the call and
 *                             flags[sweeps] != 0 afterwards means the last sweep still changed pixels: call again
 *   mte_hysteresis_finish     out = img * state/max(state), including the reference's treatment of the frame */
int mte_dee_sobel_nms(const float* pred, float scale, unsigned char* normals_u8, float* nms, int B, int H, int W, mte_stream_t stream);
int mte_hysteresis_begin(const float* img, unsigned char* state, int* info, int B, int H, int W, double t_low, double t_high,
                         mte_stream_t stream);
int mte_hysteresis_propagate(unsigned char* state, int* flags, int sweeps, int B, int H, int W, mte_stream_t stream);
int mte_hysteresis_finish(const float* img, const unsigned char* state, const int* info, float* out, int B, int H, int W,
                          mte_stream_t stream);

/* ---- chamfer edge metrics (edge half): chamfer_distance of utils/edge.py:19-64 (= edge.py:29-71), mask=None.
 * im_pred / im_gt: float [B,H,W] edge images on the 0..255 scale (a pixel is an edge iff v/255 > 0.5).  out[b] = (c_dist,
 * percentage) as doubles: mean exact Euclidean distance from the predicted edge pixels to the nearest ground-truth edge
 * pixel and the share of them closer than edge_to_edge_thresh (NaN when nothing is predicted, +inf distances when the
 * ground truth has no edge pixel -- scipy's result for that case is not reproduced).  dist_map (nullable) receives the
 * distance transform, cond_map (nullable) the reference's -1 / 0 / 1 map.  workspace: mte_chamfer_workspace_bytes(B,H,W). */
long mte_chamfer_workspace_bytes(int B, int H, int W);
int mte_chamfer_distance(const float* im_pred, const float* im_gt, int B, int H, int W, double edge_to_edge_thresh,
                         void* workspace, long workspace_bytes, double* out, float* dist_map, float* cond_map, mte_stream_t stream);

/* ---- Canny step of the validation edge metrics (models/model_wrapper.py:376-400).  PARITY UNPINNED: restates OpenCV's
 * published cv2.Canny (apertureSize 3, L1 gradient) -- see oracle/canny_oracle.py.
 * mte_canny_begin: vis = uint8(depth * (255 / max(depth))) per image (vis_u8 nullable, B*H*W bytes), 3x3 Sobel, non-maximum
 *   suppression, and classification for n_pairs (<= 4) threshold pairs `thresholds[2*p], thresholds[2*p+1]` (HOST ints)
 *   into state[n_pairs][B][H][W] bytes (0 none, 1 candidate, 2 edge).  max_ws: B unsigned ints of scratch.
 * mte_canny_propagate: hysteresis sweeps over the `maps` = n_pairs*B state maps; same flags protocol as mte_hysteresis_propagate.
 * mte_canny_finish: edges[maps][H][W] floats, 255 on edges, 0 elsewhere (the scale mte_chamfer_distance expects). */
int mte_canny_begin(const float* depth, int B, int H, int W, int n_pairs, const int* thresholds, unsigned* max_ws,
                    unsigned char* vis_u8, unsigned char* state, mte_stream_t stream);
 /* mte_resize_linear: cv2.resize(float32 [B,h,w] -> [B,H,W], INTER_LINEAR) as used in front of the Canny step
 * (models/model_wrapper.py:386-387); restated from OpenCV's resize.cpp, PARITY UNPINNED like the rest of this block. */
int mte_resize_linear(const float* src, int B, int h, int w, float* dst, int H, int W, mte_stream_t stream);
int mte_canny_propagate(unsigned char* state, int* flags, int sweeps, int maps, int H, int W, mte_stream_t stream);
int mte_canny_finish(const unsigned char* state, float* edges, int maps, int H, int W, mte_stream_t stream);
/* mte_canny_begin_fixed: the same pass at a FIXED scale, as edge_from_depth quantises (edge.py:73-93, the front end of
 *   eval_depth_edges.py:264-280): vis = uint8(clamp(depth, min_depth, max_depth) * factor) with the caller's factor
 *   (float32(255.0 / max_depth) upstream) instead of 255 / max(image); no max_ws.  n_pairs <= 12 (the twelve pairs
 *   (t/2, t), t = 20 .. 240 of the benchmark in one pass).  Same state layout; propagate / finish as above. */
int mte_canny_begin_fixed(const float* depth, int B, int H, int W, float min_depth, float max_depth, float factor, int n_pairs,
                          const int* thresholds, unsigned char* vis_u8, unsigned char* state, mte_stream_t stream);

/* ---- edge benchmark: pixel correspondence (eval_depth_edges.py:119-145,179-230: correspond_pixels.correspond_pixels of py-bsds500 with
 * thresholds=1, apply_thinning=False).  PARITY UNPINNED against py-bsds500; exact against an independent maximum-matching solver.
 * B instances, one workgroup each.  pred: float [B,H,W] and gt: float [Bg,H,W] edge images on the 0..255 scale (edge iff v/255 > 0.5);
 * instance b is matched against gt[gt_of[b]] (DEVICE ints; twelve thresholds share one annotation).  Two pixels may be paired iff
 * dx^2 + dy^2 <= r2, an integer the caller computes once in double: r2 = floor((max_dist * sqrt(H^2 + W^2))^2).
 * result: int [B,4] = (matched, n_pred, n_gt, status); matched is the size of a MAXIMUM matching.  status 0 = ok, 1 = init_mate does not
 * check out, 2 / 3 / 4 = the phase / level / path-walk bound was hit, 5 = queue overflow, 6 = gt_of[b] outside [0, Bg) -- with a non-zero
 * status `matched` is not a maximum (0 for 1 and 6).  mate_pred (nullable): int [B,H,W], the linear index of each predicted pixel's
 * partner or -1; the partners may differ between runs, the count may not.  init_mate (nullable): int [B,H,W], a matching to start from
 * (-1 = none) instead of the greedy one; checked, not trusted: an entry on a pixel that is no predicted edge, a partner that is no
 * ground-truth pixel, lies outside the image or outside r2, or is claimed twice gives status 1 for that instance and nothing else.
 * MTE_ERR_UNSUPPORTED: r2 > 64 or H*W >= 2^30.  workspace: mte_edge_match_workspace_bytes(B,H,W,r2) bytes, needs no clearing. */
long mte_edge_match_workspace_bytes(int B, int H, int W, int r2);
int mte_edge_match(const float* pred, const float* gt, const int* gt_of, int B, int Bg, int H, int W, int r2, const int* init_mate,
                   void* workspace, long workspace_bytes, int* result, int* mate_pred, mte_stream_t stream);

/* ---- per-frame depth metrics of the analysis stage (eval_depth.py:348-410,432-456: DensePredictionAnalyzer.eval_frame).
 * gt: DOUBLE [B,H,W] metres, pred: float [B,H,W].  mask = min_depth < gt < max_depth, inside columns [x0,x1) and rows [y0,y1)
 * (clipped to the image like a numpy slice) or, with mask_u8 (nullable, [B,H,W] bytes), where mask_u8 > 0 (the crop is then unused).
 * out: double [B,5] = mean_rel_err, std_rel_err (population), abs_rel_err, accuracy_1p1, accuracy_1p25; counts: long [B,3] = valid
 * pixels and the two accuracy counts.  float64 arithmetic throughout with eps = 2^-52, sums in a fixed order (bit-reproducible); NaN
 * in all of `out` when the mask is empty (np.nanmean).  One workgroup per frame, no workspace. */
int mte_frame_depth_metrics(const double* gt, const float* pred, const unsigned char* mask_u8, int B, int H, int W,
                            double min_depth, double max_depth, int x0, int x1, int y0, int y1, double* out, long* counts, mte_stream_t stream);

/* ---- sparse auxiliary (SAN) branch.  PARITY UNPINNED: dense-equivalent of the
 * MinkowskiEngine operators the reference uses (networks/layers/minkowski_encoder.py:11-132, minkowski.py:33-79); see
 * oracle/san_oracle.py.  Features are zero-filled NHWC activations (bf16 / fp32), the active set is a byte mask [B,H,W].
 * mte_sparsify_depth: mask = depth > 0, feat channel 0 = depth on the mask, channels 1..7 = 0 (feat has >= 8 channels/pixel)
 * mte_sparse_maxpool3s2: MinkowskiMaxPooling(3, stride 2): mask_out = any of the 2x2 block, value = max over the active
 *   cells of the centred 3x3 window; H and W even
 * mte_sparse_bn_relu: out = mask ? relu(batchnorm_eval(a [+ b] [+ c])) : 0   (b, c nullable)
 * mte_san_fuse: out = skip * w[0] + sparse + bias[0]   (networks/depth/PackNetSAN01.py:254-258) */
int mte_sparsify_depth(const float* depth, void* feat, long ldf, unsigned char* mask, int B, int H, int W, int dtype, mte_stream_t stream);
/* Round 3: the sparse convolutions as gather-GEMM-scatter over the ACTIVE sites.  mte_sparse_site_list: sites[0 .. *count) = raster-ordered
 * pixel indices of the active set (three small launches, no atomics; `count` stays in device memory).  mte_conv2d_igemm_sparse: the
 * implicit GEMM of mte_conv2d_igemm with GEMM row m = pixel sites[m]: the k x k taps of a site are gathered from the zero-filled dense
 * map (inactive neighbours contribute zeros = MinkowskiConvolution's sum over active neighbours), the result is scattered to the same
 * sites and nothing else is written; tiles beyond *count return at once, so the work is proportional to the active count (LiDAR: ~5 % at
 * the first level) without the count ever visiting the host.  Also the data gradient (backward pack, x := dy). */
long mte_sparse_site_list_workspace_elems(long npix);
int mte_sparse_site_list(const unsigned char* mask, long npix, int* sites, int* count, int* ws, mte_stream_t stream);
int mte_conv2d_igemm_sparse(const void* x, long ldx, const void* wpack, const float* bias, void* y, long ldy,
                            int B, int H, int W, int Cin_p, int N, int KH, int KW, int dtype,
                            const int* sites, const int* count, int accumulate, mte_stream_t stream);
int mte_sparse_maxpool3s2(const void* in, long ldi, const unsigned char* mask_in, void* out, long ldo, unsigned char* mask_out,
                          int B, int H, int W, int C, int dtype, mte_stream_t stream);
int mte_sparse_bn_relu(const void* a, long lda, const void* b, long ldb, const void* c, long ldc, const unsigned char* mask,
                       const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                       void* out, long ldo, long npix, int C, int dtype, mte_stream_t stream);
int mte_san_fuse(const void* skip, long ld_skip, const void* sparse, long ld_sparse, const float* w, const float* bias,
                 void* out, long ldo, long npix, int C, int dtype, mte_stream_t stream);
/* Training path of the branch (two-pass RGB / RGB+LiDAR step, networks/depth/PackNetSAN01.py:324-342; minkowski_encoder.py:27-84):
 * mte_sparse_bn_stats: MinkowskiBatchNorm in training mode = BatchNorm1d over the active points of the whole batch:
 *   sums[0..C) = sum x, sums[C..2C) = sum x^2 over the active pixels (x = a [+ b] [+ c]), sums[2C] = number of active pixels
 *   (fp64, zeroed here).  The caller forms mean / biased variance and runs mte_sparse_bn_relu with them.
 * mte_sparse_bn_relu_bwd: dy = dout * [out > 0];  dx = mask ? gamma * invstd * (dy - mean_active(dy) - xhat * mean_active(dy xhat)) : 0
 *   (the gradient of a, b and c alike; n_active: device pointer to the number of active pixels, i.e. mte_sparse_bn_stats' sums + 2C); sums[0..C) = sum dy (= dbeta), sums[C..2C) = sum dy * xhat (= dgamma); scratch zeroed here.
 * mte_sparse_maxpool3s2_bwd: a fine cell receives the gradient of every coarse cell whose window maximum it is (first maximum in
 *   row-major window order among the active cells).
 * mte_san_fuse_bwd: dskip = dout * w[0]; sums[0] = sum dout * skip (dw), sums[1] = sum dout (db); the sparse operand's gradient is dout.
 * mte_feat_l2: sum (nullable) = sum (a - b)^2;  db (nullable) = -2 (a - b) * inv_n * gscale[0]  -- the feature-matching loss between
 *   the RGB+LiDAR pass (a, detached) and the RGB pass (b) and its gradient (PackNetSAN01.py:340-342). */
int mte_sparse_bn_stats(const void* a, long lda, const void* b, long ldb, const void* c, long ldc, const unsigned char* mask,
                        double* sums, long npix, int C, int dtype, mte_stream_t stream);
int mte_sparse_bn_relu_bwd(const void* a, long lda, const void* b, long ldb, const void* c, long ldc, const void* out, long ldo,
                           const void* dout, long ldd, const unsigned char* mask, const float* gamma, const float* mean, const float* invstd,
                           const double* n_active, double* sums, void* dx, long ldx, long npix, int C, int dtype, mte_stream_t stream);
int mte_sparse_maxpool3s2_bwd(const void* in, long ldi, const unsigned char* mask_in, const void* dout, long ldd, void* din, long ldn,
                              int B, int H, int W, int C, int dtype, mte_stream_t stream);
int mte_san_fuse_bwd(const void* skip, long ld_skip, const void* dout, long ldd, const float* w, void* dskip, long ldk, double* sums,
                     long npix, int C, int dtype, mte_stream_t stream);
int mte_feat_l2(const void* a, long lda, const void* b, long ldb, double* sum, void* db, long ldg, const float* gscale, float inv_n,
                long npix, int C, int dtype, mte_stream_t stream);

/* ---- training-target preparation (data half)
 * mte_edge_target_from_u8:   dst = src / 255                      (datasets/augmentations.py:186-188,199-201)
 * mte_normal_target_from_u8: dst = (360 * (src/255) - 180) * pi/180   (datasets/gta_dataset.py:407-409,417-418), float64 inside
 * mte_resize_depth_preserve: resize_depth_preserve (datasets/augmentations.py:58-100) of float [B,h,w] sparse maps into
 *   [B,H,W]: valid = value > 0, target = (int(y*H/h), int(x*W/w)), last source pixel in raster order wins, zeros elsewhere.
 *   winner_ws: B*H*W ints of scratch. */
int mte_edge_target_from_u8(const unsigned char* src, float* dst, long n, mte_stream_t stream);
int mte_normal_target_from_u8(const unsigned char* src, float* dst, long n, mte_stream_t stream);
int mte_resize_depth_preserve(const float* src, int B, int h, int w, float* dst, int H, int W, int* winner_ws, mte_stream_t stream);

/* ---- evaluation-sample preparation (datasets/transforms.py:53-125).  PARITY UNPINNED restatements of OpenCV, like mte_resize_linear:
 * mte_resize_linear_u8:   cv2.resize(uint8 [B,h,w] -> [B,H,W]) with the default INTER_LINEAR: per axis f = float((d+0.5)*(double(n)/N) - 0.5),
 *   s = floor(f), f -= s, clamped to [0, n-1] with f = 0 at either end; coefficients rint(f*2048), rint((1.f-f)*2048) as 16-bit integers;
 *   horizontal pass in int32, then dst = (((b0*(R0>>4))>>16) + ((b1*(R1>>4))>>16) + 2) >> 2.  With h == 2H and w == 2W exactly it is the
 *   2x2 area average (sum + 2) >> 2 instead, as OpenCV switches.  No workspace: each output pixel recomputes its two row taps.
 * mte_resize_nearest_f32: cv2.resize(float32 [B,h,w] -> [B,H,W], INTER_NEAREST): sx = min(floor(dx * (1.0/(double(W)/w))), w-1), rows alike.
 * Null pointers, non-positive sizes, B > 65535 or a map of 2^30 pixels or more return MTE_ERR_ARG and launch nothing. */
int mte_resize_linear_u8(const unsigned char* src, int B, int h, int w, unsigned char* dst, int H, int W, mte_stream_t stream);
int mte_resize_nearest_f32(const float* src, int B, int h, int w, float* dst, int H, int W, mte_stream_t stream);

/* ---- training-image preparation (the 8-bit image half of datasets/transforms.py:17-50), bit for bit as PIL computes it
 * mte_image_resample_u8: Image.crop + Image.resize((out_w, out_h), LANCZOS) of an 8-bit RGB frame (HWC): PIL's ImagingResample, horizontal
 *   pass then vertical pass, each clipped to uint8.  src / src_stride (bytes) describe the whole frame, (crop_x, crop_y, in_w, in_h) the
 *   window the filter reads; it never reads outside of it.  kk_* are the 22-bit fixed-point coefficients int32 [out][ksize_*] and
 *   bounds_* the int32 [out][2] (first tap, tap count) of PIL's precompute_coeffs + normalize_coeffs_8bpc, on the device
 *   (datasets/image_prep.py::lanczos_coeffs builds them on the host in double precision); the identity table (ksize 1, 1 << 22) skips a pass.
 *   One launch with the intermediate rows in LDS when a tile's tap span fits, otherwise (or with two_pass != 0) two launches with a uint8
 *   [in_h][out_w][3] intermediate in `workspace`: mte_image_resample_work_bytes gives its size, 0 = none needed.  Same bytes either way.
 *   The tables MUST be the LANCZOS tables of exactly (in_w, out_w) / (in_h, out_h): the library sizes its LDS tiles from a bound of their tap
 *   span and cannot read them on the host.  With tables of a wider filter the one-launch form leaves tiles unwritten and sets
 *   MTE_DEVERR_IMAGE_RESAMPLE in the device error word (mte_device_error_poll) while the call itself returns MTE_OK.
 * mte_color_jitter_u8_to_f32: torchvision-on-PIL adjust_brightness / adjust_contrast / adjust_saturation / adjust_hue in a per-sample order
 *   on uint8 [B,H,W,3], each rounding to uint8 like PIL, then ToTensor: out = float32(u8) / 255 as [B,3,H,W]; out_original (may be null)
 *   receives the un-jittered frame.  factors: float [B][4] = brightness, contrast, saturation factor and the uint8 added to the H channel
 *   (trunc(hue_factor * 255) mod 256); order: int32 [B][4] operation ids (0 brightness, 1 contrast, 2 saturation, 3 hue) in the order they
 *   are applied, -1 = none; order == null: plain ToTensor.  any_contrast != 0 when some sample applies contrast: luma_sums (B 64-bit
 *   words, zero on entry) then receives the per-sample sum of the L channel in a first launch (integer atomics: exact, deterministic).
 *   Contract: any_contrast MUST be non-zero if any row of `order` holds 1 -- the table lives on the device, the entry point cannot check it;
 *   with any_contrast == 0 such a sample is blended towards a mean of 0. */
long mte_image_resample_work_bytes(int in_h, int in_w, int out_h, int out_w, int two_pass);
int mte_image_resample_u8(const unsigned char* src, long src_stride, int crop_x, int crop_y, int in_h, int in_w, unsigned char* dst,
                          int out_h, int out_w, const int* kk_h, const int* bounds_h, int ksize_h, const int* kk_v, const int* bounds_v,
                          int ksize_v, unsigned char* workspace, int two_pass, mte_stream_t stream);
int mte_color_jitter_u8_to_f32(const unsigned char* in, int B, int H, int W, const float* factors, const int* order, int any_contrast,
                               unsigned long long* luma_sums, float* out, float* out_original, mte_stream_t stream);

/* ---- batched training-target preparation over a descriptor table (datasets/batch_prep.py, csrc/batch_prep.hip): what
 * mte_resize_depth_preserve, the edge maps' conditional /255 and mte_normal_target_from_u8 do per map, for all maps of a batch in a fixed
 * number of launches (one fill + three kernels, whatever n_maps is) and without a host read.
 * arena: the batch's raw file contents on the device (arena_bytes bytes).  table: n_maps rows of MTE_BATCH_PREP_ROW_WORDS 64-bit integers
 *   (kind, src_off, src_h, src_w, crop_x, crop_y, crop_h, crop_w, dst_off, dst_h, dst_w, 0): the source map is src_h x src_w elements of its
 *   kind's type at byte src_off of the arena (aligned to that type), the crop window lies inside it, the result is dst_h x dst_w floats at
 *   element dst_off of `out` (out_elems floats).  table_host and table_dev hold the SAME rows: the host copy is checked before anything is
 *   launched (every offset, window and size; MTE_ERR_ARG otherwise), the kernels read the device copy.
 * kinds: MTE_PREP_EDGE_U8    crop, preserve-resize of the pixels > 0 (target (int(y*H/h), int(x*W/w)) in double, last pixel in raster order
 *                            wins, pixels that land outside are dropped), then x float32(1 / 255) if the maximum of the RESIZED map is > 1,
 *                            decided per map on the device (the product, not the quotient: what `map / 255.0` of the per-sample path gives)
 *        MTE_PREP_SPARSE_U16 16-bit depth: 0 = no return, otherwise float(v) / 256; crop, preserve-resize
 *        MTE_PREP_SPARSE_F32 float depth as it is; crop, preserve-resize
 *        MTE_PREP_NORMAL_U8  crop, (360 * (v / 255) - 180) * pi / 180 in double; the crop window must have the target's size
 * work: winner_elems + n_maps ints of scratch, content on entry ignored; every map that is not MTE_PREP_NORMAL_U8 must end at or before
 *   element winner_elems of `out` (lay the normals out last).  Integer atomics only: bit-reproducible. */
#define MTE_PREP_EDGE_U8 0
#define MTE_PREP_SPARSE_U16 1
#define MTE_PREP_SPARSE_F32 2
#define MTE_PREP_NORMAL_U8 3
#define MTE_BATCH_PREP_ROW_WORDS 12
int mte_batch_prep(const unsigned char* arena, long arena_bytes, const long* table_host, const long* table_dev, int n_maps, float* out,
                   long out_elems, int* work, long winner_elems, mte_stream_t stream);

/* ---- sparse LiDAR input (utils/depth.py:366-467 augment_depth_values; datasets/gta_dataset.py:85-104 process_lidar), csrc/lidar_prep.hip
 * Sparse maps are float32 [H,W] with 0 = no return, H * W < 2^30.  All arithmetic is double; results are rounded to float32 once, on the
 * final store.  The perturbation runs in three stages that share `work` (mte_lidar_perturb_work_bytes(H, W) bytes, 8-byte aligned, content
 * on entry ignored); its first two 32-bit words are the counts the host reads between the stages: work[0] = n, work[1] = n'.
 * mte_lidar_index:   every pixel > 0 gets its ordinal k in raster order (np.where); n = their number.
 * mte_lidar_perturb: n = the count read from work[0] (> 0; the kernels never walk past the device's own count), add_* = float64 [n] draws.
 *   d' = add_d[k] + d * scale_d0;  i' = rint(i + add_i[k]), j' = rint(j + add_j[k]) (half to even);  key = i' + H * (j' - 1);
 *   cell ii = key mod H (non-negative), jj = (key - ii) / H + 1: a row index outside [0, H) wraps into the neighbouring column and only
 *   0 <= jj < W is tested.  Every point whose key is the smallest key of the map is discarded; among points with equal key the lowest
 *   ordinal survives (the reference under a stable argsort; integer atomicMin, bit-reproducible).  Survivors with jj in range get the rank
 *   m = their order by ordinal; n' = their number.
 * mte_lidar_scatter: keep = uint8 [n_keep], n_keep = n' (0: keep may be null); out[ii,jj] = float32(d') for survivors with keep[m] == 1,
 *   every other element of out is written as 0.  n == 0 (an empty map) writes zeros without reading `work`.
 * mte_lidar_project: points float64 [3,N], K float64 [9] (row major), both on the device.  p = K P, p_norm = p / p[2]; a point is kept where
 *   0 <= p_norm[0] < W and 0 <= p_norm[1] < H (false for non-finite quotients; points behind the camera pass when their quotients do), its
 *   pixel is the truncation of p_norm, its value p[2]; the point with the highest index wins a shared pixel.  depth_map (float32 [H,W],
 *   may be null): cells with lidar > 0 and sqrt((lidar - depth)^2) > 0.1 become 0.  winner_ws: H*W ints of scratch. */
long mte_lidar_perturb_work_bytes(int H, int W);
int mte_lidar_index(const float* depth, int H, int W, void* work, mte_stream_t stream);
int mte_lidar_perturb(const float* depth, int H, int W, int n, double scale_d0, const double* add_i, const double* add_j, const double* add_d,
                      void* work, mte_stream_t stream);
int mte_lidar_scatter(int H, int W, int n, const unsigned char* keep, int n_keep, float* out, const void* work, mte_stream_t stream);
int mte_lidar_project(const double* points, int N, const double* K, const float* depth_map, float* out, int H, int W, int* winner_ws,
                      mte_stream_t stream);

/* ---- the perturbation above for a whole batch in a fixed number of launches and without a host read (datasets/lidar_prep.py::
 * perturb_batch, called by datasets/prefetch.py::DeviceStage; csrc/lidar_prep.hip).  index -> perturb -> scatter of mte_lidar_index /
 * mte_lidar_perturb / mte_lidar_scatter, the same kernel bodies with the sample in blockIdx.y, over lidar float32 [B,H,W] into out float32
 * [B,H,W] (every element written).  The host has computed both counts of every map beforehand (lidar_prep.py::resized_cells,
 * count_survivors) and has sized the draws with them.
 * arena (arena_bytes bytes, on the device) holds the draws; table: B rows of MTE_LIDAR_BATCH_ROW_WORDS 64-bit integers
 *   (n, n', bits of the double scale_d0, add_i_off, add_j_off, add_d_off, keep_off, 0): byte offsets into the arena of float64 [n] x 3
 *   (8-byte aligned) and uint8 [n'].  table_host and table_dev hold the SAME rows: the host copy is checked before anything is launched
 *   (0 <= n' <= n <= H*W, every array inside the arena; MTE_ERR_ARG otherwise), the kernels read the device copy.
 * Every loop runs to min(the table's count, the device's own count), so a table whose counts are wrong gives a wrong map, never an access
 *   outside the draws or the workspace; status int [B,4] = (n of the table, n of the device, n' of the table, n' of the device) per sample is
 *   written by the last launch for the host to compare afterwards.
 * work: mte_batch_lidar_perturb_work_bytes(B, H, W) bytes (0 for an unsupported shape; B <= 65535), 8-byte aligned, content on entry ignored;
 *   one private area per sample.  Nine launches whatever B is; double arithmetic, integer atomics only, no kernel waits on another
 *   workgroup: bit-reproducible. */
#define MTE_LIDAR_BATCH_ROW_WORDS 8
long mte_batch_lidar_perturb_work_bytes(int B, int H, int W);
int mte_batch_lidar_perturb(const float* lidar, int B, int H, int W, const unsigned char* arena, long arena_bytes, const long* table_host,
                            const long* table_dev, float* out, void* work, int* status, mte_stream_t stream);

/* ---- depth visualisation and ordinal error of the inference side (utils/depth.py:67-101 viz_inv_depth; infer_edges.py:355-366 the log
 * colouring; utils/d3r.py), csrc/depth_viz.hip.  Every result is an integer or a copy of an input value: no floating-point atomics, results
 * are bit-equal run to run.  Inputs are FINITE float32 (a NaN has no place in the order; it is not looked for).
 * mte_order_stats_f32: image b = x[b * stride .. b * stride + n) (stride 0: the same image under several k); k = int [B] on the device.
 *   out[b] = (the k[b]-th, the (k[b]+1)-th) smallest value, 0-based, both clamped to the last one; with positive_only (the reference's
 *   filter_zeros) over the values > 0 only.  count_out (nullable): int [B], the number n' of values that took part (n, or those > 0); the
 *   host reads it first where k depends on it.  n' = 0 gives (0, 0).  -0 is returned as +0.  Radix select, four 8-bit passes over the
 *   order-preserving key, two launches each; work: mte_order_stats_work_bytes(B) bytes, 4-byte aligned, content on entry ignored.
 *   B <= 65535; MTE_ERR_UNSUPPORTED for n >= 2^30.  np.percentile's interpolation between the two values is the host's (utils/depth.py).
 * mte_colormap_u8: out uint8 [B,H,W,3] = table[idx], table = uint8 [256,3] on the device (the host quantises a float table by its caller's
 *   rule: round-half-even for the cv2.imwrite path -- parity-unpinned against OpenCV's saturate_cast --, truncation for the log colouring),
 *   idx = min(int(clip(t, 0, 1) * 256), 255) -- matplotlib's rule --, NaN -> (0, 0, 0).  lo_hi null: t = x / divisor[b] (IEEE float32
 *   division).  lo_hi = float [B,2]: t = (float32(log(double(x))) - lo_hi[b][0]) / lo_hi[b][1] and divisor is not read.  A thread owns 4
 *   pixels = 12 output bytes; `out` 4-byte aligned.  MTE_ERR_UNSUPPORTED for B*H*W >= 2^30.
 * mte_d3r_count: gt, pred float32 [H,W]; index_work = the workspace mte_lidar_index(gt, H, W, ..) filled (the raster-order list of pixels
 *   > 0), n = its count as read by the host; pairs = int [P,2] ordinals into that list.  *count (int, overwritten) = the number of pairs with
 *   (g > 1 + 0.03 and p > float32(1 + 0.03)) or (g < 1 - 0.03 and p < float32(1 - 0.03)), g = the ratio of the two ground-truth values in
 *   double, p = the ratio of the two predictions in float32.  A pair with an ordinal outside [0, n) counts as disagreeing. */
long mte_order_stats_work_bytes(int B);
int mte_order_stats_f32(const float* x, long stride, int B, long n, const int* k, int positive_only, float* out, int* count_out, void* work,
                        mte_stream_t stream);
int mte_colormap_u8(const float* x, int B, int H, int W, const float* divisor, const float* lo_hi, const unsigned char* table, unsigned char* out,
                    mte_stream_t stream);
int mte_d3r_count(const float* gt, const float* pred, int H, int W, const void* index_work, int n, const int* pairs, int P, int* count,
                  mte_stream_t stream);

#ifdef MTE_DEV
/* Development knobs for same-box A/B measurements (tools/sweep.sh) and kernel-variant cross-checks (tests/).  NOT part of the
 * integration surface: exported only by libmte_hip_dev.so, the -DMTE_DEV build of the same sources (mindtheedge_amd/_build.py);
 * libmte_hip.so, the shipped library, has neither this entry point nor the ablation arms of the implicit-GEMM template.  key:
 *   0 igemm loader (1 buffer-descriptor LDS-DMA [default], 2 pointer LDS-DMA, 0 register staging)
 *   1 conv3d kernels (0 gather, 1 LDS-tiled, 2 + four-plane unpack data gradient [default]; 100/101 large/half-size tiles)
 *   2 / 3 GroupNorm launch geometry (min rows per thread / target workgroups)
 *   4 wgrad kernel (1 LDS-DMA ring [default], 0 register-staged)      6 igemm tiles (0 128x128, 1 + 256x128, 2 + 256x256, 3 + 192x96 [default])
 *   7 min tiles for the big igemm tiles (224)   8 wgrad 8/16-wave tiles (1)   9 wgrad workgroup target (512)
 *   11 patch conv: 0/1 tall 16x32 tiles, >= 100 = workgroup target of the patch wgrad (512)
 *   13 GroupNorm single-pass slab kernels (1 [default], 0 = streaming kernels only)
 *   14 GroupNorm second passes walk the samples in reverse order (Infinity-Cache reuse; 1 [default])
 *   15 implicit GEMM, 8-wave 256x128 tile: 0 [default] 4-slot LDS ring, 3-slot / two workgroups per CU for MTE_CONV_SOLO launches;
 *      1 = 6 slots, 3 = always 3 slots x 2 workgroups, 4 = always 4 slots
 *   19 implicit GEMM: two-workgroup 256x128 variant beside the
 *      weight-gradient stream for launches with at most this many K-steps and >= 512 tiles (72 [default], 0 = solo launches only)
 *   17 implicit GEMM main-loop ablation (tools/igemm_ablate.py): leave out 1 MFMAs | 2 in-loop LDS-DMA | 4 fragment reads; results are garbage
 *   33 every implicit-GEMM key (0, 6, 7, 15, 17, 19, 21, 23, 24, 28, 29, 32: IgemmKnobs, csrc/conv_plan.hpp) back to its default; the value is ignored */
int mte_debug_set(int key, int value);
#endif /* MTE_DEV */

#ifdef __cplusplus
}
#endif
#endif /* MTE_KERNELS_H */
