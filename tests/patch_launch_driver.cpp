// LDS-patch convolution driver of the launch recorder (tests/conv_launch_recorder.py --patch): linked against conv_patch.hip (and, for mte_debug_set, conv_igemm.hip
// and conv_igemm8.hip) compiled for the host with conv_launch_shim.hpp in front.  Reads one case per line from standard input,
//     <entry> <B> <H> <W> <Cin_p> <N> <KH> <KW> <ldx> <accumulate> <bias> <C2> <parts_cap> <shared> <key=value,...|->
// entry: fwd | fwd_gn | rank1 | plus1x1 | wgrad | repack (the launching entry points), supported | wgrad_supported | rank1_ok (the queries), pack_elems | gn_elems.
// bias: -1 = a null pointer, otherwise the bias pointer's offset in bytes from a 16-byte boundary; C2: channels of the 1x1 term (plus1x1); parts_cap: slabs the
// stage has room for (wgrad); shared: MTE_OPT_WGRAD_SHARES_CHIP, which this driver holds itself.  Sets the knobs, calls the entry point with dummy pointers and prints
//     {"case": <the line>, "rc": <return code or the query's answer>, "parts": <*parts_out>, "tiles": <*tiles_per_sample_out>, "launches": [...]}
// (parts only for wgrad, tiles only for fwd_gn).
#define MTE_REC_WITH_PATCH
#include "launch_driver.hpp"

extern "C" {
int mte_conv2d_patch_supported(int W, int Cin_p, int N, int KH, int KW, int dtype);
int mte_conv2d_patch_wgrad_supported(int W, int Cin_p, int N, int KH, int KW, int dtype);
long mte_conv2d_patch_pack_elems(int Cin_p, int N, int KH, int KW);
int mte_conv2d_patch_repack(const void* wgeneric, void* wpatch, int Cin_p, int N, int KH, int KW, hipStream_t stream);
int mte_conv2d_patch_fwd(const void* x, long ldx, const void* wpatch, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N, int KH, int KW,
                         int accumulate, hipStream_t stream);
long mte_conv2d_patch_fwd_gn_elems(int B, int H, int W);
int mte_conv2d_patch_fwd_gn(const void* x, long ldx, const void* wpatch, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N, int KH, int KW,
                            int accumulate, float* rec, long rec_elems, int* tiles_per_sample_out, hipStream_t stream);
int mte_conv2d_patch_fwd_rank1_ok(const float* bias, long ldx, int B, int H, int W, int Cin_p, int N);
int mte_conv2d_patch_fwd_rank1(const void* x, long ldx, const void* wpatch, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N,
                               const float* inv, const float* w1, long w1_stride, hipStream_t stream);
int mte_conv2d_patch_fwd_plus1x1(const void* x, long ldx, const void* wpatch, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N,
                                 const void* x2, long ldx2, const void* wpatch2, int C2, hipStream_t stream);
int mte_conv2d_patch_wgrad(const void* x, long ldx, const void* dy, long lddy, float* dw_stage, int stage_parts, int* parts_out,
                           int B, int H, int W, int Cin_p, int N, int KH, int KW, hipStream_t stream);
int mtei_set_gn(int, int) { return 0; }                                 // (norm_act.hip is not linked)
}
int g_mte_wgrad_shared = 0;

// a dummy buffer, never dereferenced (no launch reaches a device): slot k is 4 GiB wide; named, so that a clear says which buffer it was
static void* buf(int k, const char* name) {
    const uintptr_t p = (uintptr_t)(k + 1) << 32;
    mte_rec::buffers()[p] = name;
    return (void*)p;
}

static int run_case(const char* line) {
    char op[32], knobs[512];
    int B, H, W, C, N, KH, KW, acc, bias_off, C2, cap, shared;
    long ldx;
    if (sscanf(line, "%31s %d %d %d %d %d %d %d %ld %d %d %d %d %d %511s", op, &B, &H, &W, &C, &N, &KH, &KW, &ldx, &acc, &bias_off, &C2, &cap, &shared, knobs) != 15) return 2;
    if (!set_knobs(knobs)) return 2;
    g_mte_wgrad_shared = shared;
    void* const x = buf(0, "x"); void* const wp = buf(1, "wp"); void* const y = buf(2, "y"); void* const x2 = buf(3, "x2"); void* const wp2 = buf(4, "wp2");
    float* const rec = (float*)buf(5, "rec"); float* const inv = (float*)buf(6, "inv"); float* const w1 = (float*)buf(7, "w1"); float* const dw = (float*)buf(8, "dw");
    const float* const bias = bias_off < 0 ? nullptr : (const float*)((uintptr_t)buf(9, "bias") + bias_off);
    const long ldy = N;
    long rc;
    int parts = -1, tiles = -1;
    std::string more;
    if (!strcmp(op, "fwd")) rc = mte_conv2d_patch_fwd(x, ldx, wp, bias, y, ldy, B, H, W, C, N, KH, KW, acc, nullptr);
    else if (!strcmp(op, "fwd_gn")) {
        rc = mte_conv2d_patch_fwd_gn(x, ldx, wp, bias, y, ldy, B, H, W, C, N, KH, KW, acc, rec, mte_conv2d_patch_fwd_gn_elems(B, H, W), &tiles, nullptr);
        more = ",\"tiles\":" + std::to_string(tiles);
    } else if (!strcmp(op, "rank1")) rc = mte_conv2d_patch_fwd_rank1(x, ldx, wp, bias, y, ldy, B, H, W, C, N, inv, w1, (long)(C + 1) * 9, nullptr);
    else if (!strcmp(op, "plus1x1")) rc = mte_conv2d_patch_fwd_plus1x1(x, ldx, wp, bias, y, ldy, B, H, W, C, N, x2, C2, wp2, C2, nullptr);
    else if (!strcmp(op, "wgrad")) {
        rc = mte_conv2d_patch_wgrad(x, ldx, y, ldy, dw, cap, &parts, B, H, W, C, N, KH, KW, nullptr);
        more = ",\"parts\":" + std::to_string(parts);
    } else if (!strcmp(op, "repack")) rc = mte_conv2d_patch_repack(x, wp, C, N, KH, KW, nullptr);
    else if (!strcmp(op, "supported")) rc = mte_conv2d_patch_supported(W, C, N, KH, KW, 0);
    else if (!strcmp(op, "wgrad_supported")) rc = mte_conv2d_patch_wgrad_supported(W, C, N, KH, KW, 0);
    else if (!strcmp(op, "rank1_ok")) rc = mte_conv2d_patch_fwd_rank1_ok(bias, ldx, B, H, W, C, N);
    else if (!strcmp(op, "pack_elems")) rc = mte_conv2d_patch_pack_elems(C, N, KH, KW);
    else if (!strcmp(op, "gn_elems")) rc = mte_conv2d_patch_fwd_gn_elems(B, H, W);
    else return 2;
    printf("{\"case\":\"%s\",\"rc\":%ld%s,\"launches\":[%s]}\n", line, rc, more.c_str(), mte_rec::log().c_str());
    return 0;
}

int main() { return run_cases(run_case); }
