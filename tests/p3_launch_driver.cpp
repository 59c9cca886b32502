// conv3d pack / unpack driver of the launch recorder (tests/conv_launch_recorder.py --p3): linked against pack3d.hip (and, for mte_debug_set, conv_igemm.hip and
// conv_igemm8.hip) compiled for the host with conv_launch_shim.hpp in front.  Reads one case per line from standard input,
//     <op> <dtype> <B> <H> <W> <C> <ldx> <ldo> <key=value,...|->
// op: pack_fwd | pack_bwd_data | pack_bwd_weight | unpack_fwd | unpack_bwd_data | unpack_bwd_weight.  B, H, W, C: the un-packed side tensor; ldx its pixel stride,
// ldo that of the feature side (pack: [B,H/2,W/2,16C]; unpack: [B,2H,2W,C]).  Sets the knobs, calls the entry point with dummy pointers and prints
//     {"case": <the line>, "rc": <return code>, "launches": [...]}
#define MTE_REC_WITH_PACK3D
#include "launch_driver.hpp"

extern "C" {
int mte_pack3d_fwd(const void* x, long ldx, const float* w3, const float* b3, void* out, long ldo, int B, int H, int W, int C, int dtype, hipStream_t stream);
int mte_pack3d_bwd_data(const void* dout, long ldo, const float* w3, void* dx, long lddx, int B, int H, int W, int C, int dtype, hipStream_t stream);
int mte_pack3d_bwd_weight(const void* x, long ldx, const void* dout, long ldo, float* dwb, int B, int H, int W, int C, int dtype, hipStream_t stream);
int mte_unpack3d_fwd(const void* x, long ldx, const float* w3, const float* b3, void* out, long ldo, int B, int H, int W, int C, int dtype, hipStream_t stream);
int mte_unpack3d_bwd_data(const void* dout, long ldo, const float* w3, void* dx, long lddx, int B, int H, int W, int C, int dtype, hipStream_t stream);
int mte_unpack3d_bwd_weight(const void* x, long ldx, const void* dout, long ldo, float* dwb, int B, int H, int W, int C, int dtype, hipStream_t stream);
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
    int dtype, B, H, W, C;
    long ldx, ldo;
    if (sscanf(line, "%31s %d %d %d %d %d %ld %ld %511s", op, &dtype, &B, &H, &W, &C, &ldx, &ldo, knobs) != 9) return 2;
    if (!set_knobs(knobs)) return 2;
    void* const x = buf(0, "x"); void* const o = buf(1, "o"); float* const w3 = (float*)buf(2, "w3"); float* const b3 = (float*)buf(3, "b3"); float* const dwb = (float*)buf(4, "dwb");
    int rc;
    if (!strcmp(op, "pack_fwd")) rc = mte_pack3d_fwd(x, ldx, w3, b3, o, ldo, B, H, W, C, dtype, nullptr);
    else if (!strcmp(op, "pack_bwd_data")) rc = mte_pack3d_bwd_data(o, ldo, w3, x, ldx, B, H, W, C, dtype, nullptr);
    else if (!strcmp(op, "pack_bwd_weight")) rc = mte_pack3d_bwd_weight(x, ldx, o, ldo, dwb, B, H, W, C, dtype, nullptr);
    else if (!strcmp(op, "unpack_fwd")) rc = mte_unpack3d_fwd(x, ldx, w3, b3, o, ldo, B, H, W, C, dtype, nullptr);
    else if (!strcmp(op, "unpack_bwd_data")) rc = mte_unpack3d_bwd_data(o, ldo, w3, x, ldx, B, H, W, C, dtype, nullptr);
    else if (!strcmp(op, "unpack_bwd_weight")) rc = mte_unpack3d_bwd_weight(x, ldx, o, ldo, dwb, B, H, W, C, dtype, nullptr);
    else return 2;
    printf("{\"case\":\"%s\",\"rc\":%d,\"launches\":[%s]}\n", line, rc, mte_rec::log().c_str());
    return 0;
}

int main() { return run_cases(run_case); }
