// Weight-gradient driver of the launch recorder (tests/conv_launch_recorder.py --wgrad): linked against conv_igemm.hip, conv_igemm8.hip and conv_wgrad9.hip compiled
// for the host with conv_launch_shim.hpp in front.  Reads one case per line from standard input,
//     <entry> <dtype> <B> <H> <W> <Cin_p> <N> <KH> <KW> <ldx> <ldy> <parts_cap> <parts_out> <shared> <cus> <key=value,...|->
// entry: wgrad (mte_conv2d_wgrad) | nine_tap (the query mte_conv2d_wgrad_nine_tap: H, W, Cin_p, N, KH, KW and dtype of the line); parts_cap: slabs the stage has
// room for; parts_out: 1 = passed, 0 = a null pointer; shared: MTE_OPT_WGRAD_SHARES_CHIP, which this driver holds itself; cus: the compute units the shim's device
// query answers.  Sets the knobs, calls the entry point with dummy pointers and prints
//     {"case": <the line>, "rc": <return code or the query's answer>, "parts": <*parts_out>, "launches": [...]}
// (parts only for wgrad; -1 where nothing wrote it).
#include "launch_driver.hpp"

extern "C" {
int mte_conv2d_wgrad(const void* x, long ldx, const void* dy, long ldy, float* dw_stage, int stage_parts, int* parts_out,
                     int B, int H, int W, int Cin_p, int N, int KH, int KW, int dtype, hipStream_t stream);
int mte_conv2d_wgrad_nine_tap(int H, int W, int Cin_p, int N, int KH, int KW, int dtype);
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
    int dtype, B, H, W, C, N, KH, KW, cap, has_parts, shared, cus;
    long ldx, ldy;
    if (sscanf(line, "%31s %d %d %d %d %d %d %d %d %ld %ld %d %d %d %d %511s", op, &dtype, &B, &H, &W, &C, &N, &KH, &KW, &ldx, &ldy, &cap, &has_parts, &shared, &cus, knobs) != 16) return 2;
    if (!set_knobs(knobs)) return 2;
    g_mte_wgrad_shared = shared;
    mte_rec::cus() = cus;
    int parts = -1;
    if (!strcmp(op, "wgrad")) {
        const int rc = mte_conv2d_wgrad(buf(0, "x"), ldx, buf(1, "dy"), ldy, (float*)buf(2, "dw"), cap, has_parts ? &parts : nullptr, B, H, W, C, N, KH, KW, dtype, nullptr);
        printf("{\"case\":\"%s\",\"rc\":%d,\"parts\":%d,\"launches\":[%s]}\n", line, rc, parts, mte_rec::log().c_str());
    } else if (!strcmp(op, "nine_tap")) {
        printf("{\"case\":\"%s\",\"rc\":%d,\"launches\":[]}\n", line, mte_conv2d_wgrad_nine_tap(H, W, C, N, KH, KW, dtype));
    } else return 2;
    return 0;
}

int main() { return run_cases(run_case); }
