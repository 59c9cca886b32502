// Driver of the launch recorder (tests/conv_launch_recorder.py): linked against conv_igemm.hip and conv_igemm8.hip compiled for the host with
// conv_launch_shim.hpp in front.  Reads one case per line from standard input,
//     <entry> <dtype> <B> <H> <W> <Cin_p> <N> <KH> <KW> <ldx> <out_f32> <has_ws> <ws_elems> <accumulate> <key=value,...|->
// (entry: igemm | unshuffle | sparse), calls the C entry point with dummy non-null pointers in a child process of its own (the knobs and the once-per-kernel
// statics start fresh for every case) and prints {"case": <the line>, "rc": <return code>, "launches": [...]}.  The knobs need the -DMTE_DEV build.
#include "launch_driver.hpp"

extern "C" {
int mte_conv2d_igemm(const void* x, long ldx, const void* wpack, const float* bias, void* y, long ldy, int out_f32, int B, int H, int W, int Cin_p, int N, int KH,
                     int KW, int dtype, float* workspace, long workspace_elems, int accumulate, hipStream_t stream);
int mte_conv2d_igemm_unshuffle(const void* x, long ldx, const void* wpack, void* y, long ldy, int B, int H, int W, int Cin_p, int N, int KH, int KW, int dtype,
                               int accumulate, hipStream_t stream);
int mte_conv2d_igemm_sparse(const void* x, long ldx, const void* wpack, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N, int KH, int KW,
                            int dtype, const int* sites, const int* count, int accumulate, hipStream_t stream);
int mtei_set_gn(int, int) { return 0; }                                 // (norm_act.hip is not linked)
}
int g_mte_wgrad_shared = 0;

static int run_case(const char* line) {
    char entry[32], knobs[512];
    int dtype, B, H, W, Cin_p, N, KH, KW, out_f32, has_ws, accumulate;
    long ldx, ws_elems;
    if (sscanf(line, "%31s %d %d %d %d %d %d %d %d %ld %d %d %ld %d %511s", entry, &dtype, &B, &H, &W, &Cin_p, &N, &KH, &KW, &ldx, &out_f32, &has_ws, &ws_elems,
               &accumulate, knobs) != 15) return 2;
    if (!set_knobs(knobs)) return 2;
    void* const p = (void*)0x1000;                                      // never dereferenced: no launch reaches a device
    int rc;
    if (!strcmp(entry, "igemm"))
        rc = mte_conv2d_igemm(p, ldx, p, (const float*)p, p, N, out_f32, B, H, W, Cin_p, N, KH, KW, dtype, has_ws ? (float*)p : nullptr, ws_elems, accumulate, nullptr);
    else if (!strcmp(entry, "unshuffle"))
        rc = mte_conv2d_igemm_unshuffle(p, ldx, p, p, N / 4, B, H, W, Cin_p, N, KH, KW, dtype, accumulate, nullptr);
    else if (!strcmp(entry, "sparse"))
        rc = mte_conv2d_igemm_sparse(p, ldx, p, (const float*)p, p, N, B, H, W, Cin_p, N, KH, KW, dtype, (const int*)p, (const int*)p, accumulate, nullptr);
    else return 2;
    printf("{\"case\":\"%s\",\"rc\":%d,\"launches\":[%s]}\n", line, rc, mte_rec::log().c_str());
    return 0;
}

int main() { return run_cases(run_case); }
