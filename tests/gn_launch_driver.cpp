// GroupNorm driver of the launch recorder (tests/conv_launch_recorder.py --gn): linked against norm_act.hip (and, for mte_debug_set, conv_igemm.hip and
// conv_igemm8.hip) compiled for the host with conv_launch_shim.hpp in front.  Reads one case per line from standard input,
//     <entry> <dtype> <B> <HW> <C> <second> <dbias> <stats_ready> <prezeroed> <key=value,...|->
// entry: stats | fwd | bwd | tail.  second: 0 = one tensor; 1 = a second input y2 with its scale2 (bwd: and the second output d2); bwd only: 2 = one input whose
// gradient also leaves scaled (scale2 and d2, no y2), 3 = d2 with neither y2 nor scale2 (refused).  dbias: bwd only.  stats_ready: fwd only.
// Sets the knobs and mte_set_option(0, prezeroed), calls the entry point with dummy pointers and prints
//     {"case": <the line>, "rc": <return code>, "q": mte_gn_fwd_is_single_pass, "qb": mte_gn_fwd_is_single_pass_b, "launches": [...]}     (q, qb left out where 0)
#include "launch_driver.hpp"

extern "C" {
int mte_gn_fwd_is_single_pass(int HW, int C, int has_y2, int dtype);
int mte_gn_fwd_is_single_pass_b(int B, int HW, int C, int has_y2, int dtype);
int mte_gn_stats(const void* y1, long ld1, const void* y2, long ld2, const float* scale2, double* stats, int B, int HW, int C, int dtype, hipStream_t stream);
int mte_gn_elu_fwd(const void* y1, long ld1, const void* y2, long ld2, const float* scale2, double* stats, int stats_ready, const float* gamma, const float* beta,
                   void* z, long ldz, int B, int HW, int C, float eps, int dtype, hipStream_t stream);
int mte_gn_elu_bwd(const void* dz, long lddz, const void* y1, long ld1, const void* y2, long ld2, const float* scale2, const double* stats, const float* gamma,
                   const float* beta, float* red, void* d1, long ldd1, void* d2, long ldd2, float* dgamma, float* dbeta, float* dbias, int B, int HW, int C,
                   float eps, int dtype, hipStream_t stream);
int mte_gn_tail_fwd(const void* y1, long ld1, const double* stats1, const float* gamma1, const float* beta1, const void* y2, long ld2, const float* scale2, void* t,
                    long ldt, double* stats_t, const float* gamma_t, const float* beta_t, void* z, long ldz, int B, int HW, int C, float eps, int dtype,
                    hipStream_t stream);
int mte_set_option(int option, int value);
}
int g_mte_loss_prezeroed = 0;                                           // (edge_loss.hip is not linked)

// a dummy buffer, never dereferenced (no launch reaches a device): slot k is 4 GiB wide; named, so that a clear says which buffer it was
static void* buf(int k, const char* name) {
    const uintptr_t p = (uintptr_t)(k + 1) << 32;
    mte_rec::buffers()[p] = name;
    return (void*)p;
}

static int run_case(const char* line) {
    char entry[32], knobs[512];
    int dtype, B, HW, C, second, dbias, ready, prezeroed;
    if (sscanf(line, "%31s %d %d %d %d %d %d %d %d %511s", entry, &dtype, &B, &HW, &C, &second, &dbias, &ready, &prezeroed, knobs) != 10) return 2;
    if (!set_knobs(knobs) || mte_set_option(0, prezeroed) != 0) return 2;
    void* const y1 = buf(0, "y1"); void* const y2 = buf(1, "y2"); float* const scale2 = (float*)buf(2, "scale2"); double* const stats = (double*)buf(3, "stats");
    float* const gamma = (float*)buf(4, "gamma"); float* const beta = (float*)buf(5, "beta"); void* const z = buf(6, "z"); void* const dz = buf(7, "dz");
    float* const red = (float*)buf(8, "red"); void* const d1 = buf(9, "d1"); void* const d2 = buf(10, "d2"); float* const dgamma = (float*)buf(11, "dgamma");
    float* const dbeta = (float*)buf(12, "dbeta"); float* const db = (float*)buf(13, "dbias"); double* const stats1 = (double*)buf(14, "stats1"); void* const t = buf(15, "t");
    const bool two = second == 1;
    const int q = mte_gn_fwd_is_single_pass(HW, C, two, dtype), qb = mte_gn_fwd_is_single_pass_b(B, HW, C, two, dtype);
    if (!mte_rec::log().empty()) return 2;                              // (a query launches nothing)
    int rc;
    if (!strcmp(entry, "stats"))
        rc = mte_gn_stats(y1, C, two ? y2 : nullptr, C, two ? scale2 : nullptr, stats, B, HW, C, dtype, nullptr);
    else if (!strcmp(entry, "fwd"))
        rc = mte_gn_elu_fwd(y1, C, two ? y2 : nullptr, C, two ? scale2 : nullptr, stats, ready, gamma, beta, z, C, B, HW, C, 1e-5f, dtype, nullptr);
    else if (!strcmp(entry, "bwd"))
        rc = mte_gn_elu_bwd(dz, C, y1, C, two ? y2 : nullptr, C, second == 1 || second == 2 ? scale2 : nullptr, stats, gamma, beta, red, d1, C, second ? d2 : nullptr, C,
                            dgamma, dbeta, dbias ? db : nullptr, B, HW, C, 1e-5f, dtype, nullptr);
    else if (!strcmp(entry, "tail"))
        rc = mte_gn_tail_fwd(y1, C, stats1, gamma, beta, y2, C, two ? scale2 : nullptr, t, C, stats, gamma, beta, z, C, B, HW, C, 1e-5f, dtype, nullptr);
    else return 2;
    printf("{\"case\":\"%s\",\"rc\":%d%s%s,\"launches\":[%s]}\n", line, rc, q ? ",\"q\":1" : "", qb ? ",\"qb\":1" : "", mte_rec::log().c_str());
    return 0;
}

int main() { return run_cases(run_case); }
