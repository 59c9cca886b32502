// Driver of the launch recorder (tests/conv_launch_recorder.py): linked against conv_igemm.hip and conv_igemm8.hip compiled for the host with
// conv_launch_shim.hpp in front.  Reads one case per line from standard input,
//     <entry> <dtype> <B> <H> <W> <Cin_p> <N> <KH> <KW> <ldx> <out_f32> <has_ws> <ws_elems> <accumulate> <key=value,...|->
// (entry: igemm | unshuffle | sparse), calls the C entry point with dummy non-null pointers in a child process of its own (the knobs and the once-per-kernel
// statics start fresh for every case) and prints {"case": <the line>, "rc": <return code>, "launches": [...]}.  The knobs need the -DMTE_DEV build.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <string>
#include <unistd.h>
#include <sys/wait.h>
#include "conv_launch_shim.hpp"

extern "C" {
int mte_conv2d_igemm(const void* x, long ldx, const void* wpack, const float* bias, void* y, long ldy, int out_f32, int B, int H, int W, int Cin_p, int N, int KH,
                     int KW, int dtype, float* workspace, long workspace_elems, int accumulate, hipStream_t stream);
int mte_conv2d_igemm_unshuffle(const void* x, long ldx, const void* wpack, void* y, long ldy, int B, int H, int W, int Cin_p, int N, int KH, int KW, int dtype,
                               int accumulate, hipStream_t stream);
int mte_conv2d_igemm_sparse(const void* x, long ldx, const void* wpack, const float* bias, void* y, long ldy, int B, int H, int W, int Cin_p, int N, int KH, int KW,
                            int dtype, const int* sites, const int* count, int accumulate, hipStream_t stream);
int mte_debug_set(int key, int value);
// what the two objects need from the rest of the library
int mtei_set_pack3d_lds(int) { return 0; }
int mtei_set_gn(int, int) { return 0; }
int mtei_set_patch_tall(int) { return 0; }
int mtei_set_tap_wgrad(int) { return 0; }
int mtei_set_head_mfma(int) { return 0; }
}
// A host-only object still registers its (absent) device code at start-up: answered here, so that this too stays out of the HIP runtime
// (-fuse-cuid=none gives the fat-binary symbol one name in all objects; their one-byte __hip_cuid_ markers then collide, which the link is told to allow).
extern "C" {
char __hip_fatbin[8] = {0};
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
}
int g_wgrad9 = 1, g_wgrad9_wgs = 0, g_mte_wgrad_shared = 0;
int wgrad9_launch(const void*, long, const void*, long, float*, int, int*, int, int, int, int, int, hipStream_t) { return -3; }

#ifdef MTE_REC_COVERAGE
extern "C" void __gcov_dump(void);
#endif

static int run_case(const char* line) {
    char entry[32], knobs[512];
    int dtype, B, H, W, Cin_p, N, KH, KW, out_f32, has_ws, accumulate;
    long ldx, ws_elems;
    if (sscanf(line, "%31s %d %d %d %d %d %d %d %d %ld %d %d %ld %d %511s", entry, &dtype, &B, &H, &W, &Cin_p, &N, &KH, &KW, &ldx, &out_f32, &has_ws, &ws_elems,
               &accumulate, knobs) != 15) return 2;
    if (strcmp(knobs, "-") != 0) {
#ifdef MTE_DEV
        for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
            int key, value;
            if (sscanf(tok, "%d=%d", &key, &value) != 2 || mte_debug_set(key, value) != 0) return 2;
        }
#else
        return 2;                                                       // the product library has no knobs
#endif
    }
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
    fflush(stdout);
    return 0;
}

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\n")] = 0;
        if (!line[0]) continue;
        fflush(stdout);
        const pid_t pid = fork();
        if (pid == 0) {
            const int rc = run_case(line);
#ifdef MTE_REC_COVERAGE                                                    // a --coverage build: the counters are written at exit(), which the child skips
            __gcov_dump();
#endif
            _exit(rc);
        }
        int status = 0;
        if (pid < 0 || waitpid(pid, &status, 0) != pid || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
            fprintf(stderr, "case failed: %s\n", line);
            return 1;
        }
    }
    return 0;
}
