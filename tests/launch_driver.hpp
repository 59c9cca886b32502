// What the drivers of the launch recorder share (conv_launch_driver.cpp, gn_launch_driver.cpp, p3_launch_driver.cpp, patch_launch_driver.cpp, wgrad_launch_driver.cpp): the stand-ins for the rest of the library, the knob list of a
// case, and the loop that runs every case in a child process of its own.
#pragma once
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <string>
#include <unistd.h>
#include <sys/wait.h>
#include "conv_launch_shim.hpp"

extern "C" {
int mte_debug_set(int key, int value);
// what conv_igemm.hip needs from the sources that are not linked
#ifndef MTE_REC_WITH_PACK3D                                                 // (the conv3d driver links pack3d.hip, which has the real one)
int mtei_set_pack3d_lds(int) { return 0; }
#endif
#if !defined(MTE_REC_WITH_PATCH) || !defined(MTE_DEV)                      // (the LDS-patch driver links conv_patch.hip, whose development build has the real one)
int mtei_set_patch_tall(int) { return 0; }
#endif
int mtei_set_tap_wgrad(int) { return 0; }
int mtei_set_head_mfma(int) { return 0; }
// A host-only object still registers its (absent) device code at start-up: answered here, so that this too stays out of the HIP runtime
// (-fuse-cuid=none gives the fat-binary symbol one name in all objects; their one-byte __hip_cuid_ markers then collide, which the link is told to allow).
char __hip_fatbin[8] = {0};
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
}

#ifdef MTE_REC_COVERAGE
extern "C" void __gcov_dump(void);
#endif

// "key=value,..." or "-": through mte_debug_set, which only the -DMTE_DEV build has.  -> false: a bad list, or knobs asked of the product build
static bool set_knobs(char* knobs) {
    if (!strcmp(knobs, "-")) return true;
#ifdef MTE_DEV
    for (char* tok = strtok(knobs, ","); tok; tok = strtok(nullptr, ",")) {
        int key, value;
        if (sscanf(tok, "%d=%d", &key, &value) != 2 || mte_debug_set(key, value) != 0) return false;
    }
    return true;
#else
    return false;
#endif
}

// one case per line of standard input, each in a child process (the knobs and the once-per-kernel statics start fresh); run_case prints the case's line
static int run_cases(int (*run_case)(const char*)) {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\n")] = 0;
        if (!line[0]) continue;
        fflush(stdout);
        const pid_t pid = fork();
        if (pid == 0) {
            const int rc = run_case(line);
            fflush(stdout);
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
