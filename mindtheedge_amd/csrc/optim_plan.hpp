// What the optimizer family's entry points (optim.hip) decide on the host, and nothing else: argument rules, kernel instance, grid, the layout of the work
// buffers, and how a tensor table is cut into chunks.  No HIP in here -- plain C++17, so that a CPU test can ask for the plan of any call and enumerate the chunks
// of any table (tests/test_optim_launch_table_cpu.py).  The chunk cut is the one statement the kernels run too: MTE_PLAN_HD is __host__ __device__ under hipcc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef MTE_OK
#define MTE_OK 0
#define MTE_ERR_ARG (-1)
#define MTE_ERR_LAUNCH (-2)
#define MTE_ERR_UNSUPPORTED (-3)
#endif
#ifdef __HIPCC__
#define MTE_PLAN_HD __host__ __device__ __forceinline__
#else
#define MTE_PLAN_HD inline
#endif

namespace optim_plan {

// ---- launch shapes.  The streaming kernels: 256 threads, one 16-byte vector per thread and trip, a grid-stride loop under the 8192-workgroup cap
constexpr int OPT_THREADS = 256;
inline int opt_grid(long n4) { long g = (n4 + OPT_THREADS - 1) / OPT_THREADS; return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g)); }
constexpr int NORM_CAP = 256;                              // workgroups of the norm launch: one of 256 threads per CU (profiles/grad_clip.txt)
inline int norm_grid(long n4) { long g = (n4 + OPT_THREADS - 1) / OPT_THREADS; return (int)(g > NORM_CAP ? NORM_CAP : (g < 1 ? 1 : g)); }
constexpr long STAT_CHUNK = 32768;                         // elements: 128 KB of gradient per record (77.0 M elements: 2350 + 218 chunks)
constexpr int STAT_CAP = 1024;                             // workgroups of the chunk launches
constexpr int STAT_MAX_T = 4096;
constexpr int SEG_MAX_CLASSES = 16;
// the bound the record buffers' size rests on: for disjoint 64-aligned tensors inside [0, n), sum ceil(m_t / C) <= floor(n / C) + T
inline long stat_max_chunks(long n, long T) { return n / STAT_CHUNK + T; }
inline long stat_ticket_bytes(long T) { return (4 * T + 15) / 16 * 16; }
inline int chunk_grid(long max_chunks) { return (int)(max_chunks > STAT_CAP ? STAT_CAP : max_chunks); }

// ---- work buffers, zeroed ONCE by the caller (tickets go back to zero).  Byte offsets from a 16-byte aligned `work`.
// norm: {S (fp64), ticket, pad, one fp64 record per workgroup}
constexpr long NORM_HEAD_BYTES = 16;
struct NormLayout { long sum, ticket, records, record_bytes, bytes; };
inline NormLayout norm_layout(long n) { return {0, 8, NORM_HEAD_BYTES, 8, NORM_HEAD_BYTES + 8L * norm_grid(n >> 2)}; }
// chunk launches: {tickets[T] (unsigned, padded to 16 B), records[n / STAT_CHUNK + T][values] fp64}
constexpr int STAT_VALUES = 4, LAMB_VALUES = 2;            // {S_g, amax_g, non-finite count, S_p} and {S_p, S_d}
struct ChunkLayout { long tickets, records, record_bytes, bytes; };
inline ChunkLayout chunk_layout(long n, long T, int values) {
    return {0, stat_ticket_bytes(T), 8L * values, stat_ticket_bytes(T) + 8L * values * stat_max_chunks(n, T)};
}
inline bool chunk_sizes_ok(long n, long T) { return n > 0 && T >= 1 && T <= STAT_MAX_T; }
inline long grad_norm_work_bytes(long n) { return n <= 0 ? 0 : norm_layout(n).bytes; }
inline long tensor_stats_work_bytes(long n, long T) { return chunk_sizes_ok(n, T) ? chunk_layout(n, T, STAT_VALUES).bytes : 0; }
inline long lamb_work_bytes(long n, long T) { return chunk_sizes_ok(n, T) ? chunk_layout(n, T, LAMB_VALUES).bytes : 0; }

// ---- argument rules: MTE_ERR_ARG, or MTE_OK.  (Every rule gives the same code, so their order decides nothing.)
inline bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) != 0;
}
// two flat ranges of n floats, 16-byte aligned and disjoint (equal pointers included): -> MTE_ERR_ARG, 0 with nothing to launch (n = 0), or 1
inline int flat_pair_check(const void* a, const void* b, long n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    if (!a || !b || n < 0 || ((x | y) & 15) || x == y) return MTE_ERR_ARG;
    if (n == 0) return 0;
    const uintptr_t bytes = (uintptr_t)n * sizeof(float);
    if (x < y + bytes && y < x + bytes) return MTE_ERR_ARG;
    return 1;
}

// the step launches.  HOST: scalars by value (step >= 1); DEV: `hyper` in device memory; CTL: and `ctl`; SEG: hyper, the class tables, n % 64 == 0 (ctl may be null)
enum StepForm { STEP_HOST, STEP_DEV, STEP_CTL, STEP_SEG };
struct StepCall {
    const void *p, *g, *state[2];                          // state: Adam's m and v; SGD's buf (and nothing)
    long n;
    const void *hyper, *ctl;
    int step;
    float weight_decay, momentum, dampening;
    int decoupled, nesterov;
    const void *cls, *scales;
    int n_classes;
};
inline int step_rule_common(const StepCall& c, StepForm form) {
    if (!c.p || !c.g || c.n <= 0 || !(c.weight_decay >= 0.f)) return MTE_ERR_ARG;
    if (form == STEP_HOST ? c.step < 1 : !c.hyper) return MTE_ERR_ARG;
    if (form == STEP_CTL && !c.ctl) return MTE_ERR_ARG;
    if (form == STEP_SEG && ((c.n & 63) || !c.cls || !c.scales || c.n_classes < 1 || c.n_classes > SEG_MAX_CLASSES)) return MTE_ERR_ARG;
    return MTE_OK;
}
inline int adam_rule(const StepCall& c, StepForm form) {
    if (!c.state[0] || !c.state[1]) return MTE_ERR_ARG;
    return step_rule_common(c, form);
}
// Nesterov needs momentum > 0 and, where the call states the dampening (the host form), dampening = 0, as torch; without momentum `buf` may be null
inline int sgd_rule(const StepCall& c, StepForm form) {
    if (!(c.momentum >= 0.f) || (c.momentum > 0.f && !c.state[0])) return MTE_ERR_ARG;
    if (c.nesterov && (c.momentum <= 0.f || (form == STEP_HOST && c.dampening != 0.f))) return MTE_ERR_ARG;
    return step_rule_common(c, form);
}

// the instance: which decay and which momentum arithmetic the kernel is compiled with.  weight_decay = 0 is the no-decay instance (never `+ 0 * p`).
enum { WD_NONE = 0, WD_L2 = 1, WD_DECOUPLED = 2 };
enum { MOM_NONE = 0, MOM_PLAIN = 1, MOM_NESTEROV = 2 };
inline int wd_kind(float weight_decay, int decoupled) { return weight_decay == 0.f ? WD_NONE : decoupled ? WD_DECOUPLED : WD_L2; }
inline int mom_kind(float momentum, int nesterov) { return momentum == 0.f ? MOM_NONE : nesterov ? MOM_NESTEROV : MOM_PLAIN; }

struct StepPlan {
    int rc = MTE_OK;                                       // otherwise nothing is launched
    int wd = WD_NONE, mom = MOM_NONE;                      // Adam: wd of the three; SGD: mom, and wd as none / L2
    int grid = 0, block = OPT_THREADS;
};
inline StepPlan plan_adam(const StepCall& c, StepForm form) {
    StepPlan pl;
    if ((pl.rc = adam_rule(c, form)) != MTE_OK) return pl;
    pl.wd = wd_kind(c.weight_decay, c.decoupled);
    pl.grid = opt_grid(c.n >> 2);
    return pl;
}
inline StepPlan plan_sgd(const StepCall& c, StepForm form) {
    StepPlan pl;
    if ((pl.rc = sgd_rule(c, form)) != MTE_OK) return pl;
    pl.wd = wd_kind(c.weight_decay, 0);
    pl.mom = mom_kind(c.momentum, c.nesterov);
    pl.grid = opt_grid(c.n >> 2);
    return pl;
}

// the flat-pair launches (EMA, swap, accumulation): rc < 0 an error, launch = false with n = 0
struct PairPlan { int rc = MTE_OK; bool launch = false; int grid = 0, block = OPT_THREADS; };
inline PairPlan plan_pair(const void* a, const void* b, long n, bool extra_ok = true) {
    PairPlan pl;
    const int ok = extra_ok ? flat_pair_check(a, b, n) : MTE_ERR_ARG;
    pl.rc = ok < 0 ? ok : MTE_OK;
    pl.launch = ok > 0;
    pl.grid = opt_grid(n >> 2);
    return pl;
}

// the norm launch
struct NormPlan { int rc = MTE_OK; int grid = 0, block = OPT_THREADS; NormLayout work = {}; };
inline NormPlan plan_norm(const void* g, long n, float max_norm, const void* work, const void* ctl) {
    NormPlan pl;
    if (!g || !work || !ctl || n <= 0 || !(max_norm > 0.f)) { pl.rc = MTE_ERR_ARG; return pl; }
    pl.grid = norm_grid(n >> 2);
    pl.work = norm_layout(n);
    return pl;
}

// the chunk-table launches (mte_tensor_stats, mte_lamb_moments, mte_lamb_apply).  p, g, m, v and work are 16-byte aligned where given, sums 8-byte;
// the flags say which pointers the launch needs.  begin, numel and n, T are needed by all.
enum : unsigned {
    WITH_P = 1, WITH_G = 2, WITH_MV = 4, WITH_HYPER = 8 /* hyper, the tensor table and a weight decay */, WITH_WORK = 16, WITH_TRUST = 32,
    WITH_SUMS = 64 /* and max_trust */, WITH_OUT = 128,
};
struct ChunkCall {
    const void *p, *g, *m, *v, *hyper, *begin, *numel, *table, *work, *trust, *sums, *out;
    long n;
    int T;
    float weight_decay, max_trust;
};
struct ChunkPlan { int rc = MTE_OK; bool has_p = false /* the statistics' WITH_P instance */; long max_chunks = 0; int grid = 0, block = OPT_THREADS; ChunkLayout work = {}; };
inline int chunk_rule(const ChunkCall& c, unsigned with) {
    if (!c.begin || !c.numel || !chunk_sizes_ok(c.n, c.T)) return MTE_ERR_ARG;
    if (((with & WITH_P) && !c.p) || ((with & WITH_G) && !c.g) || ((with & WITH_MV) && (!c.m || !c.v)) || ((with & WITH_WORK) && !c.work)) return MTE_ERR_ARG;
    if ((with & WITH_HYPER) && (!c.hyper || !c.table || !(c.weight_decay >= 0.f))) return MTE_ERR_ARG;
    if (((with & WITH_TRUST) && !c.trust) || ((with & WITH_OUT) && !c.out)) return MTE_ERR_ARG;
    if ((with & WITH_SUMS) && (!c.sums || ((uintptr_t)c.sums & 7) || !(c.max_trust >= 0.f))) return MTE_ERR_ARG;
    if (misaligned16(c.p, c.g, c.m, c.v, c.work) || stat_max_chunks(c.n, c.T) > 0x7fffffffL) return MTE_ERR_ARG;
    return MTE_OK;
}
inline ChunkPlan plan_chunks(const ChunkCall& c, unsigned with, int values) {
    ChunkPlan pl;
    if ((pl.rc = chunk_rule(c, with)) != MTE_OK) return pl;
    pl.has_p = c.p != nullptr;
    pl.max_chunks = stat_max_chunks(c.n, c.T);
    pl.grid = chunk_grid(pl.max_chunks);
    pl.work = chunk_layout(c.n, c.T, values);
    return pl;
}

// ---- the chunk cut: ONE statement of how the tensor table is cut into chunks, so that every kernel that walks it -- and a host enumeration -- gives a chunk
// the same elements and the same global index.  Tensor t is elements [begin_t, begin_t + numel_t) of the flat buffers; it is cut from its start into chunks of
// STAT_CHUNK elements (the last one ragged).  A range that leaves [0, n), an empty one and a misaligned begin count as ONE empty chunk: nothing outside the buffers
// is touched.  Chunk k of tensor t has the global index first[t] + k, first the running sum of the chunk counts (first[T]: all chunks).
MTE_PLAN_HD bool chunk_range_ok(long b, long m, long n) { return b >= 0 && m > 0 && (b & 3) == 0 && b <= n && m <= n - b; }
MTE_PLAN_HD int chunk_count(long b, long m, long n) { return chunk_range_ok(b, m, n) ? (int)((m + STAT_CHUNK - 1) / STAT_CHUNK) : 1; }

// Chunk c of the table: tensor t (the last one with first[t] <= c) of `chunks` chunks, at elements [b + e0, b + e1) of the flat buffers -- nvec whole vectors,
// and in the tensor's last chunk (e1 == m) its m & 3 trailing elements.  An empty chunk has b = m = e0 = e1 = 0.
struct Chunk {
    int t, chunks; long b, m, e0, e1, nvec;
    MTE_PLAN_HD bool has_tail() const { return e1 == m && e1 > e0; }      // the chunk that takes the tensor's m & 3 trailing elements, at b + (m & ~3)
};
MTE_PLAN_HD Chunk chunk_at(long c, const int* first, const long* begin, const long* numel, int T, long n) {
    int lo = 0, hi = T - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= c) lo = mid; else hi = mid - 1;
    }
    Chunk ch;
    ch.t = lo;
    ch.chunks = first[lo + 1] - first[lo];
    const long k = c - first[lo];
    ch.b = begin[lo]; ch.m = numel[lo];
    if (!chunk_range_ok(ch.b, ch.m, n) || k < 0 || k * STAT_CHUNK > ch.m) { ch.b = 0; ch.m = 0; }
    ch.e0 = ch.m ? k * STAT_CHUNK : 0;
    ch.e1 = ch.e0 + STAT_CHUNK < ch.m ? ch.e0 + STAT_CHUNK : ch.m;
    ch.nvec = ch.e1 > ch.e0 ? (ch.e1 - ch.e0) >> 2 : 0;
    return ch;
}
// the host's form of optim.hip's chunk_table (a block scan there): first[0 .. T] <- the running sum; -> all chunks
inline long chunk_table_host(const long* begin, const long* numel, int T, long n, int* first) {
    long run = 0;                                          // (a table that overlaps itself can pass an int: the kernels' sum wraps, this one is cut)
    for (int t = 0; t < T; ++t) { first[t] = (int)run; run += chunk_count(begin[t], numel[t], n); }
    first[T] = (int)run;
    return run;
}

}  // namespace optim_plan
