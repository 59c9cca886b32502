// Optimizer driver of the launch recorder (tests/conv_launch_recorder.py --optim): linked against optim.hip compiled for the host with conv_launch_shim.hpp in
// front.  Reads one case per line from standard input,
//     <entry> <n> <T> <weight_decay> <decoupled> <momentum> <nesterov> <dampening> <step> <n_classes> <max_trust> <max_norm> <flag> <error>
// entry: an entry point of optim.hip without its mte_ prefix.  flag: assign (grad_accumulate), skip_nonfinite (grad_norm_clip), 1 = with p (tensor_stats),
// 1 = with ctl (the forms whose ctl may be null).  error: "-", or what is wrong with the call: null:<arg>, mis:<arg> (the pointer 4 bytes off), eq (the flat
// pair's pointers equal), overlap (the second 16 bytes behind the first).  Every pointer is a fake, 16-byte aligned address that nothing dereferences.  Prints
//     {"case": <the line>, "rc": <return code>, "launches": [...]}            and for a query {"case": <the line>, "q": <its answer>}
#include "launch_driver.hpp"
#include <map>

extern "C" {
int mtei_set_gn(int, int) { return 0; }                                 // (norm_act.hip is not linked)
int mte_ema_update(float* ema, const float* p, long n, float d, float omd, hipStream_t stream);
int mte_ema_update_dev(float* ema, const float* p, long n, const float* scal, const float* ctl, hipStream_t stream);
int mte_flat_swap(float* a, float* b, long n, hipStream_t stream);
int mte_grad_accumulate(float* dst, const float* src, long n, int assign, hipStream_t stream);
long mte_grad_norm_work_bytes(long n);
int mte_grad_norm_clip(const float* g, long n, float gscale, float max_norm, int skip_nonfinite, void* work, float* ctl, hipStream_t stream);
int mte_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, int step,
                   float gscale, hipStream_t stream);
int mte_adamw_step_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                       int decoupled, float gscale, hipStream_t stream);
int mte_sgd_step(float* p, const float* g, float* buf, long n, float lr, float momentum, float dampening, float weight_decay, int nesterov, int step, float gscale,
                 hipStream_t stream);
int mte_sgd_step_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov, float gscale,
                     hipStream_t stream);
int mte_adamw_step_ctl_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                           int decoupled, float gscale, const float* ctl, hipStream_t stream);
int mte_sgd_step_ctl_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov, float gscale,
                         const float* ctl, hipStream_t stream);
int mte_adamw_step_seg_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                           int decoupled, float gscale, const uint8_t* block_class, const float* class_scales, int n_classes, const float* ctl, hipStream_t stream);
int mte_sgd_step_seg_dev(float* p, const float* g, float* buf, long n, const float* hyper, float momentum, float weight_decay, int nesterov, float gscale,
                         const uint8_t* block_class, const float* class_scales, int n_classes, const float* ctl, hipStream_t stream);
long mte_tensor_stats_work_bytes(long n, int T);
int mte_tensor_stats(const float* g, const float* p, long n, const long* seg_begin, const long* seg_numel, int T, void* work, double* out, hipStream_t stream);
long mte_lamb_work_bytes(long n, int T);
int mte_lamb_moments(const float* p, const float* g, float* m, float* v, long n, const float* hyper, float beta1, float beta2, float eps, float weight_decay,
                     float gscale, float max_trust, const long* seg_begin, const long* seg_numel, const float* tensor_table, int T, void* work, float* trust,
                     double* sums, const float* ctl, hipStream_t stream);
int mte_lamb_apply(float* p, const float* m, const float* v, long n, const float* hyper, float eps, float weight_decay, const long* seg_begin, const long* seg_numel,
                   const float* tensor_table, int T, const float* trust, const float* ctl, hipStream_t stream);
}
int g_mte_wgrad_shared = 0;
int g_mte_handoff_fences = 0;                                           // (norm_act.hip is not linked)

static std::map<std::string, uintptr_t> P;                              // the call's pointers by argument name
template <typename T> static T* ptr(const char* name) { return (T*)P[name]; }

static int run_case(const char* line) {
    char entry[32], wd_s[32], mom_s[32], damp_s[32], trust_s[32], norm_s[32], err[32];
    long n;
    int T, decoupled, nesterov, step, n_classes, flag;
    if (sscanf(line, "%31s %ld %d %31s %d %31s %d %31s %d %d %31s %31s %d %31s", entry, &n, &T, wd_s, &decoupled, mom_s, &nesterov, damp_s, &step, &n_classes, trust_s,
               norm_s, &flag, err) != 14) return 2;
    const float wd = strtof(wd_s, nullptr), mom = strtof(mom_s, nullptr), damp = strtof(damp_s, nullptr), max_trust = strtof(trust_s, nullptr),
                max_norm = strtof(norm_s, nullptr);
    const char* names[] = {"p", "g", "m", "v", "buf", "hyper", "ctl", "cls", "scales", "begin", "numel", "table", "work", "trust", "sums", "out", "scal", "b"};
    int k = 0;
    for (const char* name : names) {                                        // slot k is 4 GiB wide
        P[name] = (uintptr_t)(++k) << 32;
        mte_rec::buffers()[P[name]] = name;
    }
    const bool ctl_optional = !strcmp(entry, "ema_update_dev") || strstr(entry, "_seg_dev") || !strncmp(entry, "lamb_", 5);
    if (ctl_optional && !flag) P["ctl"] = 0;
    if (!strcmp(entry, "tensor_stats") && !flag) P["p"] = 0;
    if (!strncmp(err, "null:", 5)) { if (!P.count(err + 5)) return 2; P[err + 5] = 0; }
    else if (!strncmp(err, "mis:", 4)) { if (!P.count(err + 4)) return 2; P[err + 4] += 4; }
    else if (!strcmp(err, "eq")) P["b"] = P["p"];
    else if (!strcmp(err, "overlap")) P["b"] = P["p"] + 16;
    else if (strcmp(err, "-")) return 2;
    float* const p = ptr<float>("p"); float* const g = ptr<float>("g"); float* const m = ptr<float>("m"); float* const v = ptr<float>("v");
    float* const buf = ptr<float>("buf"); float* const b = ptr<float>("b");
    const float* const hyper = ptr<float>("hyper"); const float* const ctl = ptr<float>("ctl");
    const long* const begin = ptr<long>("begin"); const long* const numel = ptr<long>("numel");
    const float lr = 1e-3f, b1 = 0.9f, b2 = 0.999f, eps = 1e-8f, gscale = 0.5f;
    long q = 0;
    int rc = 0;
    bool query = true;
    if (!strcmp(entry, "grad_norm_work_bytes")) q = mte_grad_norm_work_bytes(n);
    else if (!strcmp(entry, "tensor_stats_work_bytes")) q = mte_tensor_stats_work_bytes(n, T);
    else if (!strcmp(entry, "lamb_work_bytes")) q = mte_lamb_work_bytes(n, T);
    else query = false;
    if (query) {
        if (!mte_rec::log().empty()) return 2;                              // (a query launches nothing)
        printf("{\"case\":\"%s\",\"q\":%ld}\n", line, q);
        return 0;
    }
    if (!strcmp(entry, "ema_update")) rc = mte_ema_update(p, b, n, 0.999f, 0.001f, nullptr);
    else if (!strcmp(entry, "ema_update_dev")) rc = mte_ema_update_dev(p, b, n, ptr<float>("scal"), ctl, nullptr);
    else if (!strcmp(entry, "flat_swap")) rc = mte_flat_swap(p, b, n, nullptr);
    else if (!strcmp(entry, "grad_accumulate")) rc = mte_grad_accumulate(p, b, n, flag, nullptr);
    else if (!strcmp(entry, "grad_norm_clip")) rc = mte_grad_norm_clip(g, n, gscale, max_norm, flag, ptr<void>("work"), ptr<float>("ctl"), nullptr);
    else if (!strcmp(entry, "adamw_step")) rc = mte_adamw_step(p, g, m, v, n, lr, b1, b2, eps, wd, decoupled, step, gscale, nullptr);
    else if (!strcmp(entry, "adamw_step_dev")) rc = mte_adamw_step_dev(p, g, m, v, n, hyper, b1, b2, eps, wd, decoupled, gscale, nullptr);
    else if (!strcmp(entry, "adamw_step_ctl_dev")) rc = mte_adamw_step_ctl_dev(p, g, m, v, n, hyper, b1, b2, eps, wd, decoupled, gscale, ctl, nullptr);
    else if (!strcmp(entry, "adamw_step_seg_dev"))
        rc = mte_adamw_step_seg_dev(p, g, m, v, n, hyper, b1, b2, eps, wd, decoupled, gscale, ptr<uint8_t>("cls"), ptr<float>("scales"), n_classes, ctl, nullptr);
    else if (!strcmp(entry, "sgd_step")) rc = mte_sgd_step(p, g, buf, n, lr, mom, damp, wd, nesterov, step, gscale, nullptr);
    else if (!strcmp(entry, "sgd_step_dev")) rc = mte_sgd_step_dev(p, g, buf, n, hyper, mom, wd, nesterov, gscale, nullptr);
    else if (!strcmp(entry, "sgd_step_ctl_dev")) rc = mte_sgd_step_ctl_dev(p, g, buf, n, hyper, mom, wd, nesterov, gscale, ctl, nullptr);
    else if (!strcmp(entry, "sgd_step_seg_dev"))
        rc = mte_sgd_step_seg_dev(p, g, buf, n, hyper, mom, wd, nesterov, gscale, ptr<uint8_t>("cls"), ptr<float>("scales"), n_classes, ctl, nullptr);
    else if (!strcmp(entry, "tensor_stats")) rc = mte_tensor_stats(g, p, n, begin, numel, T, ptr<void>("work"), ptr<double>("out"), nullptr);
    else if (!strcmp(entry, "lamb_moments"))
        rc = mte_lamb_moments(p, g, m, v, n, hyper, b1, b2, eps, wd, gscale, max_trust, begin, numel, ptr<float>("table"), T, ptr<void>("work"), ptr<float>("trust"),
                              ptr<double>("sums"), ctl, nullptr);
    else if (!strcmp(entry, "lamb_apply")) rc = mte_lamb_apply(p, m, v, n, hyper, eps, wd, begin, numel, ptr<float>("table"), T, ptr<float>("trust"), ctl, nullptr);
    else return 2;
    printf("{\"case\":\"%s\",\"rc\":%d,\"launches\":[%s]}\n", line, rc, mte_rec::log().c_str());
    return 0;
}

int main() { return run_cases(run_case); }
