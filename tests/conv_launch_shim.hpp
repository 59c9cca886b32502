// Launch recorder for the host code that chooses kernels (tests/conv_launch_recorder.py): force-included in front of conv_igemm.hip / conv_igemm8.hip /
// conv_wgrad9.hip / norm_act.hip / pack3d.hip / conv_patch.hip / optim.hip when they are compiled for the host alone.  hipLaunchKernelGGL, hipFuncSetAttribute, hipMemsetAsync, hipGetLastError,
// hipGetDevice and hipDeviceGetAttribute (answered with the CU count the driver sets) are redefined, so no
// call reaches the HIP runtime: every launch is appended to a text record instead -- the kernel with its template arguments, grid, block, dynamic LDS, the
// large-LDS grant the kernel holds at that moment, and for a ConvArgs, GnArgs, P3Args, P3LArgs, PatchArgs, PatchWgradArgs, WgradArgs or Wgrad9Args argument (and the optimizer family's NormArgs, StatArgs, LambArgs, SegArgs and step scalars) the fields the host chose.  A clear (hipMemsetAsync, or the fill
// kernels of mte_memset_async in common.hpp) is a line of its own: which buffer and how many bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>
#include <map>
#include <typeinfo>
#include <string>
#include <type_traits>

struct ConvArgs;

namespace mte_rec {
inline std::string& log() { static std::string s; return s; }
inline std::map<const void*, int>& granted() { static std::map<const void*, int> m; return m; }
// the driver names the buffers it passes (base address -> name); a cleared range is printed as name+offset
inline std::map<uintptr_t, std::string>& buffers() { static std::map<uintptr_t, std::string> m; return m; }

// typeid(Tag<K>) demangles to "mte_rec::Tag<&(void (anonymous namespace)::conv_igemm_kernel<unsigned short, 2, 2, 2, 2, 2, 4, 1, 0>(ConvArgs))>"; kept of it:
// "conv_igemm_kernel<unsigned short, 2, 2, 2, 2, 2, 4, 1, 0>"  (__PRETTY_FUNCTION__ of a function templated on the address names the kernel without its arguments)
template <auto K> struct Tag {};
template <auto K> std::string kernel_name() {
    int status = 0;
    char* d = abi::__cxa_demangle(typeid(Tag<K>).name(), nullptr, nullptr, &status);
    std::string s = d ? d : typeid(Tag<K>).name();
    free(d);
    for (size_t at; (at = s.find("(anonymous namespace)::")) != std::string::npos;) s.erase(at, 23);
    size_t from = s.find("&(");
    if (from == std::string::npos) {                                        // a kernel that is no template: "mte_rec::Tag<&pack3d_fwd_lds_kernel>"
        from = s.find('&');
        if (from != std::string::npos) s = s.substr(from + 1, s.rfind('>') - from - 1);
    } else {
        from += 2;
        if (s.compare(from, 5, "void ") == 0) from += 5;
        s = s.substr(from, s.find('(', from) - from);
    }
    for (size_t at; (at = s.find("unsigned short")) != std::string::npos;) s.replace(at, 14, "bf16");
    return s;
}

inline std::string& plain() { static std::string s; return s; }      // the plain (non-struct) arguments of the launch being recorded
inline void field(const char* name, long v, long dflt) { if (v != dflt) log() += std::string(",\"") + name + "\":" + std::to_string(v); }

template <typename A, typename = void> struct is_gn_args : std::false_type {};
template <typename A> struct is_gn_args<A, std::void_t<decltype(A::cps_shift), decltype(A::blocks_per_sample), decltype(A::ppl)>> : std::true_type {};
template <typename A, typename = void> struct is_p3_args : std::false_type {};       // P3Args: the conv3d gather kernels
template <typename A> struct is_p3_args<A, std::void_t<decltype(A::dw3), decltype(A::db3), decltype(A::total)>> : std::true_type {};
template <typename A, typename = void> struct is_p3l_args : std::false_type {};      // P3LArgs: every other conv3d kernel
template <typename A> struct is_p3l_args<A, std::void_t<decltype(A::dwb), decltype(A::tiles_h), decltype(A::tshift)>> : std::true_type {};
template <typename A, typename = void> struct is_patch_args : std::false_type {};    // PatchArgs: the LDS-patch forward kernels
template <typename A> struct is_patch_args<A, std::void_t<decltype(A::r1_inv), decltype(A::x2), decltype(A::gn_rec)>> : std::true_type {};
template <typename A, typename = void> struct is_patch_wgrad_args : std::false_type {};      // PatchWgradArgs
template <typename A> struct is_patch_wgrad_args<A, std::void_t<decltype(A::lddy), decltype(A::groups), decltype(A::part_stride)>> : std::true_type {};
template <typename A, typename = void> struct is_wgrad_args : std::false_type {};          // WgradArgs: the LDS-DMA and register-staged weight gradients
template <typename A> struct is_wgrad_args<A, std::void_t<decltype(A::blocks_per_split), decltype(A::tiles_n), decltype(A::part_stride)>> : std::true_type {};
template <typename A, typename = void> struct is_wgrad9_args : std::false_type {};         // Wgrad9Args: the nine-tap weight gradient
template <typename A> struct is_wgrad9_args<A, std::void_t<decltype(A::units_per_split), decltype(A::base), decltype(A::part_stride)>> : std::true_type {};
// the optimizer family (optim.hip): NormArgs, StatArgs, LambArgs, SegArgs, and the by-value step scalars with or without their ctl pointer
template <typename A, typename = void> struct is_norm_args : std::false_type {};
template <typename A> struct is_norm_args<A, std::void_t<decltype(A::max_norm), decltype(A::skip_nonfinite), decltype(A::records)>> : std::true_type {};
template <typename A, typename = void> struct is_stat_args : std::false_type {};
template <typename A> struct is_stat_args<A, std::void_t<decltype(A::tickets), decltype(A::max_chunks), decltype(A::out)>> : std::true_type {};
template <typename A, typename = void> struct is_lamb_args : std::false_type {};
template <typename A> struct is_lamb_args<A, std::void_t<decltype(A::max_trust), decltype(A::trust), decltype(A::sums)>> : std::true_type {};
template <typename A, typename = void> struct is_seg_args : std::false_type {};
template <typename A> struct is_seg_args<A, std::void_t<decltype(A::cls), decltype(A::scales), decltype(A::n_classes)>> : std::true_type {};
template <typename A, typename = void> struct is_adam_scalars : std::false_type {};
template <typename A> struct is_adam_scalars<A, std::void_t<decltype(A::bc1), decltype(A::bc2s), decltype(A::gscale)>> : std::true_type {};
template <typename A, typename = void> struct is_sgd_scalars : std::false_type {};
template <typename A> struct is_sgd_scalars<A, std::void_t<decltype(A::mu_eff), decltype(A::omd_eff), decltype(A::gscale)>> : std::true_type {};
template <typename A, typename = void> struct has_ctl : std::false_type {};
template <typename A> struct has_ctl<A, std::void_t<decltype(A::ctl)>> : std::true_type {};
// compute units the device query answers (the weight-gradient driver sets it per case): no case depends on whether the machine has a GPU
inline int& cus() { static int n = 256; return n; }
inline hipError_t get_device(int* dev) { *dev = 0; return hipSuccess; }
inline hipError_t device_attribute(int* v, hipDeviceAttribute_t what, int) {       // the CU count and nothing else
    if (what != hipDeviceAttributeMultiprocessorCount) return hipErrorInvalidValue;
    *v = cus();
    return hipSuccess;
}

// a pointer as the driver's buffer name (+ offset), "0" when null
inline std::string ptr_name(const void* p) {
    if (!p) return "0";
    auto it = buffers().upper_bound((uintptr_t)p);
    if (it == buffers().begin()) return std::to_string((uintptr_t)p);
    --it;
    return (uintptr_t)p == it->first ? it->second : it->second + "+" + std::to_string((uintptr_t)p - it->first);
}
inline void ptrs(const char* name, std::initializer_list<const void*> ps) {
    std::string s;
    for (const void* p : ps) s += (s.empty() ? "" : " ") + ptr_name(p);
    log() += std::string(",\"") + name + "\":\"" + s + "\"";
}
inline void floats(const char* name, std::initializer_list<float> vs) {      // %.9g: every float32 has its own text
    std::string s;
    char b[32];
    for (float v : vs) { snprintf(b, sizeof b, "%.9g", (double)v); s += (s.empty() ? "" : " ") + std::string(b); }
    log() += std::string(",\"") + name + "\":\"" + s + "\"";
}
template <typename A> void adam_scalars(const A& s) { floats("adam", {s.lr, s.bc1, s.bc2s, s.b1, s.b2, s.eps, s.gscale, s.wd}); }

// (to keep the table small a field is left out where it has its usual value: grid y, z = 1, granted = 0, splits = 1, the other fields 0, a pointer null)
template <typename A> void arg_fields(const A& a) {
    if constexpr (std::is_same_v<A, ConvArgs>) {
        field("splits", a.splits, 1); field("kslice", a.kslice, 0); field("solo", a.solo, 0); field("accum", a.accum, 0); field("unshuffle_c", a.unshuffle_c, 0);
    } else if constexpr (is_gn_args<A>::value) {
        field("blocks_per_sample", a.blocks_per_sample, 0); field("reverse", a.reverse, 0); field("cps_shift", a.cps_shift, 0);
        field("ppl", a.ppl, 0); field("b0", a.b0, 0); field("nb", a.nb, 0);
        const std::string with = std::string(a.y2 ? " y2" : "") + (a.scale2 ? " scale2" : "") + (a.d2 ? " d2" : "") + (a.dbias ? " dbias" : "");
        if (!with.empty()) log() += ",\"with\":\"" + with.substr(1) + "\"";      // the optional pointers that are not null
    } else if constexpr (is_p3_args<A>::value) {
        field("total", a.total, 0); field("ldx", a.ldx, 0); field("ldo", a.ldo, 0); field("lddst", a.lddst, 0);
        const std::string with = std::string(a.x ? " x" : "") + (a.o ? " o" : "") + (a.dst ? " dst" : "") + (a.w3 ? " w3" : "") + (a.b3 ? " b3" : "") + (a.dw3 ? " dw3" : "") + (a.db3 ? " db3" : "");
        if (!with.empty()) log() += ",\"with\":\"" + with.substr(1) + "\"";
    } else if constexpr (is_p3l_args<A>::value) {
        field("TH", a.TH, 0); field("TW", a.TW, 0); field("tiles_h", a.tiles_h, 0); field("tiles_w", a.tiles_w, 0); field("ntiles", a.ntiles, 0);
        field("dshift", a.dshift, 0); field("tshift", a.tshift, 0); field("ldx", a.ldx, 0); field("ldo", a.ldo, 0); field("lddst", a.lddst, 0);
        const std::string with = std::string(a.x ? " x" : "") + (a.o ? " o" : "") + (a.dst ? " dst" : "") + (a.w3 ? " w3" : "") + (a.b3 ? " b3" : "") + (a.dwb ? " dwb" : "");
        if (!with.empty()) log() += ",\"with\":\"" + with.substr(1) + "\"";
    } else if constexpr (is_patch_args<A>::value) {
        field("accum", a.accum, 0); field("C2", a.C2, 0); field("ldx", a.ldx, 0);
        const std::string with = std::string(a.bias ? " bias" : "") + (a.r1_inv ? " r1_inv" : "") + (a.x2 ? " x2" : "") + (a.gn_rec ? " gn_rec" : "");
        if (!with.empty()) log() += ",\"with\":\"" + with.substr(1) + "\"";
    } else if constexpr (is_patch_wgrad_args<A>::value) {
        field("groups", a.groups, 0); field("part_stride", a.part_stride, 0);
    } else if constexpr (is_wgrad_args<A>::value) {
        field("tiles_n", a.tiles_n, 0); field("tiles_c", a.tiles_c, 0); field("splits", a.splits, 1); field("blocks_per_split", a.blocks_per_split, 0);
        field("part_stride", a.part_stride, 0);
    } else if constexpr (is_wgrad9_args<A>::value) {
        field("tiles_c", a.tiles_c, 0); field("base", a.base, 0); field("units", a.units, 0); field("units_per_split", a.units_per_split, 0);
        field("part_stride", a.part_stride, 0);
    } else if constexpr (is_norm_args<A>::value) {
        field("n", a.n, 0); floats("norm", {a.gscale, a.max_norm}); field("skip_nonfinite", a.skip_nonfinite, 0); field("fences", a.fences, 0);
        ptrs("ptrs", {a.g, a.sum, a.ticket, a.records, a.ctl});
    } else if constexpr (is_stat_args<A>::value) {
        field("n", a.n, 0); field("T", a.T, 0); field("fences", a.fences, 0); field("max_chunks", a.max_chunks, 0);
        ptrs("ptrs", {a.g, a.p, a.begin, a.numel, a.tickets, a.records, a.out});
    } else if constexpr (is_lamb_args<A>::value) {
        field("n", a.n, 0); field("T", a.T, 0); field("fences", a.fences, 0); field("max_chunks", a.max_chunks, 0);
        adam_scalars(a.s); floats("max_trust", {a.max_trust});
        ptrs("ptrs", {a.p, a.g, a.m, a.v, a.hyper, a.ctl, a.begin, a.numel, a.table, a.tickets, a.records, a.trust, a.sums});
    } else if constexpr (is_seg_args<A>::value) {
        field("n_classes", a.n_classes, 0); ptrs("seg", {a.cls, a.scales, a.ctl});
    } else if constexpr (is_adam_scalars<A>::value) {
        adam_scalars(a);
        if constexpr (has_ctl<A>::value) ptrs("ctl", {a.ctl});
    } else if constexpr (is_sgd_scalars<A>::value) {
        floats("sgd", {a.lr, a.mu_eff, a.omd_eff, a.mu, a.gscale, a.wd});
        if constexpr (has_ctl<A>::value) ptrs("ctl", {a.ctl});
    }
#ifdef MTE_REC_PLAIN_ARGS                                                   // (the optimizer recorder) the kernels' plain arguments too, in order: "a":"p g m v 1024 hyper"
    else if constexpr (std::is_pointer_v<A>) plain() += (plain().empty() ? "" : " ") + ptr_name((const void*)a);
    else if constexpr (std::is_integral_v<A>) plain() += (plain().empty() ? "" : " ") + std::to_string((long)a);
    else if constexpr (std::is_floating_point_v<A>) { char b[32]; snprintf(b, sizeof b, "%.9g", (double)a); plain() += (plain().empty() ? "" : " ") + std::string(b); }
#endif
}

inline hipError_t clear(const void* p, size_t bytes) {
    auto it = buffers().upper_bound((uintptr_t)p);
    std::string name = std::to_string((uintptr_t)p);
    if (it != buffers().begin()) { --it; name = it->second; if ((uintptr_t)p != it->first) name += "+" + std::to_string((uintptr_t)p - it->first); }
    log() += std::string(log().empty() ? "" : ",") + "{\"clear\":\"" + name + "\",\"bytes\":" + std::to_string(bytes) + "}";
    return hipSuccess;
}
// the two fill kernels of mte_memset_async: (p, word, 16-byte chunks, tail, tail words) and (p, byte, bytes)
template <typename... A> bool fill(const A&...) { return false; }
template <typename P> bool fill(P* const& p, const unsigned&, const size_t& n16, unsigned* const&, const int& ntail) { clear(p, n16 * 16 + (size_t)ntail * 4); return true; }
inline bool fill(unsigned char* const& p, const unsigned char&, const size_t& n) { clear(p, n); return true; }

template <auto K, typename... A> void launch(dim3 g, dim3 b, size_t lds, hipStream_t, const A&... args) {
    const std::string name = kernel_name<K>();
    if (name.compare(0, 8, "mte_fill") == 0 && fill(args...)) return;
    const auto it = granted().find((const void*)K);
    log() += std::string(log().empty() ? "" : ",") + "{\"k\":\"" + name + "\",\"grid\":" + std::to_string(g.x);
    field("grid_y", g.y, 1); field("grid_z", g.z, 1);
    field("block", b.x, -1); field("block_y", b.y, 1); field("block_z", b.z, 1);
    field("lds", (long)lds, -1); field("granted", it == granted().end() ? 0 : it->second, 0);
    plain().clear();
    (arg_fields(args), ...);
    if (!plain().empty()) log() += ",\"a\":\"" + plain() + "\"";
    log() += "}";
}
inline hipError_t set_attribute(const void* k, hipFuncAttribute, int v) { granted()[k] = v; return hipSuccess; }
}  // namespace mte_rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, ...) mte_rec::launch<kernel>(__VA_ARGS__)
#define hipFuncSetAttribute(...) mte_rec::set_attribute(__VA_ARGS__)
#define hipMemsetAsync(p, value, bytes, stream) mte_rec::clear(p, bytes)
#define hipGetLastError() hipSuccess
#define hipGetDevice(dev) mte_rec::get_device(dev)
#define hipDeviceGetAttribute(...) mte_rec::device_attribute(__VA_ARGS__)
