// Launch recorder for the implicit-GEMM host code (tests/conv_launch_recorder.py): force-included in front of conv_igemm.hip / conv_igemm8.hip when they are
// compiled for the host alone.  hipLaunchKernelGGL, hipFuncSetAttribute and hipGetLastError are redefined, so no call reaches the HIP runtime: every launch is
// appended to a text record instead -- the kernel with its template arguments, grid, block, dynamic LDS, the large-LDS grant the kernel holds at that moment, and
// for a ConvArgs argument the fields the host chose.
#pragma once
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <stdlib.h>
#include <map>
#include <typeinfo>
#include <string>
#include <type_traits>

struct ConvArgs;

namespace mte_rec {
inline std::string& log() { static std::string s; return s; }
inline std::map<const void*, int>& granted() { static std::map<const void*, int> m; return m; }

// typeid(Tag<K>) demangles to "mte_rec::Tag<&(void (anonymous namespace)::conv_igemm_kernel<unsigned short, 2, 2, 2, 2, 2, 4, 1, 0>(ConvArgs))>"; kept of it:
// "conv_igemm_kernel<unsigned short, 2, 2, 2, 2, 2, 4, 1, 0>"  (__PRETTY_FUNCTION__ of a function templated on the address names the kernel without its arguments)
template <auto K> struct Tag {};
template <auto K> std::string kernel_name() {
    int status = 0;
    char* d = abi::__cxa_demangle(typeid(Tag<K>).name(), nullptr, nullptr, &status);
    std::string s = d ? d : typeid(Tag<K>).name();
    free(d);
    for (size_t at; (at = s.find("(anonymous namespace)::")) != std::string::npos;) s.erase(at, 23);
    const size_t at = s.find("&(void "), from = at == std::string::npos ? 0 : at + 7;
    s = s.substr(from, s.find('(', from) - from);
    for (size_t at; (at = s.find("unsigned short")) != std::string::npos;) s.replace(at, 14, "bf16");
    return s;
}

inline void field(const char* name, long v, long dflt) { if (v != dflt) log() += std::string(",\"") + name + "\":" + std::to_string(v); }

// (to keep the table small a field is left out where it has its usual value: grid y, z = 1, granted = 0, splits = 1, the other ConvArgs fields 0)
template <typename A> void conv_fields(const A& a) {
    if constexpr (std::is_same_v<A, ConvArgs>) {
        field("splits", a.splits, 1); field("kslice", a.kslice, 0); field("solo", a.solo, 0); field("accum", a.accum, 0); field("unshuffle_c", a.unshuffle_c, 0);
    }
}

template <auto K, typename... A> void launch(dim3 g, dim3 b, size_t lds, hipStream_t, const A&... args) {
    const auto it = granted().find((const void*)K);
    log() += std::string(log().empty() ? "" : ",") + "{\"k\":\"" + kernel_name<K>() + "\",\"grid\":" + std::to_string(g.x);
    field("grid_y", g.y, 1); field("grid_z", g.z, 1);
    field("block", b.x, -1); field("block_y", b.y, 1); field("block_z", b.z, 1);
    field("lds", (long)lds, -1); field("granted", it == granted().end() ? 0 : it->second, 0);
    (conv_fields(args), ...);
    log() += "}";
}
inline hipError_t set_attribute(const void* k, hipFuncAttribute, int v) { granted()[k] = v; return hipSuccess; }
}  // namespace mte_rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, ...) mte_rec::launch<kernel>(__VA_ARGS__)
#define hipFuncSetAttribute(...) mte_rec::set_attribute(__VA_ARGS__)
#define hipGetLastError() hipSuccess
