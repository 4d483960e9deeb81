// qdec_kernels.h -- building the kernel families' tables (KernelEntry,
// qdec_internal.h) and launching their entries.  Included by the units that
// define kernels (qdec_bp.hip, qdec_bp_block.hip).
#pragma once
#include "qdec_device.h"
#include "qdec_internal.h"

namespace qdec {

// rocprofv3's spelling of a kernel instantiation: base<arg, arg, ...>
inline std::string targ(bool b) { return b ? "true" : "false"; }
inline std::string targ(int v) { return std::to_string(v); }
inline std::string targ(const char* s) { return s; }
template <typename T>
inline const char* tname() { return sizeof(T) == 8 ? "double" : "float"; }
template <typename... A>
inline std::string kernel_name(const char* base, A... args) {
    std::string s = std::string(base) + "<";
    bool first = true;
    ((s += (first ? std::string() : std::string(", ")) + targ(args), first = false), ...);
    return s + ">";
}

// An entry from one template argument list: QDEC_INST(block, kernel, args...)
// takes the address of kernel<args...> and spells its name and its argument
// values from the same list (every argument explicit; a leading type is the
// precision); block = threads per workgroup.
template <auto... V>
inline KernelEntry make_entry(const void* fn, const char* base, int block) {
    KernelEntry e;
    e.fn = fn;
    e.block = block;
    e.name = kernel_name(base, V...);
    for (int v : {(int)V...}) e.t[e.nt++] = v;
    return e;
}
template <typename T, auto... V>
inline KernelEntry make_entry(const void* fn, const char* base, int block) {
    KernelEntry e;
    e.fn = fn;
    e.block = block;
    e.name = kernel_name(base, tname<T>(), V...);
    for (int v : {sizeof(T) == 4 ? 1 : 0, (int)V...}) e.t[e.nt++] = v;
    return e;
}
#define QDEC_INST(block, kernel, ...) \
    make_entry<__VA_ARGS__>(reinterpret_cast<const void*>(&kernel<__VA_ARGS__>), "qdec::" #kernel, block)

// A family's kernel parameters.  launch_entry converts its arguments to exactly
// these types before their addresses go to hipLaunchKernel.
template <typename... P>
struct KernelSig {};
template <typename P>
struct AsGiven {  // keeps launch_entry's arguments out of template deduction
    using type = P;
};
using WaveSig = KernelSig<DevGraph, DecodeArgs>;  // every wave-graph family

template <typename... P>
inline int launch_entry(KernelSig<P...>, const KernelEntry& e, long long grid, size_t lds, hipStream_t stream,
                        typename AsGiven<P>::type... args) {
    void* argv[] = {&args...};
    (void)hipLaunchKernel(e.fn, dim3((unsigned)grid), dim3((unsigned)e.block), argv, lds, stream);
    return (int)hipGetLastError();
}
// as launch_resident (qdec_device.h): as many workgroups as stay resident
template <typename... P>
inline int launch_entry_resident(KernelSig<P...> sig, const KernelEntry& e, size_t lds, int num_cus, long long work,
                                 hipStream_t stream, GridRule rule, typename AsGiven<P>::type... args) {
    long long grid = 0;
    const hipError_t er = resident_grid(e.fn, e.block, lds, num_cus, work, &grid, rule);
    if (er != hipSuccess) return (int)er;
    if (grid <= 0) return 0;
    return launch_entry(sig, e, grid, lds, stream, args...);
}

}  // namespace qdec
