// qdec_kernels.h -- building the kernel families' tables (KernelEntry,
// qdec_internal.h) and launching their entries.  Host code: included by the
// units that define a kernel family (each exports one table builder, declared
// here) and by the launch units that call the builders and launch the entries
// (qdec_launch_wave.hip, qdec_launch_block.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "qdec_internal.h"

namespace qdec {

// ---------------------------------------------------------------- table builders
// Each appends every instantiation its unit builds.  Wave graphs: every shape of
// QDEC_WAVE_SHAPES has every family; bp_wave_kernel is built for product-sum
// only (min-sum has its own kernels).
// qdec_bp.hip
void add_bp_wave_kernels(KernelTable& t);
void add_ssf_wave_kernels(KernelTable& scan, KernelTable& lut);  // ssf_wave_kernel, ssf_lut_kernel
// qdec_ms_triage.hip
void add_triage_kernels(KernelTable& t);
// bp_ms_wave_kernel and bp_ms_cmp_kernel, in two units by wave shape
// (qdec_ms_rv4.hip: four variable rounds; qdec_ms_rvx.hip: the other shapes)
constexpr bool ms_shape_in_rv4(int rv) { return rv == 4; }
void add_ms_kernels_rv4(KernelTable& wave, KernelTable& cmp);
void add_ms_kernels_rvx(KernelTable& wave, KernelTable& cmp);
// Workgroup graphs.
void add_block_kernels(KernelTable& block, KernelTable& ssf);  // qdec_bp_block.hip: bp_block_kernel, the SSF kernels
void add_group_kernels(KernelTable& t);                        // qdec_bp_group.hip
void add_ms_lds_kernels(KernelTable& t);                       // qdec_ms_lds.hip
void add_ms_lds64_kernels(KernelTable& t);                     // qdec_ms_lds64.hip
// The LDS-resident kernels' BP stage, launched by their units (init kernels first)
int launch_ms_lds(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus, hipStream_t stream,
                  float* img, size_t img_bytes);
int launch_ms_lds64(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus, hipStream_t stream,
                    unsigned long long* img, size_t img_bytes);

// The rules that restrict the min-sum wave families (their builders build by
// them, the plan picks by them).
// D3R = 2 (two leading variable rounds of degree <= 3): only on shape (2, 4, 7),
// the n = 225 HGP code with its 144 degree-3 columns
constexpr bool wave_has_d3r2(int rc, int rv, int drc) { return rc == 2 && rv == 4 && drc == 7; }
// OCC = 3 (three waves per SIMD): only for double with D3R = 2, and for the
// one-pass kernel only with LEAN (the 168-VGPR build)
constexpr bool wave_has_occ3(int precision, int d3r) { return precision == 0 && d3r == 2; }

#ifdef QDEC_STAMPS
// the units' phase-timer readers (QDEC_STAMPS_READER, qdec_device.h)
int read_stamps_ms_rv4(unsigned long long* out, int reset);
int read_stamps_ms_rvx(unsigned long long* out, int reset);
int read_stamps_bp(unsigned long long* out, int reset);
int read_stamps_ms_lds64(unsigned long long* out, int reset);
#endif

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

// ---------------------------------------------------------------- resident grids
// Every persistent kernel is launched with as many workgroups as stay resident:
// raise the dynamic-LDS limit when the request needs it, ask the occupancy,
// apply the launcher's cap per CU, clamp to the work items.  *grid <= 0: nothing
// to launch.
struct GridRule {
    int cap_per_cu = 0;  // > 0: at most this many workgroups per CU
    // one-wave blocks: a multiple of 4 per CU puts the same number of waves on
    // every SIMD (11 f64 waves would sit 3/3/3/2 and run slower than 8)
    bool whole_simds = false;
};
template <typename K>
inline hipError_t resident_grid(K kern, int block, size_t lds, int num_cus, long long work, long long* grid,
                                GridRule rule = {}) {
    if (lds > 64 * 1024) {
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
    }
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, block, lds);
    if (e != hipSuccess) return e;
    if (per_cu <= 0) return hipErrorInvalidConfiguration;
    if (rule.cap_per_cu > 0 && per_cu > rule.cap_per_cu) per_cu = rule.cap_per_cu;
    if (rule.whole_simds && block == 64 && per_cu > 4) per_cu &= ~3;
    *grid = std::min((long long)num_cus * per_cu, work);
    return hipSuccess;
}
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
