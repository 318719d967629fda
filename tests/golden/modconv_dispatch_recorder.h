// modconv_dispatch_recorder.h -- force-included (-include) in front of csrc/sg3_modconv.hip and csrc/sg3_modconv_f23.hip to
// record what their host side WOULD launch, without a GPU: the launch macro, the dynamic-LDS attribute call and the device
// queries are replaced after <hip/hip_runtime.h> has declared the real ones.  Used once per change of the dispatch to regenerate
// tests/golden/modconv_dispatch.json (see make_modconv_dispatch.py); never part of the product library.  csrc/sg3_flrelu_host.hip
// (the host side of filtered_lrelu; the kernel file, csrc/sg3_filtered_lrelu.hip, is linked to it as it stands) is recorded the same
// way for tests/golden/flrelu_dispatch.json (make_flrelu_dispatch.py, flrelu_dispatch_recorder.cpp), and
// csrc/sg3_conv2d.hip, sg3_conv2d_dgrad.hip and sg3_conv2d_wgrad_sum.hip for tests/golden/conv2d_dispatch.json
// (make_conv2d_dispatch.py, conv2d_dispatch_recorder.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>

namespace rec {

inline std::string& log() { static std::string s; return s; }
inline int& pending_attr() { static int v = 0; return v; }

// demangled name of a kernel's host stub, template arguments included (link with -rdynamic, default visibility)
inline std::string kernel_name(const void* f) {
    Dl_info info;
    if (!dladdr(f, &info) || !info.dli_sname) return "?";
    std::string m = info.dli_sname;
    for (size_t i; (i = m.find("DF16_")) != std::string::npos;) m.replace(i, 5, "Dh");      // _Float16 as `half`: older demanglers stop at DF16_
    int st = 0;
    char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &st);
    std::string s = d ? d : m;
    free(d);
    return s;
}

template <class P, class = void> struct has_out_pitch : std::false_type {};
template <class P> struct has_out_pitch<P, decltype((void)std::declval<const P&>().outPitch)> : std::true_type {};

// tile geometry of the parameter block a convolution kernel takes (ConvParams / F23Params with a row pitch; PlainConvParams /
// DgradParams of the encoder convolutions with the block count); other first arguments have none
template <class P> auto geometry(const P& p, int) -> decltype((void)p.xTiles, std::string()) {
    char b[200];
    if constexpr (has_out_pitch<P>::value)
        snprintf(b, sizeof b, ",\"nch\":%d,\"xTiles\":%d,\"yTiles\":%d,\"mTiles\":%d,\"outPitch\":%d", p.nch, p.xTiles, p.yTiles, p.mTiles, p.outPitch);
    else
        snprintf(b, sizeof b, ",\"nch\":%d,\"xTiles\":%d,\"yTiles\":%d,\"mTiles\":%d,\"totalBlocks\":%d", p.nch, p.xTiles, p.yTiles, p.mTiles, p.totalBlocks);
    return b;
}
// K decomposition of the parameter block the batch-summed weight gradient takes (WgradSumParams)
template <class P> auto geometry(const P& p, int) -> decltype((void)p.chunksPerSplit, std::string()) {
    char b[200];
    snprintf(b, sizeof b, ",\"OH\":%d,\"OW\":%d,\"xSegs\":%d,\"nChunks\":%d,\"chunksPerSplit\":%d,\"oTiles\":%d,\"iTiles\":%d",
             p.OH, p.OW, p.xSegs, p.nChunks, p.chunksPerSplit, p.oTiles, p.iTiles);
    return b;
}
// work decomposition of the parameter block the filtered_lrelu streaming kernel takes (StreamParams)
template <class P> auto geometry(const P& p, int) -> decltype((void)p.wideBlocks, std::string()) {
    char b[200];
    snprintf(b, sizeof b, ",\"nStrips\":%d,\"TW\":%d,\"ox0Base\":%d,\"wideBlocks\":%d,\"nChunks\":%d,\"CH\":%d,\"totalBlocks\":%d,\"fastAct\":%d",
             p.nStrips, p.TW, p.ox0Base, p.wideBlocks, p.nChunks, p.CH, p.totalBlocks, p.fastAct);
    return b;
}
template <class P> std::string geometry(const P&, long) { return ""; }

template <class K, class A0, class... R>
inline void launch(K kern, dim3 g, dim3 b, size_t lds, const A0& a0, const R&...) {
    char buf[256];
    snprintf(buf, sizeof buf, "\",\"grid\":[%u,%u,%u],\"block\":%u,\"lds\":%zu,\"attr\":%d", g.x, g.y, g.z, b.x, lds, pending_attr());
    pending_attr() = 0;
    std::string& s = log();
    if (!s.empty()) s += ",";
    s += "{\"kernel\":\"" + kernel_name(reinterpret_cast<const void*>(kern)) + buf + geometry(a0, 0) + "}";
}

inline hipError_t func_attr(const void*, hipFuncAttribute, int v) { pending_attr() = v; return hipSuccess; }
inline hipError_t no_device(int* dev) { *dev = 0; return hipSuccess; }
inline hipError_t cu_count(int* n) { const char* e = getenv("REC_CUS"); *n = e ? atoi(e) : 256; return hipSuccess; }

} // namespace rec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, lds, st, ...) rec::launch(kern, grid, block, (size_t)(lds), __VA_ARGS__)
#define hipFuncSetAttribute(f, a, v) rec::func_attr(f, a, v)
#define hipGetLastError() hipSuccess
#define hipGetDevice(p) rec::no_device(p)
#define hipDeviceGetAttribute(p, a, d) rec::cu_count(p)
