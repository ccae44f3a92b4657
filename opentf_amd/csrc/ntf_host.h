// The host scaffold of every entry of the library, once: the check macros and allocators of a handle with an `err` string (ntf_engine, ntf_n2v, ntf_d2v,
// ntf_knn, ntf_link), the RAII device buffer of the handle-less entries (ntf_metrics, ntf_auc, ntf_cooc), the timed launch of the stand-alone entries (ntf_d2v, ntf_knn), the upload of a host table into padded device rows and the dispatch of run-time widths and flags onto the kernels' template arguments.
#pragma once
#include "../../include/opentf_amd.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <type_traits>

#define HIPCHK(h, call)                                                                                   \
    do {                                                                                                  \
        hipError_t _s = (call);                                                                           \
        if (_s != hipSuccess) {                                                                           \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(_s);                                 \
            return NTF_EHIP;                                                                              \
        }                                                                                                 \
    } while (0)
#define FAIL(h, code, msg) do { (h)->err = (msg); return (code); } while (0)

namespace ntf {

// n elements of T; n <= 0 gives a null pointer and NTF_OK
template <class H, typename T> int dev_alloc(H* h, T** p, int64_t n) {
    *p = nullptr;
    if (n <= 0) return NTF_OK;
    const hipError_t s = hipMalloc((void**)p, (size_t)n * sizeof(T));
    if (s != hipSuccess) { *p = nullptr; h->err = std::string("hipMalloc: ") + hipGetErrorString(s); return NTF_ENOMEM; }
    return NTF_OK;
}
// a buffer that only grows: at least n elements afterwards, the contents not kept
template <class H, typename T> int dev_grow(H* h, T** p, int64_t* cap, int64_t n) {
    if (n <= *cap) return NTF_OK;
    if (*p) hipFree(*p);
    *cap = 0;
    const int rc = dev_alloc(h, p, n);
    if (rc == NTF_OK) *cap = n;
    return rc;
}

// what `launch` puts on h->st, then the synchronize; device_ms (may be null): the device time between the handle's event pair ev0 / ev1, made on first use.
// A launch error is "<what> kernel launch: <HIP's text>"
template <class H, class F> int timed_launch(H* h, double* device_ms, const char* what, F&& launch) {
    if (device_ms) { if (!h->ev0) { HIPCHK(h, hipEventCreate(&h->ev0)); HIPCHK(h, hipEventCreate(&h->ev1)); } HIPCHK(h, hipEventRecord(h->ev0, h->st)); }
    launch();
    if (device_ms) HIPCHK(h, hipEventRecord(h->ev1, h->st));
    const hipError_t s = hipGetLastError();
    if (s != hipSuccess) FAIL(h, NTF_EHIP, std::string(what) + " kernel launch: " + hipGetErrorString(s));
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (device_ms) { float ms = 0.f; HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1)); *device_ms = ms; }
    return NTF_OK;
}

// a device buffer that lives as long as its owner; an empty request still allocates (16 bytes), so `p` is never null after a success
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) hipFree(p); }
    bool alloc(size_t bytes, bool zero = false) {
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { p = nullptr; return false; }
        return !zero || hipMemset(p, 0, bytes ? bytes : 16) == hipSuccess;
    }
    bool put(const void* host, size_t bytes) { return alloc(bytes) && (!bytes || hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) == hipSuccess); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// host table [rows, d] -> device rows of stride dp >= d floats; the pad columns are exact zeros (they add nothing to a dot product or a norm chain)
inline hipError_t upload_padded(float* dst, int64_t dp, const float* src, int64_t d, int64_t rows) {
    if (dp != d) { const hipError_t s = hipMemset(dst, 0, (size_t)rows * dp * 4); if (s != hipSuccess) return s; }
    return hipMemcpy2D(dst, (size_t)dp * 4, src, (size_t)d * 4, (size_t)d * 4, (size_t)rows, hipMemcpyHostToDevice);
}

// a row width of nv = d / 64 in LO .. 4 sixty-fours as a compile-time constant: f(std::integral_constant<int, nv>()) and true; any other nv calls nothing and gives false.
// LO > 1 keeps the widths below it from being instantiated at all (a kernel that is never launched does not enter the code object).
template <int LO = 1, class F> bool with_nv(int nv, F&& f) {
    if (nv < LO || nv > 4) return false;
    if constexpr (LO <= 1) if (nv == 1) f(std::integral_constant<int, 1>());
    if constexpr (LO <= 2) if (nv == 2) f(std::integral_constant<int, 2>());
    if constexpr (LO <= 3) if (nv == 3) f(std::integral_constant<int, 3>());
    if (nv == 4) f(std::integral_constant<int, 4>());
    return true;
}
// a run-time flag as a compile-time one: f(std::true_type()) or f(std::false_type())
template <class F> void with_flag(bool b, F&& f) { if (b) f(std::true_type()); else f(std::false_type()); }
// a run-time v out of the set VS (the widths a launcher has kernels for) as f(std::integral_constant<int, v>()) and true; any other v calls nothing and gives false
template <int... VS, class F> bool with_value(int v, F&& f) { return ((v == VS && (f(std::integral_constant<int, VS>()), true)) || ...); }

}  // namespace ntf
