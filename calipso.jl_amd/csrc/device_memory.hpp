// device_memory.hpp — the one owner of a handle's device memory (the sparse LDL^T plan of sparse.hip, the sparse KKT handle of sparse_kkt_handle.hpp).  Every allocation is
// on the handle's list and freed with it; every allocation is zero-filled on the HANDLE'S stream: a fill on the null stream would not be ordered with what follows, the
// stream being non-blocking.  A handle H gives three things: device_allocations() (the list), device_stream() (read at call time: a borrowed stream is honoured) and
// device_error(text) (records the text as the handle's last error, returns CALIPSO_ERR_HIP).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/calipso_hip.h"

namespace calipso {

// a buffer of the handle that grows on demand, is never shrunk and is kept (device_grown below): a call that repeats its shapes allocates nothing
template <typename T> struct Grown { T* p = nullptr; size_t cap = 0; };      // cap: entries

#define DEVICE_TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return s->device_error(std::string(#call) + ": " + hipGetErrorString(e__)); } while (0)

// a fixed allocation: made once
template <typename H, typename T> int device_fixed(H* s, T** out, size_t count) {
    count = std::max<size_t>(count, 1);
    DEVICE_TRY(hipMalloc((void**)out, sizeof(T) * count));
    s->device_allocations().push_back(*out);
    DEVICE_TRY(hipMemsetAsync(*out, 0, sizeof(T) * count, s->device_stream()));
    return CALIPSO_OK;
}
// ... and one that holds a host vector's entries
template <typename H, typename T> int device_upload(H* s, const std::vector<T>& h, const T** out) {
    T* p = nullptr;
    const int rc = device_fixed(s, &p, h.size());
    if (rc < 0) return rc;
    if (!h.empty()) DEVICE_TRY(hipMemcpyAsync(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, s->device_stream()));
    DEVICE_TRY(hipStreamSynchronize(s->device_stream()));      // (the vector may be the caller's local)
    *out = p;
    return CALIPSO_OK;
}
// a grown buffer given back: off the list, empty again.  The caller has made sure that nothing in flight reads it
template <typename H, typename T> void device_release(H* s, Grown<T>& b) {
    if (!b.p) return;
    std::vector<void*>& list = s->device_allocations();
    (void)hipFree(b.p);
    list.erase(std::find(list.begin(), list.end(), (void*)b.p));
    b = Grown<T>();
}
// a grown buffer: larger only when asked for more than it has; nothing in flight reads the one that is freed
template <typename H, typename T> int device_grown(H* s, Grown<T>& b, size_t want) {
    if (want <= b.cap) return CALIPSO_OK;
    DEVICE_TRY(hipStreamSynchronize(s->device_stream()));
    device_release(s, b);
    const int rc = device_fixed(s, &b.p, want);
    if (rc >= 0) b.cap = want;
    return rc;
}

#undef DEVICE_TRY

}  // namespace calipso
