// Device and pinned host arrays that belong together: a set is allocated whole or not at all, and released whole.
#pragma once
#include "context.hpp"

namespace evplp {
#pragma GCC visibility push(hidden)
// one array of a set; a set is any range of these (an std::array, say, built by one function for the allocation and the release alike)
struct ArrayWish { void **at; size_t bytes; bool pinned; };
template <class T> ArrayWish on_device(T *&p, size_t n) { return { (void **)&p, sizeof(T) * n, false }; }
template <class T> ArrayWish pinned(T *&p, size_t n) { return { (void **)&p, sizeof(T) * n, true }; }
template <class Set> void release_arrays(const Set &set) {
    for (const ArrayWish &a : set) { if (*a.at) { if (a.pinned) hipHostFree(*a.at); else hipFree(*a.at); } *a.at = nullptr; }
}
// the reason in c's error as "name: what: HIP's words"; the code to return
inline int hip_failure(evplp_context *c, const char *name, const char *what, hipError_t e) {
    c->set_error("%s: %s: %s", name, what, hipGetErrorString(e)); return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP;
}
// the set's arrays in order (every pointer null on entry); on a failure what this call made is freed, every pointer of the set is null,
// and the reason is in c's error
template <class Set> int alloc_arrays(evplp_context *c, const Set &set, const char *name, const char *what) {
    hipError_t e = hipSuccess;
    for (const ArrayWish &a : set) {
        if (e == hipSuccess) e = a.pinned ? hipHostMalloc(a.at, a.bytes, hipHostMallocDefault) : hipMalloc(a.at, a.bytes);
        if (e != hipSuccess) *a.at = nullptr;       // (the one that failed and those behind it)
    }
    if (e == hipSuccess) return EVPLP_OK;
    release_arrays(set);
    return hip_failure(c, name, what, e);
}
#pragma GCC visibility pop
}
