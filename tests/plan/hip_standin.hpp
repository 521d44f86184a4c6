// hip_standin.hpp -- what the plan harness sees of the host stand-in for the HIP runtime.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace standin {
struct Upload {
    const void *dst;
    size_t bytes;
    uint64_t hash;   // FNV-1a of the source bytes
};
extern std::vector<Upload> uploads;   // every hipMemcpy since the last reset()
extern int ncu;                       // what hipDeviceGetAttribute reports (< 0: the call fails)
extern int fail_malloc_at;            // the k-th hipMalloc from now fails (1-based; 0: none)
extern int fail_event;                // hipEventCreateWithFlags fails
extern int mallocs;                   // hipMalloc calls since the last reset()
void reset();
uint64_t fnv1a(const void *p, size_t n);
size_t live();                        // allocations, streams and events not yet released
size_t size_of(const void *p);        // bytes of a live allocation (0: not one)
}  // namespace standin
