// hip_standin.cpp -- host stand-ins for the HIP runtime calls that plan construction and
// the plan's owners make (tests/plan/plan_harness.cpp): "device" memory is malloc'd, so
// the harness reads the uploaded tables back directly and LeakSanitizer sees every
// allocation the plan does not release.  hipMemcpy logs (destination, bytes, FNV-1a of
// the source); the k-th hipMalloc and the event creation fail on request.  No kernel is
// ever launched: the launchers stay unresolved at link time.
#include "hip_standin.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <map>

namespace standin {
std::vector<Upload> uploads;
int ncu = 256, fail_malloc_at = 0, fail_event = 0, mallocs = 0;
static std::map<const void *, size_t> g_live;

void reset() {
    uploads.clear();
    fail_malloc_at = fail_event = mallocs = 0;
}
uint64_t fnv1a(const void *p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
size_t live() { return g_live.size(); }
size_t size_of(const void *p) {
    auto it = g_live.find(p);
    return it == g_live.end() ? 0 : it->second;
}
static void *take(size_t bytes) {
    void *p = std::malloc(bytes ? bytes : 1);
    if (p) g_live[p] = bytes;
    return p;
}
static hipError_t give(void *p) {
    if (!p) return hipSuccess;
    if (!g_live.erase(p)) std::abort();   // released twice, or never allocated here
    std::free(p);
    return hipSuccess;
}
}  // namespace standin

// amx_final.hip's LDS size of the limiter ring: small, so amx_limiter_prepare never asks
// for the raised limit (a launcher-side call)
namespace amx {
size_t limiter_lds_bytes(int) { return 0; }
}

extern "C" {

hipError_t hipMalloc(void **ptr, size_t size) {
    standin::mallocs++;
    if (standin::fail_malloc_at > 0 && --standin::fail_malloc_at == 0) {
        *ptr = nullptr;
        return hipErrorOutOfMemory;
    }
    *ptr = standin::take(size);
    return *ptr ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void *ptr) { return standin::give(ptr); }
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) {
    if (standin::size_of(dst) < n) std::abort();   // a copy past its allocation
    standin::uploads.push_back({dst, n, standin::fnv1a(src, n)});
    std::memcpy(dst, src, n);
    return hipSuccess;
}
hipError_t hipMemset(void *dst, int v, size_t n) {
    if (standin::size_of(dst) < n) std::abort();
    std::memset(dst, v, n);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipGetDevice(int *dev) {
    *dev = 0;
    return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) {
    if (standin::ncu < 0) return hipErrorInvalidDevice;
    *v = standin::ncu;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "stand-in error"; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
    *s = static_cast<hipStream_t>(standin::take(1));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { return standin::give(s); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    if (standin::fail_event) return hipErrorOutOfMemory;
    *e = static_cast<hipEvent_t>(standin::take(1));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { return standin::give(e); }

}  // extern "C"
