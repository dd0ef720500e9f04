// fake_hip.cpp -- the nine HIP entry points engine_host.h references, on the CPU and with nothing of the real runtime behind them.
// "Device" memory is malloc'd and remembered, so hipPointerGetAttributes answers as on_device() reads it; a copy is kept pending
// until the stream is waited on; the k-th allocation, the k-th copy and the wait can be made to fail (fake_hip.h).
#include "fake_hip.h"

#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

FakeHip fake;

namespace {
struct Copy {
    void *dst;
    const void *src;
    size_t bytes;
};
std::vector<Copy> g_pending;
// start -> bytes of every live allocation; the engines keep theirs until the process ends, where the device goes with it
struct Device : std::map<const char *, size_t> {
    ~Device() {
        for (auto &a : *this) std::free((void *)a.first);
    }
} g_device;
int g_stream;                                 // its address is the one stream's handle

void carry_out() {
    for (const Copy &c : g_pending) std::memcpy(c.dst, c.src, c.bytes);
    g_pending.clear();
}
}  // namespace

int FakeHip::pending() const { return (int)g_pending.size(); }
void FakeHip::reset() { *this = FakeHip(); }

extern "C" {

hipError_t hipSetDevice(int) { return fake.fail_set_device ? hipErrorInvalidDevice : hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int) {
    *stream = (hipStream_t)&g_stream;
    return hipSuccess;
}

hipError_t hipMalloc(void **ptr, size_t size) {
    ++fake.mallocs;
    if (fake.fail_malloc_at && --fake.fail_malloc_at == 0) return hipErrorOutOfMemory;
    *ptr = std::malloc(size ? size : 1);
    g_device[(const char *)*ptr] = size;
    return hipSuccess;
}

// (the runtime waits for the device before it frees: what is pending is carried out first, and this is no counted wait)
hipError_t hipFree(void *ptr) {
    if (!ptr) return hipSuccess;
    carry_out();
    g_device.erase((const char *)ptr);
    std::free(ptr);
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
    ++fake.copies;
    if (fake.fail_copy_at && --fake.fail_copy_at == 0) return hipErrorInvalidValue;
    g_pending.push_back(Copy{dst, src, bytes});
    return hipSuccess;
}

// a wait that fails leaves a broken stream behind: its copies never happen
hipError_t hipStreamSynchronize(hipStream_t) {
    ++fake.waits;
    if (fake.fail_wait) {
        g_pending.clear();
        return hipErrorUnknown;
    }
    carry_out();
    return hipSuccess;
}

hipError_t hipGetLastError(void) { return hipSuccess; }

const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e == hipSuccess ? "no error" : "fake failure"; }

hipError_t hipPointerGetAttributes(hipPointerAttribute_t *attributes, const void *ptr) {
    auto it = g_device.upper_bound((const char *)ptr);
    if (it == g_device.begin()) return hipErrorInvalidValue;
    --it;
    if ((const char *)ptr >= it->first + (it->second ? it->second : 1)) return hipErrorInvalidValue;   // pageable host memory
    std::memset(attributes, 0, sizeof(*attributes));
    attributes->type = hipMemoryTypeDevice;
    return hipSuccess;
}

}  // extern "C"
