// fake_hip.h -- the knobs and counters of fake_hip.cpp, a stand-in for the HIP entry points that engine_host.h references.
// Copies are only recorded by hipMemcpyAsync and carried out by hipStreamSynchronize, so a test sees what a stream still holds.
#pragma once
#include <cstddef>

struct FakeHip {
    // counters since reset()
    int waits = 0, copies = 0, mallocs = 0;
    // 1-based: the k-th allocation / copy from now fails once (0: none); every wait fails while fail_wait is set
    int fail_malloc_at = 0, fail_copy_at = 0;
    bool fail_wait = false, fail_set_device = false;
    int pending() const;                      // copies recorded and not yet carried out
    void reset();                             // counters and knobs back to zero; allocations and pending copies stay
};
extern FakeHip fake;
