// hip_host.hpp -- the HIP host helpers of the five host units (search_device.hip, exact_knn.hip, range_search.hip,
// symmetric_graph.hip, graph_components.hip), once.  Needs the HIP runtime: nothing that a host-only build compiles (capi.cpp, the builder, the stand-ins
// of tests/cpp) may include it, and the kernel units do not see it.  Private: not installed, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "hnswio.hpp"  // ERR_DEVICE

// inside a function that returns a status code and has a `std::string& err` in scope
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            err = std::string(#expr) + ": " + hipGetErrorString(e_);                           \
            return ERR_DEVICE;                                                                 \
        }                                                                                      \
    } while (0)

namespace hnswgpu {

// Every entry point works on the replica's device and leaves the CALLER's current HIP device as it found it (a host
// thread shared with PyTorch, a Rust or a Julia runtime keeps allocating and launching where it did before the call).
// device < 0 (a state that never got a device): nothing is asked of the runtime.
class DeviceGuard {
public:
    explicit DeviceGuard(int device) {
        if (device < 0) return;
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        if (cur == device) return;
        status_ = hipSetDevice(device);
        if (status_ == hipSuccess && cur >= 0) prev_ = cur;
        // (a refusal is status()'s to report: left in the thread's last-error slot, the next HIP_TRY(hipGetLastError()) behind an
        // unrelated launch would report it as that launch's)
        if (status_ != hipSuccess) (void)hipGetLastError();
    }
    ~DeviceGuard() { if (prev_ >= 0) (void)hipSetDevice(prev_); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    hipError_t status() const { return status_; }
private:
    int prev_ = -1;
    hipError_t status_ = hipSuccess;
};

// device memory of one call: freed when the call ends, or by release() before
struct DevMem {
    void* p = nullptr;
    ~DevMem() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
};

inline uint64_t round_up(uint64_t x, uint64_t m) { return (x + m - 1) / m * m; }

}  // namespace hnswgpu
