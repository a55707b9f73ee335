// hip_host.hpp -- the HIP host helpers of every host unit (the .hip files other than search_kernels_tu.hip), once: error handling,
// the device guard, call-scoped device memory and its layout, the grid of a one-thread-per-item launch, the wait that ends a call.
// Needs the HIP runtime: nothing that a host-only build compiles (capi.cpp, the builder, the stand-ins of tests/cpp) may include
// it, and the kernel units do not see it.  Private: not installed, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>

#include "hnswio.hpp"  // ERR_DEVICE
#include "scratch_layout.hpp"
#include "search_device.hpp"  // knobs()

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

// HNSWGPU_POISON_SCRATCH (test hook, Knobs::poison_scratch): what one call filled, per host thread.  A call is the lifetime of the
// outermost DeviceGuard of its thread -- every device entry makes one before it allocates or takes anything from a pool, and the
// entries that call each other (the graph units down to the search) nest theirs.
struct PoisonTally {
    int depth = 0;
    uint64_t blocks = 0, bytes = 0;
};
inline thread_local PoisonTally t_poison;

// Scratch that passes from nobody's to this call's: with the knob on, `bytes` at `p` are filled with its byte and the host waits
// for the fill before the block is handed on.  With the knob off (the default) nothing is asked of the runtime.
inline hipError_t poison_scratch(void* p, uint64_t bytes) {
    const int byte = knobs().poison_scratch;
    if (byte < 0 || p == nullptr || bytes == 0) return hipSuccess;
    hipError_t e = hipMemset(p, byte, (size_t)bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    t_poison.blocks += 1;
    t_poison.bytes += bytes;
    return hipSuccess;
}

// Every entry point works on the replica's device and leaves the CALLER's current HIP device as it found it (a host
// thread shared with PyTorch, a Rust or a Julia runtime keeps allocating and launching where it did before the call).
// device < 0 (a state that never got a device): nothing is asked of the runtime.
class DeviceGuard {
public:
    explicit DeviceGuard(int device) {
        ++t_poison.depth;
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
    ~DeviceGuard() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
        if (--t_poison.depth > 0 || t_poison.blocks == 0) return;
        // the call ends: one line under HNSWGPU_TRACE_LAUNCH (the tests read it to prove that the hook ran for this entry)
        if (knobs().trace_launch)
            std::fprintf(stderr, "[hnswgpu poison] blocks %llu bytes %llu byte 0x%02x\n", (unsigned long long)t_poison.blocks,
                         (unsigned long long)t_poison.bytes, (unsigned)(knobs().poison_scratch & 0xFF));
        t_poison.blocks = t_poison.bytes = 0;
    }
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
    // a fresh block of `bytes`, poisoned under HNSWGPU_POISON_SCRATCH: every call-scoped allocation goes through here
    hipError_t alloc(size_t bytes) {
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        return poison_scratch(p, bytes);
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
};

// A call's block, sized by the arrays that `lay` names and divided among them (scratch_layout.hpp).  Nothing is written before the
// layout is known to fit.  Block: DevMem, or a pooled block with the same alloc() and p (exact_internal.hpp: ScratchLease).
template <typename Block>
int alloc_layout(const char* what, Block& mem, ScratchLayout& lay, std::string& err) {
    const uint64_t bytes = lay.size() != 0 ? lay.size() : ScratchLayout::ALIGN;  // (a layout without an array: a line that nobody uses)
    HIP_TRY(mem.alloc(bytes));
    if (!lay.place(mem.p, bytes)) {
        err = std::string(what) + ": scratch layout";
        return ERR_FORMAT;
    }
    return OK;
}

// A host form's arrays go into its block, which alloc_layout has placed (scratch_layout.hpp: Uploads).  Nobody waits here.
inline int copy_uploads(const Uploads& ups, hipStream_t stream, std::string& err) {
    for (int i = 0; i < ups.count(); ++i) {
        void* to;
        const void* from;
        uint64_t bytes;
        ups.item(i, to, from, bytes);
        if (bytes != 0) HIP_TRY(hipMemcpyAsync(to, from, bytes, hipMemcpyHostToDevice, stream));
    }
    return OK;
}

// The end of a call: what the caller asked for (`to` is there) goes from scratch to the out arrays, host memory for `host`, and the
// stream is waited for.
struct CopyOut {
    void* to;
    const void* from;
    uint64_t bytes;
};
inline int copy_out(std::initializer_list<CopyOut> copies, bool host, hipStream_t stream, std::string& err) {
    for (const CopyOut& c : copies)
        if (c.to && c.bytes) HIP_TRY(hipMemcpyAsync(c.to, c.from, c.bytes, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return OK;
}

// one thread per item, 256 to a block
inline dim3 grid_of(uint64_t threads) { return dim3((uint32_t)((threads + 255) / 256)); }

// Declared behind a call's device memory, so destroyed first: whatever happens, nothing of the call is running when its memory is
// freed or goes back to a pool.
struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
};

// The entries that take a device ordinal instead of a replica: OK, or ERR_DEVICE and "<what>: no device <N>"
inline int use_device_ordinal(const char* what, int device, std::string& err) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
        (void)hipGetLastError();
        err = std::string(what) + ": no device " + std::to_string(device);
        return ERR_DEVICE;
    }
    return OK;
}

}  // namespace hnswgpu
