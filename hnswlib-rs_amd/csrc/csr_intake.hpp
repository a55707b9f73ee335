// csr_intake.hpp -- how a caller's CSR comes in, for graph_components.hip and spanning_forest.hip: the host form's arrays go up into
// one block, the validation kernels of union_find.hpp run, their word is read back and a bad CSR is refused in the entry's words.
// Host code over that header's kernels, in an unnamed namespace like them: each of the two units launches its own copy.  Private.
#pragma once
#include <string>

#include "hip_host.hpp"
#include "hnswio.hpp"
#include "union_find.hpp"

namespace hnswgpu {
namespace {

// what csr_intake leaves: the CSR in device memory (the caller's own arrays for the device form) and offsets[n], checked
struct CsrOnDevice {
    DevMem mem, word;  // the upload of the host form; the word of the checks (both are the call's until it ends)
    const uint64_t* offsets = nullptr;
    const uint32_t* cols = nullptr;
    const float* dists = nullptr;  // host form without want_dists: nullptr
    uint64_t total = 0;
};

// n rows.  host: the three arrays are host memory and have passed the same checks on the host; dists is uploaded iff want_dists.
// OK behind a wait for the stream: no kernel of the caller's follows a col that was not checked.  ERR_ARG: "<what>: <the fault>".
int csr_intake(const char* what, uint64_t n, const uint64_t* offsets, const uint32_t* cols, const float* dists, bool host, bool want_dists,
               hipStream_t stream, CsrOnDevice& out, std::string& err) {
    out.offsets = offsets;
    out.cols = cols;
    out.dists = dists;
    if (host) {
        const uint64_t total = offsets[n];
        uint64_t* up_offsets = nullptr;
        uint32_t* up_cols = nullptr;
        float* up_dists = nullptr;
        ScratchLayout lay;
        lay.array(up_offsets, n + 1);
        lay.array(up_cols, total);
        if (want_dists) lay.array(up_dists, total);
        lay.skip(256);
        const int rc = alloc_layout(what, out.mem, lay, err);
        if (rc != OK) return rc;
        HIP_TRY(hipMemcpyAsync(up_offsets, offsets, (n + 1) * 8, hipMemcpyHostToDevice, stream));
        if (total != 0) HIP_TRY(hipMemcpyAsync(up_cols, cols, total * 4, hipMemcpyHostToDevice, stream));
        if (want_dists && total != 0) HIP_TRY(hipMemcpyAsync(up_dists, dists, total * 4, hipMemcpyHostToDevice, stream));
        out.offsets = up_offsets;
        out.cols = up_cols;
        out.dists = up_dists;
    }
    // the checks, and the one word that says how they went
    HIP_TRY(out.word.alloc(256));
    unsigned long long* d_word = static_cast<unsigned long long*>(out.word.p);
    HIP_TRY(hipMemsetAsync(d_word, 0, 8, stream));
    hipLaunchKernelGGL(cc_check_offsets_kernel, grid_of(n + 1), dim3(256), 0, stream, out.offsets, (uint32_t)n, d_word);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cc_check_cols_kernel, dim3(CHECK_BLOCKS), dim3(256), 0, stream, out.offsets, out.cols, (uint32_t)n, d_word);
    HIP_TRY(hipGetLastError());
    unsigned long long word = 0;
    HIP_TRY(hipMemcpyAsync(&word, d_word, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if ((word >> 32) != 0ull) {
        err = std::string(what) + ": " + ((word & BAD_FIRST)     ? "offsets[0] is not 0"
                                          : (word & BAD_DESCENT) ? "the offsets descend"
                                          : (word & BAD_TOTAL)   ? "offsets[n] is 2^32 or more"
                                          : (word & BAD_NO_COLS) ? "null cols with entries"
                                                                 : "a col is not below n");
        return ERR_ARG;
    }
    out.total = word & 0xFFFFFFFFull;
    return OK;
}

}  // namespace
}  // namespace hnswgpu
