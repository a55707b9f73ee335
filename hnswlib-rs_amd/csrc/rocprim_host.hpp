// rocprim_host.hpp -- rocPRIM's two-call protocol (ask for the size of the temporary storage, allocate it, call again), once, for
// the graph units that scan and sort.  Beside hip_host.hpp, and apart from it so that a unit without a scan or a sort does not
// compile rocPRIM.  Both calls go on the stream and NOBODY WAITS here: `temp` is the caller's, and so is the moment when the
// stream has been waited for and the storage may go.  Private: not installed, not part of the ABI.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "hip_host.hpp"

namespace hnswgpu {

// out[i] = in[0] + .. + in[i - 1] for i < count.  In: uint32_t* or const uint32_t* (rocPRIM's kernels are instantiated per
// iterator type: a unit keeps the one it had).
template <typename In>
int exclusive_scan_u32(DevMem& temp, In in, uint32_t* out, uint64_t count, hipStream_t stream, std::string& err) {
    size_t temp_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, temp_bytes, in, out, 0u, (size_t)count, rocprim::plus<uint32_t>(), stream));
    HIP_TRY(temp.alloc(std::max<size_t>(temp_bytes, 256)));
    HIP_TRY(rocprim::exclusive_scan(temp.p, temp_bytes, in, out, 0u, (size_t)count, rocprim::plus<uint32_t>(), stream));
    return OK;
}

// (keys_in, vals_in) sorted by bits 0 .. end_bit - 1 of the key into (keys_out, vals_out); stable.  Size: as the caller counts
// (rocPRIM's kernels are instantiated per size type as well).
template <typename Key, typename Value, typename Size>
int radix_sort_pairs(DevMem& temp, Key* keys_in, Key* keys_out, Value* vals_in, Value* vals_out, Size count, unsigned end_bit, hipStream_t stream,
                     std::string& err) {
    size_t temp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, keys_out, vals_in, vals_out, count, 0u, end_bit, stream));
    HIP_TRY(temp.alloc(std::max<size_t>(temp_bytes, 256)));
    HIP_TRY(rocprim::radix_sort_pairs(temp.p, temp_bytes, keys_in, keys_out, vals_in, vals_out, count, 0u, end_bit, stream));
    return OK;
}

}  // namespace hnswgpu
