// tsq_gather_sort.h -- what tsq_gather.hip gives the runtime: the stable sort of the gather's (key, slot) pairs over key bits 0 .. 54.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace tsq {

// the temporary storage a sort of n pairs needs (asked when the scratch is reserved, not per call)
hipError_t gather_sort_storage(uint32_t n, size_t* bytes);
// enqueued on s; nothing is waited for.  keys_in / slots_in are left as they were.
hipError_t gather_sort_pairs(void* temp, size_t bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* slots_in, uint32_t* slots_out,
                       uint32_t n, hipStream_t s);

}  // namespace tsq
