// tsq_gather.hip -- the one sort of tsqa_gather_async (tsq_gather.cuh): its pieces' (key, slot) pairs, ordered by key with ROCm's
// header-only rocPRIM.  A translation unit of its own: the sort's templates take seconds to compile and megabytes of code, and the
// runtime's two other units stay as they were.  No second path: where the header is missing the library does not build.
#include <cstring>          // (in front of rocPRIM: its radix sort uses memcpy without including it)
#include <rocprim/device/device_radix_sort.hpp>

#include "tsq_gather_sort.h"

namespace tsq {

// key = block << 22 | lo, or all ones for an unused slot: bits 0 .. 54 hold every block number (below 2^32) and every lo (below
// 2^22), and the all-ones key stays behind every piece's in them.  The sort is stable: equal (block, lo) keep their slots' order.
constexpr unsigned kGatherKeyBits = 55;

hipError_t gather_sort_storage(uint32_t n, size_t* bytes)
{
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                     static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), n, 0u, kGatherKeyBits,
                                     static_cast<hipStream_t>(nullptr));
}

hipError_t gather_sort_pairs(void* temp, size_t bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint32_t* slots_in, uint32_t* slots_out,
                       uint32_t n, hipStream_t s)
{
    return rocprim::radix_sort_pairs(temp, bytes, keys_in, keys_out, slots_in, slots_out, n, 0u, kGatherKeyBits, s);
}

}  // namespace tsq
