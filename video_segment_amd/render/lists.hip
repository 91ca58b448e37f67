// lists.hip -- what every list-making family does the same way (gfx950): the library radix sorts and the plain
// scan, instantiated here and nowhere else, and the copy of a call's lists to the caller's device memory.
//
//   SortKeysU64, SortPairs*   hipcub::DeviceRadixSort on bits [0, end_bit), one instantiation per operand type
//   ExclusiveSumU32           hipcub::DeviceScan::ExclusiveSum over uint32 counts
//   k_copy_lists              up to four lists, all of them or none: their lengths are known on the device only
//
// The scans over segment heads are templates over the head functor (render_scan.h).
#include "render.h"

#include <hipcub/hipcub.hpp>

namespace vsg_render_impl {

namespace {

typedef unsigned long long u64;

template <class K, class V>
size_t PairsTempBytes(int64_t n, int end_bit) {
  size_t bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const K*)nullptr, (K*)nullptr, (const V*)nullptr,
                                           (V*)nullptr, n, 0, end_bit, (hipStream_t) nullptr);
  return bytes;
}

// The length of every list is read and checked before a word is written: a list longer than its limit, or a
// raised flag, and the block leaves.  Then the words of the lists, one behind the other, dword by dword,
// grid-stride.  The four lists are taken apart with constant indices only: the descriptor stays in registers.
__global__ __launch_bounds__(256) void k_copy_lists(CopyLists d) {
  if (d.flags && *d.flags) return;
  size_t end[4], total = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const CopyList& l = d.list[j];
    const uint32_t count = l.count ? *l.count : l.fixed;
    if (count > l.limit) return;
    total += (size_t)count * l.words;
    end[j] = total;
  }
  const size_t step = (size_t)gridDim.x * 256;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < total; k += step) {
    if (k < end[0]) d.list[0].to[k] = d.list[0].from[k];
    else if (k < end[1]) d.list[1].to[k - end[0]] = d.list[1].from[k - end[0]];
    else if (k < end[2]) d.list[2].to[k - end[1]] = d.list[2].from[k - end[1]];
    else d.list[3].to[k - end[2]] = d.list[3].from[k - end[2]];
  }
}

}  // namespace

size_t SortKeysU64TempBytes(int64_t n, int end_bit) {
  size_t bytes = 0;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, n, 0, end_bit,
                                          (hipStream_t) nullptr);
  return bytes;
}

hipError_t SortKeysU64(void* temp, size_t temp_bytes, const u64* in, u64* out, int64_t n, int end_bit,
                       hipStream_t stream) {
  return hipcub::DeviceRadixSort::SortKeys(temp, temp_bytes, in, out, n, 0, end_bit, stream);
}

size_t SortPairsU64U32TempBytes(int64_t n, int end_bit) { return PairsTempBytes<u64, uint32_t>(n, end_bit); }
size_t SortPairsU64U64TempBytes(int64_t n, int end_bit) { return PairsTempBytes<u64, u64>(n, end_bit); }
size_t SortPairsU32U32TempBytes(int64_t n, int end_bit) { return PairsTempBytes<uint32_t, uint32_t>(n, end_bit); }

hipError_t SortPairsU64U32(void* temp, size_t temp_bytes, const u64* keys_in, u64* keys_out, const uint32_t* vals_in,
                           uint32_t* vals_out, int64_t n, int end_bit, hipStream_t stream) {
  return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit,
                                            stream);
}

hipError_t SortPairsU64U64(void* temp, size_t temp_bytes, const u64* keys_in, u64* keys_out, const u64* vals_in,
                           u64* vals_out, int64_t n, int end_bit, hipStream_t stream) {
  return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit,
                                            stream);
}

hipError_t SortPairsU32U32(void* temp, size_t temp_bytes, const uint32_t* keys_in, uint32_t* keys_out,
                           const uint32_t* vals_in, uint32_t* vals_out, int64_t n, int end_bit, hipStream_t stream) {
  return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit,
                                            stream);
}

size_t ExclusiveSumU32TempBytes(int n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, n,
                                         (hipStream_t) nullptr);
  return bytes;
}

hipError_t ExclusiveSumU32(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, int n,
                           hipStream_t stream) {
  return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, n, stream);
}

void LaunchCopyLists(const CopyLists& lists, hipStream_t stream) {
  size_t words = 0;
  for (const CopyList& l : lists.list) words += (size_t)l.limit * l.words;
  if (words == 0) return;
  const size_t groups = (words + 255) / 256;
  hipLaunchKernelGGL(k_copy_lists, dim3((unsigned)(groups < 2048 ? groups : 2048)), dim3(256), 0, stream, lists);
}

}  // namespace vsg_render_impl
