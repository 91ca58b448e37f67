// render_scan.h -- the scan the families rank their sorted lists with: the inclusive sum of a head functor over
// the indices 0 .. n - 1 (the library scan over a transform of a counting iterator), and the head functors with
// the key layouts they read.  Included by render_capi.cpp, which calls the scans, and by the .hip files whose
// kernels take the same keys apart.  The library sorts and the plain scan are in lists.hip.
#ifndef VSG_RENDER_RENDER_SCAN_H_
#define VSG_RENDER_RENDER_SCAN_H_

#include <utility>

#include <hipcub/hipcub.hpp>

#include "render.h"

namespace vsg_render_impl {

// What a head functor returns for an index: the type of the sums.
template <class Head>
using HeadSum = decltype(std::declval<Head>()(0u));

template <class Head>
hipError_t HeadScanImpl(void* temp, size_t& temp_bytes, const Head& head, HeadSum<Head>* out, int64_t n,
                        hipStream_t stream) {
  typedef hipcub::CountingInputIterator<uint32_t> Counter;
  hipcub::TransformInputIterator<HeadSum<Head>, Head, Counter> heads(Counter(0), head);
  return hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, heads, out, n, stream);
}

// Work space of HeadScan over n indices.
template <class Head>
size_t HeadScanTempBytes(int64_t n) {
  size_t bytes = 0;
  (void)HeadScanImpl(nullptr, bytes, Head{}, (HeadSum<Head>*)nullptr, n, (hipStream_t) nullptr);
  return bytes;
}

// out[i] = head(0) + ... + head(i), i < n.
template <class Head>
hipError_t HeadScan(void* temp, size_t temp_bytes, const Head& head, HeadSum<Head>* out, int64_t n,
                    hipStream_t stream) {
  return HeadScanImpl(temp, temp_bytes, head, out, n, stream);
}

// ---- level.hip, boundaries.hip, contours.hip: keys sorted by the group in their high half ----------------

// Sorted key i -> 1 if it is the first of its group: the sums are the (1-based) ranks of the groups.
struct HeadFlag {
  const unsigned long long* keys;
  __host__ __device__ uint32_t operator()(uint32_t i) const {
    return (i == 0 || (uint32_t)(keys[i] >> 32) != (uint32_t)(keys[i - 1] >> 32)) ? 1u : 0u;
  }
};

// ---- components.hip: sorted labels ---------------------------------------------------------------------------

struct LabelHead {
  const uint32_t* label;
  __host__ __device__ uint32_t operator()(uint32_t k) const {
    return (k == 0 || label[k] != label[k - 1]) ? 1u : 0u;
  }
};

// ---- adjacency.hip: the fields of a key (the layout is in adjacency.hip) ----------------------------------

__device__ __host__ __forceinline__ unsigned long long AdjGroup(unsigned long long key, int group_bits) {
  return key >> (group_bits + 2);
}
__device__ __host__ __forceinline__ uint32_t AdjOther(unsigned long long key, int group_bits) {
  return (uint32_t)(key >> 1) & (uint32_t)((1ull << (group_bits + 1)) - 1);
}
__device__ __host__ __forceinline__ bool AdjReserved(unsigned long long key, int group_bits) {
  return (key >> (group_bits + 1)) & 1;
}

// Sorted key i -> 1 << 32 if it is the first of its group, + 1 if it is the first of its (group, other)
// and other is a group: HeadFlag's sum with two counters in one.
struct AdjHeads {
  const unsigned long long* keys;
  int group_bits;
  __host__ __device__ unsigned long long operator()(uint32_t i) const {
    const unsigned long long key = keys[i];
    const bool first = i == 0;
    const unsigned long long prev = first ? 0ull : keys[i - 1];
    const bool node = first || AdjGroup(key, group_bits) != AdjGroup(prev, group_bits);
    const bool edge = (first || (key >> 1) != (prev >> 1)) && !AdjReserved(key, group_bits);
    return (node ? 1ull << 32 : 0ull) | (edge ? 1ull : 0ull);
  }
};

// ---- overlap.hip: the fields of a key and of a column key (the layout is in overlap.hip) ------------------

struct OvlBits {
  int group_bits, label_bits;
  __host__ __device__ unsigned long long P(unsigned long long key) const { return key >> (label_bits + 1); }
  __host__ __device__ unsigned long long B(unsigned long long key) const {
    return key & ((1ull << (label_bits + 1)) - 1);
  }
  __host__ __device__ bool NoP(unsigned long long key) const { return (key >> (label_bits + 1 + group_bits)) & 1; }
  __host__ __device__ bool NoB(unsigned long long key) const { return (key >> label_bits) & 1; }
  __host__ __device__ unsigned long long Swapped(unsigned long long key) const {
    return B(key) << (group_bits + 1) | P(key);
  }
  __host__ __device__ unsigned long long ColB(unsigned long long ckey) const { return ckey >> (group_bits + 1); }
  __host__ __device__ bool ColNoB(unsigned long long ckey) const {
    return (ckey >> (group_bits + 1 + label_bits)) & 1;
  }
  __host__ __device__ bool ColNoP(unsigned long long ckey) const { return (ckey >> group_bits) & 1; }
};

// Sorted run i -> 1 << 32 if it is the first of a group, + 1 if it is the first of a (group, label).
struct OvlRowHeads {
  const unsigned long long* keys;
  OvlBits bits;
  __host__ __device__ unsigned long long operator()(uint32_t i) const {
    const unsigned long long key = keys[i];
    if (bits.NoP(key)) return 0ull;
    const bool first = i == 0;
    const unsigned long long prev = first ? 0ull : keys[i - 1];
    const bool row = first || bits.P(prev) != bits.P(key);
    const bool pair = !bits.NoB(key) && (first || prev != key);
    return (row ? 1ull << 32 : 0ull) | (pair ? 1ull : 0ull);
  }
};
// Sorted run i -> 1 << 32 if it is the first of its key, + its length.  The lengths of a frame sum to
// less than 2^32: the low half never carries into the high one.
struct OvlKeyHeads {
  const unsigned long long* keys;
  const uint32_t* lengths;
  __host__ __device__ unsigned long long operator()(uint32_t i) const {
    const bool head = i == 0 || keys[i - 1] != keys[i];
    return (head ? 1ull << 32 : 0ull) | lengths[i];
  }
};
// Sorted column key j -> 1 if it is the first of a label.
struct OvlColHeads {
  const unsigned long long* ckeys;
  OvlBits bits;
  __host__ __device__ uint32_t operator()(uint32_t j) const {
    const unsigned long long ckey = ckeys[j];
    if (bits.ColNoB(ckey)) return 0u;
    return (j == 0 || bits.ColB(ckeys[j - 1]) != bits.ColB(ckey)) ? 1u : 0u;
  }
};

// ---- tree_cut.hip: whole keys, and marks ---------------------------------------------------------------------

// Sorted key i -> 1 if it differs from the key before: the sums are the (1-based) ranks of the distinct keys.
struct CutKeyHead {
  const unsigned long long* keys;
  __host__ __device__ uint32_t operator()(uint32_t i) const { return (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u; }
};
// Node i -> its mark (0 or 1): the sums are the (1-based) places of the marked nodes.
struct CutMark {
  const uint32_t* marks;
  __host__ __device__ uint32_t operator()(uint32_t i) const { return marks[i]; }
};

}  // namespace vsg_render_impl

#endif  // VSG_RENDER_RENDER_SCAN_H_
