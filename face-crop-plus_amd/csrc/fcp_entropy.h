// What the entropy coders of fcp_jpeg.hip and fcp_png.hip share, each stated once: the pieces of their tables kernels (one
// wave per table: load counts -> merge -> histogram of sizes -> limit -> starts -> assign -> the kernel's own output), the
// bit writer of their emit kernels and, host side, the checks of an encode call's slots.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fcp_common.h"

namespace fcp_entropy {

constexpr long long kFib35 = 9227465;         // a Huffman tree over fewer counts than Fibonacci(35) is at most 32 deep
constexpr int kEntries = 5;                   // table entries per lane: entry i lives in lane i % 64, as fr[i / 64]

// The code size of every entry before any limit (0 for a zero frequency; all 0 with fewer than two non-zero ones), by
// the lanes of one wave.  A merge takes the two smallest non-zero frequencies, ties going to the larger index: one
// butterfly over the lanes' (smallest, second smallest) pairs of the key frequency << 9 | 511 - index.  libjpeg then walks
// the two `others` chains to add 1 to the code size of every symbol under c1 and c2 and links them; a chain is only a
// set, so here every entry carries the head of its set instead: each lane adds 1 to its entries under c1 or c2 and moves
// those under c2 to c1.  Same code sizes, no serial walk.  `entries`: how many of the 320 can be non-zero, one less the
// bound of the loop; the frequencies must not sum past 2^32.  fr[] is used up.
__device__ __forceinline__ void huffman_code_sizes(uint32_t (&fr)[kEntries], int entries, int (&cs)[kEntries]) {
  const int lane = threadIdx.x;
  int head[kEntries];
#pragma unroll
  for (int j = 0; j < kEntries; ++j) head[j] = lane + 64 * j, cs[j] = 0;
  constexpr unsigned long long kNone = ~0ull;
  for (int merges = 0; merges < entries - 1; ++merges) {                  // every merge empties one entry
    unsigned long long k1 = kNone, k2 = kNone;
#pragma unroll
    for (int j = 0; j < kEntries; ++j) {
      if (fr[j] == 0u) continue;
      const unsigned long long key = ((unsigned long long)fr[j] << 9) | (unsigned long long)(511 - (lane + 64 * j));
      if (key < k1) k2 = k1, k1 = key; else if (key < k2) k2 = key;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o1 = __shfl_xor(k1, off, 64), o2 = __shfl_xor(k2, off, 64);
      const unsigned long long lo = k1 < o1 ? k1 : o1, hi = k1 < o1 ? o1 : k1, rest = k2 < o2 ? k2 : o2;
      k1 = lo, k2 = hi < rest ? hi : rest;
    }
    if (k2 == kNone) break;                                               // one entry left: the tree is complete
    const int c1 = 511 - (int)(k1 & 511ull), c2 = 511 - (int)(k2 & 511ull);
    const uint32_t v2 = (uint32_t)(k2 >> 9);
#pragma unroll
    for (int j = 0; j < kEntries; ++j) {
      const int idx = lane + 64 * j;
      if (idx == c1) fr[j] += v2;
      if (idx == c2) fr[j] = 0u;
      if (head[j] == c1 || head[j] == c2) {
        ++cs[j];
        head[j] = c1;
      }
    }
  }
}

// libjpeg's limit of bits[0..BOUND] (codes per length) to LIMIT bits, for one lane: take a pair of the longest codes away,
// give its prefix to one of them and split a shorter code for the other.  Signed counts and the j > 0 guard only matter
// when the callers' preconditions do not hold; returns whether they did.
template <int BOUND, int LIMIT>
__device__ __forceinline__ bool limit_code_lengths(int* bits) {
  bool sane = true;
  for (int i = BOUND; i > LIMIT && sane; --i) {
    while (bits[i] > 0) {
      int j = i - 2;
      while (j > 0 && bits[j] == 0) --j;
      if (j == 0) {
        sane = false;
        break;
      }
      bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1;
    }
  }
  return sane;
}

// first_pos[1..LIMIT + 1] and first_code[1..LIMIT] from bits[1..LIMIT], for one lane: the symbols at positions first_pos[len]
// .. first_pos[len + 1] - 1 in code order get the codes of length len, counting up from first_code[len].  A count is
// clamped into 0..max_count, which a sane bits[] never needs.
template <int LIMIT>
__device__ __forceinline__ void code_starts(const int* bits, int max_count, int* first_pos, uint32_t* first_code) {
  uint32_t code = 0;
  int pos = 0;
  for (int len = 1; len <= LIMIT; ++len) {
    const int n = min(max(bits[len], 0), max_count);
    first_pos[len] = pos, first_code[len] = code;
    pos += n;
    code = (code + (uint32_t)n) << 1;
  }
  first_pos[LIMIT + 1] = pos;
}

// How many of the symbols 0..n-1 come before `sym` of size `size` > 0 in order of (size before the limit, symbol).
__device__ __forceinline__ int symbol_rank(const uint8_t* size_by_symbol, int n, int size, int sym) {
  const int mine = (size << 9) | sym;
  int p = 0;
  for (int i = 0; i < n; ++i) {
    const int other = size_by_symbol[i];
    p += (other > 0 && ((other << 9) | i) < mine) ? 1 : 0;
  }
  return p;
}

// The limited length of the symbol at position p in that order; 0 if bits[] was not sane and has no place for it.
template <int LIMIT>
__device__ __forceinline__ int length_at_rank(const int* first_pos, int p) {
  int length = 0;
  for (int len = 1; len <= LIMIT; ++len)
    if (p >= first_pos[len] && p < first_pos[len + 1]) length = len;
  return length;
}

// `acc` holds the `n` (< 32) bits not yet written of the word `word` points at, most or least significant bit first; the
// first word starts with the bits of whoever wrote before (zeros here: OR leaves them alone).  put() takes up to 27 bits:
// with n < 32 that is at most 58 bits in the 64 of `acc`.
template <bool MSB_FIRST>
struct BitWriter {
  uint32_t* word;
  uint64_t acc = 0;
  uint32_t n;
  bool shared;                  // the word `word` points at may also hold bits of the writer before this one
  __device__ __forceinline__ void put(uint32_t value, uint32_t len) {
    acc = MSB_FIRST ? (acc << len) | value : acc | ((uint64_t)value << n);
    n += len;
    if (n >= 32) {
      n -= 32;
      const uint32_t full = MSB_FIRST ? (uint32_t)(acc >> n) : (uint32_t)acc;
      if (shared) atomicOr(word, full); else *word = full;
      shared = false;
      ++word;
      acc = MSB_FIRST ? acc & ((1ull << n) - 1ull) : acc >> 32;
    }
  }
  __device__ __forceinline__ void finish() {                   // the tail shares its word with the writer after this one
    if (n > 0) atomicOr(word, MSB_FIRST ? (uint32_t)(acc << (32 - n)) : (uint32_t)acc);
  }
};

// ------------------------------------------------------------------------------------------------ host side
inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// The slots, pointers and workspace of an encode call, under the entry point's name `who`, in the order it refuses; sets
// the error and returns FCP_ERR_ARG, or 0.  With f == 0 only the slots are looked at: the call is a no-op.
inline int check_slots(const char* who, int f, bool pointers, int64_t out_stride, int64_t capacity, const void* workspace,
                       int64_t workspace_bytes, size_t need, const char* sizer) {
  FCP_REQUIRE(capacity >= 0 && out_stride >= capacity, "%s: capacity %lld must be >= 0 and fit the stride %lld", who,
              (long long)capacity, (long long)out_stride);
  if (f == 0) return 0;
  FCP_REQUIRE(pointers, "%s: null pointer", who);
  FCP_REQUIRE(workspace_bytes >= (int64_t)need, "%s: workspace of %lld bytes, %s asks for %lld", who, (long long)workspace_bytes,
              sizer, (long long)need);
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  return 0;
}

}  // namespace fcp_entropy
