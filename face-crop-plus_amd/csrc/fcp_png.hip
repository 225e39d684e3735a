// zlib streams of uint8 faces (f,h,w,c), c = 1 (gray), 3 (RGB) or 4 (RGBA), for PNG files, on the device (INTEGRATION.md section
// 2m; the definition is stated once more in tests/png_ref.py, which these kernels are held to byte for byte; the file
// around the stream is pngenc.png_file, on the host).  Six kernels after one memset:
//
//   filter   a workgroup per kRowsPerBlock scanlines, one after the other: the cost sum of min(v, 256 - v) of the five PNG
//            filters by reduction, the cheapest type (the lowest among equals); then the filtered row (type byte first) in
//            rounds of 256 bytes: the row's two Adler sums, the starts of its maximal runs of equal bytes by a scan of the
//            "differs from the byte before" flags -> the run list (byte << 24 | start) in the workspace; then one lane
//            per run counts its tokens into a 286-bin histogram in LDS, which joins the face's with integer atomics (adds
//            commute: the counts do not depend on the order)
//   tables   one wave per face: the code lengths by the merge of fcp_entropy.h over 286 entries, limited to 15 bits,
//            canonical codes bit-reversed for an LSB-first stream, and the block header (fixed code-length code),
//            written to the front of the face's bits
//   count    per row: the bits of its tokens
//   scan     one workgroup per face: exclusive scan of the rows' bits behind the header -> the bit offset of every row
//   emit     per row, one lane per run: the run's bits, shifted to its offset (a scan of the runs' bit counts), into
//            32-bit words; words a run owns alone are stored, the two it may share with its neighbours are OR-ed with
//            ordinary global atomics (OR commutes).  The last row adds the end-of-block code
//   finish   78 01, the bytes of the block, the Adler-32 folded from the rows' sums; every store is checked against the
//            caller's capacity; the true length
//
// A token walk (walk_run) feeds the histogram, the count and emit, as code_block does in fcp_jpeg.hip.
#include "fcp_block_scan.h"
#include "fcp_common.h"
#include "fcp_entropy.h"
#include "fcp_hip.h"

namespace {

using fcp_entropy::kEntries;                  // table entries per lane: 5 * 64 >= 286
using fcp_entropy::kFib35;
using fcp_entropy::round16;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRowsPerBlock = 4;              // scanlines a workgroup takes in turn: one histogram flush for all of them
constexpr int kMaxSide = 8192;
constexpr int kSymbols = 286;                // literals 0..255, end of block, lengths 257..285
constexpr int kBins = 288;                    // stride of a face's counts and codes in the workspace
constexpr int kMaxBits = 15;                  // deflate's limit of a literal/length code
constexpr int kMaxCodeLength = 48;            // the lengths the arrays hold before the limit: counts that sum to less
                                              // than 2^32 < Fibonacci(48) - 1 make no tree deeper than 44
constexpr int kHeaderWords = 64;              // 2048 bits: 17 + 19 * 3 + 287 lengths of at most 5 bits = 1509 at most
constexpr unsigned kAdler = 65521u;

struct RowInfo {
  unsigned long long sum;       // sum of the row's filtered bytes
  unsigned long long wsum;      // sum of position in the row * byte
  uint32_t nruns;               // maximal runs of equal bytes
  uint32_t bits;                // bits of the row's tokens (count kernel)
};

// ------------------------------------------------------------------------------------------------ filter
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// The neighbours of raw byte j of a scanline: left (bpp bytes back), up, up-left; zeros outside the image.
struct Neighbours {
  int x, a, b, c;
};

__device__ __forceinline__ Neighbours neighbours(const uint8_t* cur, const uint8_t* up, int j, int bpp) {
  Neighbours n;
  n.x = cur[j];
  n.a = j >= bpp ? cur[j - bpp] : 0;
  n.b = up ? up[j] : 0;
  n.c = (up && j >= bpp) ? up[j - bpp] : 0;
  return n;
}

__device__ __forceinline__ uint32_t filter_byte(int type, const Neighbours& n) {
  const int p = type == 0 ? 0 : type == 1 ? n.a : type == 2 ? n.b : type == 3 ? (n.a + n.b) >> 1 : paeth(n.a, n.b, n.c);
  return (uint32_t)(n.x - p) & 255u;
}

// Byte i of the filtered row: the type, then the filtered bytes.
__device__ __forceinline__ uint32_t row_byte(int type, const uint8_t* cur, const uint8_t* up, int i, int bpp) {
  return i == 0 ? (uint32_t)type : filter_byte(type, neighbours(cur, up, i - 1, bpp));
}

// ------------------------------------------------------------------------------------------------ tokens
// Match length 3..258 -> its symbol 257..285, the number of extra bits and their value (RFC 1951 section 3.2.5).
__device__ __forceinline__ void length_symbol(int m, int* sym, int* ebits, uint32_t* evalue) {
  const int l = m - 3;
  if (m == 258 || l < 8) {
    *sym = m == 258 ? 285 : 257 + l, *ebits = 0, *evalue = 0u;
    return;
  }
  const int e = 29 - __clz(l);                                 // floor(log2(l)) - 2: 1..5
  *sym = 261 + 4 * e + ((l >> e) & 3), *ebits = e, *evalue = (uint32_t)l & ((1u << e) - 1u);
}

// The tokens of a maximal run of n equal bytes: n literals when n < 4, else one literal and matches at distance 1 over
// the other n - 1 bytes, 258 at a time as long as at least 3 bytes stay behind.  sink.literal(byte, count) once,
// sink.match(length) per match.  What a token costs or looks like is the sink's business.
template <typename Sink>
__device__ __forceinline__ void walk_run(uint32_t byte, int n, Sink& sink) {
  if (n < 4) {
    sink.literal(byte, n);
    return;
  }
  sink.literal(byte, 1);
  int rem = n - 1;
  while (rem > 258) {
    const int m = rem - 258 >= 3 ? 258 : rem - 3;
    sink.match(m);
    rem -= m;
  }
  sink.match(rem);
}

// Run r of a row's list (byte << 24 | start): its byte and its length, which ends where the next run starts.
__device__ __forceinline__ void run_of(const uint32_t* row_runs, uint32_t r, uint32_t nruns, int len, uint32_t* byte, int* n) {
  const uint32_t e = row_runs[r];
  const int start = (int)(e & 0xffffffu), next = r + 1 < nruns ? (int)(row_runs[r + 1] & 0xffffffu) : len;
  *byte = e >> 24, *n = next - start;
}

struct HistSink {
  uint32_t* bins;               // [kBins], LDS
  __device__ __forceinline__ void literal(uint32_t byte, int count) { atomicAdd(bins + (byte & 255u), (uint32_t)count); }
  __device__ __forceinline__ void match(int m) {
    int sym, ebits;
    uint32_t evalue;
    length_symbol(m, &sym, &ebits, &evalue);
    atomicAdd(bins + min(sym, kSymbols - 1), 1u);
  }
};

// tab: reversed code | length << 16 by symbol.  A match costs its length code, the extra bits and the one distance bit.
struct CountSink {
  const uint32_t* tab;
  uint32_t bits = 0;
  __device__ __forceinline__ void literal(uint32_t byte, int count) { bits += (uint32_t)count * (tab[byte & 255u] >> 16); }
  __device__ __forceinline__ void match(int m) {
    int sym, ebits;
    uint32_t evalue;
    length_symbol(m, &sym, &ebits, &evalue);
    bits += (tab[sym] >> 16) + (uint32_t)ebits + 1u;
  }
};

// Bits go out least significant first; put() takes up to 21 bits (a 15-bit code, 5 extra bits, the distance bit).
struct BitSink : fcp_entropy::BitWriter<false> {
  const uint32_t* tab;
  __device__ __forceinline__ void literal(uint32_t byte, int count) {
    const uint32_t e = tab[byte & 255u];
    for (int k = 0; k < count; ++k) put(e & 0xffffu, e >> 16);
  }
  __device__ __forceinline__ void match(int m) {
    int sym, ebits;
    uint32_t evalue;
    length_symbol(m, &sym, &ebits, &evalue);
    const uint32_t e = tab[sym], len = e >> 16;
    put((e & 0xffffu) | (evalue << len), len + (uint32_t)ebits + 1u);      // the distance code is the bit 0 on top
  }
};

// runs (f, h, len) u32: the run list of every row, len = w * c + 1 entries at most.  hist (f, kBins), zeroed by the
// caller's memset: += the token counts of this workgroup's rows (the end-of-block symbol is the table kernel's).
__global__ void __launch_bounds__(kThreads) png_filter_kernel(const uint8_t* __restrict__ pixels, int h, int w, int c,
                                                              uint32_t* runs, RowInfo* __restrict__ rows,
                                                              uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[kBins];
  __shared__ uint32_t scratch32[kWaves];
  __shared__ unsigned long long scratch64[kWaves];
  const int wc = w * c, len = wc + 1;
  const size_t face = blockIdx.y;
  const uint8_t* face_px = pixels + face * (size_t)h * wc;
  for (int i = threadIdx.x; i < kBins; i += kThreads) bins[i] = 0;
  __syncthreads();
  for (int k = 0; k < kRowsPerBlock; ++k) {                    // uniform over the workgroup: every lane reaches the barriers
    const int y = blockIdx.x * kRowsPerBlock + k;
    if (y >= h) break;
    const uint8_t* cur = face_px + (size_t)y * wc;
    const uint8_t* up = y > 0 ? cur - wc : nullptr;
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < wc; j += kThreads) {
      const Neighbours nb = neighbours(cur, up, j, c);
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const uint32_t v = filter_byte(t, nb);
        cost[t] += v < 128u ? v : 256u - v;
      }
    }
    int type = 0;
    uint32_t best = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const uint32_t total = fcp_block_sum<kThreads>(cost[t], scratch32);
      if (t == 0 || total < best) best = total, type = t;      // ties go to the lowest type
    }
    uint32_t* row_runs = runs + (face * h + y) * (size_t)len;
    uint32_t nruns = 0;
    unsigned long long sum = 0, wsum = 0;
    for (int base = 0; base < len; base += kThreads) {
      const int i = base + threadIdx.x;
      uint32_t v = 0, flag = 0;
      if (i < len) {
        v = row_byte(type, cur, up, i, c);
        flag = (i == 0 || row_byte(type, cur, up, i - 1, c) != v) ? 1u : 0u;
        sum += v, wsum += (unsigned long long)i * v;
      }
      uint32_t total;
      const uint32_t excl = fcp_block_exclusive_scan<kThreads>(flag, scratch32, &total);
      if (flag) row_runs[nruns + excl] = (v << 24) | (uint32_t)i;      // nruns + excl <= i < len
      nruns += total;
    }
    sum = fcp_block_sum<kThreads>(sum, scratch64);
    wsum = fcp_block_sum<kThreads>(wsum, scratch64);                         // its barriers also publish the run list to the workgroup
    HistSink sink;
    sink.bins = bins;
    for (uint32_t r = threadIdx.x; r < nruns; r += kThreads) {
      uint32_t byte;
      int n;
      run_of(row_runs, r, nruns, len, &byte, &n);
      walk_run(byte, n, sink);
    }
    if (threadIdx.x == 0) {
      RowInfo info;
      info.sum = sum, info.wsum = wsum, info.nruns = nruns, info.bits = 0;
      rows[face * h + y] = info;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSymbols; i += kThreads)
    if (bins[i] != 0u) atomicAdd(hist + face * kBins + i, bins[i]);
}

// ------------------------------------------------------------------------------------------------ tables
// The fixed code-length code: 4 bits for the symbols 0, 4..13, 15, 17, 18, 5 bits for 1, 2, 3, 14, none for 16 (Kraft:
// 14/16 + 4/32 = 1); canonical, so the 4-bit codes count up in symbol order from 0 and the 5-bit ones from 28.
__device__ __forceinline__ uint32_t clen_length(int s) { return (s == 1 || s == 2 || s == 3 || s == 14) ? 5u : (s == 16 ? 0u : 4u); }

__device__ __forceinline__ uint32_t clen_code_reversed(int s) {
  const uint32_t code = s == 0 ? 0u : (s >= 4 && s <= 13) ? (uint32_t)(s - 3) : s == 15 ? 11u : s == 17 ? 12u : s == 18 ? 13u
                        : s == 14 ? 31u : (uint32_t)(27 + s);
  return __brev(code) >> (32 - clen_length(s));
}

// A bit writer into LDS words, least significant bit first, for the one lane that writes the header.
struct HeaderWriter {
  uint32_t* words;
  uint32_t nbits = 0;
  __device__ __forceinline__ void put(uint32_t value, uint32_t len) {
    if (nbits + len > kHeaderWords * 32) return;               // cannot happen (1509 bits at most); never past the array
    const uint32_t k = nbits >> 5, sh = nbits & 31u;
    words[k] |= value << sh;
    if (sh + len > 32) words[k + 1] |= value >> (32 - sh);
    nbits += len;
  }
  __device__ __forceinline__ void clen(int s) { put(clen_code_reversed(s), clen_length(s)); }
};

// Code lengths of a row of 286 frequencies, one wave per row, out of the pieces of fcp_entropy.h: the merge (no
// pseudo-symbol here); libjpeg's bits[] adjustment down to 15; the limited lengths to the symbols in order of (length
// before the limit, symbol); then the canonical codes of RFC 1951 section 3.2.2 from those lengths, bit-reversed.  Fewer
// than two non-zero frequencies make no tree: every length is 0.  count_eob: the row's entry 256 is taken as 1 (the encoder's
// histogram does not count the end-of-block symbol).  lengths (n,286) u8 or null; codes (n,code_stride) u32 or null:
// reversed code | length << 16, zeros from 286 on.  raw != null: the block header of face t goes to the front of its
// raw_words words (zeroed before) and its length in bits to header_bits[t].
// Precondition (a row sums to less than 2^32, so that no merged count wraps) is the caller's; if it does not hold the
// codes are meaningless but every index below is clamped into its array.
__global__ void __launch_bounds__(64) png_tables_kernel(const uint32_t* __restrict__ freq, int freq_stride, int count_eob,
                                                        uint8_t* __restrict__ lengths, uint32_t* __restrict__ codes,
                                                        int code_stride, uint32_t* __restrict__ raw, size_t raw_words,
                                                        uint32_t* __restrict__ header_bits) {
  __shared__ int bits[kMaxCodeLength + 1];
  __shared__ uint8_t size_by_symbol[kEntries * 64];
  __shared__ uint8_t length_by_symbol[kEntries * 64];
  __shared__ int first_pos[kMaxBits + 2];
  __shared__ uint32_t first_code[kMaxBits + 1];
  __shared__ uint32_t header[kHeaderWords];
  __shared__ uint32_t header_len;
  const int lane = threadIdx.x;
  const size_t t = blockIdx.x;
  uint32_t fr[kEntries];
  int cs[kEntries];
#pragma unroll
  for (int j = 0; j < kEntries; ++j) {
    const int idx = lane + 64 * j;
    fr[j] = idx < kSymbols ? freq[t * freq_stride + idx] : 0u;
    if (count_eob && idx == 256) fr[j] = 1u;
  }
  if (lane <= kMaxCodeLength) bits[lane] = 0;
  for (int i = lane; i < kHeaderWords; i += 64) header[i] = 0u;
  fcp_entropy::huffman_code_sizes(fr, kSymbols, cs);
#pragma unroll
  for (int j = 0; j < kEntries; ++j) cs[j] = (lane + 64 * j < kSymbols) ? min(cs[j], kMaxCodeLength) : 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kEntries; ++j) {
    if (cs[j] > 0) atomicAdd(&bits[cs[j]], 1);
    size_by_symbol[lane + 64 * j] = (uint8_t)cs[j];
    length_by_symbol[lane + 64 * j] = 0;
  }
  __syncthreads();
  if (lane == 0) {
    fcp_entropy::limit_code_lengths<kMaxCodeLength, kMaxBits>(bits);
    fcp_entropy::code_starts<kMaxBits>(bits, kSymbols, first_pos, first_code);
  }
  __syncthreads();
  // the limited lengths go to the symbols in order of (code size before the limit, symbol)
#pragma unroll
  for (int j = 0; j < kEntries; ++j) {
    if (cs[j] == 0) continue;
    const int sym = lane + 64 * j, p = fcp_entropy::symbol_rank(size_by_symbol, kSymbols, cs[j], sym);
    length_by_symbol[sym] = (uint8_t)fcp_entropy::length_at_rank<kMaxBits>(first_pos, p);
  }
  __syncthreads();
  // canonical codes: among the symbols of one length, in symbol order
#pragma unroll
  for (int j = 0; j < kEntries; ++j) {
    const int sym = lane + 64 * j;
    const uint32_t len = length_by_symbol[sym];
    uint32_t entry = 0u;
    if (len > 0u) {
      uint32_t before = 0;
      for (int i = 0; i < sym; ++i) before += length_by_symbol[i] == len ? 1u : 0u;
      entry = ((__brev(first_code[len] + before) >> (32 - len)) & 0xffffu) | (len << 16);
    }
    if (codes && sym < code_stride) codes[t * code_stride + sym] = sym < kSymbols ? entry : 0u;
    if (lengths && sym < kSymbols) lengths[t * kSymbols + sym] = (uint8_t)len;
  }
  if (raw == nullptr) return;                                             // uniform: the same for every lane
  if (lane == 0) {
    int last = kSymbols - 1;
    while (last > 256 && length_by_symbol[last] == 0) --last;
    const int nlit = last + 1;                                            // HLIT + 257: 257..286
    HeaderWriter hw;
    hw.words = header;
    hw.put(1u, 1);                                                        // BFINAL
    hw.put(2u, 2);                                                        // BTYPE: dynamic Huffman codes
    hw.put((uint32_t)(nlit - 257), 5);
    hw.put(0u, 5);                                                        // HDIST: one distance code
    hw.put(15u, 4);                                                       // HCLEN: all 19 lengths of the code-length code
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int k = 0; k < 19; ++k) hw.put(clen_length(order[k]), 3);
    // the literal/length lengths, then the one distance length (1), as one sequence; entry nlit is that 1
    int i = 0;
    while (i <= nlit) {
      const int v = i < nlit ? (int)length_by_symbol[i] : 1;
      if (v != 0) {
        hw.clen(v);
        ++i;
        continue;
      }
      int j = i;
      while (j < nlit && length_by_symbol[j] == 0) ++j;
      int n = j - i;
      while (n >= 11) {
        const int k = min(n, 138);
        hw.clen(18);
        hw.put((uint32_t)(k - 11), 7);
        n -= k;
      }
      if (n >= 3) {
        hw.clen(17);
        hw.put((uint32_t)(n - 3), 3);
      } else {
        for (int k = 0; k < n; ++k) hw.clen(0);
      }
      i = j;
    }
    header_len = hw.nbits;
  }
  __syncthreads();
  const uint32_t nbits = header_len;
  for (uint32_t k = lane; k < (nbits + 31u) / 32u; k += 64) raw[t * raw_words + k] = header[k];
  if (lane == 0) header_bits[t] = nbits;
}

// ------------------------------------------------------------------------------------------------ count, scan, emit
__global__ void __launch_bounds__(kThreads) png_count_kernel(const uint32_t* __restrict__ runs, int h, int len,
                                                             const uint32_t* __restrict__ codes, RowInfo* __restrict__ rows) {
  __shared__ uint32_t tab[kBins];
  __shared__ uint32_t scratch32[kWaves];
  const size_t face = blockIdx.y;
  for (int i = threadIdx.x; i < kBins; i += kThreads) tab[i] = codes[face * kBins + i];
  __syncthreads();
  for (int k = 0; k < kRowsPerBlock; ++k) {
    const int y = blockIdx.x * kRowsPerBlock + k;
    if (y >= h) break;
    const uint32_t* row_runs = runs + (face * h + y) * (size_t)len;
    const uint32_t nruns = min(rows[face * h + y].nruns, (uint32_t)len);
    CountSink sink;
    sink.tab = tab;
    for (uint32_t r = threadIdx.x; r < nruns; r += kThreads) {
      uint32_t byte;
      int n;
      run_of(row_runs, r, nruns, len, &byte, &n);
      walk_run(byte, n, sink);
    }
    const uint32_t total = fcp_block_sum<kThreads>(sink.bits, scratch32);
    if (threadIdx.x == 0) rows[face * h + y].bits = total;
  }
}

// bitoff (f, h + 1): where every row's bits start, behind the header; entry h is where the end-of-block code goes.
__global__ void __launch_bounds__(kThreads) png_scan_kernel(const RowInfo* __restrict__ rows, int h,
                                                            const uint32_t* __restrict__ header_bits,
                                                            uint32_t* __restrict__ bitoff) {
  __shared__ uint32_t wave_sums[kWaves];
  const size_t face = blockIdx.x;
  uint32_t* off = bitoff + face * (h + 1);
  uint32_t carry = header_bits[face];
  for (int base = 0; base < h; base += kThreads) {             // uniform trip count: every lane reaches the barriers
    const int y = base + threadIdx.x;
    const uint32_t v = y < h ? rows[face * h + y].bits : 0u;
    uint32_t total;
    const uint32_t excl = fcp_block_exclusive_scan<kThreads>(v, wave_sums, &total);
    if (y < h) off[y] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) off[h] = carry;
}

__global__ void __launch_bounds__(kThreads) png_emit_kernel(const uint32_t* __restrict__ runs, int h, int len,
                                                            const uint32_t* __restrict__ codes,
                                                            const RowInfo* __restrict__ rows,
                                                            const uint32_t* __restrict__ bitoff, uint32_t* __restrict__ raw,
                                                            size_t raw_words) {
  __shared__ uint32_t tab[kBins];
  __shared__ uint32_t wave_sums[kWaves];
  const size_t face = blockIdx.y;
  for (int i = threadIdx.x; i < kBins; i += kThreads) tab[i] = codes[face * kBins + i];
  __syncthreads();
  uint32_t* face_raw = raw + face * raw_words;
  const uint32_t* off = bitoff + face * (h + 1);
  for (int k = 0; k < kRowsPerBlock; ++k) {
    const int y = blockIdx.x * kRowsPerBlock + k;
    if (y >= h) break;
    const uint32_t* row_runs = runs + (face * h + y) * (size_t)len;
    const uint32_t nruns = min(rows[face * h + y].nruns, (uint32_t)len);
    uint32_t carry = off[y];
    for (uint32_t base = 0; base < nruns; base += kThreads) {  // uniform trip count: every lane reaches the barriers
      const uint32_t r = base + threadIdx.x;
      uint32_t byte = 0;
      int n = 0;
      CountSink count;
      count.tab = tab;
      if (r < nruns) {
        run_of(row_runs, r, nruns, len, &byte, &n);
        walk_run(byte, n, count);
      }
      uint32_t total;
      const uint32_t start = carry + fcp_block_exclusive_scan<kThreads>(count.bits, wave_sums, &total);
      if (r < nruns) {
        BitSink sink;
        sink.tab = tab;
        sink.word = face_raw + (start >> 5);
        sink.n = start & 31u;
        sink.shared = true;                                    // its first word may hold bits of the run, or the header, before it
        walk_run(byte, n, sink);
        sink.finish();
      }
      carry += total;
    }
    if (y == h - 1 && threadIdx.x == 0) {                      // the end-of-block code, behind the last row
      BitSink sink;
      sink.tab = tab;
      sink.word = face_raw + (off[h] >> 5);
      sink.n = off[h] & 31u;
      sink.shared = true;
      sink.put(tab[256] & 0xffffu, tab[256] >> 16);
      sink.finish();
    }
  }
}

// ------------------------------------------------------------------------------------------------ finish
// Workgroup x of face y copies bytes [4096 x, 4096 x + 4096) of the block behind the two header bytes; workgroup 0 also
// writes those, folds the Adler-32 and stores the length.  Adler-32 of the N filtered bytes d_i: A = 1 + sum d_i,
// B = N + sum (N - i) d_i, both mod 65521; with i = row * len + position that is, per row, (N - row * len) * sum - wsum.
__global__ void __launch_bounds__(kThreads) png_finish_kernel(const uint32_t* __restrict__ raw, size_t raw_words, int h, int len,
                                                              const RowInfo* __restrict__ rows,
                                                              const uint32_t* __restrict__ bitoff,
                                                              const uint32_t* __restrict__ codes, uint8_t* __restrict__ out,
                                                              long long out_stride, long long capacity,
                                                              int32_t* __restrict__ lengths) {
  __shared__ unsigned long long scratch64[kWaves];
  const size_t face = blockIdx.y;
  const uint32_t nbits = bitoff[face * (h + 1) + h] + (codes[face * kBins + 256] >> 16);
  const uint32_t nbytes = (nbits + 7u) >> 3;                   // the last byte's upper bits are the zeros of the memset
  uint8_t* dst = out + face * out_stride;
  const size_t first = ((size_t)blockIdx.x * kThreads + threadIdx.x) * 16;
  if (first < nbytes) {                                        // first + 16 <= 4 * raw_words: raw_words is a multiple of 4
    const uint4 v = reinterpret_cast<const uint4*>(raw + face * raw_words)[first >> 4];
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long long p = 2 + (long long)first + j;
      if (first + j < nbytes && p < capacity) dst[p] = (uint8_t)(words[j >> 2] >> (8 * (j & 3)));
    }
  }
  if (blockIdx.x != 0) return;                                 // uniform over the workgroup
  const unsigned long long total = (unsigned long long)h * len;
  unsigned long long a = 0, b = 0;
  for (int y = threadIdx.x; y < h; y += kThreads) {
    const RowInfo info = rows[face * h + y];
    a += info.sum % kAdler;
    b += ((total - (unsigned long long)y * len) % kAdler) * (info.sum % kAdler) % kAdler + kAdler - info.wsum % kAdler;
  }
  a = fcp_block_sum<kThreads>(a, scratch64);
  b = fcp_block_sum<kThreads>(b, scratch64);
  if (threadIdx.x == 0) {
    const uint32_t adler = (uint32_t)(((total + b) % kAdler) << 16) | (uint32_t)((1ull + a) % kAdler);
    const long long end = 2 + (long long)nbytes;
    if (0 < capacity) dst[0] = 0x78;
    if (1 < capacity) dst[1] = 0x01;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (end + j < capacity) dst[end + j] = (uint8_t)(adler >> (24 - 8 * j));
    lengths[face] = (int32_t)(end + 4);
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct Layout {
  int len;                      // bytes of a filtered row
  size_t raw_words;             // per face, a multiple of 4: the finish pass reads 16 bytes at a time
  size_t run_bytes, row_bytes, off_bytes, code_bytes, header_bytes, raw_bytes, hist_bytes;
  size_t total() const { return run_bytes + row_bytes + off_bytes + code_bytes + header_bytes + raw_bytes + hist_bytes; }
};

Layout layout_of(int f, int h, int w, int c) {
  Layout l;
  l.len = w * c + 1;
  const size_t bytes = (size_t)h * l.len;                      // filtered bytes of a face: at most one 15-bit code each
  l.raw_words = ((kHeaderWords * 32 + (bytes + 1) * kMaxBits + 31) / 32 + 3) & ~(size_t)3;
  l.run_bytes = round16((size_t)f * bytes * sizeof(uint32_t));
  l.row_bytes = round16((size_t)f * h * sizeof(RowInfo));
  l.off_bytes = round16((size_t)f * (h + 1) * sizeof(uint32_t));
  l.code_bytes = round16((size_t)f * kBins * sizeof(uint32_t));
  l.header_bytes = round16((size_t)f * sizeof(uint32_t));
  l.raw_bytes = (size_t)f * l.raw_words * sizeof(uint32_t);
  l.hist_bytes = (size_t)f * kBins * sizeof(uint32_t);         // right behind the bits: one memset zeroes both
  return l;
}

int check_sizes(int f, int h, int w, int channels) {
  FCP_REQUIRE(f >= 0 && h >= 1 && w >= 1, "png_encode: bad sizes (f %d, h %d, w %d)", f, h, w);
  FCP_REQUIRE(channels == 1 || channels == 3 || channels == 4, "png_encode: 1 (gray), 3 (RGB) or 4 (RGBA) channels, not %d",
              channels);
  FCP_REQUIRE(h <= kMaxSide && w <= kMaxSide, "png_encode: faces of at most %d x %d px (got h %d, w %d)", kMaxSide, kMaxSide, h,
              w);
  const long long symbols = (long long)h * ((long long)w * channels + 1) + 1;
  FCP_REQUIRE(symbols < kFib35 - 1,
              "png_encode: a face needs h * (w * channels + 1) + 1 < %lld, h %d, w %d has %lld (a deeper Huffman tree than "
              "32 levels would be possible)", kFib35 - 1, h, w, symbols);
  FCP_REQUIRE(f <= 65535, "png_encode: at most 65535 faces per call");
  return 0;
}

}  // namespace

extern "C" int64_t fcp_png_workspace_bytes(int f, int h, int w, int channels) {
  if (check_sizes(f, h, w, channels) != 0) return -1;
  return (int64_t)layout_of(f, h, w, channels).total();
}

extern "C" int fcp_png_encode_u8(const uint8_t* pixels, int f, int h, int w, int channels, uint8_t* out, int64_t out_stride,
                                 int64_t capacity, int32_t* lengths, void* workspace, int64_t workspace_bytes,
                                 fcp_stream_t stream) {
  if (check_sizes(f, h, w, channels) != 0) return FCP_ERR_ARG;
  const Layout l = layout_of(f, h, w, channels);
  if (int rc = fcp_entropy::check_slots("png_encode", f, pixels && lengths && workspace && (out || capacity == 0), out_stride,
                                        capacity, workspace, workspace_bytes, l.total(), "fcp_png_workspace_bytes"))
    return rc;
  if (f == 0) return 0;

  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* runs = reinterpret_cast<uint32_t*>(ws);
  RowInfo* rows = reinterpret_cast<RowInfo*>(ws += l.run_bytes);
  uint32_t* bitoff = reinterpret_cast<uint32_t*>(ws += l.row_bytes);
  uint32_t* codes = reinterpret_cast<uint32_t*>(ws += l.off_bytes);
  uint32_t* header_bits = reinterpret_cast<uint32_t*>(ws += l.code_bytes);
  uint32_t* raw = reinterpret_cast<uint32_t*>(ws += l.header_bytes);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws += l.raw_bytes);
  hipStream_t s = (hipStream_t)stream;
  FCP_HIP_OK(hipMemsetAsync(raw, 0, l.raw_bytes + l.hist_bytes, s));
  const dim3 per_rows(fcp_cdiv(h, kRowsPerBlock), f);
  hipLaunchKernelGGL(png_filter_kernel, per_rows, dim3(kThreads), 0, s, pixels, h, w, channels, runs, rows, hist);
  hipLaunchKernelGGL(png_tables_kernel, dim3(f), dim3(64), 0, s, hist, kBins, 1, (uint8_t*)nullptr, codes, kBins, raw, l.raw_words,
                     header_bits);
  hipLaunchKernelGGL(png_count_kernel, per_rows, dim3(kThreads), 0, s, runs, h, l.len, codes, rows);
  hipLaunchKernelGGL(png_scan_kernel, dim3(f), dim3(kThreads), 0, s, rows, h, header_bits, bitoff);
  hipLaunchKernelGGL(png_emit_kernel, per_rows, dim3(kThreads), 0, s, runs, h, l.len, codes, rows, bitoff, raw, l.raw_words);
  hipLaunchKernelGGL(png_finish_kernel, dim3(fcp_cdiv((long)(l.raw_words * 4), 16 * kThreads), f), dim3(kThreads), 0, s, raw,
                     l.raw_words, h, l.len, rows, bitoff, codes, out, (long long)out_stride, (long long)capacity, lengths);
  FCP_LAUNCH_OK();
  return 0;
}

extern "C" int fcp_png_huffman_lengths(const uint32_t* freq, int n, uint8_t* lengths, uint32_t* codes, fcp_stream_t stream) {
  FCP_REQUIRE(n >= 0 && n <= 65535, "png_huffman_lengths: 0..65535 rows, not %d", n);
  if (n == 0) return 0;
  FCP_REQUIRE(freq && lengths, "png_huffman_lengths: null pointer");
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(freq) & 3) == 0 && (reinterpret_cast<uintptr_t>(codes) & 3) == 0,
              "png_huffman_lengths: freq and codes must be 4-byte aligned");
  hipLaunchKernelGGL(png_tables_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, freq, kSymbols, 0, lengths, codes, kSymbols,
                     (uint32_t*)nullptr, (size_t)0, (uint32_t*)nullptr);
  FCP_LAUNCH_OK();
  return 0;
}
