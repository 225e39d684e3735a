// Ragged INTER_AREA level builder: cv2.resize(src, (dw, dh), interpolation=INTER_AREA) of every level of a batch, read from
// one byte blob (the decoded originals) and written into another, one launch.  Each level is a (sh, sw, 3) uint8 source
// at src_off and a (dh, dw, 3) destination at dst_off; the pixel arithmetic is the batch builder's (fcp_area.h), so a
// level equals cv2.resize byte for byte for integral and non-integral ratios alike.
//
// A thread writes four consecutive pixels of its level's row-major pixel sequence: 12 bytes at a 4-byte aligned offset
// (dst_off % 4 == 0), three dword stores instead of twelve byte stores.  Rows are not aligned, so the four pixels may span
// a row boundary; (x, y) is recomputed per pixel.  Built with -ffp-contract=off.
#include "fcp_area.h"
#include "fcp_common.h"
#include "fcp_hip.h"

namespace {

__global__ void __launch_bounds__(256) resize_area_ragged_kernel(const uint8_t* __restrict__ src,
                                                                 const fcp_area_level* __restrict__ levels,
                                                                 uint8_t* __restrict__ dst) {
  const fcp_area_level lv = levels[blockIdx.y];
  const long npx = (long)lv.dh * lv.dw;
  const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (p0 >= npx) return;
  const uint8_t* S = src + lv.src_off;
  const bool same = lv.sh == lv.dh && lv.sw == lv.dw;   // "Source and destination are of same size. Use simple copy."
  const double scale_x = 1. / ((double)lv.dw / lv.sw), scale_y = 1. / ((double)lv.dh / lv.sh);
  uint8_t px[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) px[q] = 0;
  int y = (int)(p0 / lv.dw), x = (int)(p0 - (long)y * lv.dw);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (p0 + q < npx) {
      if (same) {
        const uint8_t* p = S + ((long)y * lv.sw + x) * 3;
        px[q * 3] = p[0]; px[q * 3 + 1] = p[1]; px[q * 3 + 2] = p[2];
      } else {
        fcp_area::area_pixel(S, lv.sh, lv.sw, scale_x, scale_y, x, y, px + q * 3);
      }
    }
    if (++x == lv.dw) { x = 0; ++y; }
  }
  uint8_t* o = dst + lv.dst_off + p0 * 3;
  if (p0 + 4 <= npx) {
    uint32_t* d32 = reinterpret_cast<uint32_t*>(o);   // 12 bytes at a 4-byte aligned address
    d32[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
    d32[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
    d32[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((uint32_t)px[11] << 24);
  } else {
    for (long q = 0; p0 + q < npx; ++q) { o[q * 3] = px[q * 3]; o[q * 3 + 1] = px[q * 3 + 1]; o[q * 3 + 2] = px[q * 3 + 2]; }
  }
}

}  // namespace

extern "C" int fcp_resize_area_ragged_u8(const uint8_t* src_blob, int64_t src_bytes, const fcp_area_level* levels_host,
                                         const fcp_area_level* levels_dev, int n, uint8_t* dst_blob, int64_t dst_bytes,
                                         fcp_stream_t stream) {
  FCP_REQUIRE(n >= 0 && n <= 65535, "fcp_resize_area_ragged_u8: n=%d levels (0..65535)", n);
  if (n == 0) return 0;
  FCP_REQUIRE(src_blob && levels_host && levels_dev && dst_blob, "fcp_resize_area_ragged_u8: null pointer");
  long most = 0;
  for (int i = 0; i < n; ++i) {
    const fcp_area_level& lv = levels_host[i];
    FCP_REQUIRE(lv.sh > 0 && lv.sw > 0 && lv.dh > 0 && lv.dw > 0, "fcp_resize_area_ragged_u8: level %d is empty", i);
    FCP_REQUIRE(lv.dh <= lv.sh && lv.dw <= lv.sw, "fcp_resize_area_ragged_u8: level %d: INTER_AREA is implemented for "
                "decimation only (%dx%d -> %dx%d)", i, lv.sw, lv.sh, lv.dw, lv.dh);
    FCP_REQUIRE(lv.src_off >= 0 && lv.src_off + (int64_t)lv.sh * lv.sw * 3 <= src_bytes,
                "fcp_resize_area_ragged_u8: level %d: source lies outside the source blob", i);
    FCP_REQUIRE(lv.dst_off >= 0 && (lv.dst_off & 3) == 0 && lv.dst_off + (int64_t)lv.dh * lv.dw * 3 <= dst_bytes,
                "fcp_resize_area_ragged_u8: level %d: destination is unaligned or lies outside the destination blob", i);
    const long npx = (long)lv.dh * lv.dw;
    most = npx > most ? npx : most;
  }
  const long groups = (most + 3) / 4;
  FCP_REQUIRE(groups <= 256L * 0x7fffffffL, "fcp_resize_area_ragged_u8: level too large");
  const dim3 grid(fcp_cdiv(groups, 256), n);
  resize_area_ragged_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(src_blob, levels_dev, dst_blob);
  FCP_LAUNCH_OK();
  return 0;
}
