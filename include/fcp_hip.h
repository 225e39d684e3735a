/*
 * fcp_hip.h — C ABI of the MI355X (gfx950) hot path of face-crop-plus.
 *
 * The reference (mantasu/face-crop-plus) is pure Python: it has no FFI layer.
 * Its seam for this path is the object protocol `Cropper` uses on its three
 * models plus `crop_align`.  This header is the native side of
 * that seam: stateless entry points, plain pointers and sizes, every pointer a
 * *device* pointer unless the name ends in `_host`.  All work is enqueued on
 * the caller's HIP stream (`stream` is a hipStream_t passed as void*); nothing
 * synchronises, nothing allocates, nothing keeps global state except the
 * thread-local last-error string.  Every function returns 0 on success and a
 * negative code on misuse (message via fcp_last_error()).
 *
 * Each entry point cites the reference code it replaces (paths relative to
 * src/face_crop_plus/ of the reference tree).
 */
#ifndef FCP_HIP_H
#define FCP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCP_ABI_VERSION 15

typedef void* fcp_stream_t; /* hipStream_t */

int fcp_abi_version(void);
const char* fcp_last_error(void);

/* ------------------------------------------------------------------------
 * Convolution engine (NHWC fp32 tensors, implicit GEMM on the matrix cores).
 * Two arithmetic modes, chosen per filter at pack time (`precision`):
 *   0  exact fp32:  v_mfma_f32_32x32x2_f32, bit-for-bit an fmaf chain;
 *   1  fp16x3 split: every operand x = hi + lo (two binary16), product expanded as
 *      ah*bh + ah*bl + al*bh on v_mfma_f32_32x32x16_f16 with fp32 accumulation:
 *      ~2^-20 relative error per product (fp32-roundoff class) at 5.3x the matrix rate.
 *      Filter rows are pre-scaled by a power of two (`wscale` undoes it exactly).
 * Replaces every nn.Conv2d(+BatchNorm eval)(+ReLU/LeakyReLU)(+residual) the
 * three networks dispatch to ATen: models/_layers.py:64-162 (SSH/FPN/Head),
 * :168-200 (RRDB blocks), :206-368 (BiSeNet blocks), torchvision ResNet-50
 * body (models/retinaface.py:93-99).
 *
 * Tensor layout: activations are NHWC fp32.  `in`/`out`/`res*` may point into
 * a wider buffer: `*_ld` is the channel stride (floats per pixel) of that
 * buffer and the pointer is already offset to the first channel used.  This
 * is how torch.cat (SSH, dense blocks, FFM) is realised with no copy.
 *
 * Filter layout (produced by the host packer, see engine.py pack_conv):
 *   normal mode : [cout_pad][cin/32][kh][kw][32]     cin % 32 == 0 (taps of one 32-channel
 *                                                    slice are consecutive in K: L2 locality)
 *   cin4 mode   : [cout_pad][kh][8][4]               cin <= 4, kw <= 8
 * precision 0 stores fp32; precision 1 stores, for every 32 consecutive K values of a
 * row, 32 binary16 hi parts followed by 32 binary16 lo parts (same 128 bytes).
 * cout_pad = cout rounded up to a multiple of 128 (whatever N tile a launch uses);
 * the padding rows are zero.  BatchNorm (eval) is folded into w and bias.
 *
 * Epilogue (fp32, in this order):
 *   v = acc * wscale[co] + bias[co]        (wscale = 1 for precision 0)
 *   if (res1 && res1_pre)  v += res1[...]
 *   v = v >= 0 ? v : v * act_slope        (act_slope = 1 -> identity, 0 -> ReLU)
 *   v = v * alpha
 *   if (res1 && !res1_pre) v += res1[...]
 *   if (res2)              v = v * alpha2 + res2[...]
 * res1 may have a different spatial size (res1_h,res1_w): it is then read with
 * PyTorch's nearest rule  src = min(floor(dst * (float)src_size/dst_size), src_size-1)
 * (FPN top-down add, _layers.py:137-143).  res2 always has the output's size.
 * ------------------------------------------------------------------------ */
typedef struct fcp_conv_desc {
  const float* in;    /* (n, in_h_phys, in_w_phys, in_ld) */
  const void* w;      /* packed filter */
  const float* bias;  /* [cout] or NULL */
  float* out;         /* (n, out_h, out_w, out_ld) */
  const float* res1;  /* or NULL */
  const float* res2;  /* or NULL */
  const float* wscale; /* [cout] power-of-two filter scales (precision 1) or NULL */
  const float* in2;   /* optional second source of a 1x1 conv (see in2_* below) or NULL */
  int32_t n, in_h, in_w; /* logical input size (after the optional x2 upsample) */
  int32_t cin, in_ld;
  int32_t in_up2;     /* 1: physical input is (in_h/2, in_w/2), read at (h>>1, w>>1)
                         = F.interpolate(scale_factor=2 / exact-2x size, "nearest")
                         (rrdb.py:78-79, _layers.py:338,:343) */
  int32_t cout, kh, kw, stride, pad;
  int32_t out_h, out_w, out_ld;
  int32_t tile_n;     /* N tile: 32, 64 or 128 (128, 192 or 256 with tile_m = 256); filters are padded to 128 rows */
  int32_t cin4;       /* 1: cin4 mode */
  float act_slope, alpha, alpha2;
  int32_t res1_pre, res1_ld, res1_h, res1_w, res2_ld;
  int32_t precision;  /* 0 = fp32 exact, 1 = fp16x3 split (filter packed accordingly) */
  /* Activation tensor formats (precision 1 only): 0 = fp32 NHWC; 1 = "split32": same bytes per
   * element and the same strides, but every group of 32 channels of a pixel is stored as 32 binary16
   * hi parts followed by 32 binary16 lo parts (value = hi + lo, ~22 significant bits).  A K slice of
   * a split32 tensor is byte-for-byte the kernel's LDS operand image, so the consumer conv copies it
   * instead of converting; producers convert once in their epilogue.  Views must start on a
   * 32-channel group and in_ld / out_ld / res*_ld must be multiples of 32. */
  int32_t in_fmt, out_fmt, res1_fmt, res2_fmt;
  int32_t tile_m;     /* 0 / 128: 128-row workgroup tiles; 256: the 256-row, 8-wave kernel (precision 1,
                         split32 input, no cin4 / in_up2; tile_n 128, 192 or 256); 1: the halo-tile kernels
                         for 3x3 / stride 1 / pad 1 convs (8 x 32 pixel patches, precision 1, split32 input,
                         cin >= 64, cout % 8 == 0, wscale / bias 16-byte aligned, |out view| < 4 GiB):
                         tile_n 32 = one pass per 32 filters, cout <= 64; tile_n 64 / 128 = the wide form
                         (column tiles inner, filters through a tap ring): cin % 64 == 0, cout <= 64, or
                         cout <= 128 without residual inputs */
  /* Two-source 1x1 conv (K concatenation): the trailing cin2 of the cin input channels come from
   * in2, a split32 tensor (n, in2_h, in2_w, in2_ld) sampled at (ho*in2_stride, wo*in2_stride); the
   * leading cin - cin2 channels come from `in` as usual.  This is how a ResNet bottleneck's
   * bn3(conv3(o)) + bn_d(downsample(x)) runs as one convolution over [o | x(::s, ::s)] without ever
   * materialising the downsampled identity.  Needs kh = kw = 1, pad 0, precision 1, split32 `in`. */
  int32_t cin2, in2_ld, in2_h, in2_w, in2_stride;
  /* FCP_CONV_FLAT_ADDR (precision 0 only): use 64-bit flat addressing even when every tensor is below
   * 4 GiB.  The flat path is what tensors >= 4 GiB take on their own (RRDB's x4-resolution tail at 1024^2
   * inputs); the flag exists so that it can be exercised — and tested — at small sizes. */
  int32_t flags;
  /* FCP_CONV_BALANCE_TAIL (256-row tiles, tile_m = 256): cut the rows of the last, partial dispatch round into
   * shorter M-tiles that together occupy every CU (instead of 256-row tiles on a fraction of them).  `cu_budget` =
   * CUs the launch may count on (0 = all of the device; a caller that runs two such launches concurrently on two
   * streams passes half).  Neither changes a result. */
  int32_t cu_budget;
  /* Row bands (stride 1): the input view holds band_top real rows above and band_bottom real rows below the rows the
   * output view covers (0 <= each <= pad), instead of the zero padding a conv applies at the edge of its view:
   *     out_h = in_h - band_top - band_bottom + 2 pad - kh + 1,    input row of (output row ho, tap kh_i) = ho - pad + band_top + kh_i.
   * This is how a caller computes rows [a, b) of a larger image's convolution exactly: `in` = rows [a - band_top, b + band_bottom)
   * with band_top = 0 only at the image's top edge (where the zero padding is the right one).  RRDB's dense blocks run
   * band-major this way (rrdb.py: conv1..conv5 of a block on one row band before the next band, the growing concat
   * staying in the memory-side cache; _layers.py:168-200 of the reference).  Same arithmetic per output pixel: bit-identical to
   * the whole-image launch.  Both 0: the ordinary convolution. */
  int32_t band_top, band_bottom;
} fcp_conv_desc;

#define FCP_CONV_FLAT_ADDR 1
#define FCP_CONV_BALANCE_TAIL 2

int fcp_conv2d_nhwc_f32(const fcp_conv_desc* desc, fcp_stream_t stream);

/* ------------------------------------------------------------------------
 * Fused bottleneck chain (precision 1, split32 tensors): conv2 of ResNet block b, conv3 of block b
 * with the identity residual, and conv1 of block b + 1, in ONE launch:
 *     t2  = relu(conv2_3x3(t1) * ws2 + b2)                   c  -> c    (stays in LDS)
 *     out = relu(conv3_1x1(t2) * ws3 + b3 + res)             c  -> 4c   (written once)
 *     t1n = relu(conv1n_1x1(out) * ws1n + b1n)               4c -> cn
 * Replaces torchvision's Bottleneck.forward (the ResNet-50 body retinaface.py:93-99 wraps) from conv2 of one
 * identity block to conv1 of the next: the 4c-channel tensor crosses HBM twice (residual read, result write)
 * instead of four times and the c-channel intermediate never leaves the workgroup.  Results are bit-identical
 * to three fcp_conv2d_nhwc_f32 launches.  Filters are ordinary precision-1 packs (pack_conv): w2
 * [128][9c] (3x3 / stride 1 / pad 1), w3 [4c][c], w1n [cn padded to 128][4c]; BatchNorm folded, so every conv
 * has a bias and a per-filter scale.  All tensors are split32 views (n, h, w, *_ld), 128-byte aligned,
 * *_ld % 32 == 0.  Supported: c = 64 (ResNet-50 layer 1), nout = 256, cn = 64 or 128.
 *
 * Pair forms (w2 == NULL: no conv2, t1 is conv3's input itself, c = 128 or 256 channels):
 *     out = relu(conv3_1x1(t1) * ws3 + b3 [+ res])    c -> nout;     t1n = relu(conv1n_1x1(out) * ws1n + b1n)    nout -> cn
 *   c = 128, nout = 512,  res != NULL, cn = 128   conv3 of a layer-2 identity block + conv1 of the next block
 *   c = 128, nout = 512,  res != NULL, cn = 256   layer 2's last block + layer3.0.conv1
 *   c = 256, nout = 1024, res != NULL, cn = 256   conv3 of a layer-3 identity block + conv1 of the next block
 *   c = 128, nout = 256,  res == NULL, cn = 64    layer1.0: conv3 + downsample as one K-concatenated 1x1 conv over
 *                                                 [conv2 out | pooled stem] (engine.py packs it so), + layer1.1.conv1
 *   c = 384, nout = 512,  res == NULL, cn = 128,  t1b != NULL, cb = 256 (round 5)
 *                                                 layer2.0: conv3 + the 1x1 / 2 downsample as one K-concatenated conv over the TWO
 *                                                 sources [conv2 out (t1: 128 ch) | x(::2, ::2) (t1b: 256 ch at twice the
 *                                                 resolution)], + layer2.1.conv1: the 512-channel block output is written once
 *                                                 and not read back by a separate conv1 launch.  The operand fragments are
 *                                                 loaded straight from the two tensors (no LDS tile).
 *   c = 256, nout = 1024, res != NULL, cn = 0,    w1n == ws1n == b1n == t1n == NULL (round 5): the EXPAND form — conv3 + identity of
 *                                                 a layer-3 block alone, out = relu(conv3(t1) * ws3 + b3 + res), no conv1';
 *                                                 fragments from global memory, two workgroups per CU; bit-identical to
 *                                                 fcp_conv2d_nhwc_f32 with the fused residual epilogue (a tie with it and with the
 *                                                 pair in the A/B: opt-in).
 * ------------------------------------------------------------------------ */
typedef struct fcp_chain_desc {
  const float* t1;    /* conv2's input: c channels */
  const void* w2;  const float* ws2;  const float* b2;
  const void* w3;  const float* ws3;  const float* b3;
  const float* res;   /* identity branch x: 4c channels */
  float* out;         /* 4c channels */
  const void* w1n; const float* ws1n; const float* b1n;
  float* t1n;         /* cn channels */
  const float* t1b;   /* two-source pair form: the trailing cb of conv3's c input channels come from this split32 tensor
                       * (n, t1b_h, t1b_w, t1b_ld), sampled at (y * t1b_stride, x * t1b_stride); t1 holds the leading c - cb.
                       * NULL: one source */
  int32_t n, h, w, c, cn;
  int32_t t1_ld, res_ld, out_ld, t1n_ld;
  int32_t nout;       /* conv3's filters: 4c with conv2; see the pair forms below */
  int32_t tile_m;     /* a hint the library may ignore (0, 128, 16, 256 and 32 are accepted; same bits whichever is given):
                       * the form is chosen by shape — the conv2 forms run on 4-wave tiles that are 8 x 16 pixel patches
                       * of one image, conv2's operand staged once per channel slice as the patch's halo; the pair forms
                       * on 4-wave tiles of 128 consecutive pixels */
  int32_t flags;      /* FCP_CHAIN_OUT_EVEN_ONLY (conv2 forms only): `out` is stored at pixels with even y AND
                       * even x only — for a block whose output is read by nothing but a stride-2 consumer (ResNet-50's
                       * layer1.2: the next block's 1x1 / 2 downsample reads `out`, its conv1 is t1n, computed here): three
                       * quarters of the tensor are never written nor read.  The other pixels of the buffer keep whatever
                       * they held.  t1n is complete either way. */
  int32_t cb, t1b_ld, t1b_h, t1b_w, t1b_stride;   /* geometry of t1b (all 0 without it) */
} fcp_chain_desc;
#define FCP_CHAIN_OUT_EVEN_ONLY 1

int fcp_bottleneck_chain_f16x3(const fcp_chain_desc* desc, fcp_stream_t stream);

/* uint8 NHWC RGB (n,h,w,3) -> fp32 NHWC4 (n,h,w,4): out[c] = (in[c]-sub[c])/div, out[3]=0.
 * Replaces utils.py:222-224 (as_tensor) fused with retinaface.py:450-451 (mean
 * subtraction; the BGR swap is folded into the stem filter's channel order) or
 * with rrdb.py:142 (`.div(255)`).  sub_host: 3 floats on the host.  `in` may have any
 * byte alignment (an image of a uint8 batch whose h*w is not a multiple of 4 starts
 * mid-word; 4-byte aligned inputs take a dword-load path); `out` must be 16-byte aligned. */
int fcp_u8_to_nhwc4_f32(const uint8_t* in, float* out, int64_t npix,
                        const float* sub_host, float div, fcp_stream_t stream);

/* Same, from the reference API's float tensor: fp32 NCHW (n,3,h,w) -> fp32 NHWC4
 * (RetinaFace.predict / RRDBNet.predict take float NCHW, retinaface.py:411, rrdb.py:84). */
int fcp_f32nchw_to_nhwc4_f32(const float* in, float* out, int n, int h, int w,
                             const float* sub_host, float div, fcp_stream_t stream);

/* MaxPool2d(kernel 3, stride 2, pad 1) on NHWC fp32 (torchvision ResNet stem,
 * _layers.py:247).  c % 4 == 0.  The input is dense (c elements per pixel); the output may be a
 * channel slice of a wider buffer (out_ld elements per pixel, out_ld >= c). */
int fcp_maxpool3x3s2_nhwc_f32(const float* in, float* out, int n, int h, int w, int c, int out_ld,
                              int out_h, int out_w, fcp_stream_t stream);
/* Same on split32 tensors (c, out_ld % 32 == 0); the maximum is exact (hi + lo decodes exactly). */
int fcp_maxpool3x3s2_split32(const float* in, float* out, int n, int h, int w, int c, int out_ld,
                             int out_h, int out_w, fcp_stream_t stream);
/* RetinaFace stem in one launch (precision 1): uint8 RGB image -> (x - mean_rgb) -> 7x7 / stride 2 / pad 3
 * conv to 64 channels (BatchNorm folded into wfrag / bias) -> ReLU -> MaxPool2d(3, 2, 1), written as a 64-channel
 * slice (out_ld elements per pixel) of an fp32 (out_fmt 0) or split32 (1) NHWC tensor of size
 * (n, hp, wp) with hs = (h-1)/2+1, hp = (hs-1)/2+1.  Replaces retinaface.py:450-451 + the torchvision ResNet
 * stem (conv1, bn1, relu, maxpool; retinaface.py:93-99).  x - mean is integral, hence exact in binary16: the
 * fp16x3 product needs only a*wh + a*wl.  wfrag: the filter split hi / lo in MFMA fragment order
 * [2 column tiles][11 k-steps][hi, lo][64 lanes][8 binary16], K index = kh*24 + kw*3 + c (RGB), zero-padded
 * (engine.py::pack_stem_fused); wscale: the per-filter power-of-two scale.  mean_rgb: 3 integers in 0..255 (host). */
int fcp_stem7x7s2_relu_pool_u8(const uint8_t* images, int n, int h, int w, const int32_t* mean_rgb,
                               const void* wfrag, const float* bias, const float* wscale, float* out,
                               int out_ld, int out_fmt, fcp_stream_t stream);
/* The same launch continued by conv1 of the first bottleneck (torchvision Bottleneck.forward: relu(bn1(conv1(x))),
 * a 1x1 conv 64 -> 64 on the pooled map; retinaface.py:93-99): t1 = relu(conv1x1(pooled) * ws1 + b1), written as a
 * split32 tensor (n, hp, wp, t1_ld).  The pooled map is still written (the block's downsample branch reads it) but not
 * read back: its hi / lo bytes are conv1's operand while they are still in LDS.  w1: the conv's packed precision-1
 * filter (engine.py::pack_conv: >= 64 rows of [2 channel slices][32 hi | 32 lo binary16]); out_fmt must be 1.  Same K
 * and term order as fcp_conv2d_nhwc_f32 on the stored map: bit-identical to the two launches.  w1 == NULL: the plain stem. */
int fcp_stem7x7s2_relu_pool_conv1_u8(const uint8_t* images, int n, int h, int w, const int32_t* mean_rgb,
                                     const void* wfrag, const float* bias, const float* wscale, float* out,
                                     int out_ld, int out_fmt, const void* w1, const float* ws1, const float* b1,
                                     float* t1, int t1_ld, fcp_stream_t stream);
/* The same stem on an fp32 NHWC4 input (n, h, w, 4; channel 3 ignored) that is already normalised: BiSeNet's ResNet-18 stem
 * (conv1 7x7 / 2 + bn1 + relu + maxpool 3x3 / 2; bise.py:387-393 feeds it, _layers.py:241-247 is the stem).  The input has a lo part,
 * so the patch is staged as hi + lo binary16 planes and a k-step is the full three-term product (al*wh + ah*wl + ah*wh).  wfrag /
 * bias / wscale: engine.py::pack_stem_fused (no channel permutation).  The 256 x 256 x 64 stem map of a 512 x 512 face (537 MB for 32
 * faces) never reaches HBM. */
int fcp_stem7x7s2_relu_pool_f32(const float* x4, int n, int h, int w, const void* wfrag, const float* bias,
                                const float* wscale, float* out, int out_ld, int out_fmt, fcp_stream_t stream);
/* Format converters between fp32 NHWC and split32 (npix pixels of c channels, c % 32 == 0). */
int fcp_f32_to_split32(const float* in, float* out, int64_t npix, int c, fcp_stream_t stream);
int fcp_split32_to_f32(const float* in, float* out, int64_t npix, int c, fcp_stream_t stream);
/* Range guard of the fp16x3 path (no reference counterpart: the reference computes in fp32, _layers.py:16-35 hands it
 * arbitrary checkpoints): *out_max = max(*out_max, max |x|) over a channel-slice view of npix pixels x c channels
 * (pixel pitch ld elements; fmt 0 fp32 / 1 split32; c % 8 == 0), NaN counted as +inf.  *out_max must be initialised
 * (>= 0) by the caller; the update is an atomic max on the device. */
int fcp_absmax_nhwc(const float* x, int64_t npix, int c, int ld, int fmt, float* out_max, fcp_stream_t stream);

/* ------------------------------------------------------------------------
 * RetinaFace post-processing.
 * ------------------------------------------------------------------------ */

/* Fused softmax + analytic PriorBox + decode + strict threshold + ordered
 * compaction.  Replaces retinaface.py:144 (softmax), _layers.py:41-62
 * (PriorBox), retinaface.py:169-178/:204-210/:455-461 (decode + scale) and
 * retinaface.py:264-267 (score > vis mask + gather).
 *
 * head[l]: fused head conv output of pyramid level l (stride 8/16/32), NHWC
 * with 32 channels per pixel: [cls a0(bg,face) a1(bg,face) | box a0(4) a1(4) |
 * landm a0(10) a1(10)]; level sizes are ceil(h/stride) x ceil(w/stride).
 * Outputs (per image, capacity P = total priors, candidates in ascending
 * prior order): cand_score (n,P), cand_box (n,P,4), cand_ldm (n,P,10),
 * cand_prior (n,P) int32, cand_count (n) int32.
 * dense_* are optional (NULL to skip): full (n,P) / (n,P,4) / (n,P,10). */
int fcp_retina_decode(const float* head0, const float* head1, const float* head2,
                      int n, int img_h, int img_w, float vis_threshold,
                      float var0, float var1,
                      float* cand_score, float* cand_box, float* cand_ldm,
                      int32_t* cand_prior, int32_t* cand_count,
                      float* dense_score, float* dense_box, float* dense_ldm,
                      fcp_stream_t stream);

/* Per-image sort (score desc, candidate position asc) + greedy NMS with the
 * reference's +1-pixel IoU and `ovr <= nms_threshold` survival rule
 * (retinaface.py:270-298), followed by take_by_strategy (retinaface.py:363-408).
 * strategy: 0 = all, 1 = best, 2 = largest.
 * workspace: fcp_retina_nms_workspace_bytes(n, cap) bytes (sort keys + sorted
 * boxes; above 507904 candidates per image also the greedy pass's alive bitmap,
 * which otherwise lives in LDS), cap = candidate capacity (stride of the cand_*
 * arrays, <= 2^26; the prior count of the frame when fed by fcp_retina_decode;
 * cand_count is clamped to it).  Outputs: keep_pos (n,cap) int32 = candidate positions of
 * the kept boxes in keep order, keep_count (n); sel_pos (n,cap) / sel_count (n)
 * = the positions take_by_strategy selects (for "all" identical to keep). */
int64_t fcp_retina_nms_workspace_bytes(int n, int cap);
int fcp_retina_nms_select(const float* cand_score, const float* cand_box,
                          const int32_t* cand_count, int n, int cap,
                          float nms_threshold, int strategy, void* workspace,
                          int32_t* keep_pos, int32_t* keep_count,
                          int32_t* sel_pos, int32_t* sel_count, fcp_stream_t stream);

/* Gather the selected faces into dense, image-major arrays (the return value
 * of RetinaFace.predict, retinaface.py:465-470, minus the D2H copy) and apply
 * the landmark un-padding of cropper.py:822 (paddings (n,4) int32 t,b,l,r or NULL).
 * face_offset: (n+1) int32 exclusive prefix of sel_count (written here;
 * face_offset[n] = number of faces).  out_ldm (max_faces,5,2) f32, out_img
 * (max_faces) int32: rows >= face_offset[n] are zeroed here (no memset needed). */
int fcp_retina_gather_faces(const float* cand_ldm, const int32_t* sel_pos,
                            const int32_t* sel_count, int n, int cap,
                            const int32_t* paddings, int max_faces,
                            int32_t* face_offset, float* out_ldm, int32_t* out_img,
                            fcp_stream_t stream);

/* ------------------------------------------------------------------------
 * Align + crop.
 * ------------------------------------------------------------------------ */

/* Least-squares 2x3 transform from 5 (or k) source points to target points:
 * similarity (4 dof) = cv2.estimateAffinePartial2D, full affine (6 dof) =
 * cv2.estimateAffine2D, both with ransacReprojThreshold=inf (cropper.py:515-527).
 * src (f,k,2) f32, dst (k,2) f32 -> mat (f,6) f64 row-major, ok (f) int32
 * (0 = degenerate / non-finite: the reference drops that face, cropper.py:529-531). */
int fcp_estimate_transform(const float* src, const float* dst, int f, int k,
                           int allow_skew, double* mat, int32_t* ok, fcp_stream_t stream);

/* The same for a fixed-capacity face array whose live length is on the device
 * (the detector's face_offset[n]; RetinaFace.predict's `len(landmarks)`,
 * retinaface.py:465-470): rows >= *face_count (device int32, or NULL = all f)
 * get ok = 0 and a zero matrix, and the number of faces with ok = 1 — the faces
 * crop_align keeps, cropper.py:529-531 — is ADDED to *valid_total (device
 * int64 accumulator, or NULL).  No host read-back, no extra launches. */
int fcp_estimate_transform_counted(const float* src, const float* dst, int f, int k,
                                   int allow_skew, const int32_t* face_count,
                                   double* mat, int32_t* ok, int64_t* valid_total,
                                   fcp_stream_t stream);

/* cv2.warpAffine(image, M, dsize, flags=INTER_LINEAR, borderMode) on the
 * un-padded slice of each face's batch image (cropper.py:533-547): OpenCV's
 * fixed-point algorithm (AB_BITS=10, INTER_BITS=5, 15-bit weights).
 * images (n,h,w,3) u8; img_idx (f) int32; mat (f,6) f64 forward transforms;
 * paddings (n,4) int32 (t,b,l,r) or NULL; border: 0 constant(0), 1 replicate,
 * 2 reflect, 3 wrap, 4 reflect_101 (= cv2.BORDER_*); out (f,out_h,out_w,3) u8.
 * h and w are at most 32767 (source coordinates saturate to short, as in
 * cv::warpAffine); larger batches fail with a message, like the ragged entry
 * points below.  `images` (`blob` for the ragged entry points) and `out` are
 * expected 4-byte aligned: the interior taps are read and whole groups of four
 * output pixels are written as aligned dwords.  This holds for every warp below.
 * A matrix with ok == NULL (or ok = 1) is used as it is: a singular one inverts
 * to all zeros, and in this family and the cubic / Lanczos-4 warps a non-finite
 * coefficient goes through cvRound (INT_MIN) and int32 wrap-around exactly as in
 * cv::warpAffine, so the result is defined. */
int fcp_warp_affine_u8(const uint8_t* images, int n, int h, int w,
                       const int32_t* img_idx, const double* mat, const int32_t* ok,
                       const int32_t* paddings, int f, int out_h, int out_w, int border,
                       uint8_t* out, fcp_stream_t stream);

/* The same warp in the float32 family of cv::warpAffine(INTER_LINEAR), the SIMD
 * linear warp newer OpenCV builds run instead of the fixed-point tables; same
 * parameters, argument checks, un-padding and borders as fcp_warp_affine_u8.
 * The inverse map is computed in double as above, then each coefficient is
 * rounded to float.  Per output pixel (x,y), every step a separately rounded
 * float32 operation in this order (no FMA):
 *   sx = x*m0 + (y*m1 + m2),  sy = x*m3 + (y*m4 + m5);
 *   ix = floor(sx), ax = sx - ix (likewise iy, ay); ix, iy clamped to
 *   [-32768, 32767] in float, then converted: they select the taps and the
 *   all-outside test of the constant border (a constant-border tap reads 0);
 *   v0 = p00 + ax*(p01 - p00), v1 = p10 + ax*(p11 - p10), v = v0 + ay*(v1 - v0);
 *   out = round-half-even(v) saturated to 0..255.
 * The result of this family is unspecified for a matrix with a non-finite
 * coefficient (float-to-int conversion of NaN); the pipeline never passes one
 * with ok = 1, fcp_estimate_transform clears ok for such a face. */
int fcp_warp_affine_u8_float(const uint8_t* images, int n, int h, int w,
                             const int32_t* img_idx, const double* mat, const int32_t* ok,
                             const int32_t* paddings, int f, int out_h, int out_w, int border,
                             uint8_t* out, fcp_stream_t stream);

/* The same two warps with one source image per face, anywhere in one byte
 * blob: crop_source="original", which crops from the decoded files (or from
 * power-of-two INTER_AREA levels of them, fcp_resize_area_ragged_u8) instead of
 * the resized batch.  Face i samples the (h,w,3) uint8 image at byte `off` of
 * `blob` (blob_bytes bytes); borders act at that image's edge; the matrix
 * inversion and the per-pixel arithmetic are those of fcp_warp_affine_u8 /
 * fcp_warp_affine_u8_float.  srcs_host is validated here (each image inside the
 * blob, 1..32767 px a side); srcs_dev is the caller's device copy of the same
 * table.  mat (f,6) f64, ok (f) int32 or NULL, out (f,out_h,out_w,3) u8. */
typedef struct fcp_warp_src {
  int64_t off;        /* byte offset of the image inside the blob */
  int32_t h, w;       /* image height, width */
} fcp_warp_src;

int fcp_warp_affine_u8_ragged(const uint8_t* blob, int64_t blob_bytes,
                              const fcp_warp_src* srcs_host, const fcp_warp_src* srcs_dev,
                              const double* mat, const int32_t* ok, int f, int out_h, int out_w,
                              int border, uint8_t* out, fcp_stream_t stream);
int fcp_warp_affine_u8_float_ragged(const uint8_t* blob, int64_t blob_bytes,
                                    const fcp_warp_src* srcs_host, const fcp_warp_src* srcs_dev,
                                    const double* mat, const int32_t* ok, int f, int out_h,
                                    int out_w, int border, uint8_t* out, fcp_stream_t stream);

/* cv2.warpAffine(image, M, dsize, flags=interp, borderMode) with interp a
 * cv2.INTER_* code: 2 = INTER_CUBIC (4 x 4 taps), 4 = INTER_LANCZOS4 (8 x 8);
 * any other value fails with a message.  Parameters, argument checks,
 * un-padding and borders as fcp_warp_affine_u8 / fcp_warp_affine_u8_ragged.
 * OpenCV's fixed-point remap: the coordinates of the linear warp (AB_BITS=10,
 * INTER_BITS=5, sx0 = X >> 5), taps from sx0 - 1 (cubic) or sx0 - 3 (Lanczos)
 * on, int16 weights of initInterTab2D (sum 32768), int32 sums,
 * out = (sum + 16384) >> 15 saturated to 0..255. */
int fcp_warp_affine_u8_interp(const uint8_t* images, int n, int h, int w,
                              const int32_t* img_idx, const double* mat, const int32_t* ok,
                              const int32_t* paddings, int f, int out_h, int out_w, int border,
                              int interp, uint8_t* out, fcp_stream_t stream);
int fcp_warp_affine_u8_interp_ragged(const uint8_t* blob, int64_t blob_bytes,
                                     const fcp_warp_src* srcs_host, const fcp_warp_src* srcs_dev,
                                     const double* mat, const int32_t* ok, int f, int out_h,
                                     int out_w, int border, int interp, uint8_t* out,
                                     fcp_stream_t stream);

/* The fixed-point weight table those warps use, on the host (no device
 * needed): 1024 * K * K int16 in [fy * 32 + fx][k1][k2] order, K = 4 for
 * interp 2, 8 for interp 4. */
int fcp_warp_interp_weights(int interp, int16_t* out);

/* Sharpness of crops (f,h,w,3) uint8 RGB: the integer sums behind
 * cv2.Laplacian(cv2.cvtColor(crop, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var()
 * (INTEGRATION.md 2e).  g = (9798 R + 19235 G + 3735 B + 16384) >> 15;
 * L = g(y-1,x) + g(y+1,x) + g(y,x-1) + g(y,x+1) - 4 g(y,x) with
 * BORDER_REFLECT_101 (a dimension of size 1 maps every neighbour to index 0);
 * sums[i] = {S1 = sum L, S2 = sum L*L} over crop i, exact.  The variance is
 * (N S2 - S1^2) / N^2 with N = h*w, left to the host.  sums (f,2) is zeroed on
 * the stream first; crops with ok[i] == 0 are skipped (their sums stay 0), ok
 * may be NULL.  One launch.  f == 0 is a no-op; h < 1, w < 1, w > 8192,
 * h > 1048576 or f > 65535 fail with a message. */
int fcp_crop_sharpness_u8(const uint8_t* crops, int f, int h, int w, const int32_t* ok,
                          int64_t* sums, fcp_stream_t stream);

/* Baseline JPEG encoding of crops (f,h,w,channels) uint8, channels 3 (RGB,
 * 4:2:0 chroma) or 1 (gray), on the device: for face i the
 * entropy-coded segment and the EOI marker, i.e. every byte libjpeg-turbo's
 * default compressor (integer DCT, standard Huffman tables, no restart
 * markers, no optimisation) writes after the SOS header at this quality, go
 * to out + i * out_stride.  lengths[i] is the TRUE length of that stream even
 * when it exceeds capacity; then only its first capacity bytes are written
 * and the caller encodes the face some other way.  Nothing is written at or
 * past out + i * out_stride + capacity, every byte below
 * min(lengths[i], capacity) is written (out need not be zeroed).
 * A stream can be larger than the pixels: a block costs at most
 * 20 + 63 * 26 = 1658 bits (DC: 9-bit code + 11 bits; 63 AC: 16-bit code +
 * 10 bits), twice that after FF -> FF 00 stuffing, so 416 bytes per 8x8 block
 * (6 blocks per 16x16 MCU with 3 channels) plus 2 for EOI always suffice.
 * quality 1..100 (the IJG scale, baseline tables); subsampling must be 2
 * (4:2:0; it is ignored for gray), 0 (4:4:4) and 1 (4:2:2) are refused.
 * workspace: fcp_jpeg_workspace_bytes(f,h,w,channels) bytes of device memory,
 * 16-byte aligned, contents irrelevant (coefficients, bit offsets, the
 * unstuffed bits: 128 + 4 + 208 bytes per block at most).
 * One memset and four launches; the result does not depend on the order in
 * which anything runs.  f == 0 is a no-op; h, w < 1 or > 8192, f > 65535,
 * channels other than 1 / 3, capacity < 0 or > out_stride fail with a message
 * (fcp_jpeg_workspace_bytes then returns -1). */
int64_t fcp_jpeg_workspace_bytes(int f, int h, int w, int channels);
int fcp_jpeg_encode_u8(const uint8_t* crops, int f, int h, int w, int channels, int quality, int subsampling,
                       uint8_t* out, int64_t out_stride, int64_t capacity, int32_t* lengths,
                       void* workspace, int64_t workspace_bytes, fcp_stream_t stream);

/* The same encoder with the caller's chroma subsampling and, optionally,
 * Huffman tables made for every face: byte for byte what
 * libjpeg-turbo writes after the SOS header with these settings (Pillow's
 * subsampling= and optimize=).  fcp_jpeg_encode_u8 is this call with
 * subsampling 2 and optimize 0; everything said there about out, lengths,
 * capacity and quality holds here.
 * subsampling: 0 is 4:4:4, 1 is 4:2:2, 2 is 4:2:0; ignored for gray.  An MCU
 * is hs * vs Y blocks row by row (1x1, 2x1, 2x2), then Cb, then Cr; Y
 * positions past the block grid are dummy blocks (a zero DC difference and an
 * end-of-block).  Chroma samples: positions past the image repeat the last
 * row / column of the full-resolution plane before any averaging; 4:4:4 takes
 * the pixel's own Cb / Cr; 4:2:2 takes (c(y,2x) + c(y,2x+1) + bias) >> 1 with
 * bias 0 in even and 1 in odd output columns (libjpeg's h2v1_downsample);
 * 4:2:0 is the 2x2 average with bias 1, 2.
 * optimize: 0 codes with the standard tables; `tables` may be NULL and is not
 * touched.  1 codes every face with the tables libjpeg's optimize_coding
 * makes for it (see fcp_jpeg_huffman_tables) and writes them to `tables`,
 * (f,4,272) bytes: per face four records in the order Y DC, Y AC, chroma DC,
 * chroma AC, each 16 counts of codes per length 1..16 followed by up to 256
 * symbols in code order, zero padded.  Every byte of every record is written;
 * for gray, records 2 and 3 are zeros.  The host builds the face's DHT
 * segments from them (jpegenc.jpeg_header).
 * With optimised tables a DC code may be 16 bits long as well, so a block
 * costs at most 27 + 63 * 26 = 1665 bits, 417 bytes after stuffing.
 * workspace: fcp_jpeg_workspace_bytes_ex(f,h,w,channels,subsampling,optimize)
 * bytes, 16-byte aligned; with optimize 0 and subsampling 2 that is
 * fcp_jpeg_workspace_bytes; with optimize 1 the unstuffed bits are sized for
 * 1665 bits a block and 2 x 4096 bytes per face (symbol counts, code tables)
 * are added.
 * One memset and four launches, six with optimize (a histogram and a table
 * launch); no host round trip, one stream, nothing allocated, the same bytes
 * from run to run; nothing is written outside out[i][0..capacity), lengths,
 * tables and the workspace.
 * Refused with a message, before any HIP call: everything fcp_jpeg_encode_u8
 * refuses; a subsampling outside 0..2; an optimize other than 0 / 1; optimize
 * with a null tables; a face whose blocks times the worst case of a block
 * (1658 bits, 1665 with optimize) exceed 2^32 - 1, the range of the bit
 * offsets (4:4:4 at 8192 x 8192 does, 4:2:2 and 4:2:0 do not); with optimize,
 * a face with 64 * blocks + 1 >= 9 227 465, the 35th Fibonacci number: below
 * it no Huffman tree is deeper than 32, the limit of libjpeg's own arrays
 * (about 144 000 blocks: 4:2:0 crops up to 2048 x 2048, 4:4:4 up to about
 * 1750 x 1750).  fcp_jpeg_workspace_bytes_ex then returns -1. */
int64_t fcp_jpeg_workspace_bytes_ex(int f, int h, int w, int channels, int subsampling, int optimize);
int fcp_jpeg_encode_ex_u8(const uint8_t* crops, int f, int h, int w, int channels, int quality,
                          int subsampling, int optimize,
                          uint8_t* out, int64_t out_stride, int64_t capacity, int32_t* lengths,
                          uint8_t* tables, void* workspace, int64_t workspace_bytes, fcp_stream_t stream);

/* libjpeg's jpeg_gen_optimal_table for n rows of 256 symbol frequencies
 * (device memory, 4-byte aligned), one wave per row: a pseudo-symbol 256 of
 * frequency 1 joins the row (it keeps the all-ones code free); while two
 * non-zero entries are left, c1 is the entry with the smallest non-zero
 * frequency, the LARGEST index among equals, c2 the same search without c1;
 * freq[c1] += freq[c2], freq[c2] = 0, and the code size of every symbol under
 * c1 and under c2 grows by one, c2's symbols joining c1's.  bits[len] counts
 * the symbols of each size up to 32; for i from 32 down to 17, while
 * bits[i] > 0: j = i - 2 stepping down while bits[j] == 0, bits[i] -= 2,
 * bits[i-1] += 1, bits[j+1] += 2, bits[j] -= 1; one code is taken from the
 * longest non-empty length (the pseudo-symbol's).  Symbols are ordered by
 * code size (before the limit), then by value, and get the canonical codes of
 * the limited lengths in that order.
 * tables (n,272): row i's record as described above.  codes (n,256), or NULL:
 * code | length << 16 by symbol, 0 for a symbol without a code.  A row of
 * zeros gives a record (and codes) of zeros.
 * Precondition: a row sums to less than 9 227 464, so that no code size
 * exceeds 32 (fcp_jpeg_encode_ex_u8 guarantees it by its refusal); beyond it
 * the tables mean nothing, but nothing outside tables and codes is written.
 * One launch.  n == 0 is a no-op; n < 0 or > 262140, a null freq / tables or
 * a misaligned freq / codes fail with a message, before any HIP call. */
int fcp_jpeg_huffman_tables(const uint32_t* freq, int n, uint8_t* tables, uint32_t* codes, fcp_stream_t stream);

/* zlib streams for PNG files of faces (f,h,w,channels) uint8, channels 3 (RGB),
 * 4 (RGBA) or 1 (gray), on the device (where the stream is defined;
 * tests/png_ref.py states it in Python): face i's stream, 78 01, one dynamic
 * Huffman block, Adler-32, goes to out + i * out_stride; the host wraps it
 * into a file (pngenc.png_file).  Every scanline takes the PNG filter 0..4
 * with the smallest sum of min(v, 256 - v) over its filtered bytes (the
 * lowest type among equals); per filtered row, type byte included, a maximal
 * run of n equal bytes is n literals when n < 4, else one literal and matches
 * at distance 1 over the other n - 1 bytes (258 while at least 3 stay behind,
 * else all but 3, then the rest); the literal/length code is that of
 * fcp_png_huffman_lengths over the token counts with the end-of-block symbol
 * counted once; there is one distance code (code 0, length 1) and a fixed
 * code-length code.  The streams inflate to the filtered rows, i.e. the files
 * decode to exactly the pixels; they are NOT the bytes zlib would write.
 * lengths[i] is the TRUE length of the stream even when it exceeds capacity;
 * then only its first capacity bytes are written and the caller encodes the
 * face some other way.  Nothing is written at or past out + i * out_stride +
 * capacity, every byte below min(lengths[i], capacity) is written (out need
 * not be zeroed).  h * (w * channels + 1) + 1024 bytes hold any stream whose
 * codes average 9 bits or less; 15 bits a byte plus 270 bytes always do.
 * workspace: fcp_png_workspace_bytes(f,h,w,channels) bytes of device memory,
 * 16-byte aligned, contents irrelevant (per filtered byte 4 bytes of run list
 * and 15 bits of stream; per row 24 + 4 bytes; per face 2.5 KiB).
 * One memset and six launches; no host round trip, one stream, nothing
 * allocated, the same bytes from run to run.  f == 0 is a no-op.  Refused with
 * a message, before any HIP call: h, w < 1 or > 8192, f < 0 or > 65535,
 * channels other than 1 / 3 / 4, capacity < 0 or > out_stride, a null pointer, a
 * workspace too small or not 16-byte aligned, and a face with
 * h * (w * channels + 1) + 1 >= 9 227 464 (one below the 35th Fibonacci
 * number: below it no Huffman tree is deeper than 32, the range of the
 * lengths before the limit; about 1750 x 1750 RGB, 1500 x 1500 RGBA).  fcp_png_workspace_bytes
 * then returns -1. */
int64_t fcp_png_workspace_bytes(int f, int h, int w, int channels);
int fcp_png_encode_u8(const uint8_t* pixels, int f, int h, int w, int channels,
                      uint8_t* out, int64_t out_stride, int64_t capacity, int32_t* lengths,
                      void* workspace, int64_t workspace_bytes, fcp_stream_t stream);

/* Deflate code lengths of n rows of 286 literal/length frequencies (device
 * memory, 4-byte aligned), one wave per row: the merge of
 * fcp_jpeg_huffman_tables without its pseudo-symbol (while two non-zero
 * entries are left: c1 the smallest non-zero frequency, the LARGEST index
 * among equals, c2 the same search without c1; freq[c1] += freq[c2],
 * freq[c2] = 0, every symbol under c1 and c2 grows by one bit); the same
 * bits[] adjustment, down to 15 bits; the limited lengths go to the symbols in
 * order of (length before the limit, symbol).  lengths (n,286) uint8.  codes
 * (n,286), or NULL: bit-reversed canonical code (RFC 1951 3.2.2) | length << 16
 * by symbol, 0 for a symbol without a code.  A row with fewer than two
 * non-zero entries has no tree: all of its lengths are 0.
 * Precondition: a row sums to less than 2^32 (no tree over such counts is
 * deeper than 44; the lengths before the limit may reach 48); beyond it the
 * lengths mean nothing, but nothing outside lengths and codes is written.
 * One launch.  n == 0 is a no-op; n < 0 or > 65535, a null freq / lengths or a
 * misaligned freq / codes fail with a message, before any HIP call. */
int fcp_png_huffman_lengths(const uint32_t* freq, int n, uint8_t* lengths, uint32_t* codes, fcp_stream_t stream);

/* Background replacement of crops (f,h,w,3) uint8 RGB from label maps
 * (f,h,w) uint8, in integers throughout:
 *   m     = 255 where the label is below 32 and that bit of class_bits is
 *           set, else 0 (labels 19..255 are background);
 *   alpha = m for feather 0, else the separable fixed-point Gaussian of m
 *           with OpenCV's 8.8 taps for ksize = feather (3: 64,128,64;
 *           5: 16,64,96,64,16; 7: 8,28,56,72,56,28,8): a horizontal pass H
 *           (at most 65280, no rounding), a vertical pass and one rounding
 *           (sum + 32768) >> 16, BORDER_REFLECT_101 iterated until the index
 *           is inside (a dimension of size 1 maps everything to index 0):
 *           cv2.GaussianBlur(m, (feather, feather), 0) restated;
 *   out   = (c * alpha + bg * (255 - alpha) + 127) / 255 per channel, bg =
 *           (bg_r, bg_g, bg_b): round to nearest, there are no ties.
 * out (f,h,w,3) and alpha (f,h,w) are written once, by ordinary stores;
 * alpha may be NULL.  out MAY BE crops (in place): an output pixel depends
 * on its own crop pixel and on labels only.  labels must not overlap out or
 * alpha.  The three arrays may start at any byte; nothing outside them is
 * written.  One launch, no workspace, the same bytes from run to run.
 * f == 0 is a no-op; f < 0, h or w < 1 or > 8192, f > 65535, a feather other
 * than 0 / 3 / 5 / 7, a fill component outside 0..255, a bit of class_bits at
 * or above 19, or (f > 0) a null crops / labels / out fail with a message,
 * before any HIP call. */
int fcp_matte_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather,
                 int bg_r, int bg_g, int bg_b, uint8_t* out, uint8_t* alpha, fcp_stream_t stream);

/* Background blur of crops (f,h,w,3) uint8 RGB from label maps (f,h,w)
 * uint8, in integers throughout: the subject keeps the
 * crop, what is behind it becomes a mask-normalised Gaussian of the
 * background pixels alone.  m and alpha are exactly those of fcp_matte_u8
 * for class_bits and feather; b = 1 where m == 0, else 0;
 *   taps  = t[0..radius] on the HOST, each >= 1, t[0] + 2 sum(t[1..radius])
 *           == 4096, 3 <= radius <= 48 (matte.blur_taps makes them from a
 *           sigma; they travel in the kernel argument block);
 *   D     = sum_j sum_i t|j| t|i| b(y+j, x+i) over the positions inside the
 *           image, N_ch the same sum of b c_ch;
 *   B_ch  = D > 0 ? (N_ch + D / 2) / D : c_ch        (integer division)
 *   out   = (c * alpha + B * (255 - alpha) + 127) / 255 per channel.
 * All sums are unsigned 32 bits: N + D / 2 <= 4 286 578 688 < 2^32, which
 * is why taps that do not sum to 4096 are refused.  Wherever alpha < 255,
 * D > 0.
 * workspace: fcp_matte_blur_workspace_bytes(f,h,w) = 16 f h w bytes of
 * device memory, 16-byte aligned, contents irrelevant (the four horizontal
 * sums of every pixel); it must not overlap the other arrays.
 * out (f,h,w,3) and alpha (f,h,w) are written once, by ordinary stores;
 * alpha may be NULL.  out MAY BE crops (in place): the first launch reads
 * every crop byte a neighbour needs into the workspace, the second reads a
 * crop pixel only where it writes it.  labels must not overlap out or
 * alpha.  crops, labels, out and alpha may start at any byte; nothing
 * outside them is written.  Two launches on `stream`, nothing allocated,
 * the same bytes from run to run.
 * f == 0 is a no-op; f < 0, h or w < 1 or > 8192, f > 65535, a feather other
 * than 0 / 3 / 5 / 7, a radius outside 3..48, a bit of class_bits at or above
 * 19, null taps, a tap of 0, taps that do not sum to 4096, or (f > 0) a null
 * crops / labels / out, a workspace that is null, too small or misaligned
 * fail with a message, before any HIP call
 * (fcp_matte_blur_workspace_bytes then returns -1). */
int64_t fcp_matte_blur_workspace_bytes(int f, int h, int w);
int fcp_matte_blur_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather,
                      const uint16_t* taps, int radius, uint8_t* out, uint8_t* alpha, void* workspace, int64_t workspace_bytes,
                      fcp_stream_t stream);

/* Guided-filter matte edge: the hard mask m of
 * fcp_matte_u8 for class_bits, filtered with the gray of the crop as the
 * guide, in integers throughout.  n = (2 radius + 1)^2, 1 <= radius <= 16,
 * 1 <= eps <= 4096 (gray levels squared);
 *   I     = (9798 R + 19235 G + 3735 B + 16384) >> 15,   p = m (0 / 255);
 *   box(v) = the sum of v over the (2 radius + 1)^2 window, indices through
 *           BORDER_REFLECT_101 iterated: n terms at every pixel;
 *   cov   = n box(I p) - box(I) box(p),  var = n box(I I) - box(I)^2,
 *   den   = var + eps n n;
 *   rdiv(u, d) = sign(u) ((|u| + d / 2) / d);
 *   A     = rdiv(4096 cov, den),  B = rdiv(4096 box(p) - A box(I), n);
 *   q     = ((box(A) I + box(B) + 2048 n) >> 12) div n   (arithmetic shift,
 *           floor division);   alpha = min(255, max(0, q)).
 * workspace: fcp_matte_refine_workspace_bytes(f,h,w) = 8 f h w bytes of
 * device memory, 16-byte aligned, contents irrelevant ((A, B) of every
 * pixel); it must not overlap the other arrays.  alpha_out (f,h,w) is
 * written once, by ordinary stores; crops, labels and alpha_out may start at
 * any byte; nothing outside alpha_out and the workspace is written.  Two
 * launches on `stream`, nothing allocated, no float, no atomics, the same
 * bytes from run to run.
 * f == 0 is a no-op; f < 0, h or w < 1 or > 8192, f > 65535, a radius outside
 * 1..16, an eps outside 1..4096, a bit of class_bits at or above 19, or
 * (f > 0) a null crops / labels / alpha_out, a workspace that is null, too
 * small or misaligned fail with a message, before any HIP call
 * (fcp_matte_refine_workspace_bytes then returns -1). */
int64_t fcp_matte_refine_workspace_bytes(int f, int h, int w);
int fcp_matte_refine_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int radius, int eps,
                        uint8_t* alpha_out, void* workspace, int64_t workspace_bytes, fcp_stream_t stream);

/* The composites of fcp_matte_u8 and fcp_matte_blur_u8 through an alpha
 * plane (f,h,w) uint8 of the caller's (fcp_matte_refine_u8's) in place of
 * the feathered mask:
 *   fcp_matte_alpha_u8:       out = (c * alpha + bg * (255 - alpha) + 127) / 255;
 *   fcp_matte_blur_alpha_u8:  the same with B_ch of fcp_matte_blur_u8 as bg:
 *       N, D and B_ch come from the HARD mask of labels and class_bits, as
 *       there; where D == 0 (no background pixel in the window) B_ch = c_ch
 *       and the pixel keeps its crop whatever its alpha.
 * out MAY BE crops; alpha must not overlap out.  Arguments, workspace (16
 * bytes per pixel for the blur), alignment, launches (one; two) and failures
 * are those of the two siblings, less the feather; a null alpha fails too. */
int fcp_matte_alpha_u8(const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, int bg_r, int bg_g, int bg_b, uint8_t* out,
                       fcp_stream_t stream);
int fcp_matte_blur_alpha_u8(const uint8_t* crops, const uint8_t* labels, const uint8_t* alpha, int f, int h, int w,
                            uint32_t class_bits, const uint16_t* taps, int radius, uint8_t* out, void* workspace,
                            int64_t workspace_bytes, fcp_stream_t stream);

/* RGBA cut-outs and the subject's own edge colours, in
 * integers throughout.
 * fcp_feather_alpha_u8: alpha_out (f,h,w) = the alpha of fcp_matte_u8 for
 * labels, class_bits and feather, alone.  One launch, no workspace; labels
 * and alpha_out may start at any byte and must not overlap.  f == 0 is a
 * no-op; the sizes, feather, class_bits and null pointers fail as there, with
 * a "feather_alpha:" message, before any HIP call.
 * fcp_cutout_u8: crops (f,h,w,3) and an alpha plane (f,h,w) of the caller's
 * (fcp_feather_alpha_u8's or fcp_matte_refine_u8's) ->
 *   mode FCP_CUTOUT_RGBA: out (f,h,w,4): (F_r, F_g, F_b, alpha) where
 *       alpha > 0 and (0,0,0,0) where alpha == 0;
 *   mode FCP_CUTOUT_FILL: out (f,h,w,3):
 *       (F * alpha + bg * (255 - alpha) + 127) / 255 per channel.
 * radius == 0: F = c, the crop's colour (RGBA only: the fill mode without an
 * estimate is fcp_matte_alpha_u8 and is refused here).  radius 3..48 with
 * taps as in fcp_matte_blur_u8: F is the "blur fusion" estimate of the
 * subject's colour.  sF = 1 where alpha == 255, sB = 1 where alpha == 0;
 *   D_F   = sum_j sum_i t|j| t|i| sF(y+j, x+i) over the positions inside the
 *           image, N_F,ch the same sum of sF c_ch; D_B, N_B,ch with sB;
 *   F^_ch = D_F > 0 ? (N_F,ch + D_F / 2) / D_F : c_ch;  B^_ch likewise;
 *   R_ch  = 255 c_ch - (alpha F^_ch + (255 - alpha) B^_ch);
 *   E_ch  = clamp(floor((65025 F^_ch + alpha R_ch + 32512) / 65025), 0, 255);
 *   F_ch  = c_ch where alpha == 255, E_ch where 0 < alpha < 255.
 * The sums are unsigned 32 bits with the bounds of fcp_matte_blur_u8; the
 * correction stays below 2^25 in magnitude.
 * workspace: fcp_cutout_workspace_bytes(f,h,w) = 32 f h w bytes of device
 * memory, 16-byte aligned, contents irrelevant (the eight horizontal sums of
 * every pixel); not read with radius 0, where it may be NULL.  out is its own
 * array: it must not overlap crops, alpha or the workspace.  crops and alpha
 * may start at any byte; an RGBA out must be 4-byte aligned (one dword store
 * per pixel), a fill out may start at any byte; nothing outside out and the
 * workspace is written.  One launch with radius 0, else two, on `stream`;
 * nothing allocated, the same bytes from run to run.
 * f == 0 is a no-op; f < 0, h or w < 1 or > 8192, f > 65535, a mode other
 * than the two, a radius outside {0, 3..48}, the fill mode with radius 0, a
 * fill component outside 0..255, (radius > 0) null taps, a tap of 0, taps
 * that do not sum to 4096, or (f > 0) a null crops / alpha / out, a
 * misaligned RGBA out, (radius > 0) a workspace that is null, too small or
 * misaligned fail with a "cutout:" message, before any HIP call
 * (fcp_cutout_workspace_bytes then returns -1). */
#define FCP_CUTOUT_RGBA 0
#define FCP_CUTOUT_FILL 1
int fcp_feather_alpha_u8(const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather, uint8_t* alpha_out,
                         fcp_stream_t stream);
int64_t fcp_cutout_workspace_bytes(int f, int h, int w);
int fcp_cutout_u8(const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, int mode, int bg_r, int bg_g, int bg_b,
                  const uint16_t* taps, int radius, uint8_t* out, void* workspace, int64_t workspace_bytes, fcp_stream_t stream);

/* Crops over pictures: the composites above with the
 * fill of a pixel read from a bank of pictures that is resident on the
 * device.  pictures (k,h,w,3) uint8 RGB, 1 <= k <= 4096, with the crops' h
 * and w; picks (f,) int32 on the device, 0 <= picks[i] < k; P = the picture
 * picks[face] at the pixel's own position:
 *   fcp_matte_image_u8:       fcp_matte_u8 with P_ch as bg_ch (m, alpha and
 *       the rounding are that entry's; alpha may be NULL);
 *   fcp_matte_image_alpha_u8: fcp_matte_alpha_u8 likewise, through an alpha
 *       plane (f,h,w) of the caller's;
 *   fcp_cutout_image_u8:      the FCP_CUTOUT_FILL mode of fcp_cutout_u8
 *       likewise: out = (F * alpha + P * (255 - alpha) + 127) / 255 with the
 *       estimate F of that entry, its taps, radius 3..48 and its workspace of
 *       fcp_cutout_workspace_bytes(f,h,w) bytes; radius 0 is refused: that
 *       composite is fcp_matte_image_alpha_u8.
 * So alpha == 0 gives the picture's bytes, alpha == 255 the crop's, and a
 * picture of one colour the bytes of the sibling with that colour as bg.
 * The same kernels and launches as the siblings (one; one; two), the fill
 * source being their template parameter; a group's 12 picture bytes are read
 * beside the crop's, rows of 3 w bytes at any byte offset, and no dword is
 * read that holds no byte of the bank.  A pick outside 0..k-1 breaks the
 * precondition; the kernels clamp it, so that the read stays inside the bank.
 * out MAY BE crops for the two matte entries, as for their siblings, and is
 * its own array for the cutout; pictures and picks are only read and must
 * not overlap out or alpha.  The same bytes from run to run.
 * f == 0 is a no-op; the sizes, feather, class_bits, radius, taps and
 * workspace fail as in the siblings, a k outside 1..4096 and (f > 0) a null
 * crops / labels / alpha plane / pictures / picks / out fail too, with a
 * "matte_image:", "matte_image_alpha:" or "cutout_image:" message, before
 * any HIP call. */
int fcp_matte_image_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather,
                       const uint8_t* pictures, int k, const int32_t* picks, uint8_t* out, uint8_t* alpha, fcp_stream_t stream);
int fcp_matte_image_alpha_u8(const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, const uint8_t* pictures, int k,
                             const int32_t* picks, uint8_t* out, fcp_stream_t stream);
int fcp_cutout_image_u8(const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, const uint8_t* pictures, int k,
                        const int32_t* picks, const uint16_t* taps, int radius, uint8_t* out, void* workspace,
                        int64_t workspace_bytes, fcp_stream_t stream);

/* One connected subject in a matte: connected-component
 * labelling of the hard mask of label maps (f,h,w) uint8, every face on its
 * own, in integers.  H = h, W = w:
 *   m0(y,x) = 1 where labels(y,x) < 19 and bit labels(y,x) of class_bits is
 *             set, else 0 (the hard mask of fcp_matte_u8; label bytes at or
 *             above 19 are background, as there);
 *   keep_largest = 1: the 8-connected components of {m0 = 1}; a component's
 *             key is (its pixel count, then the SMALLER raster index y W + x
 *             of its first pixel in raster order); m1 = the component with
 *             the largest count, among equal counts the one whose first
 *             pixel comes first; no foreground pixel: m1 = m0.
 *             keep_largest = 0: m1 = m0;
 *   max_hole = N > 0: the 4-connected components of {m1 = 0}; a hole is one
 *             that has no pixel in row 0, row H - 1, column 0 or column
 *             W - 1; m2 = m1, plus every hole of at most N pixels.
 *             max_hole = 0: m2 = m1;
 *   out(y,x) = m2(y,x), one byte, 0 or 1.
 * The subject comes first, then the holes: an island that lay inside a hole
 * is background by then and counts towards that hole's area.
 * keep_largest = 0, max_hole = 0 is legal and writes m0.
 * workspace: fcp_subject_mask_workspace_bytes(f,h,w) = 12 f h w bytes of
 * device memory (three int32 planes), 16-byte aligned, contents irrelevant;
 * it must not overlap the other arrays.  labels and out may start at any
 * byte; nothing outside out and the workspace is written.  1 launch for
 * (0, 0), 5 for the subject, 4 for the holes, 9 for both, on `stream`;
 * nothing allocated, no float; the atomics are integer min / add / or whose
 * result does not depend on their order: the same bytes from run to run.
 * f == 0 is a no-op; f < 0, h or w < 1 or > 8192, f > 65535, a bit of
 * class_bits at or above 19, a keep_largest outside {0, 1}, a max_hole
 * outside 0..67108864, or (f > 0) a null labels / out, a workspace that is
 * null, too small or misaligned fail with a "subject_mask:" message, before
 * any HIP call (fcp_subject_mask_workspace_bytes then returns -1). */
int64_t fcp_subject_mask_workspace_bytes(int f, int h, int w);
int fcp_subject_mask_u8(const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int keep_largest, int max_hole, uint8_t* out,
                        void* workspace, int64_t workspace_bytes, fcp_stream_t stream);

/* Grow or shrink the matte: binary morphology of the hard
 * mask of label maps (f,h,w) uint8 with a Euclidean disc, every face on its
 * own, in integers.  r = |shift|:
 *   m0(y,x) = (class_bits >> labels(y,x)) & 1 (the hard mask of fcp_matte_u8;
 *             label bytes at or above 19 are background, as there);
 *   only positions inside the crop exist: a pixel outside the crop is
 *             neither subject nor background, and it is never a source;
 *   shift > 0 (grow): out(y,x) = 1 iff some (y',x') inside the crop has
 *             m0 = 1 and (y-y')^2 + (x-x')^2 <= r^2;
 *   shift < 0 (shrink): out(y,x) = 1 iff m0(y,x) = 1 and no (y',x') inside
 *             the crop has m0 = 0 and (y-y')^2 + (x-x')^2 <= r^2;
 *   shift = 0: out = m0 (legal, like fcp_subject_mask_u8 with (0, 0));
 *   out(y,x) is one byte, 0 or 1, read downstream as class 1.
 * That is scipy.ndimage.binary_dilation(m0, disc, border_value=0) for a grow
 * and binary_erosion(m0, disc, border_value=1) for a shrink with
 * disc = {dy^2 + dx^2 <= r^2}, and the threshold d^2 <= r^2 of the exact
 * squared Euclidean distance to the nearest source pixel.  A shrink does not
 * eat inwards from the crop's border: a subject that touches it stays there.
 * One launch on `stream`, no workspace, nothing allocated, no float and no
 * atomics: the same bytes from run to run.  labels and out may start at any
 * byte and must not overlap (a tile reads the halo its neighbours write);
 * nothing outside out is written.
 * f == 0 is a no-op; f < 0, h or w < 1 or > 8192, f > 65535, a bit of
 * class_bits at or above 19, a shift outside -64..64, or (f > 0) a null
 * labels / out fail with a "mask_shift:" message, before any HIP call. */
int fcp_mask_shift_u8(const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int shift, uint8_t* out,
                      fcp_stream_t stream);

/* Contrast-limited adaptive histogram equalisation of the luma of crops
 * (f,h,w,3) uint8 RGB: cv2.createCLAHE(clip_limit,
 * (grid, grid)).apply(Y) between cv2.cvtColor(COLOR_RGB2YCrCb) and
 * cvtColor(COLOR_YCrCb2RGB), restated.  With g = grid, c = clip_limit:
 *   colour  Y  = (4899 R + 9617 G + 1868 B + 8192) >> 14
 *           Cr = sat(((R - Y) 11682 + (128 << 14) + 8192) >> 14)
 *           Cb = sat(((B - Y) 9241 + (128 << 14) + 8192) >> 14); only Y is
 *           equalised, and from the result Y':
 *           R  = sat(Y' + (((Cr - 128) 22987 + 8192) >> 14))
 *           G  = sat(Y' + (((Cb - 128) (-5636) + (Cr - 128) (-11698) + 8192) >> 14))
 *           B  = sat(Y' + (((Cb - 128) 29049 + 8192) >> 14))
 *           sat clamps to 0..255; arithmetic shifts of signed 32-bit values;
 *   tiles   if h % g == 0 and w % g == 0 the luma plane as is, else extended
 *           by g - h % g rows below and g - w % g columns on the right with
 *           BORDER_REFLECT_101 (a divisible dimension grows by a full g
 *           when the other is not: OpenCV's rule); th, tw = extended size /
 *           g, area = th tw;
 *   LUT     per tile: the 256-bin histogram; clip = max(int(c area / 256),
 *           1) in double, truncated (area or more clips nothing); bins above
 *           clip are cut to it, the excess summed into clipped; batch =
 *           clipped / 256 is added to every bin; residual = clipped - 256
 *           batch; if residual > 0, step = max(256 / residual, 1) and bin i
 *           gets + 1 iff i % step == 0 and i / step < residual; s = the
 *           inclusive prefix sum; lut[i] = sat(rint(float(s[i]) * scale)),
 *           scale = 255.0f / float(area), round half to even;
 *   apply   per pixel (y, x), float32, each operation rounded on its own:
 *           inv_th = 1.0f / th; tyf = y inv_th - 0.5f; ty1 = floor(tyf);
 *           ya = tyf - ty1; ya1 = 1.0f - ya; then ty2 = min(ty1 + 1, g - 1),
 *           ty1 = max(ty1, 0); the same in x;
 *           res = (L[ty1][tx1][Y] xa1 + L[ty1][tx2][Y] xa) ya1
 *               + (L[ty2][tx1][Y] xa1 + L[ty2][tx2][Y] xa) ya;
 *           Y' = sat(rint(res)).
 * luts is a workspace of f * grid * grid * 256 bytes, 4-byte aligned, that
 * holds the LUTs [f][grid][grid][256] afterwards; it must not overlap crops
 * or out.  out (f,h,w,3) is written once, by ordinary stores;
 * out MAY BE crops (in place): an output pixel depends on its own crop
 * pixel and on the LUTs only.  crops and out may start at any byte; nothing
 * outside the arrays is written.  Two launches on `stream`; the histograms
 * are summed with integer atomics, which commute:
 * the same bytes from run to run.
 * f == 0 is a no-op; grid outside 1..16, f < 0 or > 65535, h or w below
 * 2 * grid or above 4096, a clip_limit that is not finite or not > 0, or
 * (f > 0) a null crops / luts / out or a misaligned luts fail with a
 * message, before any HIP call. */
int fcp_clahe_u8(const uint8_t* crops, int f, int h, int w, int grid, double clip_limit, uint8_t* luts, uint8_t* out, fcp_stream_t stream);

/* Non-local-means noise removal of crops (f,h,w,3) uint8 RGB, in integers
 * (INTEGRATION.md 2p).  With P = 3 (a 7 x 7 patch), S = 10 (a 21 x 21 search
 * window), ONE = 4096, every coordinate outside the crop reflected
 * (BORDER_REFLECT_101), and the table lut[0 .. lut_len - 1] of uint16:
 *   g        = (9798 R + 19235 G + 3735 B + 16384) >> 15
 *   d(p,o)   = sum over t in [-P,P]^2 of (g(p + t) - g(p + o + t))^2, for
 *              every offset o in [-S,S]^2
 *   k        = d >> shift;  w(p,o) = min(lut[k], ONE) if k < lut_len, else 0
 *   W        = sum over o of w(p,o)
 *   out_c(p) = (sum over o of w(p,o) c(p + o) + (W >> 1)) / W for c = R, G,
 *              B, floor division; W == 0 copies the pixel.
 * The weights come from the gray alone; the three channels are averaged
 * with them.  The clamp at ONE keeps W below 2^21 and the numerators below
 * 2^29 for any table: unsigned 32-bit sums, which commute, so the bytes do
 * not depend on the tiling or the order of the offsets and are the same
 * from run to run.  lut is device memory, 2-byte aligned
 * (denoise.weight_lut builds the table of a filter strength on the host).
 * One launch on `stream`, no workspace, no float and no atomics.  crops and
 * out may start at any byte and must not overlap (out == crops included: a
 * pixel reads its window); nothing outside out is written.
 * f == 0 is a no-op; f < 0 or > 65535, h or w below P + S + 1 = 14 or above
 * 8192, a lut_len outside 1..4096, a shift outside 0..10, or (f > 0) a null
 * crops / lut / out, a misaligned lut or overlapping arrays fail with a
 * "nlm_denoise:" message, before any HIP call. */
int fcp_nlm_denoise_u8(const uint8_t* crops, int f, int h, int w, const uint16_t* lut, int lut_len, int shift, uint8_t* out,
                       fcp_stream_t stream);

/* Unsharp-mask sharpening of crops (f,h,w,3) uint8 RGB, in integers
 * (INTEGRATION.md 2q): the gray's difference from its own Gaussian blur,
 * cored and scaled, is added to all three channels alike, so there are no
 * colour fringes.  With the taps t[0..radius] of uint16 in HOST memory
 * (matte.blur_taps makes those of a sigma; they travel in the kernel's
 * argument block):
 *   t[0..r]  : t[0] + 2 sum(t[1..r]) == 4096, 1 <= r <= 48; a tap may be 0
 *   g        = (9798 R + 19235 G + 3735 B + 16384) >> 15
 *   coordinates outside the crop are clamped to its edge (BORDER_REPLICATE):
 *   any h, w >= 1
 *   Hs(y,x)  = sum_i t|i| g(y, clamp(x + i))               <= 255 * 4096
 *   B(y,x)   = sum_j t|j| Hs(clamp(y + j), x)              <= 255 * 2^24 < 2^32
 *   b8       = (B + 32768) >> 16                           the blurred gray, 8 fraction bits
 *   d        = (g << 8) - b8                               |d| <= 65280
 *   e        = sign(d) * max(|d| - (T << 8), 0)            T = threshold, gray levels
 *   v_c      = (c << 16) + A_q * e + 32768                 c = R, G, B; A_q = amount_q8;
 *                                                          |A_q e| <= 66 846 720: signed 32 bits
 *   out_c    = v_c < 0 ? 0 : min(255, v_c >> 16)
 * amount_q8 = 256 adds the whole difference.  threshold = 255 copies the
 * crops, and so do the taps {4096, 0, ...}.  Integer sums commute: the bytes
 * do not depend on the tiling and are the same from run to run.
 * One launch on `stream`, no workspace, no float and no atomics.  crops and
 * out may start at any byte and must not overlap (out == crops included: a
 * workgroup reads its neighbours' pixels); nothing outside out is written.
 * f < 0 or > 65535, h or w below 1 or above 8192, a radius outside 1..48, an
 * amount_q8 outside 1..1024, a threshold outside 0..255, null or misaligned
 * (2 bytes) taps, or taps that do not sum to 4096 fail with an "unsharp:"
 * message; then f == 0 is a no-op; then a null crops / out or overlapping
 * arrays fail likewise, all before any HIP call. */
int fcp_unsharp_u8(const uint8_t* crops, int f, int h, int w, const uint16_t* taps, int radius, int amount_q8, int threshold,
                   uint8_t* out, fcp_stream_t stream);

/* Parser-guided skin smoothing of crops (f,h,w,3) uint8 RGB from label maps
 * (f,h,w) uint8, in integers: a bilateral filter that
 * changes only pixels labelled skin, averages only over pixels labelled
 * skin and leaves every other pixel byte-identical.  With the taps
 * t[0..radius] of uint16 in HOST memory (matte.blur_taps makes those of a
 * sigma; they travel in the kernel's argument block), the range table
 * range_lut[0..255] of uint16 in DEVICE memory (skin.range_lut makes that of
 * a strength) and ONE = 4096:
 *   g(p)     = (9798 R + 19235 G + 3735 B + 16384) >> 15
 *   m(p)     = 1 if l(p) < 32 and bit l(p) of class_bits is set, else 0;
 *              m = 0 outside the crop (nothing is reflected: any h, w >= 1)
 *   s(o)     = (t[|oy|] t[|ox|] + 2048) >> 12, o in [-radius, radius]^2
 *   w(p,o)   = m(p + o) ((s(o) min(range_lut[|g(p + o) - g(p)|], ONE)
 *              + 2048) >> 12)
 *   W(p)     = sum over o of w(p,o)
 *   b_c(p)   = (sum over o of w(p,o) c_c(p + o) + (W >> 1)) / W for c = R,
 *              G, B, floor division; W == 0: b = c(p)
 *   alpha(p) = the feather-7 alpha of fcp_matte_u8 for class_bits
 *   e(p)     = max(0, 2 alpha(p) - 255);  E(p) = (e(p) amount_q8 + 128) >> 8
 *   out_c(p) = (b_c E + c_c (255 - E) + 127) / 255 if m(p) == 1, else c_c(p)
 * Every tap is at most ONE, so s <= ONE and w <= ONE for any table, and a
 * window has at most 2401 positions: the numerators stay below 2^32,
 * unsigned 32-bit sums, which commute, so the bytes do not depend on the
 * tiling or the order of the offsets and are the same from run to run.
 * amount_q8 = 256 replaces the skin by its mean inside the ramp e.
 * One launch on `stream`, no workspace, no float and no atomics.  crops,
 * labels and out may start at any byte; out must not overlap crops (out ==
 * crops included: a pixel reads its window) or labels; nothing outside out
 * is written.
 * f < 0 or > 65535, h or w below 1 or above 8192, a bit of class_bits at or
 * above 19, a radius outside 3..24, null taps, a tap above 4096 or an
 * amount_q8 outside 1..256 fail with a "skin_smooth:" message; then f == 0
 * is a no-op; then a null crops / labels / range_lut / out, a misaligned
 * range_lut or overlapping arrays fail likewise, all before any HIP call. */
int fcp_skin_smooth_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, const uint16_t* taps,
                       int radius, const uint16_t* range_lut, int amount_q8, uint8_t* out, fcp_stream_t stream);

/* ------------------------------------------------------------------------
 * BiSeNet face parser glue (models/bise.py, _layers.py:206-368).
 * ------------------------------------------------------------------------ */

/* bise.py:387-393: faces (f,h,w,3) uint8 RGB -> `/255`, bilinear to (out_h,out_w)
 * with align_corners=False, `(x-mean)/std` -> fp32 NHWC4 (f,out_h,out_w,4).
 * mean_host/std_host: 3 floats each on the host. */
int fcp_bise_preprocess_u8(const uint8_t* faces, int f, int h, int w, float* out,
                           int out_h, int out_w, const float* mean_host,
                           const float* std_host, fcp_stream_t stream);

/* F.avg_pool2d(x, x.size()[2:]) on an NHWC slice (_layers.py:307,:332,:360):
 * in (n,hw,ld) channels [0,c) -> out (n,c). */
int fcp_avgpool_nhwc_f32(const float* in, int n, int hw, int c, int ld, float* out,
                         fcp_stream_t stream);

/* 1x1 conv on a 1x1 map (+ folded BatchNorm) (+ ReLU / sigmoid): ARM conv_atten,
 * ContextPath conv_avg, FFM conv1/conv2 (_layers.py:308-310,:333,:361-364).
 * out[n][co] = act(scale[co] * dot(w[co,:], in[n,:]) + shift[co]);
 * scale/shift may be NULL; act: 0 none, 1 relu, 2 sigmoid. */
int fcp_fc_f32(const float* in, const float* w, const float* scale, const float* shift,
               int n, int cin, int cout, int act, float* out, fcp_stream_t stream);

/* out = x * scale_nc[n,c] (+ add_nc[n,c]) (+ add_t[n,h,w,c]): torch.mul(feat, atten)
 * followed by `+ avg_up` / `+ feat32_up` / `+ feat` (_layers.py:311,:337,:342,:365-366). */
int fcp_scale_add_nhwc_f32(const float* x, int x_ld, const float* scale_nc,
                           const float* add_nc, const float* add_t, int add_t_ld,
                           int n, int hw, int c, float* out, int out_ld, fcp_stream_t stream);

/* Parse tail (bise.py:212 + :394): logits (f,lh,lw,ld) at 1/8 resolution ->
 * bilinear align_corners=True to (mid_h,mid_w) -> nearest to (out_h,out_w) ->
 * argmax (first maximum) -> labels (f,out_h,out_w) uint8.  counts (f,ncls) int32
 * = per-face class histogram (bise.py:253-254), may be NULL. */
int fcp_parse_tail(const float* logits, int f, int lh, int lw, int ld, int ncls,
                   int mid_h, int mid_w, int out_h, int out_w, uint8_t* labels,
                   int32_t* counts, fcp_stream_t stream);

/* mask = 255 where bit `label` of class_bits is set, else 0 (bise.py:314-319). */
int fcp_label_mask_u8(const uint8_t* labels, int64_t total, uint32_t class_bits,
                      uint8_t* mask, fcp_stream_t stream);

/* ------------------------------------------------------------------------
 * RRDB enhancer tail (rrdb.py:143-144): x4 (4h,4w,ld>=3) fp32 in [0,1] ->
 * bicubic x0.25 (align_corners=False, A=-0.75: taps (-3,19,19,-3)/32) ->
 * clamp(0,1)*255 -> round-half-even -> uint8 RGB (h,w,3).
 * ------------------------------------------------------------------------ */
int fcp_bicubic_down4_u8(const float* x4, int h, int w, int ld, uint8_t* out_rgb,
                         fcp_stream_t stream);

/* ------------------------------------------------------------------------
 * Batch builder (utils.py:273-342, `as_batch`): cv2.resize (INTER_AREA when the
 * image is larger than the batch, else INTER_CUBIC; uint8) of every image of a
 * ragged list + cv2.copyMakeBorder into its slot of one (n,out_h,out_w,3) uint8
 * batch, one launch.  The host computes the geometry of utils.py:316-331 and
 * fills one item per image; the images are packed back to back (RGB, HWC) in
 * one device blob.  items_host is validated here; items_dev is the caller's
 * device copy of the same table.  border = cv2.BORDER_* code as for
 * fcp_warp_affine_u8 (the reference always passes "constant", utils.py:276).
 * ------------------------------------------------------------------------ */
typedef struct fcp_batch_item {
  int64_t src_off;    /* byte offset of the (sh,sw,3) image inside src_blob */
  int32_t sh, sw;     /* source height, width */
  int32_t dh, dw;     /* resized height, width (hh, ww of utils.py:322-331) */
  int32_t top, left;  /* padding in front of the resized image (paddings[0], paddings[2]) */
  int32_t interp;     /* 0 = cv2.INTER_CUBIC, 1 = cv2.INTER_AREA (decimation only) */
  int32_t reserved;
} fcp_batch_item;

int fcp_build_batch_u8(const uint8_t* src_blob, int64_t blob_bytes,
                       const fcp_batch_item* items_host, const fcp_batch_item* items_dev,
                       int n, int out_h, int out_w, int border, uint8_t* out,
                       fcp_stream_t stream);

/* ------------------------------------------------------------------------
 * Ragged INTER_AREA levels (crop_source="original"): cv2.resize(src, (dw,dh),
 * interpolation=INTER_AREA) of n (source, destination) pairs, one launch, the
 * arithmetic of fcp_build_batch_u8's INTER_AREA.  Sources are (sh,sw,3) uint8
 * images at src_off of src_blob; destinations (dh,dw,3) at dst_off of dst_blob,
 * dst_off a multiple of 4; dh <= sh and dw <= sw.  levels_host is validated
 * here; levels_dev is the caller's device copy of the same table.
 * ------------------------------------------------------------------------ */
typedef struct fcp_area_level {
  int64_t src_off;    /* byte offset of the source inside src_blob */
  int32_t sh, sw;     /* source height, width */
  int64_t dst_off;    /* byte offset of the level inside dst_blob (multiple of 4) */
  int32_t dh, dw;     /* level height, width */
} fcp_area_level;

int fcp_resize_area_ragged_u8(const uint8_t* src_blob, int64_t src_bytes,
                              const fcp_area_level* levels_host, const fcp_area_level* levels_dev,
                              int n, uint8_t* dst_blob, int64_t dst_bytes, fcp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FCP_HIP_H */
