// PyTorch-ROCm custom ops over the C ABI of include/fcp_hip.h ("a PyTorch-ROCm extension, TORCH_LIBRARY
// namespace ... stateless ops on the current HIP stream, tensors in/out, no hidden global state").
//
//     torch.ops.fcp.conv2d / bottleneck_chain / retina_decode / nms_select / gather_faces / similarity_from_5pt /
//     warp_affine_u8 / warp_affine_u8_float / warp_affine_u8_ragged / warp_affine_u8_interp / warp_affine_u8_interp_ragged /
//     resize_area_u8_ragged / bicubic_down4_round / parse_argmax_hist / crop_sharpness / jpeg_encode / jpeg_encode_ex / jpeg_huffman_tables / png_encode / png_huffman_lengths / matte / clahe / matte_blur / matte_refine / matte_alpha / matte_blur_alpha / subject_mask / feather_alpha / cutout / mask_shift / nlm_denoise / unsharp / matte_image / matte_image_alpha / cutout_image
//
// Each op validates device / dtype / contiguity with TORCH_CHECK (-> RuntimeError), allocates its outputs with torch's
// caching allocator, borrows its inputs, enqueues the HIP kernels of libfcp_hip.so on at::hip's CURRENT stream and
// returns without synchronising: the ops are stream-ordered and safe to capture in a HIP graph.  Schemas are plain
// (Tensor / int / float / bool), so torch.library can attach fake-tensor implementations for torch.compile.
// The ops are a veneer: all arithmetic lives behind the C ABI, which stays the drop-in boundary.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include <climits>
#include <tuple>

#include "fcp_hip.h"

namespace {

using at::Tensor;

void* cur_stream() { return (void*)at::hip::getCurrentHIPStream().stream(); }

// Every op makes its first tensor's device current for its duration: the stream it enqueues on and the memory its
// outputs come from are that device's, whatever device the calling thread had selected.
#define FCP_DEVICE_GUARD(t) const c10::OptionalDeviceGuard fcp_guard_(at::device_of(t))

void ok(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " failed (", rc, "): ", fcp_last_error()); }

const Tensor& dev(const Tensor& t, const char* name, at::ScalarType dt) {
  TORCH_CHECK(t.is_cuda(), name, " must live on the GPU");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  return t;
}
template <typename T>
const T* optp(const c10::optional<Tensor>& t, const char* name, at::ScalarType dt) {
  if (!t.has_value() || !t->defined()) return nullptr;
  return dev(*t, name, dt).data_ptr<T>();
}

// ---- conv engine.  x / res1 / res2 / out are NHWC buffers (n, h, w, ld); *_c0 selects the first channel of the view.
// `out` (optional) lets the caller write a channel slice of a wider buffer (torch.cat without a copy); otherwise a
// dense (n, oh, ow, cout) tensor is allocated.
Tensor conv2d_impl(const Tensor& x, int64_t x_c0, int64_t cin, const Tensor& w, const c10::optional<Tensor>& bias,
                   const c10::optional<Tensor>& wscale, const c10::optional<Tensor>& res1, int64_t res1_c0,
                   const c10::optional<Tensor>& res2, int64_t res2_c0, const c10::optional<Tensor>& out_, int64_t out_c0,
                   int64_t cout, int64_t kh, int64_t kw, int64_t stride, int64_t pad, double act_slope, double alpha,
                   double alpha2, bool res1_pre, int64_t precision, int64_t in_fmt, int64_t out_fmt, int64_t res1_fmt,
                   int64_t res2_fmt, bool in_up2, bool cin4, int64_t tile_m, int64_t tile_n, const c10::optional<Tensor>& x2,
                   int64_t x2_c0, int64_t cin2, int64_t x2_stride, int64_t flags, int64_t cu_budget, int64_t band_top,
                   int64_t band_bottom) {
  dev(x, "x", at::kFloat);
  FCP_DEVICE_GUARD(x);
  TORCH_CHECK(x.dim() == 4, "x must be NHWC (n, h, w, ld)");
  TORCH_CHECK(w.is_cuda() && w.is_contiguous(), "w must be a contiguous GPU tensor (packed filter)");
  const int64_t n = x.size(0), ph = x.size(1), pw = x.size(2), ld = x.size(3);
  const int64_t ih = in_up2 ? 2 * ph : ph, iw = in_up2 ? 2 * pw : pw;
  const int64_t oh = (ih - band_top - band_bottom + 2 * pad - kh) / stride + 1, ow = (iw + 2 * pad - kw) / stride + 1;
  Tensor out = out_.has_value() && out_->defined() ? *out_ : at::empty({n, oh, ow, cout}, x.options());
  dev(out, "out", at::kFloat);
  TORCH_CHECK(out.dim() == 4 && out.size(0) == n && out.size(1) == oh && out.size(2) == ow && out_c0 + cout <= out.size(3),
              "out has the wrong geometry");
  TORCH_CHECK(x_c0 + (cin4 ? 4 : cin - cin2) <= ld, "input channel view exceeds the buffer");
  fcp_conv_desc d = {};
  d.in = x.data_ptr<float>() + x_c0;
  d.w = w.data_ptr();
  d.bias = optp<float>(bias, "bias", at::kFloat);
  d.wscale = optp<float>(wscale, "wscale", at::kFloat);
  d.out = out.data_ptr<float>() + out_c0;
  d.n = (int)n; d.in_h = (int)ih; d.in_w = (int)iw; d.cin = (int)cin; d.in_ld = (int)ld; d.in_up2 = in_up2;
  d.cout = (int)cout; d.kh = (int)kh; d.kw = (int)kw; d.stride = (int)stride; d.pad = (int)pad;
  d.out_h = (int)oh; d.out_w = (int)ow; d.out_ld = (int)out.size(3);
  d.tile_n = (int)tile_n; d.tile_m = (int)tile_m; d.cin4 = cin4;
  d.act_slope = (float)act_slope; d.alpha = (float)alpha; d.alpha2 = (float)alpha2;
  d.res1_pre = res1_pre; d.precision = (int)precision;
  d.in_fmt = (int)in_fmt; d.out_fmt = (int)out_fmt; d.res1_fmt = (int)res1_fmt; d.res2_fmt = (int)res2_fmt;
  if (res1.has_value() && res1->defined()) {
    dev(*res1, "res1", at::kFloat);
    d.res1 = res1->data_ptr<float>() + res1_c0;
    d.res1_ld = (int)res1->size(3); d.res1_h = (int)res1->size(1); d.res1_w = (int)res1->size(2);
  }
  if (res2.has_value() && res2->defined()) {
    dev(*res2, "res2", at::kFloat);
    d.res2 = res2->data_ptr<float>() + res2_c0;
    d.res2_ld = (int)res2->size(3);
  }
  if (x2.has_value() && x2->defined()) {                 // second source of a 1x1 conv (K concatenation)
    dev(*x2, "x2", at::kFloat);
    d.in2 = x2->data_ptr<float>() + x2_c0;
    d.cin2 = (int)cin2; d.in2_ld = (int)x2->size(3); d.in2_h = (int)x2->size(1); d.in2_w = (int)x2->size(2);
    d.in2_stride = (int)x2_stride;
  }
  d.flags = (int)flags;
  d.cu_budget = (int)cu_budget;
  d.band_top = (int)band_top; d.band_bottom = (int)band_bottom;
  ok(fcp_conv2d_nhwc_f32(&d, cur_stream()), "fcp::conv2d");
  return out;
}

// Two schemas, so that the aliasing is declared truthfully: `conv2d` allocates and returns a fresh dense tensor,
// `conv2d_out` writes channels [out_c0, out_c0 + cout) of the caller's buffer and returns nothing.
Tensor conv2d(const Tensor& x, int64_t x_c0, int64_t cin, const Tensor& w, const c10::optional<Tensor>& bias,
              const c10::optional<Tensor>& wscale, const c10::optional<Tensor>& res1, int64_t res1_c0,
              const c10::optional<Tensor>& res2, int64_t res2_c0, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
              int64_t pad, double act_slope, double alpha, double alpha2, bool res1_pre, int64_t precision, int64_t in_fmt,
              int64_t out_fmt, int64_t res1_fmt, int64_t res2_fmt, bool in_up2, bool cin4, int64_t tile_m, int64_t tile_n,
              const c10::optional<Tensor>& x2, int64_t x2_c0, int64_t cin2, int64_t x2_stride, int64_t flags, int64_t cu_budget,
              int64_t band_top, int64_t band_bottom) {
  return conv2d_impl(x, x_c0, cin, w, bias, wscale, res1, res1_c0, res2, res2_c0, c10::nullopt, 0, cout, kh, kw, stride, pad,
                     act_slope, alpha, alpha2, res1_pre, precision, in_fmt, out_fmt, res1_fmt, res2_fmt, in_up2, cin4, tile_m,
                     tile_n, x2, x2_c0, cin2, x2_stride, flags, cu_budget, band_top, band_bottom);
}

void conv2d_out(const Tensor& x, int64_t x_c0, int64_t cin, const Tensor& w, const c10::optional<Tensor>& bias,
                const c10::optional<Tensor>& wscale, const c10::optional<Tensor>& res1, int64_t res1_c0,
                const c10::optional<Tensor>& res2, int64_t res2_c0, Tensor& out, int64_t out_c0, int64_t cout, int64_t kh,
                int64_t kw, int64_t stride, int64_t pad, double act_slope, double alpha, double alpha2, bool res1_pre,
                int64_t precision, int64_t in_fmt, int64_t out_fmt, int64_t res1_fmt, int64_t res2_fmt, bool in_up2, bool cin4,
                int64_t tile_m, int64_t tile_n, const c10::optional<Tensor>& x2, int64_t x2_c0, int64_t cin2,
                int64_t x2_stride, int64_t flags, int64_t cu_budget, int64_t band_top, int64_t band_bottom) {
  conv2d_impl(x, x_c0, cin, w, bias, wscale, res1, res1_c0, res2, res2_c0, out, out_c0, cout, kh, kw, stride, pad, act_slope,
              alpha, alpha2, res1_pre, precision, in_fmt, out_fmt, res1_fmt, res2_fmt, in_up2, cin4, tile_m, tile_n, x2, x2_c0,
              cin2, x2_stride, flags, cu_budget, band_top, band_bottom);
}

std::tuple<Tensor, Tensor> bottleneck_chain(const Tensor& t1, int64_t t1_c0, const c10::optional<Tensor>& res, int64_t res_c0,
                                            const c10::optional<Tensor>& w2, const c10::optional<Tensor>& ws2,
                                            const c10::optional<Tensor>& b2, const Tensor& w3, const Tensor& ws3,
                                            const Tensor& b3, const c10::optional<Tensor>& w1n,
                                            const c10::optional<Tensor>& ws1n, const c10::optional<Tensor>& b1n, int64_t c, int64_t nout, int64_t cn, int64_t tile_m, int64_t flags,
                                            const c10::optional<Tensor>& t1b, int64_t t1b_c0, int64_t cb, int64_t t1b_stride) {
  dev(t1, "t1", at::kFloat);
  FCP_DEVICE_GUARD(t1);
  const bool two = t1b.has_value() && t1b->defined();              // two-source pair: the trailing cb input channels come from t1b
  TORCH_CHECK(t1.dim() == 4 && t1_c0 + c - (two ? cb : 0) <= t1.size(3), "t1 (n,h,w,>=c) split32 buffer");
  const bool has_res = res.has_value() && res->defined();
  if (has_res) {
    dev(*res, "res", at::kFloat);
    TORCH_CHECK(res->dim() == 4 && res_c0 + nout <= res->size(3), "res (n,h,w,>=nout) split32 buffer");
  }
  Tensor out = at::empty({t1.size(0), t1.size(1), t1.size(2), nout}, t1.options());
  Tensor t1n = at::empty({t1.size(0), t1.size(1), t1.size(2), cn}, t1.options());
  fcp_chain_desc d = {};
  d.t1 = t1.data_ptr<float>() + t1_c0; d.out = out.data_ptr<float>(); d.t1n = t1n.data_ptr<float>();
  if (has_res) { d.res = res->data_ptr<float>() + res_c0; d.res_ld = (int)res->size(3); }
  if (w2.has_value() && w2->defined()) {
    d.w2 = w2->data_ptr(); d.ws2 = optp<float>(ws2, "ws2", at::kFloat); d.b2 = optp<float>(b2, "b2", at::kFloat);
  }
  d.w3 = w3.data_ptr(); d.ws3 = dev(ws3, "ws3", at::kFloat).data_ptr<float>(); d.b3 = dev(b3, "b3", at::kFloat).data_ptr<float>();
  // expand form (cn == 0): conv3 + residual alone, no next conv1 — its filter is absent and t1n comes back with 0 channels
  const bool has_next = w1n.has_value() && w1n->defined();
  TORCH_CHECK(has_next == (cn > 0), "w1n / ws1n / b1n are given exactly when cn > 0 (cn == 0: the expand form)");
  if (has_next) {
    d.w1n = w1n->data_ptr(); d.ws1n = optp<float>(ws1n, "ws1n", at::kFloat); d.b1n = optp<float>(b1n, "b1n", at::kFloat);
    TORCH_CHECK(d.ws1n && d.b1n, "ws1n and b1n accompany w1n");
  } else {
    d.t1n = nullptr;
  }
  d.n = (int)t1.size(0); d.h = (int)t1.size(1); d.w = (int)t1.size(2); d.c = (int)c; d.cn = (int)cn; d.nout = (int)nout;
  d.t1_ld = (int)t1.size(3); d.out_ld = (int)nout; d.t1n_ld = (int)cn; d.tile_m = (int)tile_m; d.flags = (int)flags;
  if (two) {
    dev(*t1b, "t1b", at::kFloat);
    TORCH_CHECK(t1b->dim() == 4 && t1b->size(0) == t1.size(0) && t1b_c0 + cb <= t1b->size(3), "t1b (n,hb,wb,>=cb) split32 buffer");
    d.t1b = t1b->data_ptr<float>() + t1b_c0; d.cb = (int)cb; d.t1b_ld = (int)t1b->size(3);
    d.t1b_h = (int)t1b->size(1); d.t1b_w = (int)t1b->size(2); d.t1b_stride = (int)t1b_stride;
  }
  ok(fcp_bottleneck_chain_f16x3(&d, cur_stream()), "fcp::bottleneck_chain");
  return {out, t1n};
}

// ---- detect_postprocess: three fused head maps -> compacted candidates
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> retina_decode(const Tensor& h0, const Tensor& h1, const Tensor& h2,
                                                                 int64_t img_h, int64_t img_w, double vis, double var0,
                                                                 double var1) {
  dev(h0, "head0", at::kFloat); dev(h1, "head1", at::kFloat); dev(h2, "head2", at::kFloat);
  FCP_DEVICE_GUARD(h0);
  TORCH_CHECK(img_h > 0 && img_w > 0, "image size must be positive");
  TORCH_CHECK(h0.dim() == 4, "head maps are (n, ceil(h/s), ceil(w/s), 32) fp32 NHWC");
  const int64_t n = h0.size(0);
  int64_t P = 0;
  const Tensor* heads[3] = {&h0, &h1, &h2};
  int li = 0;
  for (int64_t s : {8, 16, 32}) {
    const Tensor& h = *heads[li++];
    const int64_t fh = (img_h + s - 1) / s, fw = (img_w + s - 1) / s;
    TORCH_CHECK(h.dim() == 4 && h.size(0) == n && h.size(1) == fh && h.size(2) == fw && h.size(3) == 32,
                "head map of stride ", s, " must be (", n, ", ", fh, ", ", fw, ", 32) for a ", img_h, " x ", img_w, " image, got ",
                h.sizes());
    P += 2 * fh * fw;
  }
  auto f = h0.options();
  auto i = h0.options().dtype(at::kInt);
  Tensor score = at::empty({n, P}, f), box = at::empty({n, P, 4}, f), ldm = at::empty({n, P, 10}, f);
  Tensor prior = at::empty({n, P}, i), count = at::empty({n}, i);
  ok(fcp_retina_decode(h0.data_ptr<float>(), h1.data_ptr<float>(), h2.data_ptr<float>(), (int)n, (int)img_h, (int)img_w,
                       (float)vis, (float)var0, (float)var1, score.data_ptr<float>(), box.data_ptr<float>(),
                       ldm.data_ptr<float>(), prior.data_ptr<int>(), count.data_ptr<int>(), nullptr, nullptr, nullptr,
                       cur_stream()), "fcp::retina_decode");
  return {score, box, ldm, prior, count};
}

std::tuple<Tensor, Tensor, Tensor, Tensor> nms_select(const Tensor& score, const Tensor& box, const Tensor& count,
                                                      double thr, int64_t strategy) {
  dev(score, "cand_score", at::kFloat); dev(box, "cand_box", at::kFloat); dev(count, "cand_count", at::kInt);
  FCP_DEVICE_GUARD(score);
  TORCH_CHECK(score.dim() == 2, "cand_score is (n, cap)");
  const int64_t n = score.size(0), cap = score.size(1);
  TORCH_CHECK(box.dim() == 3 && box.size(0) == n && box.size(1) == cap && box.size(2) == 4, "cand_box must be (", n, ", ", cap,
              ", 4), got ", box.sizes());
  TORCH_CHECK(count.dim() == 1 && count.size(0) == n, "cand_count must be (", n, ",), got ", count.sizes());
  TORCH_CHECK(strategy >= 0 && strategy <= 2, "strategy: 0 all, 1 best, 2 largest");
  auto i = score.options().dtype(at::kInt);
  Tensor ws = at::empty({fcp_retina_nms_workspace_bytes((int)n, (int)cap)}, score.options().dtype(at::kByte));
  Tensor keep_pos = at::empty({n, cap}, i), keep_count = at::empty({n}, i), sel_pos = at::empty({n, cap}, i), sel_count = at::empty({n}, i);
  ok(fcp_retina_nms_select(score.data_ptr<float>(), box.data_ptr<float>(), count.data_ptr<int>(), (int)n, (int)cap, (float)thr,
                           (int)strategy, ws.data_ptr(), keep_pos.data_ptr<int>(), keep_count.data_ptr<int>(),
                           sel_pos.data_ptr<int>(), sel_count.data_ptr<int>(), cur_stream()), "fcp::nms_select");
  return {keep_pos, keep_count, sel_pos, sel_count};
}

std::tuple<Tensor, Tensor, Tensor> gather_faces(const Tensor& ldm, const Tensor& sel_pos, const Tensor& sel_count,
                                                const c10::optional<Tensor>& paddings, int64_t max_faces) {
  dev(ldm, "cand_ldm", at::kFloat); dev(sel_pos, "sel_pos", at::kInt); dev(sel_count, "sel_count", at::kInt);
  FCP_DEVICE_GUARD(ldm);
  TORCH_CHECK(sel_pos.dim() == 2, "sel_pos is (n, cap)");
  const int64_t n = sel_pos.size(0), cap = sel_pos.size(1);
  TORCH_CHECK(ldm.dim() == 3 && ldm.size(0) == n && ldm.size(1) == cap && ldm.size(2) == 10, "cand_ldm must be (", n, ", ", cap,
              ", 10), got ", ldm.sizes());
  TORCH_CHECK(sel_count.dim() == 1 && sel_count.size(0) == n, "sel_count must be (", n, ",), got ", sel_count.sizes());
  TORCH_CHECK(max_faces >= 1, "max_faces must be >= 1");
  if (paddings.has_value() && paddings->defined())
    TORCH_CHECK(paddings->dim() == 2 && paddings->size(0) == n && paddings->size(1) == 4, "paddings must be (", n, ", 4)");
  auto i = ldm.options().dtype(at::kInt);
  Tensor off = at::empty({n + 1}, i), out_ldm = at::empty({max_faces, 5, 2}, ldm.options()), out_img = at::empty({max_faces}, i);
  ok(fcp_retina_gather_faces(ldm.data_ptr<float>(), sel_pos.data_ptr<int>(), sel_count.data_ptr<int>(), (int)n, (int)cap,
                             optp<int>(paddings, "paddings", at::kInt), (int)max_faces, off.data_ptr<int>(),
                             out_ldm.data_ptr<float>(), out_img.data_ptr<int>(), cur_stream()), "fcp::gather_faces");
  return {out_ldm, out_img, off};
}

// face_count: optional device int32 scalar (live rows of a fixed-capacity face array); valid_total: optional device
// int64 scalar the number of ok faces is ADDED to (declared mutable in the schema).
std::tuple<Tensor, Tensor> similarity_from_5pt(const Tensor& src, const Tensor& dst, bool allow_skew,
                                               const c10::optional<Tensor>& face_count,
                                               const c10::optional<Tensor>& valid_total) {
  dev(src, "src", at::kFloat); dev(dst, "dst", at::kFloat);
  FCP_DEVICE_GUARD(src);
  TORCH_CHECK(src.dim() == 3 && src.size(2) == 2 && dst.dim() == 2 && dst.size(0) == src.size(1), "src (f,k,2), dst (k,2)");
  const int64_t f = src.size(0);
  Tensor mat = at::empty({f, 2, 3}, src.options().dtype(at::kDouble)), okf = at::empty({f}, src.options().dtype(at::kInt));
  const int* fc = optp<int>(face_count, "face_count", at::kInt);
  int64_t* vt = const_cast<int64_t*>(optp<int64_t>(valid_total, "valid_total", at::kLong));
  TORCH_CHECK(fc == nullptr || face_count->numel() == 1, "face_count is a scalar");
  TORCH_CHECK(vt == nullptr || valid_total->numel() == 1, "valid_total is a scalar");
  ok(fcp_estimate_transform_counted(src.data_ptr<float>(), dst.data_ptr<float>(), (int)f, (int)src.size(1), allow_skew, fc,
                                    mat.data_ptr<double>(), okf.data_ptr<int>(), vt, cur_stream()),
     "fcp::similarity_from_5pt");
  return {mat, okf};
}

// Both warpAffine families and the cubic / Lanczos-4 warps share parameters and checks; only the C entry point differs
// (`fn` takes fcp_warp_affine_u8's parameters).

template <class Fn>
Tensor warp_affine_with(Fn fn, const char* what, const Tensor& images, const Tensor& img_idx, const Tensor& mat,
                        const c10::optional<Tensor>& okf, const c10::optional<Tensor>& paddings, int64_t out_w, int64_t out_h,
                        int64_t border) {
  dev(images, "images", at::kByte); dev(img_idx, "img_idx", at::kInt); dev(mat, "mat", at::kDouble);
  FCP_DEVICE_GUARD(images);
  TORCH_CHECK(images.dim() == 4 && images.size(3) == 3, "images (n,h,w,3) uint8");
  const int64_t f = img_idx.size(0);
  TORCH_CHECK(mat.dim() == 3 && mat.size(0) == f && mat.size(1) == 2 && mat.size(2) == 3, "mat must be (", f, ", 2, 3) float64");
  Tensor out = at::empty({f, out_h, out_w, 3}, images.options());
  ok(fn(images.data_ptr<uint8_t>(), (int)images.size(0), (int)images.size(1), (int)images.size(2), img_idx.data_ptr<int>(),
        mat.data_ptr<double>(), optp<int>(okf, "ok", at::kInt), optp<int>(paddings, "paddings", at::kInt), (int)f, (int)out_h,
        (int)out_w, (int)border, out.data_ptr<uint8_t>(), cur_stream()), what);
  return out;
}

Tensor warp_affine_u8(const Tensor& images, const Tensor& img_idx, const Tensor& mat, const c10::optional<Tensor>& okf,
                      const c10::optional<Tensor>& paddings, int64_t out_w, int64_t out_h, int64_t border) {
  return warp_affine_with(fcp_warp_affine_u8, "fcp::warp_affine_u8", images, img_idx, mat, okf, paddings, out_w, out_h, border);
}

Tensor warp_affine_u8_float(const Tensor& images, const Tensor& img_idx, const Tensor& mat, const c10::optional<Tensor>& okf,
                            const c10::optional<Tensor>& paddings, int64_t out_w, int64_t out_h, int64_t border) {
  return warp_affine_with(fcp_warp_affine_u8_float, "fcp::warp_affine_u8_float", images, img_idx, mat, okf, paddings, out_w,
                          out_h, border);
}

// interp: cv2.INTER_CUBIC (2) or cv2.INTER_LANCZOS4 (4); anything else is refused by the C entry point.
Tensor warp_affine_u8_interp(const Tensor& images, const Tensor& img_idx, const Tensor& mat, const c10::optional<Tensor>& okf,
                             const c10::optional<Tensor>& paddings, int64_t out_w, int64_t out_h, int64_t border,
                             int64_t interp) {
  const int ip = (int)interp;
  return warp_affine_with(
      [ip](const uint8_t* im, int n, int h, int w, const int32_t* idx, const double* m, const int32_t* okp, const int32_t* pad,
           int f, int oh, int ow, int b, uint8_t* out, fcp_stream_t st) {
        return fcp_warp_affine_u8_interp(im, n, h, w, idx, m, okp, pad, f, oh, ow, b, ip, out, st);
      },
      "fcp::warp_affine_u8_interp", images, img_idx, mat, okf, paddings, out_w, out_h, border);
}

// Host table of fixed-size records (fcp_warp_src / fcp_area_level) passed as a CPU int64 (n, words) tensor: validated by the
// C entry point on the host, copied to the device of `like` for the kernel (stream-ordered behind any earlier work).
const Tensor& host_table(const Tensor& t, const char* name, int64_t words) {
  TORCH_CHECK(!t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous() && t.dim() == 2 && t.size(1) == words, name,
              " must be a contiguous CPU int64 (n, ", words, ") tensor of records");
  return t;
}

// crop_source="original": one source image per face in a byte blob (fcp_warp_src records: srcs (f,2) int64 on the host).
// `check` runs after the tensor checks; `fn` takes fcp_warp_affine_u8_ragged's parameters.
template <class Check, class Fn>
Tensor warp_affine_ragged_with(Check check, Fn fn, const char* what, const Tensor& blob, const Tensor& srcs, const Tensor& mat,
                               const c10::optional<Tensor>& okf, int64_t out_w, int64_t out_h, int64_t border) {
  dev(blob, "blob", at::kByte); dev(mat, "mat", at::kDouble); host_table(srcs, "srcs", 2);
  FCP_DEVICE_GUARD(blob);
  check();
  const int64_t f = srcs.size(0);
  TORCH_CHECK(mat.numel() == f * 6, "mat must hold (", f, ", 6) float64");
  TORCH_CHECK(!okf.has_value() || !okf->defined() || okf->numel() == f, "ok must hold ", f, " flags");
  Tensor srcs_dev = srcs.to(blob.device(), /*non_blocking=*/true);
  Tensor out = at::empty({f, out_h, out_w, 3}, blob.options());
  const auto* host = reinterpret_cast<const fcp_warp_src*>(srcs.data_ptr<int64_t>());
  const auto* devp = reinterpret_cast<const fcp_warp_src*>(srcs_dev.data_ptr<int64_t>());
  ok(fn(blob.data_ptr<uint8_t>(), blob.numel(), host, devp, mat.data_ptr<double>(), optp<int>(okf, "ok", at::kInt), (int)f,
        (int)out_h, (int)out_w, (int)border, out.data_ptr<uint8_t>(), cur_stream()),
     what);
  return out;
}

// family 0 = fixed-point, 1 = float32 (align.WARP_FAMILIES).
Tensor warp_affine_u8_ragged(const Tensor& blob, const Tensor& srcs, const Tensor& mat, const c10::optional<Tensor>& okf,
                             int64_t out_w, int64_t out_h, int64_t border, int64_t family) {
  return warp_affine_ragged_with(
      [family] { TORCH_CHECK(family == 0 || family == 1, "family must be 0 (fixed) or 1 (float32)"); },
      family == 0 ? fcp_warp_affine_u8_ragged : fcp_warp_affine_u8_float_ragged, "fcp::warp_affine_u8_ragged", blob, srcs,
      mat, okf, out_w, out_h, border);
}

// interp: cv2.INTER_CUBIC (2) or cv2.INTER_LANCZOS4 (4), as warp_affine_u8_interp.
Tensor warp_affine_u8_interp_ragged(const Tensor& blob, const Tensor& srcs, const Tensor& mat, const c10::optional<Tensor>& okf,
                                    int64_t out_w, int64_t out_h, int64_t border, int64_t interp) {
  const int ip = (int)interp;
  return warp_affine_ragged_with(
      [] {},
      [ip](const uint8_t* b, int64_t bytes, const fcp_warp_src* sh, const fcp_warp_src* sd, const double* m, const int32_t* okp,
           int f, int oh, int ow, int bd, uint8_t* out, fcp_stream_t st) {
        return fcp_warp_affine_u8_interp_ragged(b, bytes, sh, sd, m, okp, f, oh, ow, bd, ip, out, st);
      },
      "fcp::warp_affine_u8_interp_ragged", blob, srcs, mat, okf, out_w, out_h, border);
}

// INTER_AREA levels of a ragged batch (fcp_area_level records: levels (n,4) int64 on the host), written into dst in place.
void resize_area_u8_ragged(const Tensor& src, const Tensor& levels, const Tensor& dst) {
  dev(src, "src", at::kByte); dev(dst, "dst", at::kByte); host_table(levels, "levels", 4);
  FCP_DEVICE_GUARD(src);
  const int64_t n = levels.size(0);
  if (n == 0) return;
  Tensor levels_dev = levels.to(src.device(), /*non_blocking=*/true);
  ok(fcp_resize_area_ragged_u8(src.data_ptr<uint8_t>(), src.numel(),
                               reinterpret_cast<const fcp_area_level*>(levels.data_ptr<int64_t>()),
                               reinterpret_cast<const fcp_area_level*>(levels_dev.data_ptr<int64_t>()), (int)n,
                               dst.data_ptr<uint8_t>(), dst.numel(), cur_stream()),
     "fcp::resize_area_u8_ragged");
}

// Laplacian-variance sums of crops (f,h,w,3) uint8: (f,2) int64 {S1, S2} (fcp_crop_sharpness_u8; the host divides).
Tensor crop_sharpness(const Tensor& crops, const c10::optional<Tensor>& okf) {
  dev(crops, "crops", at::kByte);
  FCP_DEVICE_GUARD(crops);
  TORCH_CHECK(crops.dim() == 4 && crops.size(3) == 3, "crops (f,h,w,3) uint8");
  const int64_t f = crops.size(0), h = crops.size(1), w = crops.size(2);
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX, "crops (f,h,w,3): sizes past int");
  TORCH_CHECK(!okf.has_value() || !okf->defined() || okf->numel() == f, "ok must hold ", f, " flags");
  Tensor sums = at::empty({f, 2}, crops.options().dtype(at::kLong));
  ok(fcp_crop_sharpness_u8(crops.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, optp<int>(okf, "ok", at::kInt),
                           sums.data_ptr<int64_t>(), cur_stream()),
     "fcp::crop_sharpness");
  return sums;
}

// JPEG entropy-coded segments + EOI of crops (f,h,w,3) or (f,h,w) uint8 into the rows of `out` (f, capacity) uint8 — rows
// may be a view of a wider buffer (unit stride inside a row) — and the true lengths (f,) int32, which may exceed the
// capacity (fcp_jpeg_encode_u8; the header is written on the host).  The workspace comes from the caching allocator.
Tensor jpeg_encode(const Tensor& crops, int64_t quality, int64_t subsampling, const Tensor& out) {
  dev(crops, "crops", at::kByte);
  FCP_DEVICE_GUARD(crops);
  TORCH_CHECK((crops.dim() == 4 && (crops.size(3) == 3 || crops.size(3) == 1)) || crops.dim() == 3,
              "crops (f,h,w,3) or (f,h,w) uint8");
  const int64_t f = crops.size(0), h = crops.size(1), w = crops.size(2), c = crops.dim() == 4 ? crops.size(3) : 1;
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX, "crops: sizes past int");
  TORCH_CHECK(quality >= INT_MIN && quality <= INT_MAX && subsampling >= INT_MIN && subsampling <= INT_MAX,
              "quality / subsampling past int");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kByte && out.get_device() == crops.get_device(),
              "out must be a uint8 tensor on the device of the crops");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == f, "out must be (", f, ", capacity)");
  const int64_t capacity = out.size(1), stride = f > 1 ? out.stride(0) : capacity;
  TORCH_CHECK(capacity == 0 || out.stride(1) == 1, "out: the bytes of a row must be contiguous");
  TORCH_CHECK(stride >= capacity, "out: rows overlap");
  Tensor lengths = at::empty({f}, crops.options().dtype(at::kInt));
  const int64_t need = fcp_jpeg_workspace_bytes((int)f, (int)h, (int)w, (int)c);
  ok(need < 0 ? -1 : 0, "fcp::jpeg_encode");
  Tensor work = at::empty({need}, crops.options());
  ok(fcp_jpeg_encode_u8(crops.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (int)c, (int)quality, (int)subsampling,
                        capacity > 0 ? out.data_ptr<uint8_t>() : nullptr, stride, capacity, lengths.data_ptr<int32_t>(),
                        work.data_ptr(), need, cur_stream()),
     "fcp::jpeg_encode");
  return lengths;
}

// jpeg_encode with the caller's chroma subsampling (0 / 1 / 2) and, when `tables` (f,4,272) uint8 is given, Huffman tables
// made for every face, which are written there (fcp_jpeg_encode_ex_u8).
Tensor jpeg_encode_ex(const Tensor& crops, int64_t quality, int64_t subsampling, const Tensor& out,
                      const c10::optional<Tensor>& tables) {
  dev(crops, "crops", at::kByte);
  FCP_DEVICE_GUARD(crops);
  TORCH_CHECK((crops.dim() == 4 && (crops.size(3) == 3 || crops.size(3) == 1)) || crops.dim() == 3,
              "crops (f,h,w,3) or (f,h,w) uint8");
  const int64_t f = crops.size(0), h = crops.size(1), w = crops.size(2), c = crops.dim() == 4 ? crops.size(3) : 1;
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX, "crops: sizes past int");
  TORCH_CHECK(quality >= INT_MIN && quality <= INT_MAX && subsampling >= INT_MIN && subsampling <= INT_MAX,
              "quality / subsampling past int");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kByte && out.get_device() == crops.get_device(),
              "out must be a uint8 tensor on the device of the crops");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == f, "out must be (", f, ", capacity)");
  const int64_t capacity = out.size(1), stride = f > 1 ? out.stride(0) : capacity;
  TORCH_CHECK(capacity == 0 || out.stride(1) == 1, "out: the bytes of a row must be contiguous");
  TORCH_CHECK(stride >= capacity, "out: rows overlap");
  const bool optimize = tables.has_value() && tables->defined();
  if (optimize) {
    const Tensor& t = *tables;
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kByte && t.get_device() == crops.get_device() && t.is_contiguous() &&
                    t.dim() == 3 && t.size(0) == f && t.size(1) == 4 && t.size(2) == 272,
                "tables must be a contiguous (", f, ",4,272) uint8 tensor on the device of the crops");
  }
  Tensor lengths = at::empty({f}, crops.options().dtype(at::kInt));
  const int64_t need = fcp_jpeg_workspace_bytes_ex((int)f, (int)h, (int)w, (int)c, (int)subsampling, optimize ? 1 : 0);
  ok(need < 0 ? -1 : 0, "fcp::jpeg_encode_ex");
  Tensor work = at::empty({need}, crops.options());
  ok(fcp_jpeg_encode_ex_u8(crops.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (int)c, (int)quality, (int)subsampling,
                           optimize ? 1 : 0, capacity > 0 ? out.data_ptr<uint8_t>() : nullptr, stride, capacity,
                           lengths.data_ptr<int32_t>(), optimize ? tables->data_ptr<uint8_t>() : nullptr, work.data_ptr(), need,
                           cur_stream()),
     "fcp::jpeg_encode_ex");
  return lengths;
}

// Rows of 256 symbol counts (n,256) int32 -> libjpeg's optimal Huffman tables: the records (n,272) uint8 and, with
// `with_codes`, code | length << 16 by symbol (n,256) int32 (else an empty tensor) (fcp_jpeg_huffman_tables).
std::tuple<Tensor, Tensor> jpeg_huffman_tables(const Tensor& freq, bool with_codes) {
  dev(freq, "freq", at::kInt);
  FCP_DEVICE_GUARD(freq);
  TORCH_CHECK(freq.dim() == 2 && freq.size(1) == 256 && freq.is_contiguous(), "freq (n,256) int32, contiguous");
  const int64_t n = freq.size(0);
  TORCH_CHECK(n <= INT_MAX, "freq: rows past int");
  Tensor tables = at::empty({n, 272}, freq.options().dtype(at::kByte));
  Tensor codes = with_codes ? at::empty({n, 256}, freq.options()) : at::empty({0}, freq.options());
  ok(fcp_jpeg_huffman_tables(reinterpret_cast<const uint32_t*>(freq.data_ptr<int32_t>()), (int)n, tables.data_ptr<uint8_t>(),
                             with_codes ? reinterpret_cast<uint32_t*>(codes.data_ptr<int32_t>()) : nullptr, cur_stream()),
     "fcp::jpeg_huffman_tables");
  return {tables, codes};
}

// zlib streams for PNG files of faces (f,h,w,3), (f,h,w,4) or (f,h,w) uint8 into the rows of `out` (f, capacity) uint8 — rows may
// be a view of a wider buffer (unit stride inside a row) — and the true lengths (f,) int32, which may exceed the capacity
// (fcp_png_encode_u8; the file around a stream is written on the host).  The workspace comes from the caching allocator.
Tensor png_encode(const Tensor& pixels, const Tensor& out) {
  dev(pixels, "pixels", at::kByte);
  FCP_DEVICE_GUARD(pixels);
  TORCH_CHECK((pixels.dim() == 4 && (pixels.size(3) == 3 || pixels.size(3) == 4 || pixels.size(3) == 1)) || pixels.dim() == 3,
              "pixels (f,h,w,3), (f,h,w,4) or (f,h,w) uint8");
  const int64_t f = pixels.size(0), h = pixels.size(1), w = pixels.size(2), c = pixels.dim() == 4 ? pixels.size(3) : 1;
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX, "pixels: sizes past int");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kByte && out.get_device() == pixels.get_device(),
              "out must be a uint8 tensor on the device of the pixels");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == f, "out must be (", f, ", capacity)");
  const int64_t capacity = out.size(1), stride = f > 1 ? out.stride(0) : capacity;
  TORCH_CHECK(capacity == 0 || out.stride(1) == 1, "out: the bytes of a row must be contiguous");
  TORCH_CHECK(stride >= capacity, "out: rows overlap");
  Tensor lengths = at::empty({f}, pixels.options().dtype(at::kInt));
  const int64_t need = fcp_png_workspace_bytes((int)f, (int)h, (int)w, (int)c);
  ok(need < 0 ? -1 : 0, "fcp::png_encode");
  Tensor work = at::empty({need}, pixels.options());
  ok(fcp_png_encode_u8(pixels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (int)c,
                       capacity > 0 ? out.data_ptr<uint8_t>() : nullptr, stride, capacity, lengths.data_ptr<int32_t>(),
                       work.data_ptr(), need, cur_stream()),
     "fcp::png_encode");
  return lengths;
}

// Rows of 286 literal/length counts (n,286) int32 -> their deflate code lengths (n,286) uint8 and, with `with_codes`,
// bit-reversed code | length << 16 by symbol (n,286) int32 (else an empty tensor) (fcp_png_huffman_lengths).
std::tuple<Tensor, Tensor> png_huffman_lengths(const Tensor& freq, bool with_codes) {
  dev(freq, "freq", at::kInt);
  FCP_DEVICE_GUARD(freq);
  TORCH_CHECK(freq.dim() == 2 && freq.size(1) == 286 && freq.is_contiguous(), "freq (n,286) int32, contiguous");
  const int64_t n = freq.size(0);
  TORCH_CHECK(n <= INT_MAX, "freq: rows past int");
  Tensor lengths = at::empty({n, 286}, freq.options().dtype(at::kByte));
  Tensor codes = with_codes ? at::empty({n, 286}, freq.options()) : at::empty({0}, freq.options());
  ok(fcp_png_huffman_lengths(reinterpret_cast<const uint32_t*>(freq.data_ptr<int32_t>()), (int)n, lengths.data_ptr<uint8_t>(),
                             with_codes ? reinterpret_cast<uint32_t*>(codes.data_ptr<int32_t>()) : nullptr, cur_stream()),
     "fcp::png_huffman_lengths");
  return {lengths, codes};
}

// The shape checks the matte family shares: crops (f,h,w,3) and a plane (f,h,w) of its own, both uint8 on one device.
static void crops_and_plane(const Tensor& crops, const Tensor& plane, const char* name, int64_t& f, int64_t& h, int64_t& w) {
  TORCH_CHECK(crops.dim() == 4 && crops.size(3) == 3, "crops (f,h,w,3) uint8");
  f = crops.size(0), h = crops.size(1), w = crops.size(2);
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX, "crops (f,h,w,3): sizes past int");
  TORCH_CHECK(plane.get_device() == crops.get_device() && plane.dim() == 3 && plane.size(0) == f && plane.size(1) == h &&
                  plane.size(2) == w, name, " must be (", f, ",", h, ",", w, ") uint8 on the device of the crops");
}

// The same for the ops that take label maps (f,h,w) uint8 alone.
static void labels_plane(const Tensor& labels, int64_t class_bits, int64_t& f, int64_t& h, int64_t& w) {
  TORCH_CHECK(labels.dim() == 3, "labels (f,h,w) uint8");
  f = labels.size(0), h = labels.size(1), w = labels.size(2);
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX, "labels (f,h,w): sizes past int");
  TORCH_CHECK(class_bits >= 0 && class_bits <= (int64_t)UINT_MAX, "class_bits past 32 bits");
}

// taps = t[0..radius] of the op `name` as the 16-bit table of the C ABI; returns the radius (0 for the empty list that
// `allow_empty` lets through).
static int taps16(const char* name, at::IntArrayRef taps, bool allow_empty, uint16_t (&t16)[49]) {
  const int64_t radius = (int64_t)taps.size() - 1;
  TORCH_CHECK((allow_empty && taps.empty()) || (radius >= 3 && radius <= 48), name, ": taps must be ", allow_empty ? "empty or " : "",
              "t[0..radius] with radius 3..48 (got ", taps.size(), " taps)");
  for (int64_t k = 0; k <= radius; ++k) {
    TORCH_CHECK(taps[k] >= 0 && taps[k] <= 65535, name, ": tap ", k, " past 16 bits");
    t16[k] = (uint16_t)taps[k];
  }
  return taps.empty() ? 0 : (int)radius;
}

// The workspace of a call: `need` bytes (an fcp_*_workspace_bytes; negative for sizes the entry point refuses) from the
// caching allocator, on the device of `like` (uint8).
static Tensor workspace(int64_t need, const Tensor& like) { return at::empty({need < 0 ? 0 : need}, like.options()); }

// Crops (f,h,w,3) uint8 over a uniform fill through the soft mask of their label maps (f,h,w) uint8: the composited
// crops and, with `with_alpha`, the alpha (f,h,w) uint8 (else an empty tensor) (fcp_matte_u8).
std::tuple<Tensor, Tensor> matte(const Tensor& crops, const Tensor& labels, int64_t class_bits, int64_t feather, int64_t bg_r,
                                 int64_t bg_g, int64_t bg_b, bool with_alpha) {
  dev(crops, "crops", at::kByte);
  dev(labels, "labels", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, labels, "labels", f, h, w);
  TORCH_CHECK(class_bits >= 0 && class_bits <= (int64_t)UINT_MAX, "class_bits past 32 bits");
  for (int64_t v : {feather, bg_r, bg_g, bg_b}) TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, "feather / fill past int");
  Tensor out = at::empty_like(crops);
  Tensor alpha = with_alpha ? at::empty({f, h, w}, crops.options()) : at::empty({0}, crops.options());
  ok(fcp_matte_u8(crops.data_ptr<uint8_t>(), labels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (uint32_t)class_bits,
                  (int)feather, (int)bg_r, (int)bg_g, (int)bg_b, out.data_ptr<uint8_t>(),
                  with_alpha ? alpha.data_ptr<uint8_t>() : nullptr, cur_stream()),
     "fcp::matte");
  return {out, alpha};
}

// Crops (f,h,w,3) uint8 over their own mask-normalised background blur through the soft mask of their label maps
// (f,h,w) uint8: the composited crops and, with `with_alpha`, the alpha (f,h,w) uint8 (else an empty tensor)
// (fcp_matte_blur_u8).  taps = t[0..radius] as integers; the 16-bytes-per-pixel workspace lives for the call.
std::tuple<Tensor, Tensor> matte_blur(const Tensor& crops, const Tensor& labels, int64_t class_bits, int64_t feather,
                                      at::IntArrayRef taps, bool with_alpha) {
  dev(crops, "crops", at::kByte);
  dev(labels, "labels", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, labels, "labels", f, h, w);
  TORCH_CHECK(class_bits >= 0 && class_bits <= (int64_t)UINT_MAX, "class_bits past 32 bits");
  TORCH_CHECK(feather >= INT_MIN && feather <= INT_MAX, "feather past int");
  uint16_t t16[49];
  const int radius = taps16("matte_blur", taps, false, t16);
  Tensor out = at::empty_like(crops);
  Tensor alpha = with_alpha ? at::empty({f, h, w}, crops.options()) : at::empty({0}, crops.options());
  Tensor work = workspace(fcp_matte_blur_workspace_bytes((int)f, (int)h, (int)w), crops);
  ok(fcp_matte_blur_u8(crops.data_ptr<uint8_t>(), labels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (uint32_t)class_bits,
                       (int)feather, t16, radius, out.data_ptr<uint8_t>(), with_alpha ? alpha.data_ptr<uint8_t>() : nullptr,
                       work.data_ptr(), work.numel(), cur_stream()),
     "fcp::matte_blur");
  return {out, alpha};
}

// The guided-filter alpha (f,h,w) uint8 of crops (f,h,w,3) uint8 and their label maps (f,h,w) uint8
// (fcp_matte_refine_u8); the 8-bytes-per-pixel workspace lives for the call.
Tensor matte_refine(const Tensor& crops, const Tensor& labels, int64_t class_bits, int64_t radius, int64_t eps) {
  dev(crops, "crops", at::kByte);
  dev(labels, "labels", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, labels, "labels", f, h, w);
  TORCH_CHECK(class_bits >= 0 && class_bits <= (int64_t)UINT_MAX, "class_bits past 32 bits");
  for (int64_t v : {radius, eps}) TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, "radius / eps past int");
  Tensor alpha = at::empty({f, h, w}, crops.options());
  Tensor work = workspace(fcp_matte_refine_workspace_bytes((int)f, (int)h, (int)w), crops);
  ok(fcp_matte_refine_u8(crops.data_ptr<uint8_t>(), labels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (uint32_t)class_bits,
                         (int)radius, (int)eps, alpha.data_ptr<uint8_t>(), work.data_ptr(), work.numel(), cur_stream()),
     "fcp::matte_refine");
  return alpha;
}

// Crops (f,h,w,3) uint8 over a uniform fill through an alpha plane (f,h,w) uint8 of the caller's (fcp_matte_alpha_u8).
Tensor matte_alpha(const Tensor& crops, const Tensor& alpha, int64_t bg_r, int64_t bg_g, int64_t bg_b) {
  dev(crops, "crops", at::kByte);
  dev(alpha, "alpha", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, alpha, "alpha", f, h, w);
  for (int64_t v : {bg_r, bg_g, bg_b}) TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, "fill past int");
  Tensor out = at::empty_like(crops);
  ok(fcp_matte_alpha_u8(crops.data_ptr<uint8_t>(), alpha.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (int)bg_r, (int)bg_g,
                        (int)bg_b, out.data_ptr<uint8_t>(), cur_stream()),
     "fcp::matte_alpha");
  return out;
}

// Crops (f,h,w,3) uint8 over their own mask-normalised background blur (the hard mask of labels) through an alpha plane
// (f,h,w) uint8 of the caller's (fcp_matte_blur_alpha_u8).  taps as in matte_blur.
Tensor matte_blur_alpha(const Tensor& crops, const Tensor& labels, const Tensor& alpha, int64_t class_bits, at::IntArrayRef taps) {
  dev(crops, "crops", at::kByte);
  dev(labels, "labels", at::kByte);
  dev(alpha, "alpha", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, labels, "labels", f, h, w);
  crops_and_plane(crops, alpha, "alpha", f, h, w);
  TORCH_CHECK(class_bits >= 0 && class_bits <= (int64_t)UINT_MAX, "class_bits past 32 bits");
  uint16_t t16[49];
  const int radius = taps16("matte_blur_alpha", taps, false, t16);
  Tensor out = at::empty_like(crops);
  Tensor work = workspace(fcp_matte_blur_workspace_bytes((int)f, (int)h, (int)w), crops);
  ok(fcp_matte_blur_alpha_u8(crops.data_ptr<uint8_t>(), labels.data_ptr<uint8_t>(), alpha.data_ptr<uint8_t>(), (int)f, (int)h,
                             (int)w, (uint32_t)class_bits, t16, radius, out.data_ptr<uint8_t>(), work.data_ptr(), work.numel(),
                             cur_stream()),
     "fcp::matte_blur_alpha");
  return out;
}

// The feathered alpha (f,h,w) uint8 of label maps (f,h,w) uint8: fcp_matte_u8's alpha alone (fcp_feather_alpha_u8).
Tensor feather_alpha(const Tensor& labels, int64_t class_bits, int64_t feather) {
  dev(labels, "labels", at::kByte);
  FCP_DEVICE_GUARD(labels);
  int64_t f, h, w;
  labels_plane(labels, class_bits, f, h, w);
  TORCH_CHECK(feather >= INT_MIN && feather <= INT_MAX, "feather past int");
  Tensor alpha = at::empty_like(labels);
  ok(fcp_feather_alpha_u8(labels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (uint32_t)class_bits, (int)feather,
                          alpha.data_ptr<uint8_t>(), cur_stream()),
     "fcp::feather_alpha");
  return alpha;
}

// Crops (f,h,w,3) uint8 and an alpha plane (f,h,w) uint8 -> the RGBA cut-out (f,h,w,4) (mode 0) or the composite over a
// uniform fill (f,h,w,3) (mode 1), with the subject's colour estimated through taps = t[0..radius] (empty: no estimate,
// RGBA only) (fcp_cutout_u8); the 32-bytes-per-pixel workspace lives for the call.
Tensor cutout(const Tensor& crops, const Tensor& alpha, int64_t mode, int64_t bg_r, int64_t bg_g, int64_t bg_b, at::IntArrayRef taps) {
  dev(crops, "crops", at::kByte);
  dev(alpha, "alpha", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, alpha, "alpha", f, h, w);
  for (int64_t v : {mode, bg_r, bg_g, bg_b}) TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, "mode / fill past int");
  uint16_t t16[49] = {};
  const int radius = taps16("cutout", taps, true, t16);
  Tensor out = at::empty({f, h, w, mode == FCP_CUTOUT_RGBA ? 4 : 3}, crops.options());
  Tensor work = workspace(taps.empty() ? 0 : fcp_cutout_workspace_bytes((int)f, (int)h, (int)w), crops);
  ok(fcp_cutout_u8(crops.data_ptr<uint8_t>(), alpha.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (int)mode, (int)bg_r, (int)bg_g,
                   (int)bg_b, t16, radius, out.data_ptr<uint8_t>(), work.data_ptr(), work.numel(), cur_stream()),
     "fcp::cutout");
  return out;
}

// The bank of the picture ops: pictures (k,h,w,3) uint8 with the crops' h and w, and picks (f,) int32, one picture per
// crop, both on the device of the crops.  Returns k.
static int bank_and_picks(const Tensor& crops, const Tensor& pictures, const Tensor& picks) {
  dev(pictures, "pictures", at::kByte);
  dev(picks, "picks", at::kInt);
  TORCH_CHECK(pictures.get_device() == crops.get_device() && pictures.dim() == 4 && pictures.size(1) == crops.size(1) &&
                  pictures.size(2) == crops.size(2) && pictures.size(3) == 3,
              "pictures must be (k,", crops.size(1), ",", crops.size(2), ",3) uint8 on the device of the crops");
  TORCH_CHECK(pictures.size(0) <= INT_MAX, "pictures (k,h,w,3): k past int");
  TORCH_CHECK(picks.get_device() == crops.get_device() && picks.dim() == 1 && picks.size(0) == crops.size(0), "picks must be (",
              crops.size(0), ",) int32 on the device of the crops");
  return (int)pictures.size(0);
}

// matte over pictures: the fill of crop i is pictures[picks[i]] (fcp_matte_image_u8).
std::tuple<Tensor, Tensor> matte_image(const Tensor& crops, const Tensor& labels, int64_t class_bits, int64_t feather,
                                       const Tensor& pictures, const Tensor& picks, bool with_alpha) {
  dev(crops, "crops", at::kByte);
  dev(labels, "labels", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, labels, "labels", f, h, w);
  const int k = bank_and_picks(crops, pictures, picks);
  TORCH_CHECK(class_bits >= 0 && class_bits <= (int64_t)UINT_MAX, "class_bits past 32 bits");
  TORCH_CHECK(feather >= INT_MIN && feather <= INT_MAX, "feather past int");
  Tensor out = at::empty_like(crops);
  Tensor alpha = with_alpha ? at::empty({f, h, w}, crops.options()) : at::empty({0}, crops.options());
  ok(fcp_matte_image_u8(crops.data_ptr<uint8_t>(), labels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (uint32_t)class_bits,
                        (int)feather, pictures.data_ptr<uint8_t>(), k, picks.data_ptr<int32_t>(), out.data_ptr<uint8_t>(),
                        with_alpha ? alpha.data_ptr<uint8_t>() : nullptr, cur_stream()),
     "fcp::matte_image");
  return {out, alpha};
}

// matte_alpha over pictures (fcp_matte_image_alpha_u8).
Tensor matte_image_alpha(const Tensor& crops, const Tensor& alpha, const Tensor& pictures, const Tensor& picks) {
  dev(crops, "crops", at::kByte);
  dev(alpha, "alpha", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, alpha, "alpha", f, h, w);
  const int k = bank_and_picks(crops, pictures, picks);
  Tensor out = at::empty_like(crops);
  ok(fcp_matte_image_alpha_u8(crops.data_ptr<uint8_t>(), alpha.data_ptr<uint8_t>(), (int)f, (int)h, (int)w,
                              pictures.data_ptr<uint8_t>(), k, picks.data_ptr<int32_t>(), out.data_ptr<uint8_t>(), cur_stream()),
     "fcp::matte_image_alpha");
  return out;
}

// The fill mode of cutout over pictures, taps = t[0..radius] (fcp_cutout_image_u8); the 32-bytes-per-pixel workspace
// lives for the call.
Tensor cutout_image(const Tensor& crops, const Tensor& alpha, const Tensor& pictures, const Tensor& picks, at::IntArrayRef taps) {
  dev(crops, "crops", at::kByte);
  dev(alpha, "alpha", at::kByte);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, alpha, "alpha", f, h, w);
  const int k = bank_and_picks(crops, pictures, picks);
  uint16_t t16[49] = {};
  const int radius = taps16("cutout_image", taps, false, t16);
  Tensor out = at::empty_like(crops);
  Tensor work = workspace(fcp_cutout_workspace_bytes((int)f, (int)h, (int)w), crops);
  ok(fcp_cutout_image_u8(crops.data_ptr<uint8_t>(), alpha.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, pictures.data_ptr<uint8_t>(),
                         k, picks.data_ptr<int32_t>(), t16, radius, out.data_ptr<uint8_t>(), work.data_ptr(), work.numel(),
                         cur_stream()),
     "fcp::cutout_image");
  return out;
}

// The cleaned binary label map (f,h,w) uint8, 0 / 1, of label maps (f,h,w) uint8: the largest 8-connected component of
// the hard mask and / or its holes of at most max_hole pixels filled (fcp_subject_mask_u8); the 12-bytes-per-pixel
// workspace lives for the call.
Tensor subject_mask(const Tensor& labels, int64_t class_bits, bool keep_largest, int64_t max_hole) {
  dev(labels, "labels", at::kByte);
  FCP_DEVICE_GUARD(labels);
  int64_t f, h, w;
  labels_plane(labels, class_bits, f, h, w);
  TORCH_CHECK(max_hole >= INT_MIN && max_hole <= INT_MAX, "max_hole past int");
  Tensor out = at::empty_like(labels);
  Tensor work = workspace(fcp_subject_mask_workspace_bytes((int)f, (int)h, (int)w), labels);
  ok(fcp_subject_mask_u8(labels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (uint32_t)class_bits, keep_largest ? 1 : 0,
                         (int)max_hole, out.data_ptr<uint8_t>(), work.data_ptr(), work.numel(), cur_stream()),
     "fcp::subject_mask");
  return out;
}

// The hard mask (f,h,w) uint8, 0 / 1, of label maps (f,h,w) uint8, grown (shift > 0) or shrunk (shift < 0) by a Euclidean
// disc of radius |shift| inside the crop (fcp_mask_shift_u8).
Tensor mask_shift(const Tensor& labels, int64_t class_bits, int64_t shift) {
  dev(labels, "labels", at::kByte);
  FCP_DEVICE_GUARD(labels);
  int64_t f, h, w;
  labels_plane(labels, class_bits, f, h, w);
  TORCH_CHECK(shift >= INT_MIN && shift <= INT_MAX, "shift past int");
  Tensor out = at::empty_like(labels);
  ok(fcp_mask_shift_u8(labels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (uint32_t)class_bits, (int)shift, out.data_ptr<uint8_t>(),
                       cur_stream()),
     "fcp::mask_shift");
  return out;
}

// Crops (f,h,w,3) uint8 with the luma equalised by CLAHE on a grid x grid tiling (fcp_clahe_u8); the LUT workspace
// lives for the call.
Tensor clahe(const Tensor& crops, int64_t grid, double clip_limit) {
  dev(crops, "crops", at::kByte);
  FCP_DEVICE_GUARD(crops);
  TORCH_CHECK(crops.dim() == 4 && crops.size(3) == 3, "crops (f,h,w,3) uint8");
  const int64_t f = crops.size(0), h = crops.size(1), w = crops.size(2);
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX, "crops (f,h,w,3): sizes past int");
  TORCH_CHECK(grid >= 1 && grid <= 16, "clahe: grid must be 1..16 (got ", grid, ")");
  Tensor out = at::empty_like(crops);
  Tensor luts = at::empty({f, grid, grid, 256}, crops.options());
  ok(fcp_clahe_u8(crops.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (int)grid, clip_limit, luts.data_ptr<uint8_t>(),
                  out.data_ptr<uint8_t>(), cur_stream()),
     "fcp::clahe");
  return out;
}

// Crops (f,h,w,3) uint8 with the noise removed by non-local means under the weight table lut (n,) uint16 and its shift
// (fcp_nlm_denoise_u8).
Tensor nlm_denoise(const Tensor& crops, const Tensor& lut, int64_t shift) {
  dev(crops, "crops", at::kByte);
  dev(lut, "lut", at::kUInt16);
  FCP_DEVICE_GUARD(crops);
  TORCH_CHECK(crops.dim() == 4 && crops.size(3) == 3, "crops (f,h,w,3) uint8");
  TORCH_CHECK(lut.dim() == 1 && lut.device() == crops.device(), "lut (n,) uint16 on the device of crops");
  const int64_t f = crops.size(0), h = crops.size(1), w = crops.size(2);
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX && lut.numel() <= INT_MAX, "crops (f,h,w,3), lut (n,): sizes past int");
  TORCH_CHECK(shift >= INT_MIN && shift <= INT_MAX, "shift past int");
  Tensor out = at::empty_like(crops);
  ok(fcp_nlm_denoise_u8(crops.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, static_cast<const uint16_t*>(lut.const_data_ptr()),
                        (int)lut.numel(), (int)shift, out.data_ptr<uint8_t>(), cur_stream()),
     "fcp::nlm_denoise");
  return out;
}

// Crops (f,h,w,3) uint8 sharpened by an unsharp mask of their gray with the taps t[0..radius] as integers, radius 1..48
// (fcp_unsharp_u8).
Tensor unsharp(const Tensor& crops, at::IntArrayRef taps, int64_t amount_q8, int64_t threshold) {
  dev(crops, "crops", at::kByte);
  FCP_DEVICE_GUARD(crops);
  TORCH_CHECK(crops.dim() == 4 && crops.size(3) == 3, "crops (f,h,w,3) uint8");
  const int64_t f = crops.size(0), h = crops.size(1), w = crops.size(2), radius = (int64_t)taps.size() - 1;
  TORCH_CHECK(f <= INT_MAX && h <= INT_MAX && w <= INT_MAX, "crops (f,h,w,3): sizes past int");
  TORCH_CHECK(radius >= 1 && radius <= 48, "unsharp: taps must be t[0..radius] with radius 1..48 (got ", taps.size(), " taps)");
  TORCH_CHECK(amount_q8 >= INT_MIN && amount_q8 <= INT_MAX && threshold >= INT_MIN && threshold <= INT_MAX, "amount_q8, threshold past int");
  uint16_t t16[49] = {};
  for (int64_t k = 0; k <= radius; ++k) {
    TORCH_CHECK(taps[k] >= 0 && taps[k] <= 65535, "unsharp: tap ", k, " past 16 bits");
    t16[k] = (uint16_t)taps[k];
  }
  Tensor out = at::empty_like(crops);
  ok(fcp_unsharp_u8(crops.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, t16, (int)radius, (int)amount_q8, (int)threshold,
                    out.data_ptr<uint8_t>(), cur_stream()),
     "fcp::unsharp");
  return out;
}

// Crops (f,h,w,3) uint8 with the pixels their label maps (f,h,w) uint8 call skin smoothed by a bilateral filter over the
// skin alone: taps t[0..radius] as integers, radius 3..24, the range table (256,) uint16 and the amount 1..256
// (fcp_skin_smooth_u8).
Tensor skin_smooth(const Tensor& crops, const Tensor& labels, int64_t class_bits, at::IntArrayRef taps, const Tensor& range_lut,
                   int64_t amount_q8) {
  dev(crops, "crops", at::kByte);
  dev(labels, "labels", at::kByte);
  dev(range_lut, "range_lut", at::kUInt16);
  FCP_DEVICE_GUARD(crops);
  int64_t f, h, w;
  crops_and_plane(crops, labels, "labels", f, h, w);
  TORCH_CHECK(range_lut.dim() == 1 && range_lut.numel() == 256 && range_lut.device() == crops.device(),
              "range_lut (256,) uint16 on the device of crops");
  TORCH_CHECK(class_bits >= 0 && class_bits <= (int64_t)UINT_MAX, "class_bits past 32 bits");
  TORCH_CHECK(amount_q8 >= INT_MIN && amount_q8 <= INT_MAX, "amount_q8 past int");
  const int64_t radius = (int64_t)taps.size() - 1;
  TORCH_CHECK(radius >= 3 && radius <= 24, "skin_smooth: taps must be t[0..radius] with radius 3..24 (got ", taps.size(), " taps)");
  uint16_t t16[25] = {};
  for (int64_t k = 0; k <= radius; ++k) {
    TORCH_CHECK(taps[k] >= 0 && taps[k] <= 65535, "skin_smooth: tap ", k, " past 16 bits");
    t16[k] = (uint16_t)taps[k];
  }
  Tensor out = at::empty_like(crops);
  ok(fcp_skin_smooth_u8(crops.data_ptr<uint8_t>(), labels.data_ptr<uint8_t>(), (int)f, (int)h, (int)w, (uint32_t)class_bits, t16,
                        (int)radius, static_cast<const uint16_t*>(range_lut.const_data_ptr()), (int)amount_q8,
                        out.data_ptr<uint8_t>(), cur_stream()),
     "fcp::skin_smooth");
  return out;
}

Tensor bicubic_down4_round(const Tensor& x4) {
  dev(x4, "x4", at::kFloat);
  FCP_DEVICE_GUARD(x4);
  TORCH_CHECK(x4.dim() == 3 && x4.size(0) % 4 == 0 && x4.size(1) % 4 == 0 && x4.size(2) >= 3, "x4 (4h,4w,ld>=3) fp32");
  const int64_t h = x4.size(0) / 4, w = x4.size(1) / 4;
  Tensor out = at::empty({h, w, 3}, x4.options().dtype(at::kByte));
  ok(fcp_bicubic_down4_u8(x4.data_ptr<float>(), (int)h, (int)w, (int)x4.size(2), out.data_ptr<uint8_t>(), cur_stream()),
     "fcp::bicubic_down4_round");
  return out;
}

std::tuple<Tensor, Tensor> parse_argmax_hist(const Tensor& logits, int64_t ncls, int64_t mid_h, int64_t mid_w, int64_t out_h,
                                             int64_t out_w) {
  dev(logits, "logits", at::kFloat);
  FCP_DEVICE_GUARD(logits);
  TORCH_CHECK(logits.dim() == 4 && logits.size(3) >= ncls, "logits (f,lh,lw,ld>=ncls)");
  const int64_t f = logits.size(0);
  Tensor labels = at::empty({f, out_h, out_w}, logits.options().dtype(at::kByte));
  Tensor counts = at::empty({f, ncls}, logits.options().dtype(at::kInt));
  ok(fcp_parse_tail(logits.data_ptr<float>(), (int)f, (int)logits.size(1), (int)logits.size(2), (int)logits.size(3), (int)ncls,
                    (int)mid_h, (int)mid_w, (int)out_h, (int)out_w, labels.data_ptr<uint8_t>(), counts.data_ptr<int>(), cur_stream()),
     "fcp::parse_argmax_hist");
  return {labels, counts};
}

}  // namespace

TORCH_LIBRARY(fcp, m) {
  m.def("conv2d(Tensor x, int x_c0, int cin, Tensor w, Tensor? bias, Tensor? wscale, Tensor? res1, int res1_c0, Tensor? res2, "
        "int res2_c0, int cout, int kh, int kw, int stride, int pad, float act_slope, float alpha, "
        "float alpha2, bool res1_pre, int precision, int in_fmt, int out_fmt, int res1_fmt, int res2_fmt, bool in_up2, "
        "bool cin4, int tile_m, int tile_n, Tensor? x2, int x2_c0, int cin2, int x2_stride, int flags, int cu_budget=0, int band_top=0, "
        "int band_bottom=0) -> Tensor");
  m.def("conv2d_out(Tensor x, int x_c0, int cin, Tensor w, Tensor? bias, Tensor? wscale, Tensor? res1, int res1_c0, Tensor? res2, "
        "int res2_c0, Tensor(a!) out, int out_c0, int cout, int kh, int kw, int stride, int pad, float act_slope, float alpha, "
        "float alpha2, bool res1_pre, int precision, int in_fmt, int out_fmt, int res1_fmt, int res2_fmt, bool in_up2, "
        "bool cin4, int tile_m, int tile_n, Tensor? x2, int x2_c0, int cin2, int x2_stride, int flags, int cu_budget=0, int band_top=0, "
        "int band_bottom=0) -> ()");
  m.def("bottleneck_chain(Tensor t1, int t1_c0, Tensor? res, int res_c0, Tensor? w2, Tensor? ws2, Tensor? b2, Tensor w3, Tensor ws3, "
        "Tensor b3, Tensor? w1n, Tensor? ws1n, Tensor? b1n, int c, int nout, int cn, int tile_m=0, int flags=0, Tensor? t1b=None, "
        "int t1b_c0=0, int cb=0, int t1b_stride=1) -> (Tensor, Tensor)");
  m.def("retina_decode(Tensor head0, Tensor head1, Tensor head2, int img_h, int img_w, float vis, float var0, float var1) "
        "-> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("nms_select(Tensor cand_score, Tensor cand_box, Tensor cand_count, float nms_threshold, int strategy) "
        "-> (Tensor, Tensor, Tensor, Tensor)");
  m.def("gather_faces(Tensor cand_ldm, Tensor sel_pos, Tensor sel_count, Tensor? paddings, int max_faces) -> (Tensor, Tensor, Tensor)");
  m.def("similarity_from_5pt(Tensor src, Tensor dst, bool allow_skew, Tensor? face_count=None, Tensor(a!)? valid_total=None) "
        "-> (Tensor, Tensor)");
  m.def("warp_affine_u8(Tensor images, Tensor img_idx, Tensor mat, Tensor? ok, Tensor? paddings, int out_w, int out_h, int border) -> Tensor");
  m.def("warp_affine_u8_float(Tensor images, Tensor img_idx, Tensor mat, Tensor? ok, Tensor? paddings, int out_w, int out_h, "
        "int border) -> Tensor");
  m.def("warp_affine_u8_ragged(Tensor blob, Tensor srcs, Tensor mat, Tensor? ok, int out_w, int out_h, int border, int family) "
        "-> Tensor");
  m.def("warp_affine_u8_interp(Tensor images, Tensor img_idx, Tensor mat, Tensor? ok, Tensor? paddings, int out_w, int out_h, "
        "int border, int interp) -> Tensor");
  m.def("warp_affine_u8_interp_ragged(Tensor blob, Tensor srcs, Tensor mat, Tensor? ok, int out_w, int out_h, int border, "
        "int interp) -> Tensor");
  m.def("resize_area_u8_ragged(Tensor src, Tensor levels, Tensor(a!) dst) -> ()");
  m.def("crop_sharpness(Tensor crops, Tensor? ok) -> Tensor");
  m.def("jpeg_encode(Tensor crops, int quality, int subsampling, Tensor(a!) out) -> Tensor");
  m.def("jpeg_encode_ex(Tensor crops, int quality, int subsampling, Tensor(a!) out, Tensor(b!)? tables) -> Tensor");
  m.def("jpeg_huffman_tables(Tensor freq, bool with_codes) -> (Tensor, Tensor)");
  m.def("png_encode(Tensor pixels, Tensor(a!) out) -> Tensor");
  m.def("png_huffman_lengths(Tensor freq, bool with_codes) -> (Tensor, Tensor)");
  m.def("matte(Tensor crops, Tensor labels, int class_bits, int feather, int bg_r, int bg_g, int bg_b, bool with_alpha) "
        "-> (Tensor, Tensor)");
  m.def("clahe(Tensor crops, int grid, float clip_limit) -> Tensor");
  m.def("matte_blur(Tensor crops, Tensor labels, int class_bits, int feather, int[] taps, bool with_alpha) -> (Tensor, Tensor)");
  m.def("matte_refine(Tensor crops, Tensor labels, int class_bits, int radius, int eps) -> Tensor");
  m.def("matte_alpha(Tensor crops, Tensor alpha, int bg_r, int bg_g, int bg_b) -> Tensor");
  m.def("matte_blur_alpha(Tensor crops, Tensor labels, Tensor alpha, int class_bits, int[] taps) -> Tensor");
  m.def("subject_mask(Tensor labels, int class_bits, bool keep_largest, int max_hole) -> Tensor");
  m.def("feather_alpha(Tensor labels, int class_bits, int feather) -> Tensor");
  m.def("cutout(Tensor crops, Tensor alpha, int mode, int bg_r, int bg_g, int bg_b, int[] taps) -> Tensor");
  m.def("mask_shift(Tensor labels, int class_bits, int shift) -> Tensor");
  m.def("nlm_denoise(Tensor crops, Tensor lut, int shift) -> Tensor");
  m.def("unsharp(Tensor crops, int[] taps, int amount_q8, int threshold) -> Tensor");
  m.def("matte_image(Tensor crops, Tensor labels, int class_bits, int feather, Tensor pictures, Tensor picks, bool with_alpha) "
        "-> (Tensor, Tensor)");
  m.def("matte_image_alpha(Tensor crops, Tensor alpha, Tensor pictures, Tensor picks) -> Tensor");
  m.def("cutout_image(Tensor crops, Tensor alpha, Tensor pictures, Tensor picks, int[] taps) -> Tensor");
  m.def("skin_smooth(Tensor crops, Tensor labels, int class_bits, int[] taps, Tensor range_lut, int amount_q8) -> Tensor");
  m.def("bicubic_down4_round(Tensor x4) -> Tensor");
  m.def("parse_argmax_hist(Tensor logits, int ncls, int mid_h, int mid_w, int out_h, int out_w) -> (Tensor, Tensor)");
  // ABI the veneer was COMPILED against (struct layouts of include/fcp_hip.h) and the ABI of the libfcp_hip.so it is
  // running on: torch_ops.load() refuses a stale veneer (its shorter structs would be read past their end)
  m.def("abi_version() -> (int, int)", []() -> std::tuple<int64_t, int64_t> {
    return {(int64_t)FCP_ABI_VERSION, (int64_t)fcp_abi_version()};
  });
}

TORCH_LIBRARY_IMPL(fcp, CUDA, m) {
  m.impl("conv2d", &conv2d);
  m.impl("conv2d_out", &conv2d_out);
  m.impl("bottleneck_chain", &bottleneck_chain);
  m.impl("retina_decode", &retina_decode);
  m.impl("nms_select", &nms_select);
  m.impl("gather_faces", &gather_faces);
  m.impl("similarity_from_5pt", &similarity_from_5pt);
  m.impl("warp_affine_u8", &warp_affine_u8);
  m.impl("warp_affine_u8_float", &warp_affine_u8_float);
  m.impl("warp_affine_u8_ragged", &warp_affine_u8_ragged);
  m.impl("warp_affine_u8_interp", &warp_affine_u8_interp);
  m.impl("warp_affine_u8_interp_ragged", &warp_affine_u8_interp_ragged);
  m.impl("resize_area_u8_ragged", &resize_area_u8_ragged);
  m.impl("crop_sharpness", &crop_sharpness);
  m.impl("jpeg_encode", &jpeg_encode);
  m.impl("jpeg_encode_ex", &jpeg_encode_ex);
  m.impl("jpeg_huffman_tables", &jpeg_huffman_tables);
  m.impl("png_encode", &png_encode);
  m.impl("png_huffman_lengths", &png_huffman_lengths);
  m.impl("matte", &matte);
  m.impl("clahe", &clahe);
  m.impl("matte_blur", &matte_blur);
  m.impl("matte_refine", &matte_refine);
  m.impl("matte_alpha", &matte_alpha);
  m.impl("matte_blur_alpha", &matte_blur_alpha);
  m.impl("subject_mask", &subject_mask);
  m.impl("feather_alpha", &feather_alpha);
  m.impl("cutout", &cutout);
  m.impl("mask_shift", &mask_shift);
  m.impl("nlm_denoise", &nlm_denoise);
  m.impl("unsharp", &unsharp);
  m.impl("matte_image", &matte_image);
  m.impl("matte_image_alpha", &matte_image_alpha);
  m.impl("cutout_image", &cutout_image);
  m.impl("skin_smooth", &skin_smooth);
  m.impl("bicubic_down4_round", &bicubic_down4_round);
  m.impl("parse_argmax_hist", &parse_argmax_hist);
}
