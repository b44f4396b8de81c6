// torch.ops.pfk.* — the thin PyTorch-ROCm face of libpfk.so.
//
// The only translation unit that sees torch headers.  Each op checks device/dtype/layout,
// unwraps tensors to raw pointers + strides, picks up torch's *current* HIP stream and forwards
// to the C ABI of include/pfk.h; a non-zero status becomes a RuntimeError (the convention of
// the reference's own extension, ptlflow/utils/external/alt_cuda_corr/correlation.cpp:19-21).
// No kernel code, no allocation on the hot path (callers pass output/workspace tensors).
//
// Pixel-major activations are passed as 2-D tensors [M, C] whose row stride is the buffer's
// `ld` — a channel slice of a wider buffer (buf[:, 128:384]) is just a view.
//
// Tensors become pointers in pfk_torch_views.h only: rows() for pixel-major views, dense() for contiguous tensors,
// up8() for the upsampled outputs, fill_sources() for a convolution's inputs.
#include <torch/library.h>

#include <type_traits>
#include <vector>

#include "pfk_torch_views.h"

namespace {

// out[b,i,j] = scale * <f1[b,i,:], f2[b,j,:]>: fp32 [B,N,D] inputs -> fp32 [B,N1,N2] out (corr_volume), or all three bf16 (corr_volume_bf16)
void corr_volume_impl(const char* op, Elem e, const Tensor& f1, const Tensor& f2, double scale, const Tensor& out) {
  OpScope scope(f1);
  const Ptr a = dense(op, f1, "f1", e), b = dense(op, f2, "f2", e), o = dense(op, out, "out", e);
  TORCH_CHECK(f1.dim() == 3 && f2.dim() == 3 && out.dim() == 3, op, ": [B,N,D] inputs, [B,N1,N2] out");
  const int B = f1.size(0), N1 = f1.size(1), D = f1.size(2), N2 = f2.size(1);
  TORCH_CHECK(f2.size(0) == B && f2.size(2) == D && out.size(0) == B && out.size(1) == N1 && out.size(2) == N2, op, ": shape mismatch");
  if (e == B16) check_ok(pfk_corr_volume_bf16(a.raw(), D, b.raw(), D, o.raw(), B, N1, N2, D, (float)scale, cur_stream()), op);
  else check_ok(pfk_corr_volume_f32(a.f32(), D, b.f32(), D, o.f32(), B, N1, N2, D, (float)scale, cur_stream()), op);
}
void corr_volume(const Tensor& f1, const Tensor& f2, double scale, Tensor out) { corr_volume_impl("corr_volume", F32, f1, f2, scale, out); }
void corr_volume_bf16(const Tensor& f1, const Tensor& f2, double scale, Tensor out) { corr_volume_impl("corr_volume_bf16", B16, f1, f2, scale, out); }

void corr_pool2x2(const Tensor& in, Tensor out) {
  OpScope scope(in);
  const Ptr i = dense("corr_pool2x2", in, "inp", Any);
  TORCH_CHECK(in.dim() == 3, "corr_pool2x2: inp must be [M,H,W] contiguous");
  const int64_t M = in.size(0); const int H = in.size(1), W = in.size(2);
  const Ptr o = dense("corr_pool2x2", out, "out", i.b16 ? B16 : F32, M * (H / 2) * (W / 2));
  if (out.numel() == 0) return;
  if (i.b16) check_ok(pfk_corr_pool2x2_bf16(i.raw(), o.raw(), M, H, W, cur_stream()), "corr_pool2x2 (bf16)");
  else check_ok(pfk_corr_pool2x2_f32(i.f32(), o.f32(), M, H, W, cur_stream()), "corr_pool2x2");
}

// pixel-major feature map [B*H*W, C] -> [B*(H/2)*(W/2), C]: 2x2 average == bilinear x0.5 (align_corners=False)
void fmap_pool2x2(const Tensor& in, Tensor out, int64_t B, int64_t H, int64_t W) {
  OpScope scope(in);
  const Rows i = rows("fmap_pool2x2", in, "inp", F32).expect(B * H * W, AtLeast{0});
  const Rows o = rows("fmap_pool2x2", out, "out", F32).expect(B * (H / 2) * (W / 2), i.cols);
  if (out.numel() == 0) return;
  check_ok(pfk_fmap_pool2x2_f32(i.f32(), i.ld, o.f32(), o.ld, (int)B, (int)H, (int)W, (int)i.cols, cur_stream()), "fmap_pool2x2");
}

// corr_lookup: levels are [B*N, h_l, w_l] maps, which carry their sizes.  corr_lookup_blocked (include/pfk.h "K1-K3 on the BLOCKED
// volume layout"): levels are [B*N, pfk_blocked_map_elems(h_l, w_l)] and the map sizes come in lvl_h / lvl_w
void corr_lookup_impl(const char* op, bool blocked, at::TensorList levels, at::IntArrayRef lvl_h, at::IntArrayRef lvl_w, const Tensor& coords,
                      int64_t radius, const Tensor& out) {
  OpScope scope(coords);
  const Ptr c = dense(op, coords, "coords", F32);
  TORCH_CHECK(coords.dim() == 4 && coords.size(1) == 2, op, ": coords [B,2,h,w] contiguous");
  TORCH_CHECK(levels.size() >= 1 && levels.size() <= PFK_MAX_LEVELS, op, ": 1..8 levels");
  TORCH_CHECK(!blocked || (lvl_h.size() == levels.size() && lvl_w.size() == levels.size()), op, ": one map size per level");
  pfk_lookup_desc d{};
  d.B = coords.size(0); d.h = coords.size(2); d.w = coords.size(3);
  const int64_t M = (int64_t)d.B * d.h * d.w;
  const bool bf = levels[0].scalar_type() == at::kBFloat16;      // levels must all be float32 or all bfloat16
  for (size_t l = 0; l < levels.size(); ++l) {
    const Tensor& v = levels[l];
    d.levels[l] = dense(op, v, "level", bf ? B16 : F32).raw();
    if (blocked) {
      TORCH_CHECK(lvl_h[l] > 0 && lvl_w[l] > 0 && v.dim() == 2 && v.size(0) == M && v.size(1) == pfk_blocked_map_elems((int)lvl_h[l], (int)lvl_w[l]),
                  op, ": level must be [B*N, blocked_map_elems(h_l, w_l)] contiguous");
      d.lvl_h[l] = (int)lvl_h[l]; d.lvl_w[l] = (int)lvl_w[l];
    } else {
      TORCH_CHECK(v.dim() == 3 && v.size(0) == M, op, ": level must be [B*N,h_l,w_l] contiguous");
      d.lvl_h[l] = v.size(1); d.lvl_w[l] = v.size(2);
    }
  }
  d.num_levels = levels.size(); d.radius = radius;
  const int n = 2 * radius + 1;
  const Rows o = rows(op, out, "out", Any).expect(M, AtLeast{(int64_t)d.num_levels * n * n});
  d.coords = c.f32(); d.out = o.raw(); d.out_ld = o.ld; d.out_bf16 = o.b16;
  if (blocked) check_ok(bf ? pfk_corr_lookup_blocked_bf16(&d, cur_stream()) : pfk_corr_lookup_blocked_f32(&d, cur_stream()), op);
  else check_ok(bf ? pfk_corr_lookup_bf16(&d, cur_stream()) : pfk_corr_lookup_f32(&d, cur_stream()), op);
}
void corr_lookup(at::TensorList levels, const Tensor& coords, int64_t radius, Tensor out) {
  corr_lookup_impl("corr_lookup", false, levels, {}, {}, coords, radius, out);
}
void corr_lookup_blocked(at::TensorList levels, at::IntArrayRef lvl_h, at::IntArrayRef lvl_w, const Tensor& coords, int64_t radius, Tensor out) {
  corr_lookup_impl("corr_lookup_blocked", true, levels, lvl_h, lvl_w, coords, radius, out);
}

// hidden width of the GRU epilogues (include/pfk.h): cout = 2*Ch for PFK_EPI_GRU_ZR, Ch for PFK_EPI_GRU_Q; h / aux_z / aux_rh are [M][Ch]
int64_t gru_hidden(int64_t epilogue, int64_t cout) {
  return epilogue == PFK_EPI_GRU_ZR ? cout / 2 : epilogue == PFK_EPI_GRU_Q ? cout : 0;
}

void conv2d(at::TensorList srcs, int64_t B, int64_t H, int64_t W, int64_t kh, int64_t kw,
            const Tensor& weight, const c10::optional<Tensor>& bias, int64_t cout, int64_t epilogue,
            bool relu, double scale, const c10::optional<Tensor>& out, const c10::optional<Tensor>& h,
            const c10::optional<Tensor>& aux_z, const c10::optional<Tensor>& aux_rh,
            const c10::optional<Tensor>& workspace, const c10::optional<Tensor>& residual, int64_t stride,
            bool relu_after_residual, int64_t cout_active, int64_t cout_split) {
  OpScope scope(weight);
  TORCH_CHECK(stride >= 1, "conv2d: stride");
  pfk_conv_desc d{};
  d.stride = (int)stride;
  d.cout_active = (int)cout_active;
  d.cout_split = (int)cout_split;
  d.relu_after_residual = relu_after_residual;
  const int64_t M = out_rows(B, H, W, stride), Ch = gru_hidden(epilogue, cout);
  fill_sources(d, srcs, B * H * W, F32, "conv2d");
  d.B = B; d.H = H; d.W = W; d.kh = kh; d.kw = kw; d.cout = cout;
  d.epilogue = epilogue; d.relu = relu; d.scale = (float)scale;
  // fp32 packed weight [cout, ktot] -> fp32 MFMA path; bf16 planes [nsplit, cout, ktot64] -> split-bf16 path
  const bool split = weight.scalar_type() == at::kBFloat16;
  const Ptr wp = dense("conv2d", weight, "weight", split ? B16 : F32);
  if (split) {
    TORCH_CHECK(weight.dim() == 3 && weight.size(1) == cout && weight.size(0) >= 1 && weight.size(0) <= 3,
                "conv2d: bf16 weight planes [nsplit, cout, ktot]");
    TORCH_CHECK(weight.size(2) == pfk_conv_ktot_bf16(&d), "conv2d: bf16 weight planes have ktot ", weight.size(2),
                ", expected ", pfk_conv_ktot_bf16(&d));
  } else {
    TORCH_CHECK(weight.dim() == 2 && weight.size(0) == cout, "conv2d: packed weight [cout, ktot]");
    TORCH_CHECK(weight.size(1) == pfk_conv_ktot(&d), "conv2d: packed weight has ktot ", weight.size(1), ", expected ", pfk_conv_ktot(&d));
    d.weight = wp.f32();
  }
  d.bias = dense("conv2d", bias, "bias", F32, cout).f32();
  if (out.has_value()) {
    const Rows o = rows("conv2d", *out, "out", F32).expect(M, cout);
    d.out = o.f32(); d.out_ld = o.ld; d.out_coff = 0;
  }
  if (h.has_value()) { const Rows v = rows("conv2d", *h, "h", F32).expect(M, AtLeast{Ch}); d.h = v.f32(); d.h_ld = v.ld; }
  d.aux_z = dense("conv2d", aux_z, "aux_z", F32, AtLeast{M * Ch}).f32();
  d.aux_rh = dense("conv2d", aux_rh, "aux_rh", F32, AtLeast{M * Ch}).f32();
  if (residual.has_value()) {
    const Rows r = rows("conv2d", *residual, "residual", F32).expect(M, cout);
    d.residual = r.f32(); d.residual_ld = r.ld;
  }
  if (workspace.has_value()) { d.workspace = dense("conv2d", *workspace, "workspace", Raw).raw(); d.workspace_bytes = (long long)workspace->nbytes(); }
  if (split) check_ok(pfk_conv2d_bf16s(&d, wp.raw(), (int)weight.size(0), cur_stream()), "conv2d (split bf16)");
  else check_ok(pfk_conv2d_f32(&d, cur_stream()), "conv2d");
}

// Winograd F(2x2,3x3) 3x3 convolution (pfk_conv2d_wino_f32): one fp32 source [B*H*W, cin] view, the transformed weight of
// packing.pack_wino_weight (flat, pfk_conv_wino_weight_floats(cin, cout) floats), LINEAR epilogue into an [M, cout] view;
// with `residual` the residual-block epilogue (pfk_conv2d_wino_res_f32): out = relu2?(residual + relu?(conv + bias) * scale)
pfk_conv_desc wino_desc(const char* op, const Tensor& src, int64_t B, int64_t H, int64_t W, const Tensor& weight,
                        const c10::optional<Tensor>& bias, int64_t cout, bool relu, double scale, const Tensor& out, int64_t cout_active) {
  TORCH_CHECK(B >= 1 && H >= 1 && W >= 1 && cout >= 1, op, ": sizes");
  pfk_conv_desc d{};
  fill_sources(d, {src}, B * H * W, F32, op);
  const int cin = d.src[0].channels;
  TORCH_CHECK(cin % 32 == 0, op, ": input channels must be a multiple of 32, got ", cin);
  d.B = B; d.H = H; d.W = W; d.kh = 3; d.kw = 3; d.stride = 1; d.cout = cout;
  d.epilogue = PFK_EPI_LINEAR; d.relu = relu; d.scale = (float)scale;
  d.cout_active = (int)cout_active;
  d.weight = dense(op, weight, "weight (transformed)", F32, pfk_conv_wino_weight_floats(cin, (int)cout)).f32();
  d.bias = dense(op, bias, "bias", F32, cout).f32();
  const Rows o = rows(op, out, "out", F32).expect(B * H * W, cout);
  d.out = o.f32(); d.out_ld = o.ld; d.out_coff = 0;
  return d;
}
void conv2d_wino_impl(const Tensor& src, int64_t B, int64_t H, int64_t W, const Tensor& weight, const c10::optional<Tensor>& bias,
                      int64_t cout, bool relu, double scale, const Tensor& out, int64_t cout_active, const Tensor* residual,
                      bool relu_after_residual) {
  OpScope scope(weight);
  pfk_conv_desc d = wino_desc("conv2d_wino", src, B, H, W, weight, bias, cout, relu, scale, out, cout_active);
  if (residual) {
    const Rows r = rows("conv2d_wino_res", *residual, "residual", F32).expect(B * H * W, cout);
    d.residual = r.f32(); d.residual_ld = r.ld; d.relu_after_residual = relu_after_residual;
    check_ok(pfk_conv2d_wino_res_f32(&d, cur_stream()), "conv2d_wino_res");
    return;
  }
  check_ok(pfk_conv2d_wino_f32(&d, cur_stream()), "conv2d_wino");
}
void conv2d_wino(const Tensor& src, int64_t B, int64_t H, int64_t W, const Tensor& weight, const c10::optional<Tensor>& bias,
                 int64_t cout, bool relu, double scale, const Tensor& out, int64_t cout_active) {
  conv2d_wino_impl(src, B, H, W, weight, bias, cout, relu, scale, out, cout_active, nullptr, false);
}
void conv2d_wino_res(const Tensor& src, int64_t B, int64_t H, int64_t W, const Tensor& weight, const c10::optional<Tensor>& bias,
                     int64_t cout, bool relu, double scale, const Tensor& out, const Tensor& residual, bool relu_after_residual) {
  conv2d_wino_impl(src, B, H, W, weight, bias, cout, relu, scale, out, 0, &residual, relu_after_residual);
}

// The instance norm in front of the convolution applied on load (pfk_conv2d_wino_norm_f32): `src` is the raw output of the previous
// convolution, in_mean / in_rstd [B*cin] its statistics
void conv2d_wino_norm(const Tensor& src, int64_t B, int64_t H, int64_t W, const Tensor& weight, const c10::optional<Tensor>& bias,
                      int64_t cout, bool relu, double scale, const Tensor& out, const Tensor& in_mean, const Tensor& in_rstd, bool in_relu) {
  OpScope scope(weight);
  const pfk_conv_desc d = wino_desc("conv2d_wino_norm", src, B, H, W, weight, bias, cout, relu, scale, out, 0);
  const int64_t cin = d.src[0].channels;
  const float* mp = dense("conv2d_wino_norm", in_mean, "in_mean [B*cin]", F32, B * cin).f32();
  const float* rp = dense("conv2d_wino_norm", in_rstd, "in_rstd [B*cin]", F32, B * cin).f32();
  check_ok(pfk_conv2d_wino_norm_f32(&d, mp, rp, in_relu, cur_stream()), "conv2d_wino_norm");
}

// ... and / or the statistics of the instance norm behind it out of the epilogue (pfk_conv2d_wino_stats_f32; bias only: the
// convolution in front of a norm has no relu and no scale)
int64_t conv_wino_stats_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t cout) {
  return pfk_conv_wino_stats_workspace_bytes((int)B, (int)H, (int)W, (int)cout);
}
void conv2d_wino_stats(const Tensor& src, int64_t B, int64_t H, int64_t W, const Tensor& weight, const c10::optional<Tensor>& bias,
                       int64_t cout, const Tensor& out, const c10::optional<Tensor>& in_mean, const c10::optional<Tensor>& in_rstd,
                       bool in_relu, double eps, Tensor out_mean, Tensor out_rstd, Tensor workspace) {
  OpScope scope(weight);
  const pfk_conv_desc d = wino_desc("conv2d_wino_stats", src, B, H, W, weight, bias, cout, false, 1.0, out, 0);
  const int64_t cin = d.src[0].channels;
  TORCH_CHECK(in_mean.has_value() == in_rstd.has_value(), "conv2d_wino_stats: in_mean and in_rstd come together");
  const float* mp = dense("conv2d_wino_stats", in_mean, "in_mean [B*cin]", F32, B * cin).f32();
  const float* rp = dense("conv2d_wino_stats", in_rstd, "in_rstd [B*cin]", F32, B * cin).f32();
  float* om = dense("conv2d_wino_stats", out_mean, "out_mean [B*cout]", F32, B * cout).f32();
  float* orr = dense("conv2d_wino_stats", out_rstd, "out_rstd [B*cout]", F32, B * cout).f32();
  void* ws = dense("conv2d_wino_stats", workspace, "workspace", Raw).raw();
  check_ok(pfk_conv2d_wino_stats_f32(&d, mp, rp, in_relu, (float)eps, om, orr, ws, (long long)workspace.nbytes(), cur_stream()),
           "conv2d_wino_stats");
}

// 1-D Winograd F(4,5) form of a 1x5 / 5x1 convolution (pfk_conv1d_wino_f32): one or two fp32 sources ([B*H*W, channels_i] views,
// channels % 8 == 0), the transformed weight of packing.pack_wino1d_weight (flat), the LINEAR epilogue into `out` or the GRU gate
// epilogues with h / aux_z / aux_rh / residual as in conv2d
void conv2d_wino1d(at::TensorList srcs, int64_t B, int64_t H, int64_t W, int64_t kh, int64_t kw, const Tensor& weight,
                   const c10::optional<Tensor>& bias, int64_t cout, int64_t epilogue, bool relu, double scale,
                   const c10::optional<Tensor>& out, const c10::optional<Tensor>& h, const c10::optional<Tensor>& aux_z,
                   const c10::optional<Tensor>& aux_rh, const c10::optional<Tensor>& residual) {
  OpScope scope(weight);
  TORCH_CHECK(B >= 1 && H >= 1 && W >= 1 && cout >= 1, "conv2d_wino1d: sizes");
  TORCH_CHECK(srcs.size() <= 2, "conv2d_wino1d: one or two sources");
  pfk_conv_desc d{};
  const int64_t M = B * H * W, Ch = gru_hidden(epilogue, cout);
  fill_sources(d, srcs, M, F32, "conv2d_wino1d");
  int64_t ktot = 0;
  for (int i = 0; i < d.num_src; ++i) {
    TORCH_CHECK(d.src[i].channels % 8 == 0, "conv2d_wino1d: source channels must be a multiple of 8, got ", d.src[i].channels);
    ktot += d.src[i].channels;
  }
  d.B = B; d.H = H; d.W = W; d.kh = kh; d.kw = kw; d.stride = 1; d.cout = cout;
  d.epilogue = epilogue; d.relu = relu; d.scale = (float)scale;
  d.weight = dense("conv2d_wino1d", weight, "weight (transformed)", F32, pfk_conv_wino1d_weight_floats((int)ktot, (int)cout)).f32();
  d.bias = dense("conv2d_wino1d", bias, "bias", F32, cout).f32();
  if (out.has_value()) {
    const Rows o = rows("conv2d_wino1d", *out, "out", F32).expect(M, cout);
    d.out = o.f32(); d.out_ld = o.ld; d.out_coff = 0;
  }
  if (h.has_value()) { const Rows v = rows("conv2d_wino1d", *h, "h", F32).expect(M, AtLeast{Ch}); d.h = v.f32(); d.h_ld = v.ld; }
  d.aux_z = dense("conv2d_wino1d", aux_z, "aux_z", F32, AtLeast{M * Ch}).f32();
  d.aux_rh = dense("conv2d_wino1d", aux_rh, "aux_rh", F32, AtLeast{M * Ch}).f32();
  if (residual.has_value()) {
    const Rows r = rows("conv2d_wino1d", *residual, "residual", F32).expect(M, cout);
    d.residual = r.f32(); d.residual_ld = r.ld;
  }
  check_ok(pfk_conv1d_wino_f32(&d, cur_stream()), "conv2d_wino1d");
}

// Grouped launch (pfk_conv2d_group_f32): problem i = one fp32 source srcs[i] ([B*H*W, cin_i] view), k[i] x k[i] taps, stride 1, packed
// weight weights[i] [cout_i, ktot_i], bias biases[i] (an empty tensor = none), relu[i], scale[i], out = outs[i] ([B*H*W, cout_i] view),
// residuals[i] (optional; an empty tensor = none): added after relu / scale
void conv2d_group(at::TensorList srcs, int64_t B, int64_t H, int64_t W, at::IntArrayRef k, at::TensorList weights, at::TensorList biases,
                  at::IntArrayRef relu, at::ArrayRef<double> scale, at::TensorList outs, at::TensorList residuals) {
  const size_t n = srcs.size();
  TORCH_CHECK(n >= 1 && n <= PFK_CONV_GROUP_MAX, "conv2d_group: 1..", PFK_CONV_GROUP_MAX, " problems");
  TORCH_CHECK(k.size() == n && weights.size() == n && biases.size() == n && relu.size() == n && scale.size() == n && outs.size() == n &&
              (residuals.size() == n || residuals.size() == 0), "conv2d_group: one entry per problem in every list (residuals: n or none)");
  OpScope scope(srcs[0]);
  pfk_conv_desc d[PFK_CONV_GROUP_MAX] = {};
  for (size_t i = 0; i < n; ++i) {
    fill_sources(d[i], {srcs[i]}, B * H * W, F32, "conv2d_group");
    const Rows o = rows("conv2d_group", outs[i], "out", F32).expect(B * H * W, AtLeast{0});
    const int cout = o.cols;
    d[i].B = B; d[i].H = H; d[i].W = W; d[i].kh = k[i]; d[i].kw = k[i]; d[i].cout = cout; d[i].stride = 1;
    d[i].epilogue = PFK_EPI_LINEAR; d[i].relu = relu[i] != 0; d[i].scale = (float)scale[i];
    d[i].weight = dense("conv2d_group", weights[i], "weight", F32).f32();
    TORCH_CHECK(weights[i].dim() == 2 && weights[i].size(0) == cout && weights[i].size(1) == pfk_conv_ktot(&d[i]),
                "conv2d_group: packed weight [cout, ktot] of problem ", i);
    if (biases[i].numel() > 0) d[i].bias = dense("conv2d_group", biases[i], "bias", F32, cout).f32();
    d[i].out = o.f32(); d[i].out_ld = o.ld; d[i].out_coff = 0;
    if (residuals.size() == n && residuals[i].numel() > 0) {      // out = residual + scale * relu?(conv + bias)  (an empty tensor = none)
      const Rows r = rows("conv2d_group", residuals[i], "residual", F32).expect(B * H * W, cout);
      d[i].residual = r.f32(); d[i].residual_ld = r.ld;
    }
  }
  check_ok(pfk_conv2d_group_f32(d, (int)n, cur_stream()), "conv2d_group");
}

// K8b: bf16 sources / weight (pfk_conv2d_b16); `out` may be bf16 or fp32, h / aux_z / residual fp32, aux_rh / h_b16 bf16.
// `gelu_entry`: the descriptor goes to pfk_conv2d_gelu_b16 instead (torch.ops.pfk.conv2d_gelu_b16)
void conv2d_b16_run(at::TensorList srcs, int64_t B, int64_t H, int64_t W, int64_t kh, int64_t kw, const Tensor& weight,
                    const c10::optional<Tensor>& bias, int64_t cout, int64_t epilogue, bool relu, double scale,
                    const c10::optional<Tensor>& out, const c10::optional<Tensor>& h, const c10::optional<Tensor>& h_b16,
                    const c10::optional<Tensor>& aux_z, const c10::optional<Tensor>& aux_rh, const c10::optional<Tensor>& residual,
                    int64_t stride, bool relu_after_residual, bool gelu_entry) {
  OpScope scope(weight);
  const char* op = gelu_entry ? "conv2d_gelu_b16" : "conv2d_b16";
  const bool lin = epilogue == PFK_EPI_LINEAR || (gelu_entry && epilogue == PFK_EPI_LINEAR_GELU);
  pfk_conv_b16_desc d{};
  d.weight = dense(op, weight, "weight", B16).raw();
  d.bias = dense(op, bias, "bias", F32, cout).f32();
  if (weight.dim() == 3) {
    // batched GEMM (pfk_conv_b16_desc.batches): src [Bt, M, K] bf16, weight [Bt, cout, K] bf16, out [Bt, M, cout], residual [Bt, M, cout]
    TORCH_CHECK(srcs.size() == 1 && srcs[0].dim() == 3 && srcs[0].size(0) >= 1 && kh == 1 && kw == 1 && epilogue == PFK_EPI_LINEAR &&
                out.has_value() && out->dim() == 3 && (!residual.has_value() || residual->dim() == 3),
                "conv2d_b16 (batched): one [Bt, M, K] source, [Bt, cout, K] weight, [Bt, M, cout] out / residual, 1x1, linear epilogue");
    const Tensor& a = srcs[0];
    const int64_t Bt = a.size(0), M = a.size(1), K = a.size(2);
    TORCH_CHECK(weight.size(0) == Bt && weight.size(1) == cout && weight.size(2) == (K + 63) / 64 * 64 && B == 1 && H * W == M &&
                out->size(0) == Bt && (!residual.has_value() || residual->size(0) == Bt), "conv2d_b16 (batched): shapes");
    // batch 0 of each operand as a row view (the batch strides go to the descriptor; every batch lies inside its own tensor)
    fill_sources(d, {a.select(0, 0)}, M, B16, "conv2d_b16 (batched)");
    d.B = 1; d.H = H; d.W = W; d.kh = 1; d.kw = 1; d.cout = cout; d.epilogue = PFK_EPI_LINEAR; d.relu = relu; d.scale = (float)scale;
    const Rows o = rows("conv2d_b16 (batched)", out->select(0, 0), "out", Any).expect(M, cout);
    d.out = o.raw(); d.out_ld = o.ld; d.out_bf16 = o.b16;
    d.batches = Bt; d.src_batch_stride = a.stride(0); d.weight_batch_stride = weight.stride(0); d.out_batch_stride = out->stride(0);
    if (residual.has_value()) {
      const Rows r = rows("conv2d_b16 (batched)", residual->select(0, 0), "residual", Any).expect(M, cout);
      d.residual = r.raw(); d.residual_ld = r.ld; d.residual_bf16 = r.b16; d.residual_batch_stride = residual->stride(0);
    }
    check_ok(pfk_conv2d_b16(&d, cur_stream()), "conv2d_b16 (batched)");
    return;
  }
  TORCH_CHECK(stride >= 1, "conv2d_b16: stride");
  d.stride = (int)stride;
  d.relu_after_residual = relu_after_residual;
  const int64_t M = out_rows(B, H, W, stride), Ch = gru_hidden(epilogue, cout);
  fill_sources(d, srcs, B * H * W, B16, op);
  d.B = B; d.H = H; d.W = W; d.kh = kh; d.kw = kw; d.cout = cout;
  d.epilogue = epilogue; d.relu = relu; d.scale = (float)scale;
  TORCH_CHECK(weight.dim() == 2 && weight.size(0) == cout, "conv2d_b16: bf16 packed weight [cout, ktot]");
  TORCH_CHECK(weight.size(1) == pfk_conv_ktot_b16(&d), "conv2d_b16: packed weight has ktot ", weight.size(1), ", expected ",
              pfk_conv_ktot_b16(&d));
  if (out.has_value()) {
    const Rows o = rows(op, *out, "out", Any).expect(M, cout);
    d.out = o.raw(); d.out_ld = o.ld; d.out_coff = 0; d.out_bf16 = o.b16;
  }
  if (h.has_value()) { const Rows v = rows(op, *h, "h", F32).expect(M, AtLeast{Ch}); d.h = v.f32(); d.h_ld = v.ld; }
  if (h_b16.has_value()) { const Rows v = rows(op, *h_b16, "h_b16", B16).expect(M, AtLeast{Ch}); d.h_b16 = v.raw(); d.h_b16_ld = v.ld; }
  d.aux_z = dense(op, aux_z, "aux_z", B16, AtLeast{M * Ch}).raw();
  d.aux_rh = dense(op, aux_rh, "aux_rh", B16, AtLeast{M * Ch}).raw();
  if (residual.has_value()) {
    const Rows r = rows(op, *residual, "residual", Any).expect(M, cout);
    TORCH_CHECK(lin || r.b16, "conv2d_b16: the GRU epilogues take a bfloat16 residual (the context term)");
    d.residual = r.raw(); d.residual_ld = r.ld; d.residual_bf16 = r.b16 && lin;
  }
  if (gelu_entry) {
    check_ok(pfk_conv2d_gelu_b16(&d, cur_stream()), "conv2d_gelu_b16");
    return;
  }
  check_ok(pfk_conv2d_b16(&d, cur_stream()), "conv2d_b16");
}

void conv2d_b16(at::TensorList srcs, int64_t B, int64_t H, int64_t W, int64_t kh, int64_t kw, const Tensor& weight,
                const c10::optional<Tensor>& bias, int64_t cout, int64_t epilogue, bool relu, double scale,
                const c10::optional<Tensor>& out, const c10::optional<Tensor>& h, const c10::optional<Tensor>& h_b16,
                const c10::optional<Tensor>& aux_z, const c10::optional<Tensor>& aux_rh, const c10::optional<Tensor>& residual,
                int64_t stride, bool relu_after_residual) {
  conv2d_b16_run(srcs, B, H, W, kh, kw, weight, bias, cout, epilogue, relu, scale, out, h, h_b16, aux_z, aux_rh, residual, stride,
                 relu_after_residual, false);
}

// K8b + exact GELU (pfk_conv2d_gelu_b16): SEA-RAFT's pwconv1 + nn.GELU() on bf16 rows; `out` bf16 or fp32, residual as LINEAR
void conv2d_gelu_b16(at::TensorList srcs, int64_t B, int64_t H, int64_t W, int64_t kh, int64_t kw, const Tensor& weight,
                     const c10::optional<Tensor>& bias, int64_t cout, double scale, const Tensor& out,
                     const c10::optional<Tensor>& residual) {
  TORCH_CHECK(weight.dim() == 2, "conv2d_gelu_b16: bf16 packed weight [cout, ktot] (no batched form)");
  conv2d_b16_run(srcs, B, H, W, kh, kw, weight, bias, cout, PFK_EPI_LINEAR_GELU, false, scale, out, c10::nullopt, c10::nullopt,
                 c10::nullopt, c10::nullopt, residual, 1, false, true);
}

void debug_set_b16(int64_t cfg) { check_ok(pfk_debug_set_b16((int)cfg), "debug_set_b16"); }
void debug_set_stem_valu(int64_t on) { check_ok(pfk_debug_set_stem_valu((int)on), "debug_set_stem_valu"); }
void debug_set_cin2_valu(int64_t on) { check_ok(pfk_debug_set_cin2_valu((int)on), "debug_set_cin2_valu"); }

void conv_cin2(const Tensor& in, const Tensor& weight, const c10::optional<Tensor>& bias, Tensor out,
               int64_t B, int64_t H, int64_t W, int64_t k, bool relu) {
  OpScope scope(in);
  const Rows i = rows("conv_cin2", in, "inp", F32).expect(B * H * W, AtLeast{2});
  const Rows o = rows("conv_cin2", out, "out", Any).expect(B * H * W, AtLeast{0});
  const int cout = o.cols;
  const float* wp = dense("conv_cin2", weight, "weight [k*k,2,cout]", F32, k * k * 2 * cout).f32();
  const float* bp = dense("conv_cin2", bias, "bias", F32, AtLeast{cout}).f32();
  if (o.b16) check_ok(pfk_conv_cin2_b16(i.f32(), i.ld, wp, bp, o.raw(), o.ld, 0, B, H, W, k, cout, relu, cur_stream()), "conv_cin2 (bf16 out)");
  else check_ok(pfk_conv_cin2_f32(i.f32(), i.ld, wp, bp, o.f32(), o.ld, 0, B, H, W, k, cout, relu, cur_stream()), "conv_cin2");
}

void flow_delta(const Tensor& in, const Tensor& weight, const c10::optional<Tensor>& bias, const Tensor& coords0,
                Tensor coords1, const c10::optional<Tensor>& delta_out, const c10::optional<Tensor>& flow_out,
                const c10::optional<Tensor>& flow_out_b16) {
  OpScope scope(in);
  const float* c0 = dense("flow_delta", coords0, "coords0", F32).f32();
  TORCH_CHECK(coords0.dim() == 4 && coords0.size(1) == 2, "flow_delta: coords0 must be [B,2,h,w] contiguous");
  const int B = coords0.size(0), H = coords0.size(2), W = coords0.size(3);
  const int64_t M = (int64_t)B * H * W;
  float* c1 = dense("flow_delta", coords1, "coords1", F32, 2 * M).f32();
  const Rows i = rows("flow_delta", in, "inp", Any).expect(M, AtLeast{0});
  const int cin = i.cols;
  const float* wp = dense("flow_delta", weight, "weight", F32, 9 * 2 * cin).f32();
  const float* bp = dense("flow_delta", bias, "bias", F32, AtLeast{2}).f32();
  float* dp = dense("flow_delta", delta_out, "delta_out", F32, 2 * M).f32();
  TORCH_CHECK(coords1.sizes() == coords0.sizes() && (!delta_out.has_value() || delta_out->sizes() == coords0.sizes()),
              "flow_delta: coords1 and delta_out must have coords0's shape");
  float* fp = nullptr; int fld = 0;
  if (flow_out.has_value()) { const Rows f = rows("flow_delta", *flow_out, "flow_out", F32).expect(M, AtLeast{2}); fp = f.f32(); fld = f.ld; }
  if (i.b16) {
    void* fb = nullptr; int fbld = 0;
    if (flow_out_b16.has_value()) {
      const Rows f = rows("flow_delta", *flow_out_b16, "flow_out_b16", B16).expect(M, AtLeast{2});
      fb = f.raw(); fbld = f.ld;
    }
    check_ok(pfk_flow_delta_b16(i.raw(), i.ld, cin, wp, bp, c0, c1, dp, fp, fld, fb, fbld, B, H, W, cur_stream()), "flow_delta (bf16 in)");
    return;
  }
  TORCH_CHECK(!flow_out_b16.has_value(), "flow_delta: flow_out_b16 goes with a bfloat16 input");
  check_ok(pfk_flow_delta_f32(i.f32(), i.ld, cin, wp, bp, c0, c1, dp, fp, fld, B, H, W, cur_stream()), "flow_delta");
}

void flow_from_coords(const Tensor& coords0, const Tensor& coords1, Tensor flow_out) {
  OpScope scope(coords0);
  const float* c0 = dense("flow_from_coords", coords0, "coords0", F32).f32();
  TORCH_CHECK(coords0.dim() == 4 && coords0.size(1) == 2, "flow_from_coords: coords0 must be [B,2,h,w] contiguous");
  const float* c1 = dense("flow_from_coords", coords1, "coords1", F32, coords0.numel()).f32();
  TORCH_CHECK(coords1.sizes() == coords0.sizes(), "flow_from_coords: coords1 must have coords0's shape");
  const int64_t B = coords0.size(0), H = coords0.size(2), W = coords0.size(3);
  const Rows f = rows("flow_from_coords", flow_out, "flow_out", F32).expect(B * H * W, AtLeast{2});
  check_ok(pfk_flow_from_coords_f32(c0, c1, f.f32(), f.ld, B, H, W, cur_stream()), "flow_from_coords");
}

void convex_upsample(const Tensor& flow, const Tensor& mask, Tensor out) {
  OpScope scope(flow);
  const float* fp = dense("convex_upsample", flow, "flow", F32).f32();
  TORCH_CHECK(flow.dim() == 4 && flow.size(1) == 2, "convex_upsample: flow must be [B,2,H,W] contiguous");
  const int B = flow.size(0), H = flow.size(2), W = flow.size(3);
  const int64_t M = (int64_t)B * H * W;
  const Rows m = rows("convex_upsample", mask, "mask", F32).expect(M, 576);
  float* dst = dense("convex_upsample", out, "out [B,2,8H,8W]", F32, M * 2 * 64).f32();
  check_ok(pfk_convex_upsample_f32(fp, m.f32(), m.ld, dst, B, H, W, cur_stream()), "convex_upsample");
}

void upflow8(const Tensor& coords0, const Tensor& coords1, Tensor out) {
  OpScope scope(coords0);
  const Up8 o = up8("upflow8", out, "out");
  const float* c0 = dense("upflow8", coords0, "coords0", F32, 2 * o.rows()).f32();
  const float* c1 = dense("upflow8", coords1, "coords1", F32, 2 * o.rows()).f32();
  TORCH_CHECK(coords0.dim() == 4 && coords0.size(0) == o.B && coords0.size(1) == 2 && coords0.size(2) == o.H && coords0.size(3) == o.W &&
              coords1.sizes() == coords0.sizes(), "upflow8: coords [B, 2, H, W] contiguous, out [B, 2, 8H, 8W]");
  check_ok(pfk_upflow8_f32(c0, c1, o.ptr, o.B, o.H, o.W, cur_stream()), "upflow8");
}

void convex_upsample_pm(const Tensor& flow_pm, const Tensor& mask, Tensor out) {
  OpScope scope(flow_pm);
  const Up8 o = up8("convex_upsample_pm", out, "out");
  const Rows f = rows("convex_upsample_pm", flow_pm, "flow_pm", F32).expect(o.rows(), AtLeast{2});
  const Rows m = rows("convex_upsample_pm", mask, "mask", Any).expect(o.rows(), 576);
  if (m.b16) {
    check_ok(pfk_convex_upsample_pm_b16(f.f32(), f.ld, m.raw(), m.ld, o.ptr, o.B, o.H, o.W, cur_stream()), "convex_upsample_pm (bf16 mask)");
    return;
  }
  check_ok(pfk_convex_upsample_pm_f32(f.f32(), f.ld, m.f32(), m.ld, o.ptr, o.B, o.H, o.W, cur_stream()), "convex_upsample_pm");
}

// `upsample_flow(flow, mask, scale=2)` (ccmr/ccmr.py:128-139): flow NCHW [B, 2, H, W] contiguous (convex_upsample2) or pixel-major
// [M, >=2] rows (convex_upsample2_pm), mask [M, 36] fp32 rows, out [B, 2, 2H, 2W]
void convex_upsample2_impl(const char* op, bool pm, const Tensor& flow, const Tensor& mask, const Tensor& out) {
  OpScope scope(flow);
  const Up8 o = up8(op, out, "out", 2);
  const Rows m = rows(op, mask, "mask", F32).expect(o.rows(), 36);
  const float* fp;
  int flow_ld = 0;
  if (pm) {
    const Rows f = rows(op, flow, "flow_pm", F32).expect(o.rows(), AtLeast{2});
    fp = f.f32(); flow_ld = (int)f.ld;
  } else {
    fp = dense(op, flow, "flow", F32, 2 * o.rows()).f32();
    TORCH_CHECK(flow.dim() == 4 && flow.size(0) == o.B && flow.size(1) == 2 && flow.size(2) == o.H && flow.size(3) == o.W, op,
                ": flow [B, 2, H, W] contiguous, out [B, 2, 2H, 2W]");
  }
  check_ok(pfk_convex_upsample2_f32(fp, flow_ld, m.f32(), m.ld, o.ptr, o.B, o.H, o.W, cur_stream()), op);
}
void convex_upsample2(const Tensor& flow, const Tensor& mask, Tensor out) { convex_upsample2_impl("convex_upsample2", false, flow, mask, out); }
void convex_upsample2_pm(const Tensor& flow_pm, const Tensor& mask, Tensor out) { convex_upsample2_impl("convex_upsample2_pm", true, flow_pm, mask, out); }

// SEARAFT.upsample_data: flow_pm [M, >=2] / info_pm [M, >=n] / mask [M, 576] views, flow_out [B, 2, 8H, 8W], info_out [B, n, 8H, 8W];
// the mask fp32 (convex_upsample_info_pm) or bf16 (convex_upsample_info_pm_b16)
void convex_upsample_info_pm_impl(const char* op, Elem mask_elem, const Tensor& flow_pm, const Tensor& info_pm, const Tensor& mask,
                                  const Tensor& flow_out, const Tensor& info_out) {
  OpScope scope(flow_pm);
  const Up8 o = up8(op, flow_out, "flow_out");
  float* io = dense(op, info_out, "info_out", F32).f32();
  TORCH_CHECK(info_out.dim() == 4 && info_out.size(0) == o.B && info_out.size(2) == 8 * o.H && info_out.size(3) == 8 * o.W,
              op, ": info_out [B, n, 8H, 8W] contiguous");
  const int n = info_out.size(1);
  const Rows f = rows(op, flow_pm, "flow_pm", F32).expect(o.rows(), AtLeast{2});
  const Rows i = rows(op, info_pm, "info_pm", F32).expect(o.rows(), AtLeast{n});
  const Rows m = rows(op, mask, "mask", mask_elem).expect(o.rows(), 576);
  if (m.b16) check_ok(pfk_convex_upsample_info_pm_b16(f.f32(), f.ld, i.f32(), i.ld, n, m.raw(), m.ld, o.ptr, io, o.B, o.H, o.W, cur_stream()), op);
  else check_ok(pfk_convex_upsample_info_pm_f32(f.f32(), f.ld, i.f32(), i.ld, n, m.f32(), m.ld, o.ptr, io, o.B, o.H, o.W, cur_stream()), op);
}
void convex_upsample_info_pm(const Tensor& flow_pm, const Tensor& info_pm, const Tensor& mask, Tensor flow_out, Tensor info_out) {
  convex_upsample_info_pm_impl("convex_upsample_info_pm", F32, flow_pm, info_pm, mask, flow_out, info_out);
}
void convex_upsample_info_pm_b16(const Tensor& flow_pm, const Tensor& info_pm, const Tensor& mask, Tensor flow_out, Tensor info_out) {
  convex_upsample_info_pm_impl("convex_upsample_info_pm_b16", B16, flow_pm, info_pm, mask, flow_out, info_out);
}

// ConvNextBlock dwconv + LayerNorm: in [B*H*W, C] view (e.g. a slice of the update engine's hx), dw_weight [C, 1, k, k] or [C, k*k]
// contiguous, out [B*H*W, >= C] view; weights fp32.  Rows fp32 (dwconv_layernorm) or bf16 (pfk_dwconv_layernorm_b16)
void dwconv_layernorm_impl(const char* op, Elem e, const Tensor& in, const Tensor& dw_weight, const c10::optional<Tensor>& dw_bias,
                           const Tensor& ln_weight, const Tensor& ln_bias, double eps, const Tensor& out, int64_t B, int64_t H, int64_t W,
                           int64_t k) {
  OpScope scope(in);
  const Rows i = rows(op, in, "inp", e).expect(B * H * W, AtLeast{0});
  const int64_t C = i.cols;
  const Rows o = rows(op, out, "out", e).expect(B * H * W, AtLeast{C});
  const float* dw = dense(op, dw_weight, "dw_weight [C, k*k]", F32, C * k * k).f32();
  const float* db = dense(op, dw_bias, "dw_bias", F32, C).f32();
  const float* lw = dense(op, ln_weight, "ln_weight", F32, C).f32();
  const float* lb = dense(op, ln_bias, "ln_bias", F32, C).f32();
  if (e == B16) check_ok(pfk_dwconv_layernorm_b16(i.raw(), i.ld, dw, db, lw, lb, (float)eps, o.raw(), o.ld, B, H, W, C, k, cur_stream()), op);
  else check_ok(pfk_dwconv_layernorm_f32(i.f32(), i.ld, dw, db, lw, lb, (float)eps, o.f32(), o.ld, B, H, W, C, k, cur_stream()), op);
}
void dwconv_layernorm(const Tensor& in, const Tensor& dw_weight, const c10::optional<Tensor>& dw_bias, const Tensor& ln_weight,
                      const Tensor& ln_bias, double eps, Tensor out, int64_t B, int64_t H, int64_t W, int64_t k) {
  dwconv_layernorm_impl("dwconv_layernorm", F32, in, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, B, H, W, k);
}
void dwconv_layernorm_b16(const Tensor& in, const Tensor& dw_weight, const c10::optional<Tensor>& dw_bias, const Tensor& ln_weight,
                          const Tensor& ln_bias, double eps, Tensor out, int64_t B, int64_t H, int64_t W, int64_t k) {
  dwconv_layernorm_impl("dwconv_layernorm_b16", B16, in, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, B, H, W, k);
}

// ---- K12d: training the ConvNeXt block (pfk_convnext_bwd.hip).  Row views [M, C] of wider buffers are fine; only C columns are touched.

// dwconv_layernorm that also saves xhat [M, >= C] and rstd [M] for the backward; `out` has dwconv_layernorm's bits.  Each op of this
// block has one body for its fp32 and its bf16 (K12f: `_b16`) form: rows of element type `e`, parameters and their gradients fp32
void dwconv_layernorm_train_impl(const char* op, Elem e, const Tensor& in, const Tensor& dw_weight, const c10::optional<Tensor>& dw_bias,
                                 const Tensor& ln_weight, const Tensor& ln_bias, double eps, const Tensor& out, const Tensor& xhat,
                                 const Tensor& rstd, int64_t B, int64_t H, int64_t W, int64_t k) {
  OpScope scope(in);
  const int64_t M = B * H * W;
  const Rows i = rows(op, in, "inp", e).expect(M, AtLeast{0});
  const int64_t C = i.cols;
  const Rows o = rows(op, out, "out", e).expect(M, C), x = rows(op, xhat, "xhat", e).expect(M, C);
  const float* dw = dense(op, dw_weight, "dw_weight", F32, C * k * k).f32();
  const float* db = dense(op, dw_bias, "dw_bias", F32, C).f32();
  const float* lw = dense(op, ln_weight, "ln_weight", F32, C).f32();
  const float* lb = dense(op, ln_bias, "ln_bias", F32, C).f32();
  float* rs = dense(op, rstd, "rstd", F32, M).f32();
  if (e == B16)
    check_ok(pfk_dwconv_layernorm_train_b16(i.raw(), i.ld, dw, db, lw, lb, (float)eps, o.raw(), o.ld, x.raw(), x.ld, rs, B, H, W, C, k,
                                            cur_stream()), op);
  else
    check_ok(pfk_dwconv_layernorm_train_f32(i.f32(), i.ld, dw, db, lw, lb, (float)eps, o.f32(), o.ld, x.f32(), x.ld, rs, B, H, W, C, k,
                                            cur_stream()), op);
}
void dwconv_layernorm_train(const Tensor& in, const Tensor& dw_weight, const c10::optional<Tensor>& dw_bias, const Tensor& ln_weight,
                            const Tensor& ln_bias, double eps, Tensor out, Tensor xhat, Tensor rstd, int64_t B, int64_t H, int64_t W,
                            int64_t k) {
  dwconv_layernorm_train_impl("dwconv_layernorm_train", F32, in, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, xhat, rstd, B, H, W, k);
}
void dwconv_layernorm_train_b16(const Tensor& in, const Tensor& dw_weight, const c10::optional<Tensor>& dw_bias, const Tensor& ln_weight,
                                const Tensor& ln_bias, double eps, Tensor out, Tensor xhat, Tensor rstd, int64_t B, int64_t H, int64_t W,
                                int64_t k) {
  dwconv_layernorm_train_impl("dwconv_layernorm_train_b16", B16, in, dw_weight, dw_bias, ln_weight, ln_bias, eps, out, xhat, rstd, B, H, W, k);
}

void layernorm_bwd_impl(const char* op, Elem e, const Tensor& xhat, const Tensor& rstd, const Tensor& ln_weight, const Tensor& dy,
                        const Tensor& du, const Tensor& dgamma, const Tensor& dbeta) {
  OpScope scope(xhat);
  const Rows x = rows(op, xhat, "xhat", e);
  const int64_t M = x.rows, C = x.cols;
  const Rows g = rows(op, dy, "dy", e).expect(M, C), u = rows(op, du, "du", e).expect(M, C);
  const float* rs = dense(op, rstd, "rstd", F32, M).f32();
  const float* lw = dense(op, ln_weight, "ln_weight", F32, C).f32();
  float* dg = dense(op, dgamma, "dgamma", F32, C).f32();
  float* dbt = dense(op, dbeta, "dbeta", F32, C).f32();
  const long long need = pfk_layernorm_bwd_workspace_bytes(M, C);
  const auto ws = byte_workspace(need, xhat);
  if (e == B16) check_ok(pfk_layernorm_bwd_b16(x.raw(), x.ld, rs, lw, g.raw(), g.ld, u.raw(), u.ld, dg, dbt, ws.second, need, M, C, cur_stream()), op);
  else check_ok(pfk_layernorm_bwd_f32(x.f32(), x.ld, rs, lw, g.f32(), g.ld, u.f32(), u.ld, dg, dbt, ws.second, need, M, C, cur_stream()), op);
}
void layernorm_bwd(const Tensor& xhat, const Tensor& rstd, const Tensor& ln_weight, const Tensor& dy, Tensor du, Tensor dgamma,
                   Tensor dbeta) {
  layernorm_bwd_impl("layernorm_bwd", F32, xhat, rstd, ln_weight, dy, du, dgamma, dbeta);
}
void layernorm_bwd_b16(const Tensor& xhat, const Tensor& rstd, const Tensor& ln_weight, const Tensor& dy, Tensor du, Tensor dgamma,
                       Tensor dbeta) {
  layernorm_bwd_impl("layernorm_bwd_b16", B16, xhat, rstd, ln_weight, dy, du, dgamma, dbeta);
}

void dwconv_bwd_impl(const char* op, Elem e, const Tensor& in, const Tensor& du, const Tensor& dw_weight, const Tensor& dx,
                     const Tensor& dweight, const c10::optional<Tensor>& dbias, int64_t B, int64_t H, int64_t W, int64_t k) {
  OpScope scope(in);
  const int64_t M = B * H * W;
  const Rows i = rows(op, in, "inp", e).expect(M, AtLeast{0});
  const int64_t C = i.cols;
  const Rows u = rows(op, du, "du", e).expect(M, C), x = rows(op, dx, "dx", e).expect(M, C);
  const float* w = dense(op, dw_weight, "dw_weight", F32, C * k * k).f32();
  float* dw = dense(op, dweight, "dweight", F32, C * k * k).f32();
  float* db = dense(op, dbias, "dbias", F32, C).f32();
  const long long need = pfk_dwconv_bwd_workspace_bytes(B, H, W, C, k);
  const auto ws = byte_workspace(need, in);
  if (e == B16) check_ok(pfk_dwconv_bwd_b16(i.raw(), i.ld, u.raw(), u.ld, w, x.raw(), x.ld, dw, db, ws.second, need, B, H, W, C, k, cur_stream()), op);
  else check_ok(pfk_dwconv_bwd_f32(i.f32(), i.ld, u.f32(), u.ld, w, x.f32(), x.ld, dw, db, ws.second, need, B, H, W, C, k, cur_stream()), op);
}
void dwconv_bwd(const Tensor& in, const Tensor& du, const Tensor& dw_weight, Tensor dx, Tensor dweight, const c10::optional<Tensor>& dbias,
                int64_t B, int64_t H, int64_t W, int64_t k) {
  dwconv_bwd_impl("dwconv_bwd", F32, in, du, dw_weight, dx, dweight, dbias, B, H, W, k);
}
void dwconv_bwd_b16(const Tensor& in, const Tensor& du, const Tensor& dw_weight, Tensor dx, Tensor dweight, const c10::optional<Tensor>& dbias,
                    int64_t B, int64_t H, int64_t W, int64_t k) {
  dwconv_bwd_impl("dwconv_bwd_b16", B16, in, du, dw_weight, dx, dweight, dbias, B, H, W, k);
}

// y = gelu(x), or with `dy` the derivative dx = dy * gelu'(x), into `out`
void gelu_rows_impl(const char* op, Elem e, const Tensor& x, const Tensor* dy, const Tensor& out, const char* out_name) {
  OpScope scope(x);
  const Rows a = rows(op, x, "x", e), o = rows(op, out, out_name, e).expect(a.rows, a.cols);
  if (dy == nullptr) {
    if (e == B16) check_ok(pfk_gelu_b16(a.raw(), a.ld, o.raw(), o.ld, a.rows, a.cols, cur_stream()), op);
    else check_ok(pfk_gelu_f32(a.f32(), a.ld, o.f32(), o.ld, a.rows, a.cols, cur_stream()), op);
    return;
  }
  const Rows g = rows(op, *dy, "dy", e).expect(a.rows, a.cols);
  if (e == B16) check_ok(pfk_gelu_bwd_b16(a.raw(), a.ld, g.raw(), g.ld, o.raw(), o.ld, a.rows, a.cols, cur_stream()), op);
  else check_ok(pfk_gelu_bwd_f32(a.f32(), a.ld, g.f32(), g.ld, o.f32(), o.ld, a.rows, a.cols, cur_stream()), op);
}
void gelu_rows(const Tensor& x, Tensor y) { gelu_rows_impl("gelu", F32, x, nullptr, y, "y"); }
void gelu_rows_b16(const Tensor& x, Tensor y) { gelu_rows_impl("gelu_b16", B16, x, nullptr, y, "y"); }
void gelu_rows_bwd(const Tensor& x, const Tensor& dy, Tensor dx) { gelu_rows_impl("gelu_bwd", F32, x, &dy, dx, "dx"); }
void gelu_rows_bwd_b16(const Tensor& x, const Tensor& dy, Tensor dx) { gelu_rows_impl("gelu_bwd_b16", B16, x, &dy, dx, "dx"); }

// fused mask conv2 + softmax + convex upsampling: x [M, cin] (a view of the fh|mask hidden buffer), weight / bias row-permuted (pfk.h)
void mask_upsample(const Tensor& x, const Tensor& weight_perm, const c10::optional<Tensor>& bias_perm, double scale,
                   const Tensor& flow_pm, Tensor out) {
  OpScope scope(x);
  const Up8 o = up8("mask_upsample", out, "out");
  const Rows a = rows("mask_upsample", x, "x", Any).expect(o.rows(), AtLeast{0});
  const Rows f = rows("mask_upsample", flow_pm, "flow_pm", F32).expect(o.rows(), AtLeast{2});
  const int cin = a.cols;
  // a bf16 activation needs the bf16 permuted weight
  const Ptr w = dense("mask_upsample", weight_perm, "weight_perm", a.b16 ? B16 : F32, 640 * (int64_t)cin);
  TORCH_CHECK(weight_perm.dim() == 2 && weight_perm.size(0) == 640, "mask_upsample: weight_perm [640, cin] (packing.permute_mask_head)");
  const float* bp = dense("mask_upsample", bias_perm, "bias_perm", F32, 640).f32();
  if (a.b16) {
    check_ok(pfk_mask_upsample_b16(a.raw(), a.ld, cin, w.raw(), bp, (float)scale, f.f32(), f.ld, o.ptr, o.B, o.H, o.W, cur_stream()),
             "mask_upsample (bf16)");
    return;
  }
  check_ok(pfk_mask_upsample_f32(a.f32(), a.ld, cin, w.f32(), bp, (float)scale, f.f32(), f.ld, o.ptr, o.B, o.H, o.W, cur_stream()),
           "mask_upsample");
}

// alt_cuda_corr.forward semantics (correlation.cpp:23-37): returns [B, N, (2r+1)^2, H1, W1], unscaled
Tensor altcorr_forward(const Tensor& fmap1, const Tensor& fmap2, const Tensor& coords, int64_t radius) {
  OpScope scope(fmap1);
  const char* op = "altcorr_forward";
  // fp32 maps (the reference extension's only type, correlation_kernel.cu:275) or bf16 maps (pfk_altcorr_forward_bf16: exact widening,
  // fp32 products and accumulation; the result is fp32 either way — coords stay fp32)
  const Ptr f1 = dense(op, fmap1, "fmap1", Any), f2 = dense(op, fmap2, "fmap2", f1.b16 ? B16 : F32);    // CHECK_CONTIGUOUS in the reference
  dense(op, coords, "coords", F32);
  TORCH_CHECK(fmap1.dim() == 4 && fmap2.dim() == 4 && coords.dim() == 5 && coords.size(4) == 2, "altcorr_forward: fmap [B,H,W,C], coords [B,N,H1,W1,2]");
  const int B = fmap1.size(0), H1 = fmap1.size(1), W1 = fmap1.size(2), C = fmap1.size(3);
  const int H2 = fmap2.size(1), W2 = fmap2.size(2), N = coords.size(1);
  TORCH_CHECK(fmap2.size(0) == B && fmap2.size(3) == C && coords.size(0) == B && coords.size(2) == H1 && coords.size(3) == W1,
              "altcorr_forward: fmap2 / coords do not match fmap1's [B,H1,W1,C]");
  const int rd = 2 * radius + 1;
  Tensor out = at::empty({B, N, rd * rd, H1, W1}, coords.options());
  // the launch-wide gate's per-block counts (pfk.h): a few hundred bytes from the caching allocator, written before they are read
  Tensor ws = at::empty({std::max<int64_t>(1, pfk_altcorr_workspace_bytes(B, H1, W1) / 4)}, coords.options().dtype(at::kInt));
  void* wsp = dense(op, ws, "workspace", Raw).raw();
  for (int n = 0; n < N; ++n) {
    Tensor cn = coords.select(1, n).contiguous();
    Tensor on = N == 1 ? out.view({B, rd * rd, H1, W1}) : at::empty({B, rd * rd, H1, W1}, coords.options());
    const float* cp = dense(op, cn, "coords", F32, (int64_t)B * H1 * W1 * 2).f32();
    float* dst = dense(op, on, "out", F32, (int64_t)B * rd * rd * H1 * W1).f32();
    if (f1.b16)
      check_ok(pfk_altcorr_forward_bf16(f1.raw(), f2.raw(), cp, dst, B, H1, W1, H2, W2, C, radius, wsp, cur_stream()), "altcorr_forward (bf16 maps)");
    else
      check_ok(pfk_altcorr_forward_f32(f1.f32(), f2.f32(), cp, dst, B, H1, W1, H2, W2, C, radius, wsp, cur_stream()), "altcorr_forward");
    if (N != 1) out.select(1, n).copy_(on);
  }
  return out;
}

// alt_cuda_corr.backward semantics (correlation.cpp:39-49): returns {fmap1_grad, fmap2_grad, coords_grad (zeros)}
std::vector<Tensor> altcorr_backward(const Tensor& fmap1, const Tensor& fmap2, const Tensor& coords, const Tensor& corr_grad,
                                     int64_t radius) {
  OpScope scope(fmap1);
  const char* op = "altcorr_backward";
  const float* f1 = dense(op, fmap1, "fmap1", F32).f32();
  const float* f2 = dense(op, fmap2, "fmap2", F32).f32();
  dense(op, coords, "coords", F32); dense(op, corr_grad, "corr_grad", F32);
  TORCH_CHECK(fmap1.dim() == 4 && fmap2.dim() == 4 && coords.dim() == 5 && corr_grad.dim() == 5,
              "altcorr_backward: fmap [B,H,W,C], coords [B,N,H1,W1,2], corr_grad [B,N,(2r+1)^2,H1,W1]");
  const int B = fmap1.size(0), H1 = fmap1.size(1), W1 = fmap1.size(2), C = fmap1.size(3);
  const int H2 = fmap2.size(1), W2 = fmap2.size(2), N = coords.size(1);
  const int rd = 2 * radius + 1;
  TORCH_CHECK(corr_grad.size(0) == B && corr_grad.size(1) == N && corr_grad.size(2) == rd * rd && corr_grad.size(3) == H1 &&
              corr_grad.size(4) == W1, "altcorr_backward: corr_grad [B,N,(2r+1)^2,H1,W1]");
  Tensor g1 = at::empty_like(fmap1), g2 = at::empty_like(fmap2), gc = at::zeros_like(coords);
  // correlation_kernel.cu:122-256 loops over the N coordinate sets inside the kernel; here one launch per set, summed
  for (int n = 0; n < N; ++n) {
    Tensor cn = N == 1 ? coords.view({B, H1, W1, 2}) : coords.select(1, n).contiguous();
    Tensor gn = N == 1 ? corr_grad.view({B, rd * rd, H1, W1}) : corr_grad.select(1, n).contiguous();
    Tensor t1 = n == 0 ? g1 : at::empty_like(fmap1), t2 = n == 0 ? g2 : at::empty_like(fmap2);
    check_ok(pfk_altcorr_backward_f32(f1, f2, dense(op, cn, "coords", F32).f32(), dense(op, gn, "corr_grad", F32).f32(),
                                      dense(op, t1, "fmap1_grad", F32, fmap1.numel()).f32(), dense(op, t2, "fmap2_grad", F32, fmap2.numel()).f32(),
                                      B, H1, W1, H2, W2, C, radius, cur_stream()), op);
    if (n) { g1.add_(t1); g2.add_(t2); }
  }
  return {g1, g2, gc};
}

// ---- blocked volume layout (include/pfk.h "K1-K3 on the BLOCKED volume layout"): levels are [M, pfk_blocked_map_elems(h_l, w_l)]
void fmap_to_blocked(const Tensor& in, Tensor out, int64_t B, int64_t H, int64_t W) {
  OpScope scope(in);
  const Rows i = rows("fmap_to_blocked", in, "inp", F32).expect(B * H * W, AtLeast{0});
  const Rows o = rows("fmap_to_blocked", out, "out [B*blocked_map_elems(H, W), C]", F32).expect(B * pfk_blocked_map_elems((int)H, (int)W), i.cols);
  check_ok(pfk_fmap_to_blocked_f32(i.f32(), i.ld, o.f32(), o.ld, (int)B, (int)H, (int)W, (int)i.cols, cur_stream()), "fmap_to_blocked");
}

void corr_pool2x2_blocked(const Tensor& in, Tensor out, int64_t H, int64_t W) {
  OpScope scope(in);
  const char* op = "corr_pool2x2_blocked";
  const Ptr i = dense(op, in, "inp", Any), o = dense(op, out, "out", i.b16 ? B16 : F32);
  TORCH_CHECK(in.dim() == 2 && out.dim() == 2 && in.size(0) == out.size(0), "corr_pool2x2_blocked: [M, elems] contiguous");
  TORCH_CHECK(in.size(1) == pfk_blocked_map_elems((int)H, (int)W) && out.size(1) == pfk_blocked_map_elems((int)(H / 2), (int)(W / 2)),
              "corr_pool2x2_blocked: map sizes");
  if (out.numel() == 0) return;
  if (i.b16) check_ok(pfk_corr_pool2x2_blocked_bf16(i.raw(), o.raw(), in.size(0), (int)H, (int)W, cur_stream()), "corr_pool2x2_blocked (bf16)");
  else check_ok(pfk_corr_pool2x2_blocked_f32(i.f32(), o.f32(), in.size(0), (int)H, (int)W, cur_stream()), op);
}

int64_t blocked_map_elems(int64_t H, int64_t W) { return pfk_blocked_map_elems((int)H, (int)W); }

// backward of corr_lookup: accumulates into grad_levels[l] ([B*N, ld_l] buffers holding one [h_l][w_l] map per row)
void corr_lookup_bwd(at::TensorList grad_levels, at::IntArrayRef lvl_h, at::IntArrayRef lvl_w, const Tensor& coords,
                     int64_t radius, const Tensor& grad_out) {
  OpScope scope(coords);
  const char* op = "corr_lookup_bwd";
  TORCH_CHECK(grad_levels.size() >= 1 && grad_levels.size() <= PFK_MAX_LEVELS && lvl_h.size() == grad_levels.size() &&
              lvl_w.size() == grad_levels.size(), "corr_lookup_bwd: 1..8 levels with their map sizes");
  pfk_lookup_bwd_desc d{};
  d.coords = dense(op, coords, "coords", F32).f32();
  TORCH_CHECK(coords.dim() == 4 && coords.size(1) == 2, "corr_lookup_bwd: coords [B,2,h,w] contiguous");
  d.B = coords.size(0); d.h = coords.size(2); d.w = coords.size(3);
  const int64_t M = (int64_t)d.B * d.h * d.w;
  for (size_t l = 0; l < grad_levels.size(); ++l) {
    const Rows v = rows(op, grad_levels[l], "grad_level", F32).expect(M, AtLeast{lvl_h[l] * lvl_w[l]});
    d.grad_levels[l] = v.f32(); d.lvl_h[l] = lvl_h[l]; d.lvl_w[l] = lvl_w[l]; d.lvl_ld[l] = v.ld;
  }
  d.num_levels = grad_levels.size(); d.radius = radius;
  const int n = 2 * radius + 1;
  const Rows g = rows(op, grad_out, "grad_out", F32).expect(M, AtLeast{(int64_t)d.num_levels * n * n});
  d.grad_out = g.f32(); d.grad_out_ld = g.ld;
  check_ok(pfk_corr_lookup_bwd_f32(&d, cur_stream()), op);
}

// coordinate gradient of corr_lookup: levels [B*N, h_l, w_l] row-major fp32 maps (the training pyramid), grad_coords [B, 2, h, w] written
void corr_lookup_coords_bwd(at::TensorList levels, const Tensor& coords, int64_t radius, const Tensor& grad_out, Tensor grad_coords) {
  OpScope scope(coords);
  const char* op = "corr_lookup_coords_bwd";
  TORCH_CHECK(levels.size() >= 1 && levels.size() <= PFK_MAX_LEVELS, op, ": 1..8 levels");
  pfk_lookup_coords_bwd_desc d{};
  d.coords = dense(op, coords, "coords", F32).f32();
  TORCH_CHECK(coords.dim() == 4 && coords.size(1) == 2, op, ": coords [B,2,h,w] contiguous");
  d.B = coords.size(0); d.h = coords.size(2); d.w = coords.size(3);
  const int64_t M = (int64_t)d.B * d.h * d.w;
  for (size_t l = 0; l < levels.size(); ++l) {
    const Tensor& t = levels[l];
    TORCH_CHECK(t.dim() == 3 && t.size(0) == M && t.size(1) >= 1 && t.size(2) >= 1, op, ": every level must be a [B*h*w, h_l, w_l] map");
    d.levels[l] = dense(op, t, "level", F32).f32();
    d.lvl_h[l] = t.size(1); d.lvl_w[l] = t.size(2); d.lvl_ld[l] = t.size(1) * t.size(2);
  }
  d.num_levels = levels.size(); d.radius = radius;
  const int n = 2 * radius + 1;
  const Rows g = rows(op, grad_out, "grad_out", F32).expect(M, AtLeast{(int64_t)d.num_levels * n * n});
  d.grad_out = g.f32(); d.grad_out_ld = g.ld;
  d.grad_coords = dense(op, grad_coords, "grad_coords [B,2,h,w]", F32, 2 * M).f32();
  check_ok(pfk_corr_lookup_coords_bwd_f32(&d, cur_stream()), op);
}

// backward of corr_volume for one pyramid level, all batch elements: dC [B,N1,ldc] (columns >= N2 zero), f1 [B,N1,D],
// f2cm [B,D,ld2cm] channel-major zero-padded -> df1 [B,N1,D] (+= when accumulate), df2 [B,ldc,Dpad]
void corr_volume_bwd(const Tensor& dC, int64_t N2, const Tensor& f1, const Tensor& f2cm, double scale, Tensor df1, bool accumulate,
                     Tensor df2) {
  OpScope scope(dC);
  const char* op = "corr_volume_bwd";
  const float* dc = dense(op, dC, "dC", F32).f32();
  const float* a = dense(op, f1, "f1", F32).f32();
  const float* b = dense(op, f2cm, "f2cm", F32).f32();
  float* da = dense(op, df1, "df1", F32).f32();
  float* db = dense(op, df2, "df2", F32).f32();
  TORCH_CHECK(dC.dim() == 3 && f1.dim() == 3 && f2cm.dim() == 3 && df1.dim() == 3 && df2.dim() == 3, "corr_volume_bwd: 3-D tensors");
  const int B = dC.size(0), N1 = dC.size(1), ldc = dC.size(2), D = f1.size(2), ld2cm = f2cm.size(2);
  TORCH_CHECK(f1.size(0) == B && f1.size(1) == N1 && f2cm.size(0) == B && f2cm.size(1) == D && df1.sizes() == f1.sizes() &&
              df2.size(0) == B && df2.size(1) == ldc && df2.size(2) == (D + 31) / 32 * 32, "corr_volume_bwd: shape mismatch");
  const long long need = pfk_corr_volume_bwd_workspace_bytes(N1, ldc, D);
  const auto ws = byte_workspace(need, dC);
  for (int i = 0; i < B; ++i)
    check_ok(pfk_corr_volume_bwd_f32(dc + (int64_t)i * N1 * ldc, ldc, N1, (int)N2, a + (int64_t)i * N1 * D, D,
                                     b + (int64_t)i * D * ld2cm, ld2cm, D, (float)scale, da + (int64_t)i * N1 * D, D,
                                     accumulate, db + (int64_t)i * ldc * df2.size(2), ws.second, need, cur_stream()),
             op);
}

// backward of convex_upsample(_pm): flow NCHW [B,2,H,W] or pixel-major [M, >=2]
void convex_upsample_bwd(const Tensor& flow, const Tensor& mask, const Tensor& grad_out, Tensor grad_mask, Tensor grad_flow) {
  OpScope scope(mask);
  const char* op = "convex_upsample_bwd";
  const Up8 g = up8(op, grad_out, "grad_out");
  const int64_t M = g.rows();
  const float* fp; int flow_ld = 0;
  if (flow.dim() == 2) { const Rows f = rows(op, flow, "flow", F32).expect(M, AtLeast{2}); fp = f.f32(); flow_ld = f.ld; }
  else {
    fp = dense(op, flow, "flow", F32, 2 * M).f32();
    TORCH_CHECK(flow.dim() == 4 && flow.size(0) == g.B && flow.size(1) == 2 && flow.size(2) == g.H && flow.size(3) == g.W,
                "convex_upsample_bwd: flow [B,2,H,W] contiguous or pixel-major [M,2+]");
  }
  const Rows m = rows(op, mask, "mask", F32).expect(M, 576), gm = rows(op, grad_mask, "grad_mask", F32).expect(M, 576);
  float* gf = dense(op, grad_flow, "grad_flow [B,2,H,W]", F32, 2 * M).f32();
  const long long need = pfk_convex_upsample_bwd_workspace_bytes(g.B, g.H, g.W);
  const auto ws = byte_workspace(need, mask);
  check_ok(pfk_convex_upsample_bwd_f32(fp, flow_ld, m.f32(), m.ld, g.ptr, gm.f32(), gm.ld, gf, ws.second, need, g.B, g.H, g.W, cur_stream()), op);
}

// backward of convex_upsample2(_pm): flow and grad_flow NCHW [B,2,H,W] contiguous or pixel-major [M, >=2] / [M, 2] rows, each on its own;
// mask / grad_mask [M, 36] row views, grad_out [B, 2, 2H, 2W]
void convex_upsample2_bwd(const Tensor& flow, const Tensor& mask, const Tensor& grad_out, Tensor grad_mask, Tensor grad_flow) {
  OpScope scope(mask);
  const char* op = "convex_upsample2_bwd";
  const Up8 g = up8(op, grad_out, "grad_out", 2);
  const int64_t M = g.rows();
  const float* fp; int flow_ld = 0;
  if (flow.dim() == 2) { const Rows f = rows(op, flow, "flow", F32).expect(M, AtLeast{2}); fp = f.f32(); flow_ld = f.ld; }
  else {
    fp = dense(op, flow, "flow", F32, 2 * M).f32();
    TORCH_CHECK(flow.dim() == 4 && flow.size(0) == g.B && flow.size(1) == 2 && flow.size(2) == g.H && flow.size(3) == g.W, op,
                ": flow [B,2,H,W] contiguous or pixel-major [M,2+]");
  }
  float* gf; int gflow_ld = 0;
  if (grad_flow.dim() == 2) { const Rows r = rows(op, grad_flow, "grad_flow", F32).expect(M, 2); gf = r.f32(); gflow_ld = r.ld; }
  else {
    gf = dense(op, grad_flow, "grad_flow [B,2,H,W]", F32, 2 * M).f32();
    TORCH_CHECK(grad_flow.dim() == 4 && grad_flow.size(0) == g.B && grad_flow.size(1) == 2 && grad_flow.size(2) == g.H &&
                grad_flow.size(3) == g.W, op, ": grad_flow [B,2,H,W] contiguous or pixel-major [M,2]");
  }
  const Rows m = rows(op, mask, "mask", F32).expect(M, 36), gm = rows(op, grad_mask, "grad_mask", F32).expect(M, 36);
  const long long need = pfk_convex_upsample2_bwd_workspace_bytes(g.B, g.H, g.W);
  const auto ws = byte_workspace(need, mask);
  check_ok(pfk_convex_upsample2_bwd_f32(fp, flow_ld, m.f32(), m.ld, g.ptr, gm.f32(), gm.ld, gf, gflow_ld, ws.second, need, g.B, g.H, g.W,
                                        cur_stream()), op);
}

// backward of convex_upsample_info_pm (fp32 mask): row views as the forward's, grad_flow_up [B, 2, 8H, 8W], grad_info_up
// [B, n, 8H, 8W] or None (= zero), n = grad_info_pm's columns; grad_flow_pm [M, 2] / grad_info_pm [M, n] may be slices of one buffer
void convex_upsample_info_bwd(const Tensor& flow_pm, const Tensor& info_pm, const Tensor& mask, const Tensor& grad_flow_up,
                              const c10::optional<Tensor>& grad_info_up, Tensor grad_mask, Tensor grad_flow_pm, Tensor grad_info_pm) {
  OpScope scope(mask);
  const char* op = "convex_upsample_info_bwd";
  const Up8 g = up8(op, grad_flow_up, "grad_flow_up");
  const int64_t M = g.rows();
  const Rows gi = rows(op, grad_info_pm, "grad_info_pm", F32).expect(M, AtLeast{0});
  const int64_t n = gi.cols;
  TORCH_CHECK(n <= 8, op, ": at most 8 info channels, grad_info_pm has ", n);
  const Rows f = rows(op, flow_pm, "flow_pm", F32).expect(M, AtLeast{2});
  const Rows i = rows(op, info_pm, "info_pm", F32).expect(M, AtLeast{n});
  const Rows m = rows(op, mask, "mask", F32).expect(M, 576), gm = rows(op, grad_mask, "grad_mask", F32).expect(M, 576);
  const Rows gf = rows(op, grad_flow_pm, "grad_flow_pm", F32).expect(M, 2);
  const Ptr gu = dense(op, grad_info_up, "grad_info_up [B, n, 8H, 8W]", F32, n * M * 64);
  TORCH_CHECK(!grad_info_up.has_value() || (grad_info_up->dim() == 4 && grad_info_up->size(0) == g.B && grad_info_up->size(1) == n &&
                                            grad_info_up->size(2) == 8 * g.H && grad_info_up->size(3) == 8 * g.W),
              op, ": grad_info_up must be [B, n, 8H, 8W] contiguous with n = grad_info_pm's columns");
  const long long need = pfk_convex_upsample_info_bwd_workspace_bytes(g.B, g.H, g.W, (int)n);
  const auto ws = byte_workspace(need, mask);
  check_ok(pfk_convex_upsample_info_bwd_pm_f32(f.f32(), f.ld, i.f32(), i.ld, (int)n, m.f32(), m.ld, g.ptr, gu.ptr ? gu.f32() : nullptr,
                                               gm.f32(), gm.ld, gf.f32(), gf.ld, gi.f32(), gi.ld, ws.second, need, g.B, g.H, g.W,
                                               cur_stream()),
           op);
}

void nchw_to_pm(const Tensor& in, Tensor out) {
  OpScope scope(in);
  const float* ip = dense("nchw_to_pm", in, "inp", F32).f32();
  TORCH_CHECK(in.dim() == 4, "nchw_to_pm: inp must be [B,C,H,W] contiguous");
  const int B = in.size(0), C = in.size(1), H = in.size(2), W = in.size(3);
  const Rows o = rows("nchw_to_pm", out, "out", F32).expect((int64_t)B * H * W, C);
  check_ok(pfk_nchw_to_pm_f32(ip, o.f32(), o.ld, 0, B, C, H, W, cur_stream()), "nchw_to_pm");
}

void pm_to_nchw(const Tensor& in, Tensor out) {
  OpScope scope(in);
  float* dst = dense("pm_to_nchw", out, "out", F32).f32();
  TORCH_CHECK(out.dim() == 4, "pm_to_nchw: out must be [B,C,H,W] contiguous");
  const int B = out.size(0), C = out.size(1), H = out.size(2), W = out.size(3);
  const Rows i = rows("pm_to_nchw", in, "inp", F32).expect((int64_t)B * H * W, C);
  check_ok(pfk_pm_to_nchw_f32(i.f32(), i.ld, 0, dst, B, C, H, W, cur_stream()), "pm_to_nchw");
}

// in [B*N, C] pixel-major view -> out [B, C, Npad] channel-major (row stride = out.stride(1))
void pm_to_cm(const Tensor& in, Tensor out) {
  OpScope scope(in);
  TORCH_CHECK(out.dim() == 3 && out.size(0) >= 1 && out.stride(2) == 1 && out.stride(0) == out.size(1) * out.stride(1), "pm_to_cm: out [B,C,Npad]");
  const int B = out.size(0), C = out.size(1);
  const Rows i = rows("pm_to_cm", in, "inp", F32);
  TORCH_CHECK(i.cols == C && i.rows % B == 0, "pm_to_cm: inp must be [B*N, C] for out [B,C,Npad], got [", i.rows, ", ", i.cols, "]");
  const int N = i.rows / B;
  const Rows o = rows("pm_to_cm", out.view({(int64_t)B * C, out.size(2)}), "out", F32).expect((int64_t)B * C, AtLeast{N});      // the B*C channel rows
  check_ok(pfk_pm_to_cm_f32(i.f32(), i.ld, o.f32(), o.ld, B, C, N, cur_stream()), "pm_to_cm");
}

void conv_stem(const Tensor& img, const Tensor& weight, const c10::optional<Tensor>& bias, Tensor out, bool relu) {
  OpScope scope(img);
  const float* ip = dense("conv_stem", img, "img", F32).f32();
  TORCH_CHECK(img.dim() == 4 && img.size(1) == 3, "conv_stem: img [B,3,H,W] contiguous");
  const int B = img.size(0), H = img.size(2), W = img.size(3);
  const Rows o = rows("conv_stem", out, "out", Any).expect(out_rows(B, H, W, 2), AtLeast{0});
  const int cout = o.cols;
  const float* wp = dense("conv_stem", weight, "weight [49,3,cout]", F32, 49 * 3 * cout).f32();
  const float* b = dense("conv_stem", bias, "bias", F32, cout).f32();
  if (o.b16) {
    check_ok(pfk_conv_stem_b16(ip, wp, b, o.raw(), o.ld, B, H, W, cout, relu, cur_stream()), "conv_stem (bf16 out)");
    return;
  }
  check_ok(pfk_conv_stem_f32(ip, wp, b, o.f32(), o.ld, B, H, W, cout, relu, cur_stream()), "conv_stem");
}

// the stem for one or two 3-channel images (SEA-RAFT's ResNetFPN): img_a / img_b are [B,3,H,W] views whose three planes are dense
// (any batch stride >= 3*H*W: the channel halves of a [B,6,H,W] tensor are read in place); weight [49,cin,cout], cin = 3 or 6
void conv_stem2(const Tensor& img_a, const c10::optional<Tensor>& img_b, const Tensor& weight, const c10::optional<Tensor>& bias,
                Tensor out, bool relu) {
  OpScope scope(img_a);
  TORCH_CHECK(img_a.dim() == 4 && img_a.size(0) >= 1 && img_a.size(1) == 3, "conv_stem2: img_a [B,3,H,W]");
  const int B = img_a.size(0), H = img_a.size(2), W = img_a.size(3);
  // one image's three planes are a dense tensor; the batch stride goes to the kernel
  auto planes = [&](const Tensor& t, const char* what, long long* batch_stride) {
    TORCH_CHECK(t.dim() == 4 && t.size(0) == B && t.size(1) == 3 && t.size(2) == H && t.size(3) == W, "conv_stem2: ", what, " [B,3,H,W]");
    TORCH_CHECK(t.stride(3) == 1 && t.stride(2) == W && t.stride(1) == (int64_t)H * W && (B == 1 || t.stride(0) >= (int64_t)3 * H * W),
                "conv_stem2: ", what, " needs dense channel planes");
    *batch_stride = B == 1 ? (long long)3 * H * W : (long long)t.stride(0);
    return dense("conv_stem2", t.select(0, 0), what, F32, (int64_t)3 * H * W).f32();
  };
  long long sa = 0, sb = 0;
  const float* pa = planes(img_a, "img_a", &sa);
  const float* pb = img_b.has_value() ? planes(*img_b, "img_b", &sb) : nullptr;
  const int cin = pb ? 6 : 3;
  const Rows o = rows("conv_stem2", out, "out", Any).expect(out_rows(B, H, W, 2), AtLeast{0});
  const int cout = o.cols;
  const float* wp = dense("conv_stem2", weight, "weight [49,cin,cout]", F32, (int64_t)49 * cin * cout).f32();
  const float* b = dense("conv_stem2", bias, "bias", F32, cout).f32();
  if (o.b16) {
    check_ok(pfk_conv_stem2_b16(pa, sa, pb, sb, wp, b, o.raw(), o.ld, B, H, W, cin, cout, relu, cur_stream()), "conv_stem2 (bf16 out)");
    return;
  }
  check_ok(pfk_conv_stem2_f32(pa, sa, pb, sb, wp, b, o.f32(), o.ld, B, H, W, cin, cout, relu, cur_stream()), "conv_stem2");
}

// weight / bias gradient in PyTorch's layouts: dw [cout, sum(reals), kh, kw], db [cout] (optional); dy [B*Ho*Wo, cout4].
// K12b (conv_wgrad_unpacked_b16): the same on bf16 sources and a bf16 dy (pfk_conv_wgrad_unpacked_b16), stride 1; dw / db stay fp32
template <class Desc>
void conv_wgrad_unpacked_impl(const char* op, at::TensorList srcs, const Tensor& dy, int64_t B, int64_t H, int64_t W, int64_t kh,
                              int64_t kw, const Tensor& dw, const c10::optional<Tensor>& db, at::IntArrayRef reals, int64_t stride,
                              bool accumulate) {
  OpScope scope(dy);
  constexpr bool b16 = std::is_same<Desc, pfk_conv_b16_desc>::value;
  const Elem e = b16 ? B16 : F32;
  TORCH_CHECK(stride >= 1, op, ": stride");
  Desc d{};
  fill_sources(d, srcs, B * H * W, e, op);
  TORCH_CHECK(reals.size() == srcs.size(), op, ": one real count per source");
  int real[3] = {0, 0, 0};
  int64_t cin = 0;
  for (size_t i = 0; i < srcs.size(); ++i) { real[i] = (int)reals[i]; cin += reals[i]; }
  const Rows g = rows(op, dy, "dy", e).expect(out_rows(B, H, W, stride), AtLeast{0});
  d.B = B; d.H = H; d.W = W; d.kh = kh; d.kw = kw; d.cout = g.cols; d.stride = (int)stride;
  float* dwp = dense(op, dw, "dw", F32).f32();
  TORCH_CHECK(dw.dim() == 4 && dw.size(0) <= d.cout && dw.size(1) == cin && dw.size(2) == kh && dw.size(3) == kw,
              op, ": dw [cout, sum(reals), kh, kw] contiguous");
  float* dbp = dense(op, db, "db [cout]", F32, dw.size(0)).f32();
  if constexpr (b16) {
    for (int i = 0; i < d.num_src; ++i)
      TORCH_CHECK(d.src[i].channels % 8 == 0 && d.src[i].ld % 8 == 0, op, ": src channels and row stride must be multiples of 8");
    TORCH_CHECK(g.cols % 8 == 0 && g.ld % 8 == 0, op, ": dy channels and row stride must be multiples of 8");
    const long long need = pfk_conv_wgrad_unpacked_b16_workspace_bytes(&d, dbp != nullptr);
    TORCH_CHECK(need > 0, op, ": unsupported shape (stride 1; 1x1, 3x3, 1x5, 5x1)");
    const auto ws = byte_workspace(need, dy);
    check_ok(pfk_conv_wgrad_unpacked_b16(&d, real, g.raw(), g.ld, (int)dw.size(0), dwp, dbp, accumulate ? 1 : 0, ws.second, need, cur_stream()), op);
  } else {
    const long long need = pfk_conv_wgrad_unpacked_workspace_bytes(&d, dbp != nullptr);
    const auto ws = byte_workspace(need, dy);
    check_ok(pfk_conv_wgrad_unpacked_f32(&d, real, g.f32(), g.ld, (int)dw.size(0), dwp, dbp, accumulate ? 1 : 0, ws.second, need, cur_stream()), op);
  }
}
void conv_wgrad_unpacked(at::TensorList srcs, const Tensor& dy, int64_t B, int64_t H, int64_t W, int64_t kh, int64_t kw, Tensor dw,
                         const c10::optional<Tensor>& db, at::IntArrayRef reals, int64_t stride, bool accumulate) {
  conv_wgrad_unpacked_impl<pfk_conv_desc>("conv_wgrad_unpacked", srcs, dy, B, H, W, kh, kw, dw, db, reals, stride, accumulate);
}
void conv_wgrad_unpacked_b16(at::TensorList srcs, const Tensor& dy, int64_t B, int64_t H, int64_t W, int64_t kh, int64_t kw, Tensor dw,
                             const c10::optional<Tensor>& db, at::IntArrayRef reals, bool accumulate) {
  conv_wgrad_unpacked_impl<pfk_conv_b16_desc>("conv_wgrad_unpacked_b16", srcs, dy, B, H, W, kh, kw, dw, db, reals, 1, accumulate);
}

int64_t instnorm_workspace_bytes(int64_t B, int64_t C) { return pfk_instnorm_workspace_bytes((int)B, (int)C); }

void instnorm_stats(const Tensor& x, int64_t B, int64_t HW, double eps, Tensor mean, Tensor rstd, Tensor workspace) {
  OpScope scope(x);
  const Rows a = rows("instnorm_stats", x, "x", Any).expect(B * HW, AtLeast{0});
  const int C = a.cols;
  float* mp = dense("instnorm_stats", mean, "mean [B*C]", F32, B * C).f32();
  float* rp = dense("instnorm_stats", rstd, "rstd [B*C]", F32, B * C).f32();
  void* ws = dense("instnorm_stats", workspace, "workspace", Raw).raw();
  const long long ws_bytes = workspace.nbytes();
  if (a.b16) {
    check_ok(pfk_instnorm_stats_b16(a.raw(), a.ld, (int)B, (int)HW, C, (float)eps, mp, rp, ws, ws_bytes, cur_stream()), "instnorm_stats (bf16 rows)");
    return;
  }
  check_ok(pfk_instnorm_stats_f32(a.f32(), a.ld, (int)B, (int)HW, C, (float)eps, mp, rp, ws, ws_bytes, cur_stream()), "instnorm_stats");
}

void norm_apply(const Tensor& x, const Tensor& mean, const Tensor& rstd, const c10::optional<Tensor>& residual, Tensor out,
                int64_t B, int64_t HW, bool relu, bool relu_after_residual) {
  OpScope scope(x);
  const Rows a = rows("norm_apply", x, "x", Any).expect(B * HW, AtLeast{0});
  const int C = a.cols;
  // the K8b encoders: bf16 rows in need a bf16 output; a bf16 output takes bf16 residual rows (if any)
  const Rows o = rows("norm_apply", out, "out", a.b16 ? B16 : Any).expect(B * HW, C);
  const float* mp = dense("norm_apply", mean, "mean [B*C]", F32, B * C).f32();
  const float* rp = dense("norm_apply", rstd, "rstd [B*C]", F32, B * C).f32();
  Rows r;
  if (residual.has_value()) r = rows("norm_apply", *residual, "residual", o.b16 ? B16 : F32).expect(B * HW, C);
  if (o.b16) {
    check_ok(pfk_norm_apply_b16(a.raw(), a.b16 ? 1 : 0, a.ld, mp, rp, r.raw(), r.ld, o.raw(), o.ld, (int)B, (int)HW, C, relu, relu_after_residual,
                                cur_stream()), "norm_apply (bf16 out)");
    return;
  }
  check_ok(pfk_norm_apply_f32(a.f32(), a.ld, mp, rp, r.f32(), r.ld, o.f32(), o.ld, (int)B, (int)HW, C, relu, relu_after_residual, cur_stream()),
           "norm_apply");
}

// norm_apply with a raw residual and its own statistics (pfk_norm_apply_res_f32), fp32 rows
void norm_apply_res(const Tensor& x, const Tensor& mean, const Tensor& rstd, const Tensor& residual, const Tensor& res_mean,
                    const Tensor& res_rstd, bool res_relu, Tensor out, int64_t B, int64_t HW, bool relu, bool relu_after_residual) {
  OpScope scope(x);
  const Rows a = rows("norm_apply_res", x, "x", F32).expect(B * HW, AtLeast{0});
  const int C = a.cols;
  const Rows o = rows("norm_apply_res", out, "out", F32).expect(B * HW, C);
  const Rows r = rows("norm_apply_res", residual, "residual", F32).expect(B * HW, C);
  const float* mp = dense("norm_apply_res", mean, "mean [B*C]", F32, B * C).f32();
  const float* rp = dense("norm_apply_res", rstd, "rstd [B*C]", F32, B * C).f32();
  const float* rmp = dense("norm_apply_res", res_mean, "res_mean [B*C]", F32, B * C).f32();
  const float* rrp = dense("norm_apply_res", res_rstd, "res_rstd [B*C]", F32, B * C).f32();
  check_ok(pfk_norm_apply_res_f32(a.f32(), a.ld, mp, rp, r.f32(), r.ld, rmp, rrp, res_relu, o.f32(), o.ld, (int)B, (int)HW, C, relu,
                                  relu_after_residual, cur_stream()), "norm_apply_res");
}

int64_t norm_bwd_workspace_bytes(int64_t B, int64_t C) { return pfk_norm_bwd_workspace_bytes((int)B, (int)C); }

// backward of relu?((x - mean) * rstd): dx, and the two per-(image, channel) sums (d beta / d gamma of an affine batch norm)
void norm_bwd(const Tensor& x, const Tensor& dy, const Tensor& mean, const Tensor& rstd, Tensor dx, Tensor sum_g, Tensor sum_gxhat,
              int64_t B, int64_t HW, bool relu) {
  OpScope scope(x);
  const char* op = "norm_bwd";
  const Rows a = rows(op, x, "x", F32).expect(B * HW, AtLeast{0});
  const int C = a.cols;
  const Rows g = rows(op, dy, "dy", F32).expect(B * HW, C), d = rows(op, dx, "dx", F32).expect(B * HW, C);
  const float* mp = dense(op, mean, "mean [B*C]", F32, B * C).f32();
  const float* rp = dense(op, rstd, "rstd [B*C]", F32, B * C).f32();
  float* s1 = dense(op, sum_g, "sum_g [B*C]", F32, B * C).f32();
  float* s2 = dense(op, sum_gxhat, "sum_gxhat [B*C]", F32, B * C).f32();
  const long long need = pfk_norm_bwd_workspace_bytes((int)B, C);
  const auto ws = byte_workspace(need, x);
  check_ok(pfk_norm_bwd_f32(a.f32(), a.ld, g.f32(), g.ld, mp, rp, d.f32(), d.ld, s1, s2, (int)B, (int)HW, C, relu, ws.second, need, cur_stream()), op);
}

// stem weight / bias gradient: img [B,3,H,W], dy pixel-major [B*Ho*Wo, cout] -> dw [49,3,cout], db [cout]
void conv_stem_wgrad(const Tensor& img, const Tensor& dy, Tensor dw, Tensor db) {
  OpScope scope(img);
  const char* op = "conv_stem_wgrad";
  const float* ip = dense(op, img, "img", F32).f32();
  TORCH_CHECK(img.dim() == 4 && img.size(1) == 3, "conv_stem_wgrad: img [B,3,H,W] contiguous");
  const int B = img.size(0), H = img.size(2), W = img.size(3);
  const Rows g = rows(op, dy, "dy", F32).expect(out_rows(B, H, W, 2), AtLeast{0});
  const int cout = g.cols;
  float* dwp = dense(op, dw, "dw [49,3,cout]", F32, 49 * 3 * cout).f32();
  float* dbp = dense(op, db, "db [cout]", F32, cout).f32();
  const long long need = pfk_conv_stem_wgrad_workspace_bytes();
  const auto ws = byte_workspace(need, img);
  check_ok(pfk_conv_stem_wgrad_f32(ip, g.f32(), g.ld, dwp, dbp, B, H, W, cout, ws.second, need, cur_stream()), op);
}

void softmax_rows(Tensor x) {
  OpScope scope(x);
  float* p = dense("softmax_rows", x, "x", F32).f32();
  TORCH_CHECK(x.dim() >= 2, "softmax_rows: contiguous [..., rows, cols]");
  const int64_t cols = x.size(-1), n_rows = x.numel() / cols;
  check_ok(pfk_softmax_rows_f32(p, n_rows, (int)cols, cols, cur_stream()), "softmax_rows");
}

// backward of softmax_rows: p, dp [rows, cols] views with contiguous columns (dp float32 or bfloat16), ds [rows, ld_out] contiguous
// float32 (columns >= cols come out zero); ds may be the buffer dp is a view of (float32, same row stride)
void softmax_rows_bwd(const Tensor& p, const Tensor& dp, Tensor ds) {
  OpScope scope(p);
  const char* op = "softmax_rows_bwd";
  const Rows a = rows(op, p, "p", F32);
  TORCH_CHECK(a.rows > 0 && a.cols > 0, "softmax_rows_bwd: p must not be empty");
  const Rows g = rows(op, dp, "dp", Any).expect(a.rows, a.cols), s = rows(op, ds, "ds", F32).expect(a.rows, AtLeast{a.cols});
  TORCH_CHECK(ds.is_contiguous(), "softmax_rows_bwd: ds must be contiguous [rows, ld_out]");
  if (g.b16) check_ok(pfk_softmax_rows_bwd_bf16(a.f32(), a.ld, g.raw(), g.ld, s.f32(), s.cols, a.rows, (int)a.cols, cur_stream()),
                      "softmax_rows_bwd (bf16)");
  else check_ok(pfk_softmax_rows_bwd_f32(a.f32(), a.ld, g.f32(), g.ld, s.f32(), s.cols, a.rows, (int)a.cols, cur_stream()), op);
}

// inp [B, N, N] float32 (row stride inp.stride(1), batches N rows apart) -> outT [B, N, ld_out] = its transpose, out (optional, same
// shape) = its copy; float32 or bfloat16, contiguous, pad columns zero
void transpose_pack(const Tensor& inp, Tensor outT, const c10::optional<Tensor>& out) {
  OpScope scope(inp);
  const char* op = "transpose_pack";
  TORCH_CHECK(inp.dim() == 3 && inp.size(1) == inp.size(2) && inp.stride(2) == 1 && inp.stride(0) == inp.size(1) * inp.stride(1),
              "transpose_pack: inp [B, N, N] with contiguous columns and batches N rows apart");
  const int64_t B = inp.size(0), N = inp.size(1);
  const Rows i = rows(op, inp.view({B * N, N}), "inp", F32).expect(B * N, N);      // the B*N rows
  const Ptr t = dense(op, outT, "outT", Any);
  TORCH_CHECK(outT.dim() == 3 && outT.size(0) == B && outT.size(1) == N && outT.size(2) >= N, "transpose_pack: outT [B, N, ld_out >= N] contiguous");
  const Ptr o = dense(op, out, "out", t.b16 ? B16 : F32, outT.numel());
  TORCH_CHECK(!out.has_value() || out->sizes() == outT.sizes(), "transpose_pack: out must match outT");
  if (t.b16) check_ok(pfk_transpose_pack_b16(i.f32(), i.ld, t.raw(), o.raw(), outT.size(2), (int)B, (int)N, cur_stream()), "transpose_pack (bf16)");
  else check_ok(pfk_transpose_pack_f32(i.f32(), i.ld, t.f32(), o.f32(), outT.size(2), (int)B, (int)N, cur_stream()), op);
}

void forward_interpolate(const Tensor& flow, Tensor out) {
  OpScope scope(flow);
  const float* fp = dense("forward_interpolate", flow, "flow", F32).f32();
  float* dst = dense("forward_interpolate", out, "out", F32, flow.numel()).f32();
  TORCH_CHECK(flow.dim() == 4 && flow.size(1) == 2 && out.sizes() == flow.sizes(), "forward_interpolate: flow/out [B,2,H,W] contiguous");
  check_ok(pfk_forward_interpolate_f32(fp, dst, flow.size(0), flow.size(2), flow.size(3), cur_stream()), "forward_interpolate");
}

// weight gradient in the packed [cout, ktot] layout; dy [M, cout] (cout % 4 == 0)
void conv_wgrad(at::TensorList srcs, const Tensor& dy, int64_t B, int64_t H, int64_t W, int64_t kh, int64_t kw, Tensor out,
                bool with_bias, int64_t stride) {
  OpScope scope(dy);
  TORCH_CHECK(stride >= 1, "conv_wgrad: stride");
  pfk_conv_desc d{};
  fill_sources(d, srcs, B * H * W, F32, "conv_wgrad");
  const Rows g = rows("conv_wgrad", dy, "dy", F32).expect(out_rows(B, H, W, stride), AtLeast{0});
  d.B = B; d.H = H; d.W = W; d.kh = kh; d.kw = kw; d.cout = g.cols; d.stride = (int)stride;
  float* dst = dense("conv_wgrad", out, "out", F32).f32();
  TORCH_CHECK(out.dim() == 2 && out.size(0) == d.cout && out.size(1) == pfk_conv_ktot(&d) + (with_bias ? 32 : 0),
              "conv_wgrad: out [cout, ktot (+32 with the bias column)]");
  const long long need = pfk_conv_wgrad_workspace_bytes(&d, with_bias);
  const auto ws = byte_workspace(need, dy);
  check_ok(pfk_conv_wgrad_f32(&d, g.f32(), g.ld, dst, with_bias, ws.second, need, cur_stream()), "conv_wgrad");
}

// The GRU gate kernels (include/pfk.h): h / dh_new are [M, C] row views; every other tensor is dense fp32 with M*C elements
// (a_zr / da_zr: [M, 2C]), possibly the head of a longer buffer
void gru_gates_zr(const Tensor& a_zr, const Tensor& h, Tensor z, Tensor r, Tensor rh) {
  OpScope scope(h);
  const char* op = "gru_gates_zr";
  const Rows hv = rows(op, h, "h", F32);
  const int64_t M = hv.rows, C = hv.cols;
  const float* a = dense(op, a_zr, "a_zr", F32, AtLeast{M * 2 * C}).f32();
  TORCH_CHECK(a_zr.dim() == 2 && a_zr.size(0) == M && a_zr.size(1) == 2 * C, "gru_gates_zr: a_zr must be [M, 2C] for h [M, C]");
  check_ok(pfk_gru_gates_zr_f32(a, hv.f32(), hv.ld, dense(op, z, "z", F32, AtLeast{M * C}).f32(), dense(op, r, "r", F32, AtLeast{M * C}).f32(),
                                dense(op, rh, "rh", F32, AtLeast{M * C}).f32(), M, (int)C, cur_stream()), op);
}
void gru_gates_q(const Tensor& a_q, const Tensor& z, const Tensor& h, Tensor q, Tensor h_new) {
  OpScope scope(h);
  const char* op = "gru_gates_q";
  const Rows hv = rows(op, h, "h", F32);
  const int64_t M = hv.rows, C = hv.cols;
  const float* a = dense(op, a_q, "a_q", F32, AtLeast{M * C}).f32();
  TORCH_CHECK(a_q.dim() == 2 && a_q.size(0) == M && a_q.size(1) == C, "gru_gates_q: a_q must be [M, C] like h");
  check_ok(pfk_gru_gates_q_f32(a, dense(op, z, "z", F32, AtLeast{M * C}).f32(), hv.f32(), hv.ld, dense(op, q, "q", F32, AtLeast{M * C}).f32(),
                               dense(op, h_new, "h_new", F32, AtLeast{M * C}).f32(), M, (int)C, cur_stream()), op);
}
void gru_backward_q(const Tensor& dh_new, const Tensor& z, const Tensor& q, const Tensor& h, Tensor da_q, Tensor da_zr, Tensor dh) {
  OpScope scope(h);
  const char* op = "gru_backward_q";
  const Rows hv = rows(op, h, "h", F32);
  const int64_t M = hv.rows, C = hv.cols;
  const Rows g = rows(op, dh_new, "dh_new", F32).expect(M, C);
  float* dzr = dense(op, da_zr, "da_zr", F32, AtLeast{M * 2 * C}).f32();
  TORCH_CHECK(da_zr.dim() == 2 && da_zr.size(1) == 2 * C, "gru_backward_q: da_zr must be [M, 2C] for h [M, C]");
  check_ok(pfk_gru_backward_q_f32(g.f32(), g.ld, dense(op, z, "z", F32, AtLeast{M * C}).f32(), dense(op, q, "q", F32, AtLeast{M * C}).f32(),
                                  hv.f32(), hv.ld, dense(op, da_q, "da_q", F32, AtLeast{M * C}).f32(), dzr,
                                  dense(op, dh, "dh", F32, AtLeast{M * C}).f32(), M, (int)C, cur_stream()), op);
}
void gru_backward_zr(const Tensor& d_rh, const Tensor& h, const Tensor& r, Tensor da_zr, Tensor dh) {
  OpScope scope(h);
  const char* op = "gru_backward_zr";
  const Rows hv = rows(op, h, "h", F32);
  const int64_t M = hv.rows, C = hv.cols;
  float* dzr = dense(op, da_zr, "da_zr", F32, AtLeast{M * 2 * C}).f32();
  TORCH_CHECK(da_zr.dim() == 2 && da_zr.size(1) == 2 * C, "gru_backward_zr: da_zr must be [M, 2C] for h [M, C]");
  check_ok(pfk_gru_backward_zr_f32(dense(op, d_rh, "d_rh", F32, AtLeast{M * C}).f32(), hv.f32(), hv.ld, dense(op, r, "r", F32, AtLeast{M * C}).f32(),
                                   dzr, dense(op, dh, "dh", F32, AtLeast{M * C}).f32(), M, (int)C, cur_stream()), op);
}

// ---- K14: CCMR's XCiT motion aggregator (pfk_xcit.hip).  fp32 row views [M, C] of wider buffers; only C columns are touched.
void layernorm_rows(const Tensor& in, const c10::optional<Tensor>& weight, const c10::optional<Tensor>& bias, double eps, Tensor out) {
  OpScope scope(in);
  const Rows i = rows("layernorm_rows", in, "inp", F32);
  const Rows o = rows("layernorm_rows", out, "out", F32).expect(i.rows, i.cols);
  const float* w = dense("layernorm_rows", weight, "weight", F32, i.cols).f32();
  const float* b = dense("layernorm_rows", bias, "bias", F32, i.cols).f32();
  check_ok(pfk_layernorm_rows_f32(i.f32(), i.ld, w, b, (float)eps, o.f32(), o.ld, i.rows, (int)i.cols, cur_stream()), "layernorm_rows");
}

// qk [B*N, 2 * heads * dh] view (q | k), temperature [heads] (any shape with that many elements), A [B, heads, dh, dh] contiguous
void xca_map(const Tensor& qk, const Tensor& temperature, Tensor A, int64_t B, int64_t N) {
  OpScope scope(qk);
  TORCH_CHECK(A.dim() == 4 && A.size(0) == B && A.size(2) == A.size(3), "xca_map: A must be [B, heads, dh, dh]");
  const int64_t heads = A.size(1), dh = A.size(2);
  const Rows q = rows("xca_map", qk, "qk", F32).expect(B * N, 2 * heads * dh);
  const float* t = dense("xca_map", temperature, "temperature", F32, heads).f32();
  float* a = dense("xca_map", A, "A", F32, B * heads * dh * dh).f32();
  const long long need = pfk_xca_map_workspace_bytes((int)B, N, (int)heads, (int)dh);
  check_ok(need < 0 ? (int)need : PFK_OK, "xca_map");
  auto ws = byte_workspace(need, qk);
  check_ok(pfk_xca_map_f32(q.f32(), q.ld, t, a, ws.second, need, (int)B, N, (int)heads, (int)dh, cur_stream()), "xca_map");
}

int64_t xcit_lpi_workspace_bytes(int64_t B, int64_t H, int64_t W) { return pfk_xcit_lpi_workspace_bytes((int)B, (int)H, (int)W); }

// x [B*H*W, C] view -> u [B*H*W, C] view; dw_weight [C, 1, 3, 3] or [C, 9] contiguous; workspace: xcit_lpi_workspace_bytes(B, H, W) bytes
void xcit_lpi1(const Tensor& x, const Tensor& ln_weight, const Tensor& ln_bias, double ln_eps, const Tensor& dw_weight,
               const Tensor& dw_bias, Tensor u, Tensor workspace, int64_t B, int64_t H, int64_t W) {
  OpScope scope(x);
  const Rows i = rows("xcit_lpi1", x, "x", F32).expect(B * H * W, AtLeast{0});
  const int64_t C = i.cols;
  const Rows o = rows("xcit_lpi1", u, "u", F32).expect(B * H * W, C);
  const float* lw = dense("xcit_lpi1", ln_weight, "ln_weight", F32, C).f32();
  const float* lb = dense("xcit_lpi1", ln_bias, "ln_bias", F32, C).f32();
  const float* dw = dense("xcit_lpi1", dw_weight, "dw_weight [C, 9]", F32, C * 9).f32();
  const float* db = dense("xcit_lpi1", dw_bias, "dw_bias", F32, C).f32();
  void* ws = dense("xcit_lpi1", workspace, "workspace", Raw).raw();
  check_ok(pfk_xcit_lpi1_f32(i.f32(), i.ld, lw, lb, (float)ln_eps, dw, db, o.f32(), o.ld, ws, (long long)workspace.nbytes(), (int)B, (int)H,
                             (int)W, (int)C, cur_stream()),
           "xcit_lpi1");
}

// u, x [B*H*W, C] views -> x2, t [B*H*W, C] views; the workspace xcit_lpi1 filled for this u
void xcit_lpi2(const Tensor& u, const Tensor& gn_weight, const Tensor& gn_bias, double gn_eps, int64_t groups, const Tensor& dw_weight,
               const Tensor& dw_bias, const Tensor& gamma, const Tensor& x, Tensor x2, const c10::optional<Tensor>& ln_weight,
               const c10::optional<Tensor>& ln_bias, double ln_eps, Tensor t, Tensor workspace, int64_t B, int64_t H, int64_t W) {
  OpScope scope(u);
  const Rows ui = rows("xcit_lpi2", u, "u", F32).expect(B * H * W, AtLeast{0});
  const int64_t C = ui.cols;
  const Rows xi = rows("xcit_lpi2", x, "x", F32).expect(B * H * W, C);
  const Rows xo = rows("xcit_lpi2", x2, "x2", F32).expect(B * H * W, C);
  const Rows to = rows("xcit_lpi2", t, "t", F32).expect(B * H * W, C);
  const float* gw = dense("xcit_lpi2", gn_weight, "gn_weight", F32, C).f32();
  const float* gb = dense("xcit_lpi2", gn_bias, "gn_bias", F32, C).f32();
  const float* dw = dense("xcit_lpi2", dw_weight, "dw_weight [C, 9]", F32, C * 9).f32();
  const float* db = dense("xcit_lpi2", dw_bias, "dw_bias", F32, C).f32();
  const float* gm = dense("xcit_lpi2", gamma, "gamma", F32, C).f32();
  const float* lw = dense("xcit_lpi2", ln_weight, "ln_weight", F32, C).f32();
  const float* lb = dense("xcit_lpi2", ln_bias, "ln_bias", F32, C).f32();
  void* ws = dense("xcit_lpi2", workspace, "workspace", Raw).raw();
  check_ok(pfk_xcit_lpi2_f32(ui.f32(), ui.ld, gw, gb, (float)gn_eps, (int)groups, dw, db, gm, xi.f32(), xi.ld, xo.f32(), xo.ld, lw, lb,
                             (float)ln_eps, to.f32(), to.ld, ws, (long long)workspace.nbytes(), (int)B, (int)H, (int)W, (int)C, cur_stream()),
           "xcit_lpi2");
}

// ---- K17: CCMR's per-scale context grouping (pfk_xcit.hip) ----
// inp [B, 128, H, W] contiguous, pos [H*W, 128] contiguous or None -> x0, xh [B*H*W, 128] views
void xcit_tokens(const Tensor& in, const c10::optional<Tensor>& pos, double eps, Tensor x0, Tensor xh) {
  OpScope scope(in);
  const float* ip = dense("xcit_tokens", in, "inp", F32).f32();
  TORCH_CHECK(in.dim() == 4, "xcit_tokens: inp must be [B,C,H,W] contiguous");
  const int64_t B = in.size(0), C = in.size(1), H = in.size(2), W = in.size(3);
  const Rows a = rows("xcit_tokens", x0, "x0", F32).expect(B * H * W, C);
  const Rows h = rows("xcit_tokens", xh, "xh", F32).expect(B * H * W, C);
  const float* pp = dense("xcit_tokens", pos, "pos [H*W, C]", F32, H * W * C).f32();
  check_ok(pfk_xcit_tokens_f32(ip, pp, (float)eps, a.f32(), a.ld, h.f32(), h.ld, (int)B, (int)C, (int)H, (int)W, cur_stream()), "xcit_tokens");
}

// the same from the pixel-major rows inp [B*H*W, 128] (a view) of a channels-last tensor
void xcit_tokens_pm(const Tensor& in, const c10::optional<Tensor>& pos, double eps, Tensor x0, Tensor xh, int64_t B, int64_t H, int64_t W) {
  OpScope scope(in);
  const Rows i = rows("xcit_tokens_pm", in, "inp", F32).expect(B * H * W, AtLeast{0});
  const int64_t C = i.cols;
  const Rows a = rows("xcit_tokens_pm", x0, "x0", F32).expect(B * H * W, C);
  const Rows h = rows("xcit_tokens_pm", xh, "xh", F32).expect(B * H * W, C);
  const float* pp = dense("xcit_tokens_pm", pos, "pos [H*W, C]", F32, H * W * C).f32();
  check_ok(pfk_xcit_tokens_pm_f32(i.f32(), i.ld, pp, (float)eps, a.f32(), a.ld, h.f32(), h.ld, (int)B, (int)C, (int)H, (int)W, cur_stream()),
           "xcit_tokens_pm");
}

// A [B, heads, dh, dh], wv / wp [C, C], bv / bp [C] -> M [B, C, C], c [B, C], all contiguous
void xca_fold(const Tensor& A, const Tensor& wv, const Tensor& bv, const Tensor& wp, const Tensor& bp, Tensor M, Tensor c) {
  OpScope scope(A);
  TORCH_CHECK(A.dim() == 4 && A.size(2) == A.size(3), "xca_fold: A must be [B, heads, dh, dh]");
  const int64_t B = A.size(0), heads = A.size(1), dh = A.size(2), C = heads * dh;
  const float* ap = dense("xca_fold", A, "A", F32, B * heads * dh * dh).f32();
  const float* wvp = dense("xca_fold", wv, "wv [C, C]", F32, C * C).f32();
  const float* bvp = dense("xca_fold", bv, "bv", F32, C).f32();
  const float* wpp = dense("xca_fold", wp, "wp [C, C]", F32, C * C).f32();
  const float* bpp = dense("xca_fold", bp, "bp", F32, C).f32();
  float* mp = dense("xca_fold", M, "M [B, C, C]", F32, B * C * C).f32();
  float* cp = dense("xca_fold", c, "c [B, C]", F32, B * C).f32();
  check_ok(pfk_xca_fold_f32(ap, wvp, bvp, wpp, bpp, mp, cp, (int)B, (int)heads, (int)dh, cur_stream()), "xca_fold");
}

// ---- K15: the multi-scale GroupNorm encoders (pfk_msenc.hip) ----
int64_t groupnorm_workspace_bytes(int64_t B, int64_t HW, int64_t C) { return pfk_groupnorm_workspace_bytes((int)B, (int)HW, (int)C); }

// x [B*HW, C] view, gamma / beta [C] -> scale, shift [B*C]; workspace: groupnorm_workspace_bytes(B, HW, C) bytes
void groupnorm_stats(const Tensor& x, int64_t B, int64_t HW, int64_t group_size, const Tensor& gamma, const Tensor& beta, double eps,
                     Tensor scale, Tensor shift, Tensor workspace) {
  OpScope scope(x);
  const Rows a = rows("groupnorm_stats", x, "x", F32).expect(B * HW, AtLeast{0});
  const int64_t C = a.cols;
  const float* gp = dense("groupnorm_stats", gamma, "gamma [C]", F32, C).f32();
  const float* bp = dense("groupnorm_stats", beta, "beta [C]", F32, C).f32();
  float* sc = dense("groupnorm_stats", scale, "scale [B*C]", F32, B * C).f32();
  float* sh = dense("groupnorm_stats", shift, "shift [B*C]", F32, B * C).f32();
  void* ws = dense("groupnorm_stats", workspace, "workspace", Raw).raw();
  check_ok(pfk_groupnorm_stats_f32(a.f32(), a.ld, (int)B, (int)HW, (int)C, (int)group_size, gp, bp, (float)eps, sc, sh, ws,
                                   (long long)workspace.nbytes(), cur_stream()), "groupnorm_stats");
}

void affine_apply(const Tensor& x, const Tensor& scale, const Tensor& shift, const c10::optional<Tensor>& residual, Tensor out, int64_t B,
                  int64_t HW, bool relu, bool relu_after_residual) {
  OpScope scope(x);
  const Rows a = rows("affine_apply", x, "x", F32).expect(B * HW, AtLeast{0});
  const int64_t C = a.cols;
  const Rows o = rows("affine_apply", out, "out", F32).expect(B * HW, C);
  const float* sc = dense("affine_apply", scale, "scale [B*C]", F32, B * C).f32();
  const float* sh = dense("affine_apply", shift, "shift [B*C]", F32, B * C).f32();
  Rows r;
  if (residual.has_value()) r = rows("affine_apply", *residual, "residual", F32).expect(B * HW, C);
  check_ok(pfk_affine_apply_f32(a.f32(), a.ld, sc, sh, r.f32(), r.ld, o.f32(), o.ld, (int)B, (int)HW, (int)C, relu, relu_after_residual,
                                cur_stream()), "affine_apply");
}

// inp [B*Hi*Wi, C] view -> out [B*Ho*Wo, C] view
void resize_bilinear_pm(const Tensor& in, Tensor out, int64_t B, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo) {
  OpScope scope(in);
  const Rows i = rows("resize_bilinear_pm", in, "inp", F32).expect(B * Hi * Wi, AtLeast{0});
  const Rows o = rows("resize_bilinear_pm", out, "out", F32).expect(B * Ho * Wo, i.cols);
  check_ok(pfk_resize_bilinear_pm_f32(i.f32(), i.ld, o.f32(), o.ld, (int)B, (int)Hi, (int)Wi, (int)Ho, (int)Wo, (int)i.cols, cur_stream()),
           "resize_bilinear_pm");
}

int64_t abi_version() { return pfk_abi_version(); }
int64_t conv_workspace_bytes() { return pfk_conv_workspace_bytes(); }
int64_t conv_workspace_fault_offset() { return pfk_conv_workspace_fault_offset(); }
// inert (RuntimeError) unless the process opted in with PFK_DEBUG_KNOBS=1: process-global kernel selection (include/pfk.h)
void debug_set_tile(int64_t cfg) { check_ok(pfk_debug_set_tile((int)cfg), "debug_set_tile"); }
void debug_set_lookup_pix(int64_t pix) { check_ok(pfk_debug_set_lookup_pix((int)pix), "debug_set_lookup_pix"); }
void debug_set_wgrad(int64_t v) { check_ok(pfk_debug_set_wgrad((int)v), "debug_set_wgrad"); }
void debug_set_wgrad_b16(int64_t v) { check_ok(pfk_debug_set_wgrad_b16((int)v), "debug_set_wgrad_b16"); }
void debug_set_altcorr(int64_t v) { check_ok(pfk_debug_set_altcorr((int)v), "debug_set_altcorr"); }
#ifndef PFK_SOURCE_HASH
#define PFK_SOURCE_HASH "unstamped"
#endif
// the same stamp as a record that ptlflow_amd/_build.py finds in the FILE (embedded_hash): staleness is decided without loading it
__attribute__((used)) static const char pfk_ext_stamp_record[] = "PFK_EXT_SOURCE_HASH=" PFK_SOURCE_HASH;
std::string source_hash() { return std::string(pfk_ext_stamp_record + 20) + ":" + pfk_source_hash(); }   // "<this extension's stamp>:<libpfk.so's stamp>"

}  // namespace

TORCH_LIBRARY(pfk, m) {
  m.def("abi_version() -> int", &abi_version);
  m.def("source_hash() -> str", &source_hash);
  m.def("gru_gates_zr(Tensor a_zr, Tensor h, Tensor(a!) z, Tensor(b!) r, Tensor(c!) rh) -> ()");
  m.def("gru_gates_q(Tensor a_q, Tensor z, Tensor h, Tensor(a!) q, Tensor(b!) h_new) -> ()");
  m.def("gru_backward_q(Tensor dh_new, Tensor z, Tensor q, Tensor h, Tensor(a!) da_q, Tensor(b!) da_zr, Tensor(c!) dh) -> ()");
  m.def("gru_backward_zr(Tensor d_rh, Tensor h, Tensor r, Tensor(a!) da_zr, Tensor(b!) dh) -> ()");
  m.def("conv_wgrad(Tensor[] srcs, Tensor dy, int B, int H, int W, int kh, int kw, Tensor(a!) out, bool with_bias=False, int stride=1) -> ()");
  m.def("conv_wgrad_unpacked(Tensor[] srcs, Tensor dy, int B, int H, int W, int kh, int kw, Tensor(a!) dw, Tensor(b!)? db, int[] reals, int stride=1, bool accumulate=False) -> ()");
  m.def("conv_wgrad_unpacked_b16(Tensor[] srcs, Tensor dy, int B, int H, int W, int kh, int kw, Tensor(a!) dw, Tensor(b!)? db, int[] reals, bool accumulate=False) -> ()");
  m.def("forward_interpolate(Tensor flow, Tensor(a!) out) -> ()");
  m.def("softmax_rows(Tensor(a!) x) -> ()");
  m.def("softmax_rows_bwd(Tensor p, Tensor dp, Tensor(a!) ds) -> ()");
  m.def("transpose_pack(Tensor inp, Tensor(a!) outT, Tensor(b!)? out) -> ()");
  m.def("norm_bwd(Tensor x, Tensor dy, Tensor mean, Tensor rstd, Tensor(a!) dx, Tensor(b!) sum_g, Tensor(c!) sum_gxhat, int B, int HW, bool relu) -> ()");
  m.def("conv_stem_wgrad(Tensor img, Tensor dy, Tensor(a!) dw, Tensor(b!) db) -> ()");
  m.def("instnorm_workspace_bytes(int B, int C) -> int", &instnorm_workspace_bytes);
  m.def("conv_stem(Tensor img, Tensor weight, Tensor? bias, Tensor(a!) out, bool relu) -> ()");
  m.def("conv_stem2(Tensor img_a, Tensor? img_b, Tensor weight, Tensor? bias, Tensor(a!) out, bool relu) -> ()");
  m.def("instnorm_stats(Tensor x, int B, int HW, float eps, Tensor(a!) mean, Tensor(b!) rstd, Tensor(c!) workspace) -> ()");
  m.def("norm_apply(Tensor x, Tensor mean, Tensor rstd, Tensor? residual, Tensor(a!) out, int B, int HW, bool relu, "
        "bool relu_after_residual) -> ()");
  m.def("norm_apply_res(Tensor x, Tensor mean, Tensor rstd, Tensor residual, Tensor res_mean, Tensor res_rstd, bool res_relu, "
        "Tensor(a!) out, int B, int HW, bool relu, bool relu_after_residual) -> ()");
  m.def("debug_set_tile(int cfg) -> ()", &debug_set_tile);
  m.def("debug_set_lookup_pix(int pix) -> ()", &debug_set_lookup_pix);
  m.def("debug_set_wgrad(int variant) -> ()", &debug_set_wgrad);
  m.def("debug_set_wgrad_b16(int splits) -> ()", &debug_set_wgrad_b16);
  m.def("debug_set_altcorr(int mode) -> ()", &debug_set_altcorr);
  m.def("corr_volume(Tensor f1, Tensor f2, float scale, Tensor(a!) out) -> ()");
  m.def("corr_pool2x2(Tensor inp, Tensor(a!) out) -> ()");
  m.def("corr_volume_bf16(Tensor f1, Tensor f2, float scale, Tensor(a!) out) -> ()");
  m.def("fmap_pool2x2(Tensor inp, Tensor(a!) out, int B, int H, int W) -> ()");
  m.def("corr_lookup(Tensor[] levels, Tensor coords, int radius, Tensor(a!) out) -> ()");
  m.def("fmap_to_blocked(Tensor inp, Tensor(a!) out, int B, int H, int W) -> ()");
  m.def("corr_pool2x2_blocked(Tensor inp, Tensor(a!) out, int H, int W) -> ()");
  m.def("corr_lookup_blocked(Tensor[] levels, int[] lvl_h, int[] lvl_w, Tensor coords, int radius, Tensor(a!) out) -> ()");
  m.def("blocked_map_elems(int H, int W) -> int", &blocked_map_elems);
  m.def("conv2d(Tensor[] srcs, int B, int H, int W, int kh, int kw, Tensor weight, Tensor? bias, int cout, "
        "int epilogue, bool relu, float scale, Tensor(a!)? out, Tensor(b!)? h, Tensor(c!)? aux_z, Tensor(d!)? aux_rh, "
        "Tensor(e!)? workspace=None, Tensor? residual=None, int stride=1, bool relu_after_residual=False, int cout_active=0, int cout_split=0) -> ()");
  m.def("conv2d_wino(Tensor src, int B, int H, int W, Tensor weight, Tensor? bias, int cout, bool relu, float scale, Tensor(a!) out, "
        "int cout_active=0) -> ()");
  m.def("conv2d_wino_norm(Tensor src, int B, int H, int W, Tensor weight, Tensor? bias, int cout, bool relu, float scale, Tensor(a!) out, "
        "Tensor in_mean, Tensor in_rstd, bool in_relu) -> ()");
  m.def("conv_wino_stats_workspace_bytes(int B, int H, int W, int cout) -> int", &conv_wino_stats_workspace_bytes);
  m.def("conv2d_wino_stats(Tensor src, int B, int H, int W, Tensor weight, Tensor? bias, int cout, Tensor(a!) out, Tensor? in_mean, "
        "Tensor? in_rstd, bool in_relu, float eps, Tensor(b!) out_mean, Tensor(c!) out_rstd, Tensor(d!) workspace) -> ()");
  m.def("conv2d_wino1d(Tensor[] srcs, int B, int H, int W, int kh, int kw, Tensor weight, Tensor? bias, int cout, int epilogue, "
        "bool relu, float scale, Tensor(a!)? out=None, Tensor(b!)? h=None, Tensor(c!)? aux_z=None, Tensor(d!)? aux_rh=None, "
        "Tensor? residual=None) -> ()");
  m.def("conv2d_wino_res(Tensor src, int B, int H, int W, Tensor weight, Tensor? bias, int cout, bool relu, float scale, Tensor(a!) out, "
        "Tensor residual, bool relu_after_residual) -> ()");
  m.def("conv2d_group(Tensor[] srcs, int B, int H, int W, int[] k, Tensor[] weights, Tensor[] biases, int[] relu, float[] scale, Tensor(a!)[] outs, Tensor[] residuals) -> ()");
  m.def("conv2d_b16(Tensor[] srcs, int B, int H, int W, int kh, int kw, Tensor weight, Tensor? bias, int cout, int epilogue, bool relu, "
        "float scale, Tensor(a!)? out, Tensor(b!)? h=None, Tensor(c!)? h_b16=None, Tensor(d!)? aux_z=None, Tensor(e!)? aux_rh=None, "
        "Tensor? residual=None, int stride=1, bool relu_after_residual=False) -> ()");
  m.def("debug_set_b16(int cfg) -> ()", &debug_set_b16);
  m.def("debug_set_stem_valu(int on) -> ()", &debug_set_stem_valu);
  m.def("debug_set_cin2_valu(int on) -> ()", &debug_set_cin2_valu);
  m.def("conv_workspace_bytes() -> int", &conv_workspace_bytes);
  m.def("conv_workspace_fault_offset() -> int", &conv_workspace_fault_offset);
  m.def("conv_cin2(Tensor inp, Tensor weight, Tensor? bias, Tensor(a!) out, int B, int H, int W, int k, bool relu) -> ()");
  m.def("flow_delta(Tensor inp, Tensor weight, Tensor? bias, Tensor coords0, Tensor(a!) coords1, Tensor(b!)? delta_out, "
        "Tensor(c!)? flow_out, Tensor(d!)? flow_out_b16=None) -> ()");
  m.def("flow_from_coords(Tensor coords0, Tensor coords1, Tensor(a!) flow_out) -> ()");
  m.def("convex_upsample(Tensor flow, Tensor mask, Tensor(a!) out) -> ()");
  m.def("convex_upsample_pm(Tensor flow_pm, Tensor mask, Tensor(a!) out) -> ()");
  m.def("convex_upsample2(Tensor flow, Tensor mask, Tensor(a!) out) -> ()");
  m.def("convex_upsample2_pm(Tensor flow_pm, Tensor mask, Tensor(a!) out) -> ()");
  m.def("convex_upsample_info_pm(Tensor flow_pm, Tensor info_pm, Tensor mask, Tensor(a!) flow_out, Tensor(b!) info_out) -> ()");
  m.def("dwconv_layernorm(Tensor inp, Tensor dw_weight, Tensor? dw_bias, Tensor ln_weight, Tensor ln_bias, float eps, Tensor(a!) out, "
        "int B, int H, int W, int k) -> ()");
  m.def("dwconv_layernorm_train(Tensor inp, Tensor dw_weight, Tensor? dw_bias, Tensor ln_weight, Tensor ln_bias, float eps, "
        "Tensor(a!) out, Tensor(b!) xhat, Tensor(c!) rstd, int B, int H, int W, int k) -> ()");
  m.def("dwconv_layernorm_train_b16(Tensor inp, Tensor dw_weight, Tensor? dw_bias, Tensor ln_weight, Tensor ln_bias, float eps, "
        "Tensor(a!) out, Tensor(b!) xhat, Tensor(c!) rstd, int B, int H, int W, int k) -> ()");
  m.def("layernorm_bwd(Tensor xhat, Tensor rstd, Tensor ln_weight, Tensor dy, Tensor(a!) du, Tensor(b!) dgamma, Tensor(c!) dbeta) -> ()");
  m.def("layernorm_bwd_b16(Tensor xhat, Tensor rstd, Tensor ln_weight, Tensor dy, Tensor(a!) du, Tensor(b!) dgamma, Tensor(c!) dbeta) -> ()");
  m.def("dwconv_bwd(Tensor inp, Tensor du, Tensor dw_weight, Tensor(a!) dx, Tensor(b!) dweight, Tensor(c!)? dbias, int B, int H, int W, "
        "int k) -> ()");
  m.def("dwconv_bwd_b16(Tensor inp, Tensor du, Tensor dw_weight, Tensor(a!) dx, Tensor(b!) dweight, Tensor(c!)? dbias, int B, int H, int W, "
        "int k) -> ()");
  m.def("gelu(Tensor x, Tensor(a!) y) -> ()");
  m.def("gelu_b16(Tensor x, Tensor(a!) y) -> ()");
  m.def("gelu_bwd(Tensor x, Tensor dy, Tensor(a!) dx) -> ()");
  m.def("gelu_bwd_b16(Tensor x, Tensor dy, Tensor(a!) dx) -> ()");
  m.def("dwconv_layernorm_b16(Tensor inp, Tensor dw_weight, Tensor? dw_bias, Tensor ln_weight, Tensor ln_bias, float eps, "
        "Tensor(a!) out, int B, int H, int W, int k) -> ()");
  m.def("conv2d_gelu_b16(Tensor[] srcs, int B, int H, int W, int kh, int kw, Tensor weight, Tensor? bias, int cout, float scale, "
        "Tensor(a!) out, Tensor? residual=None) -> ()");
  m.def("convex_upsample_info_pm_b16(Tensor flow_pm, Tensor info_pm, Tensor mask, Tensor(a!) flow_out, Tensor(b!) info_out) -> ()");
  m.def("mask_upsample(Tensor x, Tensor weight_perm, Tensor? bias_perm, float scale, Tensor flow_pm, Tensor(a!) out) -> ()");
  m.def("upflow8(Tensor coords0, Tensor coords1, Tensor(a!) out) -> ()");
  m.def("altcorr_forward(Tensor fmap1, Tensor fmap2, Tensor coords, int radius) -> Tensor");
  m.def("altcorr_backward(Tensor fmap1, Tensor fmap2, Tensor coords, Tensor corr_grad, int radius) -> Tensor[]");
  m.def("corr_lookup_bwd(Tensor(a!)[] grad_levels, int[] lvl_h, int[] lvl_w, Tensor coords, int radius, Tensor grad_out) -> ()");
  m.def("corr_volume_bwd(Tensor dC, int N2, Tensor f1, Tensor f2cm, float scale, Tensor(a!) df1, bool accumulate, Tensor(b!) df2) -> ()");
  m.def("convex_upsample_bwd(Tensor flow, Tensor mask, Tensor grad_out, Tensor(a!) grad_mask, Tensor(b!) grad_flow) -> ()");
  m.def("convex_upsample2_bwd(Tensor flow, Tensor mask, Tensor grad_out, Tensor(a!) grad_mask, Tensor(b!) grad_flow) -> ()");
  m.def("corr_lookup_coords_bwd(Tensor[] levels, Tensor coords, int radius, Tensor grad_out, Tensor(a!) grad_coords) -> ()");
  m.def("convex_upsample_info_bwd(Tensor flow_pm, Tensor info_pm, Tensor mask, Tensor grad_flow_up, Tensor? grad_info_up, "
        "Tensor(a!) grad_mask, Tensor(b!) grad_flow_pm, Tensor(c!) grad_info_pm) -> ()");
  m.def("layernorm_rows(Tensor inp, Tensor? weight, Tensor? bias, float eps, Tensor(a!) out) -> ()");
  m.def("xca_map(Tensor qk, Tensor temperature, Tensor(a!) A, int B, int N) -> ()");
  m.def("xcit_lpi_workspace_bytes(int B, int H, int W) -> int", &xcit_lpi_workspace_bytes);
  m.def("xcit_lpi1(Tensor x, Tensor ln_weight, Tensor ln_bias, float ln_eps, Tensor dw_weight, Tensor dw_bias, Tensor(a!) u, "
        "Tensor(b!) workspace, int B, int H, int W) -> ()");
  m.def("xcit_lpi2(Tensor u, Tensor gn_weight, Tensor gn_bias, float gn_eps, int groups, Tensor dw_weight, Tensor dw_bias, Tensor gamma, "
        "Tensor x, Tensor(a!) x2, Tensor? ln_weight, Tensor? ln_bias, float ln_eps, Tensor(b!) t, Tensor(c!) workspace, int B, int H, "
        "int W) -> ()");
  m.def("xcit_tokens(Tensor inp, Tensor? pos, float eps, Tensor(a!) x0, Tensor(b!) xh) -> ()");
  m.def("xcit_tokens_pm(Tensor inp, Tensor? pos, float eps, Tensor(a!) x0, Tensor(b!) xh, int B, int H, int W) -> ()");
  m.def("xca_fold(Tensor A, Tensor wv, Tensor bv, Tensor wp, Tensor bp, Tensor(a!) M, Tensor(b!) c) -> ()");
  m.def("groupnorm_workspace_bytes(int B, int HW, int C) -> int", &groupnorm_workspace_bytes);
  m.def("groupnorm_stats(Tensor x, int B, int HW, int group_size, Tensor gamma, Tensor beta, float eps, Tensor(a!) scale, "
        "Tensor(b!) shift, Tensor(c!) workspace) -> ()");
  m.def("affine_apply(Tensor x, Tensor scale, Tensor shift, Tensor? residual, Tensor(a!) out, int B, int HW, bool relu, "
        "bool relu_after_residual) -> ()");
  m.def("resize_bilinear_pm(Tensor inp, Tensor(a!) out, int B, int Hi, int Wi, int Ho, int Wo) -> ()");
  m.def("nchw_to_pm(Tensor inp, Tensor(a!) out) -> ()");
  m.def("pm_to_nchw(Tensor inp, Tensor(a!) out) -> ()");
  m.def("pm_to_cm(Tensor inp, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(pfk, CUDA, m) {
  m.impl("corr_volume", &corr_volume);
  m.impl("corr_pool2x2", &corr_pool2x2);
  m.impl("corr_volume_bf16", &corr_volume_bf16);
  m.impl("fmap_pool2x2", &fmap_pool2x2);
  m.impl("corr_lookup", &corr_lookup);
  m.impl("fmap_to_blocked", &fmap_to_blocked);
  m.impl("corr_pool2x2_blocked", &corr_pool2x2_blocked);
  m.impl("corr_lookup_blocked", &corr_lookup_blocked);
  m.impl("conv2d", &conv2d);
  m.impl("conv2d_b16", &conv2d_b16);
  m.impl("conv2d_group", &conv2d_group);
  m.impl("conv2d_wino", &conv2d_wino);
  m.impl("conv2d_wino_res", &conv2d_wino_res);
  m.impl("conv2d_wino_norm", &conv2d_wino_norm);
  m.impl("conv2d_wino_stats", &conv2d_wino_stats);
  m.impl("conv2d_wino1d", &conv2d_wino1d);
  m.impl("conv_cin2", &conv_cin2);
  m.impl("flow_delta", &flow_delta);
  m.impl("flow_from_coords", &flow_from_coords);
  m.impl("convex_upsample", &convex_upsample);
  m.impl("convex_upsample_pm", &convex_upsample_pm);
  m.impl("convex_upsample2", &convex_upsample2);
  m.impl("convex_upsample2_pm", &convex_upsample2_pm);
  m.impl("mask_upsample", &mask_upsample);
  m.impl("convex_upsample_info_pm", &convex_upsample_info_pm);
  m.impl("dwconv_layernorm", &dwconv_layernorm);
  m.impl("dwconv_layernorm_b16", &dwconv_layernorm_b16);
  m.impl("dwconv_layernorm_train", &dwconv_layernorm_train);
  m.impl("dwconv_layernorm_train_b16", &dwconv_layernorm_train_b16);
  m.impl("layernorm_bwd", &layernorm_bwd);
  m.impl("layernorm_bwd_b16", &layernorm_bwd_b16);
  m.impl("dwconv_bwd", &dwconv_bwd);
  m.impl("dwconv_bwd_b16", &dwconv_bwd_b16);
  m.impl("gelu", &gelu_rows);
  m.impl("gelu_b16", &gelu_rows_b16);
  m.impl("gelu_bwd", &gelu_rows_bwd);
  m.impl("gelu_bwd_b16", &gelu_rows_bwd_b16);
  m.impl("conv2d_gelu_b16", &conv2d_gelu_b16);
  m.impl("convex_upsample_info_pm_b16", &convex_upsample_info_pm_b16);
  m.impl("upflow8", &upflow8);
  m.impl("altcorr_forward", &altcorr_forward);
  m.impl("altcorr_backward", &altcorr_backward);
  m.impl("corr_lookup_bwd", &corr_lookup_bwd);
  m.impl("corr_volume_bwd", &corr_volume_bwd);
  m.impl("convex_upsample_bwd", &convex_upsample_bwd);
  m.impl("convex_upsample2_bwd", &convex_upsample2_bwd);
  m.impl("corr_lookup_coords_bwd", &corr_lookup_coords_bwd);
  m.impl("convex_upsample_info_bwd", &convex_upsample_info_bwd);
  m.impl("layernorm_rows", &layernorm_rows);
  m.impl("xca_map", &xca_map);
  m.impl("xcit_lpi1", &xcit_lpi1);
  m.impl("xcit_lpi2", &xcit_lpi2);
  m.impl("xcit_tokens", &xcit_tokens);
  m.impl("xcit_tokens_pm", &xcit_tokens_pm);
  m.impl("xca_fold", &xca_fold);
  m.impl("groupnorm_stats", &groupnorm_stats);
  m.impl("affine_apply", &affine_apply);
  m.impl("resize_bilinear_pm", &resize_bilinear_pm);
  m.impl("nchw_to_pm", &nchw_to_pm);
  m.impl("pm_to_nchw", &pm_to_nchw);
  m.impl("pm_to_cm", &pm_to_cm);
  m.impl("conv_stem", &conv_stem);
  m.impl("conv_stem2", &conv_stem2);
  m.impl("gru_gates_zr", &gru_gates_zr);
  m.impl("gru_gates_q", &gru_gates_q);
  m.impl("gru_backward_q", &gru_backward_q);
  m.impl("gru_backward_zr", &gru_backward_zr);
  m.impl("conv_wgrad", &conv_wgrad);
  m.impl("conv_wgrad_unpacked", &conv_wgrad_unpacked);
  m.impl("conv_wgrad_unpacked_b16", &conv_wgrad_unpacked_b16);
  m.impl("forward_interpolate", &forward_interpolate);
  m.impl("softmax_rows", &softmax_rows);
  m.impl("softmax_rows_bwd", &softmax_rows_bwd);
  m.impl("transpose_pack", &transpose_pack);
  m.impl("norm_bwd", &norm_bwd);
  m.impl("conv_stem_wgrad", &conv_stem_wgrad);
  m.impl("instnorm_stats", &instnorm_stats);
  m.impl("norm_apply", &norm_apply);
  m.impl("norm_apply_res", &norm_apply_res);
}
