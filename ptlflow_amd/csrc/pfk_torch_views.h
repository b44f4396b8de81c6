// Checked views for pfk_torch.cpp: the one place where an at::Tensor becomes the raw pointer, stride and extents that the kernels
// behind include/pfk.h trust.  The C ABI can check alignment and null pointers; it never sees a tensor, so devices, dtypes and extents
// are checked here or nowhere.  Every tensor argument of every op passes through exactly one of rows() / dense() / up8() /
// fill_sources(), and every message names the op and the argument.
#pragma once

#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <utility>

#include "pfk.h"

namespace {

using at::Tensor;

void check_ok(int status, const char* what) {
  TORCH_CHECK(status == PFK_OK, "pfk::", what, " failed: ", pfk_status_string(status), " (", status, ")");
}

// Every op opens an OpScope on one of its tensors: the HIP device becomes that tensor's device for the duration of the
// op (kernels, torch's current stream and any at::empty are then on the GPU that owns the data, whatever the caller's
// current device is — model.to("cuda:1") with device 0 current), and every tensor checked afterwards must live there too.
thread_local const c10::Device* tl_op_device = nullptr;
struct OpScope {
  c10::Device dev;
  c10::DeviceGuard guard;   // generic guard: resolves to the (CUDA-masquerading) HIP implementation registered for the tensor's device type
  explicit OpScope(const Tensor& t) : dev(t.device()), guard(t.device()) {
    TORCH_CHECK(t.is_cuda(), "pfk ops need GPU tensors");
    tl_op_device = &dev;
  }
  ~OpScope() { tl_op_device = nullptr; }
};

pfk_stream_t cur_stream() { return static_cast<pfk_stream_t>(c10::hip::getCurrentHIPStream().stream()); }

// element types a view may be asked for: Any = float32 or bfloat16, Raw = whatever the tensor holds (byte workspaces)
enum Elem { F32, B16, Any, Raw };

struct AtLeast { int64_t n; };   // a lower bound where a plain count means equality

// the op's device and the dtype; true for bfloat16
bool check_elem(const char* op, const Tensor& t, const char* name, Elem e) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(tl_op_device == nullptr || t.device() == *tl_op_device, op, ": ", name, " is on ", t.device(), " but the op runs on ", *tl_op_device);
  const bool f32 = t.scalar_type() == at::kFloat, b16 = t.scalar_type() == at::kBFloat16;
  TORCH_CHECK(e != F32 || f32, op, ": ", name, " must be float32");
  TORCH_CHECK(e != B16 || b16, op, ": ", name, " must be bfloat16");
  TORCH_CHECK(e != Any || f32 || b16, op, ": ", name, " must be float32 or bfloat16");
  return b16;
}

// a checked pointer: f32() only where the elements are float32, raw() for bf16 / byte / either-dtype arguments of the C ABI
struct Ptr {
  void* ptr = nullptr;
  bool b16 = false;
  float* f32() const { TORCH_CHECK(!b16, "pfk: a bfloat16 tensor was read as float32"); return static_cast<float*>(ptr); }
  void* raw() const { return ptr; }
};

// Pixel-major activations: a 2-D row-strided view [rows, cols] with unit channel stride whose row stride is the buffer's `ld` — a
// channel slice of a wider buffer (buf[:, 128:384]) is just a view.
struct Rows : Ptr {
  int64_t ld = 0, rows = 0, cols = 0;
  const char *op = "", *name = "";
  const Rows& expect(int64_t r, int64_t c) const {
    TORCH_CHECK(rows == r && cols == c, op, ": ", name, " must be a [", r, ", ", c, "] view, got [", rows, ", ", cols, "]");
    return *this;
  }
  const Rows& expect(int64_t r, AtLeast c) const {
    TORCH_CHECK(rows == r && cols >= c.n, op, ": ", name, " must be a [", r, ", >= ", c.n, "] view, got [", rows, ", ", cols, "]");
    return *this;
  }
};

Rows rows(const char* op, const Tensor& t, const char* name, Elem e) {
  Rows v;
  v.b16 = check_elem(op, t, name, e);
  TORCH_CHECK(t.dim() == 2 && (t.size(1) == 1 || t.stride(1) == 1), op, ": ", name,
              " must be a [pixels, channels] view with contiguous channels");
  v.ptr = t.data_ptr(); v.ld = t.stride(0); v.rows = t.size(0); v.cols = t.size(1);
  v.op = op; v.name = name;
  return v;
}

// A contiguous tensor of the given element type with at least n elements (the shape, where it matters, is the op's to state) ...
Ptr dense(const char* op, const Tensor& t, const char* name, Elem e, AtLeast n = {0}) {
  const bool b16 = check_elem(op, t, name, e);
  TORCH_CHECK(t.is_contiguous() && t.numel() >= n.n, op, ": ", name, " must be contiguous with at least ", n.n, " elements, got ", t.numel());
  return {t.data_ptr(), b16};
}
// ... or with exactly n
Ptr dense(const char* op, const Tensor& t, const char* name, Elem e, int64_t n) {
  const bool b16 = check_elem(op, t, name, e);
  TORCH_CHECK(t.is_contiguous() && t.numel() == n, op, ": ", name, " must be contiguous with ", n, " elements, got ", t.numel());
  return {t.data_ptr(), b16};
}
// an optional one: a null pointer for None
Ptr dense(const char* op, const c10::optional<Tensor>& t, const char* name, Elem e, AtLeast n) {
  return t.has_value() ? dense(op, *t, name, e, n) : Ptr{};
}
Ptr dense(const char* op, const c10::optional<Tensor>& t, const char* name, Elem e, int64_t n) {
  return t.has_value() ? dense(op, *t, name, e, n) : Ptr{};
}

// the sources of a convolution: 1..3 [rows, channels_i] views into pfk_conv_desc / pfk_conv_b16_desc (same src[] / num_src fields)
template <class Desc>
void fill_sources(Desc& d, at::TensorList srcs, int64_t n_rows, Elem e, const char* op) {
  TORCH_CHECK(srcs.size() >= 1 && srcs.size() <= 3, op, ": 1..3 sources");
  for (size_t i = 0; i < srcs.size(); ++i) {
    const Rows s = rows(op, srcs[i], "src", e).expect(n_rows, AtLeast{0});
    d.src[i].ptr = static_cast<decltype(d.src[i].ptr)>(s.raw()); d.src[i].ld = s.ld; d.src[i].channels = s.cols;
  }
  d.num_src = srcs.size();
}

// output rows of a strided convolution (padding k/2): B * Ho * Wo
int64_t out_rows(int64_t B, int64_t H, int64_t W, int64_t stride) { return B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1); }

// B, H, W of the 1/8-resolution grid, taken from a contiguous float32 [B, 2, 8H, 8W] tensor (`scale`: of the 1/scale grid)
struct Up8 {
  int B = 0, H = 0, W = 0;
  float* ptr = nullptr;
  int64_t rows() const { return (int64_t)B * H * W; }
};
Up8 up8(const char* op, const Tensor& t, const char* name, int scale = 8) {
  const Ptr p = dense(op, t, name, F32);
  TORCH_CHECK(t.dim() == 4 && t.size(1) == 2 && t.size(2) % scale == 0 && t.size(3) % scale == 0, op, ": ", name, " must be [B, 2, ", scale,
              "H, ", scale, "W] contiguous");
  return {(int)t.size(0), (int)(t.size(2) / scale), (int)(t.size(3) / scale), p.f32()};
}

// scratch from the caching allocator on `like`'s device: the tensor that owns it and its pointer (null when need == 0)
std::pair<Tensor, void*> byte_workspace(long long need, const Tensor& like) {
  if (need <= 0) return {Tensor(), nullptr};
  Tensor ws = at::empty({(int64_t)need}, like.options().dtype(at::kByte));
  return {ws, ws.data_ptr()};
}

}  // namespace
