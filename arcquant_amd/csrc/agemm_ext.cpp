// The reference's boundary in the reference's own form: a CPython extension module named `agemm` (pybind11 + libtorch) with the
// four hot-path functions of kernels/src/bindings.cpp:551-575 -- same names, keyword names, argument meaning, return shapes and
// dtypes, RuntimeError on an unsupported shape -- and the six KV-cache names as stubs (bindings.cpp:576-581, out of scope).  Every
// function body is argument checking + one call into the C-ABI of include/arcq.h (libarcq_hip.so, hand-written gfx950 kernels);
// torch is used for device memory and the current HIP stream only.  Drop-in:
//     sys.path.append("<repo>/arcquant_amd/lib"); import agemm          # instead of kernels/build/ (model/qLinearLayer.py:7-8)
// The ctypes mirror arcquant_amd/agemm.py has the same surface plus the extensions; this module exists because a ctypes call
// costs 9.5-13 us of host time (18 marshalled arguments) and an eager decode step makes ~170 of them: here a call is ~3 us.
//
// Differences from the reference a caller can observe (deviations D2-D4): launches go to torch's CURRENT stream; `scale`
// may be a 0-dim CUDA fp32 tensor and is then read on the device (the reference's `const float scale` forces `.item()`); KQ is not
// limited to the reference's template list.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>      // torch-ROCm tensors say "cuda": the guard / stream types that accept it
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <stdexcept>
#include <string>
#include <tuple>

#include "../../include/arcq.h"

namespace {

// Every function validates in one order (the ctypes mirror's): dtype / rank / contiguity of its tensors (need), the shape and size relations
// between them, out_dtype, the optional tensors (out_of, opt_ptr: dtype, rank, contiguity and shape at once), and LAST where everything lives
// (same_device).  So every rejection but the last is reachable with CPU tensors, and a call built from CPU tensors cannot reach a launch.
void need(const torch::Tensor& t, c10::ScalarType dt, const char* name, int64_t ndim = -1) {
  if (t.scalar_type() != dt) throw std::runtime_error(std::string("agemm: ") + name + " has the wrong dtype");   // reference: data_ptr<T>() throws
  if (ndim >= 0 && t.dim() != ndim) throw std::runtime_error(std::string("agemm: ") + name + " has the wrong rank");
  if (!t.is_contiguous()) throw std::runtime_error(std::string("agemm: ") + name + " must be contiguous");
}

// the device guard and the stream of a call are those of its first operand: a tensor elsewhere would hand the kernel a pointer it cannot read
void same_device(const char* who, const torch::Tensor& A, std::initializer_list<const torch::Tensor*> ts) {
  if (!A.is_cuda()) throw std::runtime_error(std::string("agemm.") + who + ": the operands must live on the GPU (there is no CPU path)");
  for (const torch::Tensor* t : ts)
    if (t && t->defined() && t->device() != A.device())
      throw std::runtime_error(std::string("agemm.") + who + ": every operand must live on the GPU of the first one");
}
const torch::Tensor* opt_t(const c10::optional<torch::Tensor>& t) { return t.has_value() ? &*t : nullptr; }

void check(int status, const char* what) {
  if (status != ARCQ_OK) throw std::runtime_error(std::string(what) + ": " + arcq_last_error());
}

void* stream_of(const torch::Tensor& t) { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

// The reference's `scale`: a Python float, or a tensor.  A 1-element fp32 CUDA tensor is consumed on the device (no .item() sync), any other
// tensor through the reference's implicit __float__.  any_as_f32 (the SiLU-epilogue GEMMs, as the mirror): ANY CUDA tensor is read on the
// device, as fp32.
struct Alpha {
  float host = 1.0f;
  const float* dev = nullptr;
  torch::Tensor keep;
  const torch::Tensor* tensor() const { return keep.defined() ? &keep : nullptr; }
};
Alpha alpha_of(const py::object& scale, double scale_host, bool any_as_f32 = false) {
  Alpha a;
  a.host = (float)scale_host;
  if (!THPVariable_Check(scale.ptr())) {
    a.host *= scale.cast<float>();
    return a;
  }
  const torch::Tensor& t = THPVariable_Unpack(scale.ptr());
  if (t.is_cuda() && any_as_f32) {
    a.keep = t.reshape({-1}).slice(0, 0, 1).to(torch::kFloat32);
  } else if (t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.numel() == 1) {
    a.keep = t;
  } else {
    a.host *= t.item<float>();
    return a;
  }
  a.dev = a.keep.data_ptr<float>();
  return a;
}
const void* opt_ptr(const c10::optional<torch::Tensor>& t, c10::ScalarType dt, const char* name, std::initializer_list<int64_t> shape) {
  if (!t.has_value()) return nullptr;
  need(*t, dt, name, (int64_t)shape.size());
  int i = 0;
  for (int64_t d : shape)
    if (t->size(i++) != d) throw std::runtime_error(std::string("agemm: ") + name + " has the wrong shape");
  return t->data_ptr();
}
struct OutDtype {
  c10::ScalarType dt;
  int code;
};
OutDtype out_dtype_of(const py::object& out_dtype, const char* who) {
  const auto dt = out_dtype.is_none() ? torch::kBFloat16 : torch::python::detail::py_object_to_dtype(out_dtype);
  if (dt == torch::kBFloat16) return {dt, ARCQ_OUT_BF16};
  if (dt == torch::kFloat32) return {dt, ARCQ_OUT_F32};
  throw std::runtime_error(std::string("agemm.") + who + ": out_dtype must be bfloat16 or float32");
}
// the caller's `out` if it is [M, N] of this dtype, else a new tensor next to `like`; same_device then takes it with the other operands
torch::Tensor out_of(const c10::optional<torch::Tensor>& out, int64_t M, int64_t N, c10::ScalarType dt, const torch::Tensor& like, const char* who) {
  if (!out.has_value()) return torch::empty({M, N}, like.options().dtype(dt));
  if (out->dim() != 2 || out->size(0) != M || out->size(1) != N || out->scalar_type() != dt || !out->is_contiguous())
    throw std::runtime_error(std::string("agemm.") + who + ": out has the wrong shape / dtype");
  return *out;
}
void need_repacked(const torch::Tensor& RW, const torch::Tensor& RSF, int64_t N, int64_t K, const char* who, int64_t n_mult = 1) {
  need(RW, torch::kUInt8, "RW", 1);
  need(RSF, torch::kUInt8, "RSF", 1);
  if (K % 64 || N % n_mult || RW.numel() != arcq_repacked_w_bytes(N, K) || RSF.numel() != arcq_repacked_sf_bytes(N, K))
    throw std::runtime_error(std::string("Value error in ") + who + ": RW / RSF do not belong to a [N, K] weight of this shape" +
                             (n_mult > 1 ? ", or N % " + std::to_string(n_mult) + " != 0" : ""));
}
// the opening of a GEMM over a repacked weight: A [M, K/2], its scales SFA, and (RW, RSF) of N rows over the same K
struct GemmShape {
  int64_t M, K;
};
GemmShape open_repacked(const char* who, const torch::Tensor& A, const torch::Tensor& RW, const torch::Tensor& SFA, const torch::Tensor& RSF, int64_t N,
                        int64_t n_mult = 1) {
  need(A, torch::kUInt8, "A", 2);
  need(SFA, torch::kUInt8, "SFA");
  const GemmShape g{A.size(0), A.size(1) * 2};
  need_repacked(RW, RSF, N, g.K, who, n_mult);
  if (SFA.numel() < arcq_sf_used_bytes(g.M, g.K)) throw std::runtime_error(std::string("Value error in ") + who + ": SFA smaller than the swizzled layout of A");
  return g;
}

// agemm.matmul(A, B, SFA, SFB, scale) -> bf16 [M, N]   (bindings.cpp:99-120)
torch::Tensor matmul(const torch::Tensor& A, const torch::Tensor& B, const torch::Tensor& SFA, const torch::Tensor& SFB, const py::object& scale) {
  need(A, torch::kUInt8, "A", 2);
  need(B, torch::kUInt8, "B", 2);
  need(SFA, torch::kUInt8, "SFA");
  need(SFB, torch::kUInt8, "SFB");
  const int64_t M = A.size(0), N = B.size(0), K = A.size(1) * 2;      // bindings.cpp:107-109
  if (B.size(1) * 2 != K) throw std::runtime_error("agemm.matmul: A and B disagree on K");
  if (SFA.numel() < arcq_sf_used_bytes(M, K) || SFB.numel() < arcq_sf_used_bytes(N, K))
    throw std::runtime_error("agemm.matmul: SFA / SFB smaller than the swizzled layout of its operand");
  const Alpha al = alpha_of(scale, 1.0);
  same_device("matmul", A, {&B, &SFA, &SFB, al.tensor()});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
  auto D = torch::empty({M, N}, A.options().dtype(torch::kBFloat16));
  const int64_t ws_bytes = arcq_gemm_workspace_bytes(M, N, K);
  torch::Tensor ws;
  if (ws_bytes) ws = torch::empty({ws_bytes}, A.options());
  check(arcq_gemm_nvfp4(A.data_ptr<uint8_t>(), B.data_ptr<uint8_t>(), SFA.data_ptr<uint8_t>(), SFB.data_ptr<uint8_t>(), D.data_ptr(), M, N, K, al.host, al.dev,
                        nullptr, nullptr, ARCQ_OUT_BF16, ws_bytes ? ws.data_ptr() : nullptr, ws_bytes, stream_of(A)),
        "matmul");
  return D;
}

std::tuple<torch::Tensor, torch::Tensor> quantize(bool is_x, const torch::Tensor& X, const torch::Tensor& reorder_index, int64_t KE) {
  const char* who = is_x ? "reorder_quantize_x" : "reorder_quantize_w";
  need(X, torch::kBFloat16, is_x ? "X" : "W", 2);
  need(reorder_index, torch::kInt16, "reorder_index", 1);
  const int64_t rows = X.size(0), KQ = X.size(1), K = KQ + KE;
  if (reorder_index.numel() != KQ || KQ % 64 || KE % 64 || KE < 0 || KE > KQ)
    throw std::runtime_error(std::string("Value error in ") + who + ": KQ / KE / reorder_index are not valid");       // bindings.cpp:157-160
  same_device(who, X, {&reorder_index});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  auto Q = torch::empty({rows, K / 2}, X.options().dtype(torch::kUInt8));
  auto SF = torch::empty({arcq_sf_alloc_bytes(rows, K)}, X.options().dtype(torch::kUInt8));      // bindings.cpp:83-95
  const int variant = arcq_variant_for_kq(KQ);
  auto fn = is_x ? arcq_quantize_x : arcq_quantize_w;
  check(fn(X.data_ptr(), reorder_index.data_ptr<int16_t>(), Q.data_ptr<uint8_t>(), SF.data_ptr<uint8_t>(), rows, KQ, KE, variant, stream_of(X)), who);
  return {Q, SF};
}

std::tuple<torch::Tensor, torch::Tensor> reorder_quantize_x(const torch::Tensor& X, const torch::Tensor& reorder_index, int64_t KE) {
  return quantize(true, X, reorder_index, KE);           // bindings.cpp:122-163
}
std::tuple<torch::Tensor, torch::Tensor> reorder_quantize_w(const torch::Tensor& W, const torch::Tensor& reorder_index, int64_t KE) {
  return quantize(false, W, reorder_index, KE);          // bindings.cpp:170-210
}

// agemm.rmsnorm_quantize_x(X, W, eps, reorder_index, KE)   (bindings.cpp:216-254)
std::tuple<torch::Tensor, torch::Tensor> rmsnorm_quantize_x(const torch::Tensor& X, const torch::Tensor& W, double eps, const torch::Tensor& reorder_index,
                                                            int64_t KE) {
  need(X, torch::kBFloat16, "X", 2);
  need(W, torch::kBFloat16, "W", 1);
  need(reorder_index, torch::kInt16, "reorder_index", 1);
  const int64_t M = X.size(0), KQ = X.size(1), K = KQ + KE;
  if (W.numel() != KQ || reorder_index.numel() != KQ || KQ % 64 || KE % 64 || KE < 0 || KE > KQ || KQ < 2048 || KQ > 8192)
    throw std::runtime_error("Value error in run_rmsnorm_x_bf16_nvfp4: K value is not valid: " + std::to_string(KQ));   // bindings.cpp:248-251
  same_device("rmsnorm_quantize_x", X, {&W, &reorder_index});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  auto Q = torch::empty({M, K / 2}, X.options().dtype(torch::kUInt8));
  auto SF = torch::empty({arcq_sf_alloc_bytes(M, K)}, X.options().dtype(torch::kUInt8));
  check(arcq_rmsnorm_quantize_x(X.data_ptr(), W.data_ptr(), (float)eps, reorder_index.data_ptr<int16_t>(), Q.data_ptr<uint8_t>(), SF.data_ptr<uint8_t>(), M, KQ,
                                KE, arcq_variant_for_kq(KQ), stream_of(X)),
        "rmsnorm_quantize_x");
  return {Q, SF};
}

// ---- the decode extensions of arcquant_amd/agemm.py under the same names and keywords: an eager decode step of
//      the model harness makes ~170 calls, at the ctypes mirror's 8-12 us each it is host-paced
torch::Tensor matmul_repacked(const torch::Tensor& A, const torch::Tensor& RW, const torch::Tensor& SFA, const torch::Tensor& RSF, const py::object& scale,
                              int64_t N, const c10::optional<torch::Tensor>& bias, const c10::optional<torch::Tensor>& residual, py::object out_dtype,
                              const c10::optional<torch::Tensor>& out, double scale_host) {
  const char* who = "matmul_repacked";
  const auto [M, K] = open_repacked(who, A, RW, SFA, RSF, N);
  if (!arcq_gemm_repacked_supported(M, N, K)) throw std::runtime_error("matmul_repacked: this shape is outside the repacked path (see repacked_supported)");
  const OutDtype od = out_dtype_of(out_dtype, who);
  const Alpha al = alpha_of(scale, scale_host);
  torch::Tensor D = out_of(out, M, N, od.dt, A, who);
  const void* bp = opt_ptr(bias, torch::kBFloat16, "bias", {N});
  const void* rp = opt_ptr(residual, torch::kBFloat16, "residual", {M, N});
  same_device(who, A, {&RW, &SFA, &RSF, al.tensor(), &D, opt_t(bias), opt_t(residual)});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
  check(arcq_gemm_nvfp4_repacked(A.data_ptr<uint8_t>(), RW.data_ptr<uint8_t>(), SFA.data_ptr<uint8_t>(), RSF.data_ptr<uint8_t>(), D.data_ptr(), M, N, K, al.host,
                                 al.dev, bp, rp, od.code, stream_of(A)),
        who);
  return D;
}

// ---- one weight copy for every M (include/arcq.h, arcq_gemm_nvfp4_rw)
torch::Tensor matmul_rw(const torch::Tensor& A, const torch::Tensor& RW, const torch::Tensor& SFA, const torch::Tensor& RSF, const py::object& scale, int64_t N,
                        const c10::optional<torch::Tensor>& bias, const c10::optional<torch::Tensor>& residual, py::object out_dtype,
                        const c10::optional<torch::Tensor>& out, double scale_host) {
  const char* who = "matmul_rw";
  const auto [M, K] = open_repacked(who, A, RW, SFA, RSF, N);
  const OutDtype od = out_dtype_of(out_dtype, who);
  const Alpha al = alpha_of(scale, scale_host);
  torch::Tensor D = out_of(out, M, N, od.dt, A, who);
  const void* bp = opt_ptr(bias, torch::kBFloat16, "bias", {N});
  const void* rp = opt_ptr(residual, torch::kBFloat16, "residual", {M, N});
  same_device(who, A, {&RW, &SFA, &RSF, al.tensor(), &D, opt_t(bias), opt_t(residual)});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
  const int64_t ws_bytes = arcq_gemm_rw_workspace_bytes(M, N, K);
  torch::Tensor ws;
  if (ws_bytes) ws = torch::empty({ws_bytes}, A.options());
  check(arcq_gemm_nvfp4_rw(A.data_ptr<uint8_t>(), RW.data_ptr<uint8_t>(), SFA.data_ptr<uint8_t>(), RSF.data_ptr<uint8_t>(), D.data_ptr(), M, N, K, al.host, al.dev,
                           bp, rp, od.code, ws_bytes ? ws.data_ptr() : nullptr, ws_bytes, stream_of(A)),
        who);
  return D;
}

std::tuple<torch::Tensor, torch::Tensor> matmul_rw_silu_mul(const torch::Tensor& A, const torch::Tensor& RW, const torch::Tensor& SFA, const torch::Tensor& RSF,
                                                            const py::object& scale, int64_t N, double scale_host, const c10::optional<torch::Tensor>& bias) {
  const char* who = "matmul_rw_silu_mul";
  const auto [M, K] = open_repacked(who, A, RW, SFA, RSF, N, 8);
  const Alpha al = alpha_of(scale, scale_host, true);
  const void* bp = opt_ptr(bias, torch::kBFloat16, "bias", {N});
  same_device(who, A, {&RW, &SFA, &RSF, al.tensor(), opt_t(bias)});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
  auto act = torch::empty({M, N / 2}, A.options().dtype(torch::kBFloat16));
  auto slots = torch::empty({std::max<int64_t>(1, arcq_gemm_rw_silu_mul_slots(M, N, K))}, A.options().dtype(torch::kInt32));
  check(arcq_gemm_nvfp4_rw_silu_mul(A.data_ptr<uint8_t>(), RW.data_ptr<uint8_t>(), SFA.data_ptr<uint8_t>(), RSF.data_ptr<uint8_t>(), act.data_ptr(),
                                    (uint32_t*)slots.data_ptr<int32_t>(), M, N, K, al.host, al.dev, bp, stream_of(A)),
        who);
  return {act, slots};
}

// the inverse of agemm.repack_w (data movement only, on RW's device): (QW [N, K/2], SFW [arcq_sf_alloc_bytes(N, K)], unused bytes zero)
std::tuple<torch::Tensor, torch::Tensor> unrepack_w(const torch::Tensor& RW, const torch::Tensor& RSF, int64_t N, int64_t K) {
  need(RW, torch::kUInt8, "RW", 1);
  need(RSF, torch::kUInt8, "RSF", 1);
  if (N <= 0 || K <= 0 || K % 64 || RW.numel() != arcq_repacked_w_bytes(N, K) || RSF.numel() != arcq_repacked_sf_bytes(N, K))
    throw std::runtime_error("Value error in unrepack_w: RW / RSF do not belong to a [N, K] weight of this shape");
  const int64_t Np = (N + 15) / 16 * 16, Kp = (K + 255) / 256 * 256, RB = Np / 16, T = Kp / 128;
  auto QW = RW.view({RB, T, 4, 16, 16}).permute({0, 3, 1, 2, 4}).reshape({Np, Kp / 2}).slice(0, 0, N).slice(1, 0, K / 2).contiguous();
  auto sf = RSF.view({RB, T / 2, 4, 16, 2, 2}).permute({0, 3, 1, 4, 2, 5}).reshape({Np, Kp / 16}).slice(0, 0, N).slice(1, 0, K / 16);
  const auto io = RW.options().dtype(torch::kInt64);
  auto r = torch::arange(N, io).unsqueeze(1), g = torch::arange(K / 16, io).unsqueeze(0);
  auto off = (r.div(128, "floor") * (K / 64) + g.div(4, "floor")) * 512 + r.remainder(32) * 16 + r.div(32, "floor").remainder(4) * 4 + g.remainder(4);
  auto SFW = torch::zeros({arcq_sf_alloc_bytes(N, K)}, RW.options());
  SFW.index_put_({off}, sf);
  return {QW, SFW};
}

struct FusedShape {
  int64_t M, KQ, KE, K;
  int variant;
};
FusedShape fused_common(const char* who, const torch::Tensor& X, const torch::Tensor& reorder_index, const torch::Tensor& RW, const torch::Tensor& RSF, int64_t N,
                        int64_t KE, const py::object& variant) {
  need(X, torch::kBFloat16, "X", 2);
  need(reorder_index, torch::kInt16, "reorder_index", 1);
  FusedShape f{X.size(0), X.size(1), KE, X.size(1) + KE, 0};
  if (f.KQ % 64 || KE % 64 || KE < 0 || KE > f.KQ || reorder_index.numel() != f.KQ) throw std::runtime_error(std::string("Value error in ") + who + ": KQ / KE / reorder_index are not valid");
  need_repacked(RW, RSF, N, f.K, who);
  f.variant = variant.is_none() ? arcq_variant_for_kq(f.KQ) : variant.cast<int>();
  return f;
}

torch::Tensor rmsnorm_matmul_repacked(const torch::Tensor& X, const torch::Tensor& W, double eps, const torch::Tensor& reorder_index, int64_t KE,
                                      const torch::Tensor& RW, const torch::Tensor& RSF, const py::object& scale, int64_t N,
                                      const c10::optional<torch::Tensor>& bias, const c10::optional<torch::Tensor>& residual, py::object out_dtype,
                                      const c10::optional<torch::Tensor>& out, double scale_host, const py::object& variant) {
  const char* who = "rmsnorm_matmul_repacked";
  const FusedShape f = fused_common(who, X, reorder_index, RW, RSF, N, KE, variant);
  need(W, torch::kBFloat16, "W", 1);
  if (W.numel() != f.KQ) throw std::runtime_error("agemm: W has the wrong shape");
  if (!arcq_linear_fused_supported(ARCQ_SRC_RMSNORM, f.M, N, f.KQ, KE)) throw std::runtime_error("rmsnorm_matmul_repacked: outside the fused path (see fused_supported)");
  const OutDtype od = out_dtype_of(out_dtype, who);
  const Alpha al = alpha_of(scale, scale_host);
  torch::Tensor D = out_of(out, f.M, N, od.dt, X, who);
  const void* bp = opt_ptr(bias, torch::kBFloat16, "bias", {N});
  const void* rp = opt_ptr(residual, torch::kBFloat16, "residual", {f.M, N});
  same_device(who, X, {&W, &reorder_index, &RW, &RSF, al.tensor(), &D, opt_t(bias), opt_t(residual)});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  check(arcq_linear_rmsnorm_repacked(X.data_ptr(), W.data_ptr(), (float)eps, reorder_index.data_ptr<int16_t>(), RW.data_ptr<uint8_t>(), RSF.data_ptr<uint8_t>(), D.data_ptr(),
                                     f.M, N, f.KQ, KE, f.variant, al.host, al.dev, bp, rp, od.code, stream_of(X)),
        who);
  return D;
}

std::tuple<torch::Tensor, torch::Tensor> rmsnorm_matmul_repacked_silu(const torch::Tensor& X, const torch::Tensor& W, double eps, const torch::Tensor& reorder_index,
                                                                      int64_t KE, const torch::Tensor& RW, const torch::Tensor& RSF, const py::object& scale, int64_t N,
                                                                      double scale_host, const py::object& variant, const c10::optional<torch::Tensor>& bias,
                                                                      const c10::optional<torch::Tensor>& act_scatter_index) {
  const char* who = "rmsnorm_matmul_repacked_silu";
  const FusedShape f = fused_common(who, X, reorder_index, RW, RSF, N, KE, variant);
  need(W, torch::kBFloat16, "W", 1);
  if (W.numel() != f.KQ) throw std::runtime_error("agemm: W has the wrong shape");
  if (N % 4 || !arcq_linear_fused_supported(ARCQ_SRC_RMSNORM, f.M, N, f.KQ, KE))
    throw std::runtime_error("rmsnorm_matmul_repacked_silu: outside the fused path (see fused_supported; N % 4 == 0)");
  const Alpha al = alpha_of(scale, scale_host);
  const void* bp = opt_ptr(bias, torch::kBFloat16, "bias", {N});
  // (act_scatter_index must be a permutation of 0 .. N/2-1: the ctypes mirror checks it once per index tensor; callers of this binding
  //  pass an index that went through that check or through their own)
  const void* sp = opt_ptr(act_scatter_index, torch::kInt16, "act_scatter_index", {N / 2});
  same_device(who, X, {&W, &reorder_index, &RW, &RSF, al.tensor(), opt_t(bias), opt_t(act_scatter_index)});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  auto act = torch::empty({f.M, N / 2}, X.options());
  auto slots = torch::empty({(N + 15) / 16}, X.options().dtype(torch::kInt32));
  check(arcq_linear_rmsnorm_silu_repacked(X.data_ptr(), W.data_ptr(), (float)eps, reorder_index.data_ptr<int16_t>(), RW.data_ptr<uint8_t>(), RSF.data_ptr<uint8_t>(),
                                          act.data_ptr(), (uint32_t*)slots.data_ptr<int32_t>(), f.M, N, f.KQ, KE, f.variant, al.host, al.dev, bp, (const int16_t*)sp,
                                          stream_of(X)),
        who);
  return {act, slots};
}

std::tuple<torch::Tensor, torch::Tensor> dynamic_matmul_repacked(const torch::Tensor& X, const torch::Tensor& reorder_index, int64_t KE, const torch::Tensor& RW,
                                                                 const torch::Tensor& RSF, double scale_w, int64_t N, const c10::optional<torch::Tensor>& absmax_slots,
                                                                 const c10::optional<torch::Tensor>& bias, const c10::optional<torch::Tensor>& residual,
                                                                 py::object out_dtype, const c10::optional<torch::Tensor>& out, const py::object& variant) {
  const char* who = "dynamic_matmul_repacked";
  const FusedShape f = fused_common(who, X, reorder_index, RW, RSF, N, KE, variant);
  if (!arcq_linear_fused_supported(ARCQ_SRC_DYNAMIC, f.M, N, f.KQ, KE)) throw std::runtime_error("dynamic_matmul_repacked: outside the fused path (see fused_supported)");
  const OutDtype od = out_dtype_of(out_dtype, who);
  const uint32_t* sl = nullptr;
  int64_t nsl = 0;
  if (absmax_slots.has_value()) {
    need(*absmax_slots, torch::kInt32, "absmax_slots", 1);
    if (absmax_slots->numel() == 0) throw std::runtime_error("agemm.dynamic_matmul_repacked: absmax_slots must not be empty");
    sl = (const uint32_t*)absmax_slots->data_ptr<int32_t>();
    nsl = absmax_slots->numel();
  }
  torch::Tensor D = out_of(out, f.M, N, od.dt, X, who);
  const void* bp = opt_ptr(bias, torch::kBFloat16, "bias", {N});
  const void* rp = opt_ptr(residual, torch::kBFloat16, "residual", {f.M, N});
  same_device(who, X, {&reorder_index, &RW, &RSF, opt_t(absmax_slots), &D, opt_t(bias), opt_t(residual)});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  auto scale = torch::empty({1}, X.options().dtype(torch::kFloat32));
  check(arcq_linear_dynamic_repacked(X.data_ptr(), reorder_index.data_ptr<int16_t>(), RW.data_ptr<uint8_t>(), RSF.data_ptr<uint8_t>(), D.data_ptr(), scale.data_ptr<float>(), sl,
                                     nsl, f.M, N, f.KQ, KE, f.variant, (float)scale_w, bp, rp, od.code, stream_of(X)),
        who);
  return {D, scale.reshape({})};
}

// reorder_quantize_x_dynamic with the abs-max words of the producing kernel (one launch); reorder_index = None: X is already in reordered order
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> reorder_quantize_x_dynamic(const torch::Tensor& X, const c10::optional<torch::Tensor>& reorder_index, int64_t KE,
                                                                                 const py::object& variant, const torch::Tensor& absmax_slots) {
  need(X, torch::kBFloat16, "X", 2);
  need(absmax_slots, torch::kInt32, "absmax_slots", 1);
  const int64_t M = X.size(0), KQ = X.size(1), K = KQ + KE;
  if (reorder_index.has_value()) need(*reorder_index, torch::kInt16, "reorder_index", 1);
  if (KQ % 64 || KE % 64 || KE < 0 || KE > KQ || (reorder_index.has_value() && reorder_index->numel() != KQ) || absmax_slots.numel() == 0)
    throw std::runtime_error("Value error in reorder_quantize_x_dynamic: KQ / KE / reorder_index / absmax_slots are not valid");
  const int var = variant.is_none() ? arcq_variant_for_kq(KQ) : variant.cast<int>();
  same_device("reorder_quantize_x_dynamic", X, {opt_t(reorder_index), &absmax_slots});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  auto Q = torch::empty({M, K / 2}, X.options().dtype(torch::kUInt8));
  auto SF = torch::empty({arcq_sf_alloc_bytes(M, K)}, X.options().dtype(torch::kUInt8));
  auto scale = torch::empty({1}, X.options().dtype(torch::kFloat32));
  check(arcq_quantize_x_dyn_slots(X.data_ptr(), reorder_index.has_value() ? reorder_index->data_ptr<int16_t>() : nullptr, Q.data_ptr<uint8_t>(), SF.data_ptr<uint8_t>(),
                                  scale.data_ptr<float>(), (const uint32_t*)absmax_slots.data_ptr<int32_t>(), absmax_slots.numel(), M, KQ, KE, var, stream_of(X)),
        "reorder_quantize_x_dynamic");
  return {Q, SF, scale.reshape({})};
}

py::object kv_stub(const char* name) {
  return py::cpp_function([name](py::args, py::kwargs) -> py::object {
    PyErr_SetString(PyExc_NotImplementedError, (std::string("agemm.") + name + ": the int4 paged-KV attention is outside the ARC-NVFP4 GEMM hot path").c_str());
    throw py::error_already_set();
  });
}

// ---- MXFP4 (include/arcq.h "MXFP4"): the names and keywords of arcquant_amd/agemm.py's mx_* functions
std::tuple<torch::Tensor, torch::Tensor> mx_quantize(bool is_x, const torch::Tensor& X, const torch::Tensor& reorder_index, int64_t KE) {
  const char* who = is_x ? "mx_reorder_quantize_x" : "mx_reorder_quantize_w";
  need(X, torch::kBFloat16, is_x ? "X" : "W", 2);
  need(reorder_index, torch::kInt16, "reorder_index", 1);
  const int64_t rows = X.size(0), KQ = X.size(1), Kp = arcq_mx_k_padded(KQ + KE);
  if (reorder_index.numel() != KQ || KQ % 64 || KE % 64 || KE < 0 || KE > KQ || KQ > 32767)
    throw std::runtime_error(std::string("Value error in ") + who + ": KQ / KE / reorder_index are not valid");
  same_device(who, X, {&reorder_index});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  auto Q = torch::empty({rows, Kp / 2}, X.options().dtype(torch::kUInt8));
  auto SF = torch::empty({rows, Kp / 32}, X.options().dtype(torch::kUInt8));
  auto fn = is_x ? arcq_mx_quantize_x : arcq_mx_quantize_w;
  check(fn(X.data_ptr(), reorder_index.data_ptr<int16_t>(), Q.data_ptr<uint8_t>(), SF.data_ptr<uint8_t>(), rows, KQ, KE, stream_of(X)), who);
  return {Q, SF};
}

torch::Tensor mx_matmul(const torch::Tensor& A, const torch::Tensor& B, const torch::Tensor& SFA, const torch::Tensor& SFB, const py::object& scale,
                        const c10::optional<torch::Tensor>& bias, const c10::optional<torch::Tensor>& residual, py::object out_dtype,
                        const c10::optional<torch::Tensor>& out, double scale_host) {
  const char* who = "mx_matmul";
  need(A, torch::kUInt8, "A", 2);
  need(B, torch::kUInt8, "B", 2);
  need(SFA, torch::kUInt8, "SFA", 2);
  need(SFB, torch::kUInt8, "SFB", 2);
  const int64_t M = A.size(0), N = B.size(0), K = A.size(1) * 2;
  if (B.size(1) * 2 != K) throw std::runtime_error("agemm.mx_matmul: A and B disagree on K");
  if (K % 128 || N % 16) throw std::runtime_error("agemm.mx_matmul: K must be a multiple of 128 and N of 16");
  if (SFA.size(0) != M || SFA.size(1) != K / 32 || SFB.size(0) != N || SFB.size(1) != K / 32)
    throw std::runtime_error("agemm.mx_matmul: SFA / SFB must be [rows, K/32]");
  const OutDtype od = out_dtype_of(out_dtype, who);
  const Alpha al = alpha_of(scale, scale_host);
  torch::Tensor D = out_of(out, M, N, od.dt, A, who);
  const void* bp = opt_ptr(bias, torch::kBFloat16, "bias", {N});
  const void* rp = opt_ptr(residual, torch::kBFloat16, "residual", {M, N});
  same_device(who, A, {&B, &SFA, &SFB, al.tensor(), &D, opt_t(bias), opt_t(residual)});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
  check(arcq_gemm_mxfp4(A.data_ptr<uint8_t>(), B.data_ptr<uint8_t>(), SFA.data_ptr<uint8_t>(), SFB.data_ptr<uint8_t>(), D.data_ptr(), M, N, K, al.host, al.dev, bp, rp,
                        od.code, nullptr, 0, stream_of(A)),
        who);
  return D;
}

}  // namespace

PYBIND11_MODULE(agemm, m) {
  m.doc() = "ARC-NVFP4 hot path on MI355X (gfx950): drop-in for the reference's pybind11 module (kernels/src/bindings.cpp:551-575)";
  m.def("matmul", &matmul, py::arg("A"), py::arg("B"), py::arg("SFA"), py::arg("SFB"), py::arg("scale"));
  m.def("reorder_quantize_x", &reorder_quantize_x, py::arg("X"), py::arg("reorder_index"), py::arg("KE"));
  m.def("reorder_quantize_w", &reorder_quantize_w, py::arg("W"), py::arg("reorder_index"), py::arg("KE"));
  m.def("rmsnorm_quantize_x", &rmsnorm_quantize_x, py::arg("X"), py::arg("W"), py::arg("eps"), py::arg("reorder_index"), py::arg("KE"));
  // decode extensions (arcquant_amd/agemm.py has the same functions through ctypes, and more)
  m.def("repacked_supported", [](int64_t M, int64_t N, int64_t K) { return arcq_gemm_repacked_supported(M, N, K) != 0; });
  m.def("rw_route", [](int64_t M, int64_t N, int64_t K) { return arcq_gemm_rw_route(M, N, K); });
  m.def("fused_supported", [](int kind, int64_t M, int64_t N, int64_t KQ, int64_t KE) { return arcq_linear_fused_supported(kind, M, N, KQ, KE) != 0; });
  m.attr("SRC_RMSNORM") = ARCQ_SRC_RMSNORM;
  m.attr("SRC_DYNAMIC") = ARCQ_SRC_DYNAMIC;
  m.def("matmul_repacked", &matmul_repacked, py::arg("A"), py::arg("RW"), py::arg("SFA"), py::arg("RSF"), py::arg("scale"), py::arg("N"), py::kw_only(),
        py::arg("bias") = py::none(), py::arg("residual") = py::none(), py::arg("out_dtype") = py::none(), py::arg("out") = py::none(), py::arg("scale_host") = 1.0);
  m.def("matmul_rw", &matmul_rw, py::arg("A"), py::arg("RW"), py::arg("SFA"), py::arg("RSF"), py::arg("scale"), py::arg("N"), py::kw_only(),
        py::arg("bias") = py::none(), py::arg("residual") = py::none(), py::arg("out_dtype") = py::none(), py::arg("out") = py::none(), py::arg("scale_host") = 1.0);
  m.def("matmul_rw_silu_mul", &matmul_rw_silu_mul, py::arg("A"), py::arg("RW"), py::arg("SFA"), py::arg("RSF"), py::arg("scale"), py::arg("N"), py::kw_only(),
        py::arg("scale_host") = 1.0, py::arg("bias") = py::none());
  m.def("unrepack_w", &unrepack_w, py::arg("RW"), py::arg("RSF"), py::arg("N"), py::arg("K"));
  m.def("rmsnorm_matmul_repacked", &rmsnorm_matmul_repacked, py::arg("X"), py::arg("W"), py::arg("eps"), py::arg("reorder_index"), py::arg("KE"), py::arg("RW"),
        py::arg("RSF"), py::arg("scale"), py::arg("N"), py::kw_only(), py::arg("bias") = py::none(), py::arg("residual") = py::none(),
        py::arg("out_dtype") = py::none(), py::arg("out") = py::none(), py::arg("scale_host") = 1.0, py::arg("variant") = py::none());
  m.def("rmsnorm_matmul_repacked_silu", &rmsnorm_matmul_repacked_silu, py::arg("X"), py::arg("W"), py::arg("eps"), py::arg("reorder_index"), py::arg("KE"),
        py::arg("RW"), py::arg("RSF"), py::arg("scale"), py::arg("N"), py::kw_only(), py::arg("scale_host") = 1.0, py::arg("variant") = py::none(),
        py::arg("bias") = py::none(), py::arg("act_scatter_index") = py::none());
  m.def("dynamic_matmul_repacked", &dynamic_matmul_repacked, py::arg("X"), py::arg("reorder_index"), py::arg("KE"), py::arg("RW"), py::arg("RSF"), py::arg("scale_w"),
        py::arg("N"), py::kw_only(), py::arg("absmax_slots") = py::none(), py::arg("bias") = py::none(), py::arg("residual") = py::none(),
        py::arg("out_dtype") = py::none(), py::arg("out") = py::none(), py::arg("variant") = py::none());
  m.def("reorder_quantize_x_dynamic", &reorder_quantize_x_dynamic, py::arg("X"), py::arg("reorder_index"), py::arg("KE"), py::arg("variant") = py::none(),
        py::kw_only(), py::arg("absmax_slots"));
  m.def("mx_reorder_quantize_x", [](const torch::Tensor& X, const torch::Tensor& idx, int64_t KE) { return mx_quantize(true, X, idx, KE); }, py::arg("X"),
        py::arg("reorder_index"), py::arg("KE"));
  m.def("mx_reorder_quantize_w", [](const torch::Tensor& W, const torch::Tensor& idx, int64_t KE) { return mx_quantize(false, W, idx, KE); }, py::arg("W"),
        py::arg("reorder_index"), py::arg("KE"));
  m.def("mx_matmul", &mx_matmul, py::arg("A"), py::arg("B"), py::arg("SFA"), py::arg("SFB"), py::arg("scale"), py::kw_only(), py::arg("bias") = py::none(),
        py::arg("residual") = py::none(), py::arg("out_dtype") = py::none(), py::arg("out") = py::none(), py::arg("scale_host") = 1.0);
  for (const char* n : {"batch_decode_i4", "init_kv_i4", "append_kv_i4", "batch_decode_f16", "init_kv_f16", "append_kv_f16"}) m.attr(n) = kv_stub(n);
  m.attr("abi_version") = arcq_abi_version();
}
