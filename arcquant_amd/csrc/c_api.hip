// extern "C" entry points of libarcq_hip.so (declared in include/arcq.h): argument validation,
// dispatch between the GEMM kernels, error text.  No allocation, no synchronisation; the only state is the
// per-device record of LDS opt-ins already made (ensure_dynamic_lds) and the thread-local error text.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "arcq_device.hpp"
#include "arcq_internal.hpp"
#include "quantize_device.hpp"

namespace arcq {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int ensure_dynamic_lds(const void* kernel, LdsOptIn& cache, int bytes, const char* who) {
  if (bytes <= 48 * 1024) return ARCQ_OK;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(ARCQ_ERR_LAUNCH, "%s: hipGetDevice failed", who);
  const bool cached = dev >= 0 && dev < kMaxDevices;
  if (cached && __atomic_load_n(&cache.granted[dev], __ATOMIC_RELAXED) >= bytes) return ARCQ_OK;
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return fail(ARCQ_ERR_LAUNCH, "%s: cannot reserve %d B of LDS: %s", who, bytes, hipGetErrorString(e));
  if (cached) {     // keep the maximum: a smaller request after a larger one must not shrink the record
    int seen = __atomic_load_n(&cache.granted[dev], __ATOMIC_RELAXED);
    while (seen < bytes && !__atomic_compare_exchange_n(&cache.granted[dev], &seen, bytes, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  }
  return ARCQ_OK;
}

static const int64_t kSkinnyMaxM = 16;

static uintptr_t bits(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// bias / residual views the kernel's epilogue loads cannot take (align = 1: no rule)
static int check_epi_align(const char* who, const void* bias, const void* residual, int align) {
  if ((bits(bias) | bits(residual)) & (uintptr_t)(align - 1)) return fail(ARCQ_ERR_SHAPE, "%s: bias and residual must be %d-byte aligned", who, align);
  return ARCQ_OK;
}
// the decode epilogues fetch the four bias / residual values of an output quad with ONE 8-byte load when N % 4 == 0
static int repacked_epi_align(int64_t N) { return (N % 4) == 0 ? 8 : 1; }

int gemm_checks(const GemmRule& r, const void* A, const void* B, const void* SFA, const void* SFB, const void* D, const void* absmax_slots, int64_t M,
                int64_t N, int64_t K, const void* bias, const void* residual, int out_dtype) {
  if (M < 0 || N < 0 || K <= 0 || (K % r.k_mult) || (N % r.n_mult)) {
    if (r.n_mult == 1)
      return fail(ARCQ_ERR_SHAPE, "%s: need M,N >= 0 and K %% %d == 0 (M=%lld N=%lld K=%lld)", r.who, r.k_mult, (long long)M, (long long)N, (long long)K);
    return fail(ARCQ_ERR_SHAPE, "%s: need M,N >= 0, K %% %d == 0 and N %% %d == 0 (M=%lld N=%lld K=%lld)", r.who, r.k_mult, r.n_mult, (long long)M,
                (long long)N, (long long)K);
  }
  if (out_dtype != ARCQ_OUT_BF16 && out_dtype != ARCQ_OUT_F32) return fail(ARCQ_ERR_SHAPE, "%s: bad out_dtype %d", r.who, out_dtype);
  if (M == 0 || N == 0) return 1;                              // nothing to do
  if (r.prefill_only && M <= kSkinnyMaxM) return fail(ARCQ_ERR_UNSUPPORTED, "%s: %s", r.who, r.prefill_only);
  if ((!r.no_a && (!A || !SFA)) || !B || !SFB || !D || (r.slots && !absmax_slots)) return fail(ARCQ_ERR_NULL, "%s: NULL pointer", r.who);
  // (max_m == 0: the kernel's predicate bounds M, but only an M that survives the parameter blocks' int reaches it)
  if ((r.max_m ? (M > r.max_m || M * N > ((int64_t)1 << 40)) : M > INT32_MAX) || N > INT32_MAX / 2 || K > INT32_MAX / 2)
    return fail(ARCQ_ERR_UNSUPPORTED, "%s: shape too large", r.who);
  if (r.no_a) {
    if ((bits(B) | bits(D)) & 15) return fail(ARCQ_ERR_SHAPE, "%s: %s and %s must be 16-byte aligned", r.who, r.b, r.d);
    if (bits(SFB) & 3) return fail(ARCQ_ERR_SHAPE, "%s: %s must be 4-byte aligned", r.who, r.sfb);
    return check_epi_align(r.who, bias, residual, r.epi_align);
  }
  if ((bits(A) | bits(B) | bits(D)) & 15) return fail(ARCQ_ERR_SHAPE, "%s: A, %s and %s must be 16-byte aligned", r.who, r.b, r.d);
  if ((bits(SFA) | bits(SFB) | (r.slots ? bits(absmax_slots) : 0)) & 3)
    return fail(ARCQ_ERR_SHAPE, r.slots ? "%s: SFA, %s and absmax_slots must be 4-byte aligned" : "%s: SFA and %s must be 4-byte aligned", r.who, r.sfb);
  return check_epi_align(r.who, bias, residual, r.epi_align);
}

int quant_checks(const QuantRule& r, const QuantArgs& a) {
  const bool nv = r.family == kQuantNv, lin = r.family == kQuantMxLinear, mx = r.family == kQuantMx || r.family == kQuantMxFused || lin;
  if (r.layout && a.layout != ARCQ_GU_HALVES && a.layout != ARCQ_GU_PAIRS) return fail(ARCQ_ERR_SHAPE, "%s: unknown layout %d", r.who, a.layout);
  // pinned quirks: the dynamic entries report scale_out / state / slots ahead of the shape, and arcq_rmsnorm_quantize_x a misaligned norm weight
  if (r.dyn == kQuantState && (!a.scale_out || !a.dyn)) return fail(ARCQ_ERR_NULL, "%s: NULL scale_out / state", r.who);
  if (r.dyn == kQuantSlots && (!a.scale_out || !a.dyn || a.nslots <= 0 || a.nslots > INT32_MAX))
    return fail(ARCQ_ERR_NULL, "%s: NULL scale_out / absmax_slots, or no slots", r.who);
  if (nv && r.extra && a.rows > 0 && (bits(a.extra) & 15)) return fail(ARCQ_ERR_SHAPE, "%s: the norm weight must be 16-byte aligned", r.who);
  // KQ and KE in whole scale-factor atoms (64 elements = 4 groups): every size the reference dispatches (bindings.cpp:141-160), every
  // select_num it produces (multiples of 64) and every 64-aligned TP shard.  The kernels rely on it: the four lanes of a quad store the
  // four scale bytes of one aligned dword of the swizzled layout.
  const int64_t rows = r.x_alone && a.rows < 0 ? 0 : a.rows, rows_said = r.x_alone ? 0 : rows;
  if (rows < 0 || a.KQ <= 0 || (a.KQ % 64) || (a.KE % 64) || a.KE < 0 || a.KE > a.KQ || (!nv && (a.KQ < r.kq_min || a.KQ > r.kq_max))) {
    char range[48] = "";
    if (r.family == kQuantMxFused || (lin && r.extra)) snprintf(range, sizeof(range), ", %lld<=KQ<=%lld", (long long)r.kq_min, (long long)r.kq_max);
    else if (!nv) snprintf(range, sizeof(range), "<=%lld", (long long)r.kq_max);
    return fail(ARCQ_ERR_SHAPE, "%s: need KQ%%64==0, KE%%64==0, 0<=KE<=KQ%s (%s=%lld KQ=%lld KE=%lld)", r.who, range,
                r.family == kQuantNvContig ? "M" : "rows", (long long)rows_said, (long long)a.KQ, (long long)a.KE);
  }
  if (!mx && a.variant != ARCQ_VARIANT_G16 && a.variant != ARCQ_VARIANT_G32) return fail(ARCQ_ERR_SHAPE, "%s: unknown variant %d", r.who, a.variant);
  if (nv && a.KQ > 32767)   // int16 reorder_index (bindings.cpp:137)
    return fail(ARCQ_ERR_UNSUPPORTED, "%s: KQ=%lld does not fit an int16 reorder_index", r.who, (long long)a.KQ);
  if (nv && (a.KQ < r.kq_min || a.KQ > r.kq_max))   // the reduction tree of rmsnorm.cu:130-146 is defined for 128..512 threads
    return fail(ARCQ_ERR_UNSUPPORTED, "%s: KQ=%lld outside the reference's RMSNorm range [%lld, %lld]", r.who, (long long)a.KQ, (long long)r.kq_min,
                (long long)r.kq_max);
  if (rows == 0) return 1;                                     // nothing to do
  if (!a.X || (r.family != kQuantNvContig && !a.idx) || (!lin && (!a.Q || !a.SF)) || (r.extra && !a.extra)) return fail(ARCQ_ERR_NULL, "%s: NULL pointer", r.who);
  if (r.x_alone && (bits(a.X) & 15)) return fail(ARCQ_ERR_SHAPE, "%s: %s must be 16-byte aligned", r.who, r.x_alone);
  if (rows > INT32_MAX) return fail(ARCQ_ERR_UNSUPPORTED, "%s: too many rows", r.who);
  // 16-byte row / index loads; NVFP4: 8-byte code stores, 4-byte scale stores; MXFP4: 16-byte code stores (Kp/2 is a multiple of 64), scale bytes
  const bool in_bad = (bits(a.X) | bits(a.idx) | bits(a.extra)) & 15,
             out_bad = lin ? false : mx ? (bits(a.Q) & 15) != 0 : (bits(a.Q) & 7) || (bits(a.SF) & 3);
  static const char* const kAlignText[] = {"%s: X and reorder_index must be 16-byte aligned", "%s: X must be 16-byte, QX 8-byte and SFX 4-byte aligned",
                                           "%s: X, reorder_index and the packed output must be 16-byte aligned",
                                           "%s: the inputs, reorder_index and the packed output must be 16-byte aligned",
                                           "%s: X, the norm weight and reorder_index must be 16-byte aligned"};
  static_assert(sizeof(kAlignText) / sizeof(kAlignText[0]) == kQuantMxLinear + 1, "one text per family");
  // (kQuantMxLinear without a norm weight has X and reorder_index alone: kQuantNv's text)
  if (in_bad || (!nv && out_bad)) return fail(ARCQ_ERR_SHAPE, kAlignText[lin && !r.extra ? kQuantNv : r.family], r.who);
  if (out_bad) return fail(ARCQ_ERR_SHAPE, "%s: the packed output must be 8-byte and the scale buffer 4-byte aligned", r.who);
  return ARCQ_OK;
}

static GemmArgs gemm_args(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* D, int64_t M, int64_t N, int64_t K, float alpha_host,
                          const float* alpha_dev, const void* bias, const void* residual, int out_dtype, void* workspace, int64_t workspace_bytes) {
  GemmArgs a;
  a.A = A; a.B = B; a.SFA = SFA; a.SFB = SFB; a.D = D;
  a.M = (int)M; a.N = (int)N; a.K = (int)K;
  a.alpha_host = alpha_host; a.alpha_dev = alpha_dev; a.bias = (const uint16_t*)bias; a.residual = (const uint16_t*)residual; a.out_dtype = out_dtype;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes;
  return a;
}

}  // namespace arcq

using namespace arcq;

extern "C" {

int arcq_abi_version(void) { return ARCQ_ABI_VERSION; }
const char* arcq_last_error(void) { return g_err; }

// KQ-generic replacement of the closed switch in bindings.cpp:141-160: the reference routes
// {3584, 18944} to the 32-per-thread kernels and {27648, 28672} to the "down" kernels (same layout);
// every other size it supports uses the 16-per-thread layout, which is also our default elsewhere.
int arcq_variant_for_kq(int64_t KQ) {
  return (KQ == 3584 || KQ == 18944 || KQ == 27648 || KQ == 28672) ? ARCQ_VARIANT_G32 : ARCQ_VARIANT_G16;
}

int64_t arcq_sf_alloc_bytes(int64_t rows, int64_t K) { return (rows / 128 + 1) * 128 * K / 16; }   // bindings.cpp:83-95
int64_t arcq_sf_used_bytes(int64_t rows, int64_t K) { return ((rows + 127) / 128) * 128 * K / 16; }
int64_t arcq_sf_offset(int64_t row, int64_t pos, int64_t K) { return sf_offset(row, pos, K); }

int64_t arcq_primary_pos(int64_t g, int64_t KQ, int64_t KE, int variant) {
  const int64_t P = (KQ - KE) / 16;                          // the kernels' rule (quantize_device.hpp)
  return variant == ARCQ_VARIANT_G16 ? aug_group_pos<ARCQ_VARIANT_G16>(g, P) : aug_group_pos<ARCQ_VARIANT_G32>(g, P);
}
int64_t arcq_residual_pos(int64_t g, int64_t KQ, int64_t KE, int variant) {
  if (g < (KQ - KE) / 16) return -1;
  return arcq_primary_pos(g, KQ, KE, variant) + (variant == ARCQ_VARIANT_G16 ? aug_twin_step<ARCQ_VARIANT_G16> : aug_twin_step<ARCQ_VARIANT_G32>);
}

int arcq_quantize_x(const void* X, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE,
                    int variant, void* stream) {
  return quantize_x(X, reorder_index, QX, SFX, M, KQ, KE, variant, (hipStream_t)stream);
}

int arcq_quantize_w(const void* W, const int16_t* reorder_index, uint8_t* QW, uint8_t* SFW, int64_t N, int64_t KQ, int64_t KE,
                    int variant, void* stream) {
  return quantize_w(W, reorder_index, QW, SFW, N, KQ, KE, variant, (hipStream_t)stream);
}

int arcq_rmsnorm_quantize_x(const void* X, const void* W, float eps, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX,
                            int64_t M, int64_t KQ, int64_t KE, int variant, void* stream) {
  return rmsnorm_quantize_x(X, W, eps, reorder_index, QX, SFX, M, KQ, KE, variant, (hipStream_t)stream);
}

int arcq_quantize_x_dyn(const void* X, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX, float* scale_out, void* state,
                        int64_t M, int64_t KQ, int64_t KE, int variant, void* stream) {
  return quantize_x_dyn(X, reorder_index, QX, SFX, scale_out, state, M, KQ, KE, variant, (hipStream_t)stream);
}

int arcq_silu_mul_quantize_x_dyn(const void* GU, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX, float* scale_out, void* state,
                                 int64_t M, int64_t KQ, int64_t KE, int variant, int layout, void* stream) {
  return silu_mul_quantize_x_dyn(GU, reorder_index, QX, SFX, scale_out, state, M, KQ, KE, variant, layout, (hipStream_t)stream);
}

int arcq_absmax_scale(const void* X, int64_t n, float* scale_out, void* stream) {
  return absmax_scale(X, n, scale_out, (hipStream_t)stream);
}


// M <= 16: the 32-row-tile kernel needs enough tiles to occupy the chip without split-K (its tiles are twice as
// tall); below that the 16-row-tile kernel wins.  Measured crossover (tools/decode_bench.py, M=4, K=4160, us):
// N=4096 7.3 vs 9.3, N=5120 9.2 vs 8.5, N=8192 10.2 vs 9.5, N=14336 16.0 vs 14.6, N=37888 28.7 vs 23.9.
// ARCQ_DECODE=1|2 forces the 16-row / 32-row kernel (tuning).
static bool use_decode_v2(int64_t N) {
  static const int forced = env_int("ARCQ_DECODE", 0);
  if (forced == 1) return false;
  if (forced == 2) return true;
  return ((N + 127) / 128) * 4 >= 160;
}

int64_t arcq_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  if (tile_overlap_tail_forced(M, N)) return gemm_tile_workspace_bytes(M, N, K);      // (debug setter: whole 256 x 256 tiles take the LDS-tiled kernel)
  if (gemm_regtile_cfg(M, N, K, kEpiPlain)) return 0;
  if (M <= kSkinnyMaxM) return use_decode_v2(N) ? gemm_decode_workspace_bytes(M, N, K) : gemm_skinny_workspace_bytes(M, N, K);
  return gemm_tile_workspace_bytes(M, N, K);
}

int arcq_gemm_nvfp4(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* D, int64_t M, int64_t N,
                    int64_t K, float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  GemmRule r{"arcq_gemm_nvfp4"};
  const int rc = gemm_checks(r, A, B, SFA, SFB, D, nullptr, M, N, K, bias, residual, out_dtype);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  const GemmArgs a = gemm_args(A, B, SFA, SFB, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, workspace, workspace_bytes);
  if (tile_overlap_tail_forced(M, N)) return gemm_tile(a, (hipStream_t)stream);
  if (const int cfg = gemm_regtile_cfg(M, N, K, kEpiPlain)) return gemm_regtile(a, cfg, (hipStream_t)stream);
  if (M <= kSkinnyMaxM) return use_decode_v2(N) ? gemm_decode(a, (hipStream_t)stream) : gemm_skinny(a, (hipStream_t)stream);
  return gemm_tile(a, (hipStream_t)stream);
}

int64_t arcq_gemm_silu_mul_slots(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return M <= kSkinnyMaxM ? gemm_decode_silu_slots(M, N, K) : gemm_tile_silu_slots(M, N, K);
}

int arcq_gemm_nvfp4_silu_mul(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* ACT, uint32_t* absmax_slots,
                             int64_t M, int64_t N, int64_t K, float alpha_host, const float* alpha_dev, const void* bias, void* stream) {
  GemmRule r{"arcq_gemm_nvfp4_silu_mul"};
  r.n_mult = 8; r.d = "ACT"; r.slots = true;
  const int rc = gemm_checks(r, A, B, SFA, SFB, ACT, absmax_slots, M, N, K, nullptr, nullptr, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  GemmArgs a = gemm_args(A, B, SFA, SFB, ACT, M, N, K, alpha_host, alpha_dev, bias, nullptr, ARCQ_OUT_BF16, nullptr, 0);
  a.epilogue = kEpiSiluMul; a.absmax_slots = absmax_slots;
  if (bias && M <= kSkinnyMaxM) return fail(ARCQ_ERR_UNSUPPORTED, "%s: bias is supported by the tile kernel only (M > 16); decode uses arcq_linear_rmsnorm_silu_repacked", r.who);
  // the 16-row decode kernel has no fused epilogue: every M <= 16 shape takes the 32-row kernel here
  if (M <= kSkinnyMaxM) return gemm_decode(a, (hipStream_t)stream);
  return gemm_tile(a, (hipStream_t)stream);
}

int arcq_quantize_x_dyn_slots(const void* X, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX, float* scale_out,
                              const uint32_t* absmax_slots, int64_t nslots, int64_t M, int64_t KQ, int64_t KE, int variant, void* stream) {
  return quantize_x_dyn_slots(X, reorder_index, QX, SFX, scale_out, absmax_slots, nslots, M, KQ, KE, variant, (hipStream_t)stream);
}

int64_t arcq_repacked_w_bytes(int64_t N, int64_t K) { return (N > 0 && K > 0) ? gemm_repacked_w_bytes(N, K) : 0; }
int64_t arcq_repacked_sf_bytes(int64_t N, int64_t K) { return (N > 0 && K > 0) ? gemm_repacked_sf_bytes(N, K) : 0; }
int arcq_gemm_repacked_supported(int64_t M, int64_t N, int64_t K) { return gemm_repacked_supported(M, N, K); }

static int gemm_repacked_entry(bool via_stream, const char* who, const uint8_t* A, const uint8_t* RW, const uint8_t* SFA, const uint8_t* RSF, void* D, int64_t M, int64_t N,
                             int64_t K, float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype,
                             void* stream) {
  GemmRule r{who};
  r.max_m = 0; r.b = "RW"; r.sfb = "RSF"; r.epi_align = repacked_epi_align(N);
  const int rc = gemm_checks(r, A, RW, SFA, RSF, D, nullptr, M, N, K, bias, residual, out_dtype);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  const GemmArgs a = gemm_args(A, nullptr, SFA, nullptr, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, nullptr, 0);
  return via_stream ? gemm_repacked_stream(a, RW, RSF, (hipStream_t)stream) : gemm_repacked(a, RW, RSF, (hipStream_t)stream);
}

int arcq_gemm_nvfp4_repacked(const uint8_t* A, const uint8_t* RW, const uint8_t* SFA, const uint8_t* RSF, void* D, int64_t M, int64_t N,
                             int64_t K, float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype,
                             void* stream) {
  return gemm_repacked_entry(false, "arcq_gemm_nvfp4_repacked", A, RW, SFA, RSF, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, stream);
}
int arcq_gemm_nvfp4_repacked_stream(const uint8_t* A, const uint8_t* RW, const uint8_t* SFA, const uint8_t* RSF, void* D, int64_t M, int64_t N,
                                    int64_t K, float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype,
                                    void* stream) {
  return gemm_repacked_entry(true, "arcq_gemm_nvfp4_repacked_stream", A, RW, SFA, RSF, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, stream);
}

int arcq_gemm_nvfp4_repacked_silu_absmax(const uint8_t* A, const uint8_t* RW, const uint8_t* SFA, const uint8_t* RSF, void* D,
                                         uint32_t* absmax_slots, int64_t M, int64_t N, int64_t K, float alpha_host, const float* alpha_dev,
                                         void* stream) {
  GemmRule r{"arcq_gemm_nvfp4_repacked_silu_absmax"};
  r.n_mult = 4; r.max_m = 0; r.b = "RW"; r.sfb = "RSF"; r.slots = true;
  const int rc = gemm_checks(r, A, RW, SFA, RSF, D, absmax_slots, M, N, K, nullptr, nullptr, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  GemmArgs a = gemm_args(A, nullptr, SFA, nullptr, D, M, N, K, alpha_host, alpha_dev, nullptr, nullptr, ARCQ_OUT_BF16, nullptr, 0);
  a.epilogue = kEpiSiluMul; a.absmax_slots = absmax_slots;
  return gemm_repacked(a, RW, RSF, (hipStream_t)stream);
}

// ---- one weight copy for every M: arcq_gemm_nvfp4's contract over the repacked weight (RW, RSF) -----------------------------------------
// Route 1 = the repacked decode kernels (exactly arcq_gemm_nvfp4_repacked); otherwise the RW instantiation of the kernel and configuration
// arcq_gemm_nvfp4 would take (route 2 = register-tiled, 3 = LDS-tiled: bit-identical to it), except where that is an LDS-transposing decode
// kernel (gemm_skinny / gemm_decode): those shapes take the register-tiled 16 x 16 configuration (id 9), also as route 2.
static const int kRwDecodeCfg = 9;

static int rw_route(int64_t M, int64_t N, int64_t K, bool epi_aligned, int* cfg) {
  *cfg = 0;
  if (M <= 0 || N <= 0 || K <= 0 || (K % 64) || M > INT32_MAX / 2 || N > INT32_MAX / 2 || K > INT32_MAX / 2 || M * N > ((int64_t)1 << 40)) return 0;
  if (tile_overlap_tail_forced(M, N)) return 3;
  if (epi_aligned && gemm_repacked_supported(M, N, K)) return 1;
  *cfg = gemm_regtile_cfg(M, N, K, kEpiPlain);
  if (*cfg == 0 && M <= kSkinnyMaxM) *cfg = kRwDecodeCfg;
  if (*cfg) return gemm_regtile_fits(M, N, K, kBRepacked) ? 2 : 0;
  return 3;
}

int arcq_gemm_rw_route(int64_t M, int64_t N, int64_t K) {
  int cfg;
  return rw_route(M, N, K, true, &cfg);
}

int64_t arcq_gemm_rw_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  int cfg;       // (a route-1 shape takes route 2 or 3 with a misaligned bias / residual view: size for that)
  return rw_route(M, N, K, false, &cfg) == 3 ? gemm_tile_workspace_bytes(M, N, K) : 0;
}

int arcq_gemm_nvfp4_rw(const uint8_t* A, const uint8_t* RW, const uint8_t* SFA, const uint8_t* RSF, void* D, int64_t M, int64_t N, int64_t K,
                       float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  GemmRule r{"arcq_gemm_nvfp4_rw"};
  r.b = "RW"; r.sfb = "RSF";
  const int rc = gemm_checks(r, A, RW, SFA, RSF, D, nullptr, M, N, K, nullptr, nullptr, out_dtype);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  // the repacked decode kernels reject bias / residual views that are not 8-byte aligned: those calls take route 2 / 3
  const bool epi_aligned = ((bits(bias) | bits(residual)) & 7) == 0;
  int cfg;
  const int route = rw_route(M, N, K, epi_aligned, &cfg);
  if (route == 1) return arcq_gemm_nvfp4_repacked(A, RW, SFA, RSF, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, stream);
  if (route == 0) return fail(ARCQ_ERR_UNSUPPORTED, "%s: the repacked weight of N=%lld K=%lld exceeds the register-tiled kernel's 32-bit offsets", r.who,
                              (long long)N, (long long)K);
  GemmArgs a = gemm_args(A, RW, SFA, RSF, D, M, N, K, alpha_host, alpha_dev, bias, residual, out_dtype, workspace, workspace_bytes);
  a.b_layout = kBRepacked;
  if (route == 2) return gemm_regtile(a, cfg, (hipStream_t)stream);
  return gemm_tile(a, (hipStream_t)stream);
}

int64_t arcq_gemm_rw_silu_mul_slots(int64_t M, int64_t N, int64_t K) {
  if (M <= kSkinnyMaxM || N <= 0 || K <= 0) return 0;
  return gemm_tile_silu_slots(M, N, K);
}

int arcq_gemm_nvfp4_rw_silu_mul(const uint8_t* A, const uint8_t* RW, const uint8_t* SFA, const uint8_t* RSF, void* ACT, uint32_t* absmax_slots,
                                int64_t M, int64_t N, int64_t K, float alpha_host, const float* alpha_dev, const void* bias, void* stream) {
  GemmRule r{"arcq_gemm_nvfp4_rw_silu_mul"};
  r.n_mult = 8; r.b = "RW"; r.sfb = "RSF"; r.d = "ACT"; r.slots = true;
  r.prefill_only = "M <= 16 is decode: use arcq_gemm_nvfp4_repacked_silu_absmax or arcq_linear_rmsnorm_silu_repacked";
  const int rc = gemm_checks(r, A, RW, SFA, RSF, ACT, absmax_slots, M, N, K, nullptr, nullptr, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  GemmArgs a = gemm_args(A, RW, SFA, RSF, ACT, M, N, K, alpha_host, alpha_dev, bias, nullptr, ARCQ_OUT_BF16, nullptr, 0);
  a.epilogue = kEpiSiluMul; a.absmax_slots = absmax_slots;
  a.b_layout = kBRepacked;
  return gemm_tile(a, (hipStream_t)stream);
}

int arcq_linear_fused_supported(int kind, int64_t M, int64_t N, int64_t KQ, int64_t KE) { return gemm_fused_supported(kind, M, N, KQ, KE); }

static int fused_common_checks(const char* who, const void* X, const int16_t* idx, const uint8_t* RW, const uint8_t* RSF, void* D, int64_t M,
                               int64_t N, int64_t KQ, int64_t KE, int variant, int out_dtype) {
  if (M < 0 || N < 0 || KQ <= 0 || (KQ % 64) || (KE % 64) || KE < 0 || KE > KQ)
    return fail(ARCQ_ERR_SHAPE, "%s: need M,N >= 0, KQ%%64==0, KE%%64==0, 0<=KE<=KQ (M=%lld N=%lld KQ=%lld KE=%lld)", who, (long long)M,
                (long long)N, (long long)KQ, (long long)KE);
  if (variant != ARCQ_VARIANT_G16 && variant != ARCQ_VARIANT_G32) return fail(ARCQ_ERR_SHAPE, "%s: unknown variant %d", who, variant);
  if (out_dtype != ARCQ_OUT_BF16 && out_dtype != ARCQ_OUT_F32) return fail(ARCQ_ERR_SHAPE, "%s: bad out_dtype %d", who, out_dtype);
  if (M == 0 || N == 0) return 1;                              // nothing to do
  if (!X || !idx || !RW || !RSF || !D) return fail(ARCQ_ERR_NULL, "%s: NULL pointer", who);
  if (M > INT32_MAX || N > INT32_MAX / 2 || KQ > 32767) return fail(ARCQ_ERR_UNSUPPORTED, "%s: shape too large", who);
  if ((bits(X) | bits(idx) | bits(RW) | bits(D)) & 15)
    return fail(ARCQ_ERR_SHAPE, "%s: X, reorder_index, RW and D must be 16-byte aligned", who);
  if (bits(RSF) & 3) return fail(ARCQ_ERR_SHAPE, "%s: RSF must be 4-byte aligned", who);
  return ARCQ_OK;
}

int arcq_linear_rmsnorm_repacked(const void* X, const void* Wn, float eps, const int16_t* reorder_index, const uint8_t* RW, const uint8_t* RSF,
                                 void* D, int64_t M, int64_t N, int64_t KQ, int64_t KE, int variant, float alpha_host, const float* alpha_dev,
                                 const void* bias, const void* residual, int out_dtype, void* stream) {
  const char* who = "arcq_linear_rmsnorm_repacked";
  const int rc = fused_common_checks(who, X, reorder_index, RW, RSF, D, M, N, KQ, KE, variant, out_dtype);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  if (!Wn || (bits(Wn) & 15)) return fail(Wn ? ARCQ_ERR_SHAPE : ARCQ_ERR_NULL, "%s: the norm weight must be a 16-byte aligned pointer", who);
  if (const int e = check_epi_align(who, bias, residual, repacked_epi_align(N))) return e;
  FusedArgs f{};
  f.kind = ARCQ_SRC_RMSNORM; f.X = (const uint16_t*)X; f.Wn = (const uint16_t*)Wn; f.eps = eps; f.idx = reorder_index;
  f.RW = RW; f.RSF = RSF; f.D = D; f.M = (int)M; f.N = (int)N; f.KQ = (int)KQ; f.KE = (int)KE; f.variant = variant;
  f.alpha_host = alpha_host; f.alpha_dev = alpha_dev; f.bias = (const uint16_t*)bias; f.residual = (const uint16_t*)residual; f.out_dtype = out_dtype;
  return gemm_fused(f, (hipStream_t)stream);
}

int arcq_linear_rmsnorm_silu_repacked(const void* X, const void* Wn, float eps, const int16_t* reorder_index, const uint8_t* RW,
                                      const uint8_t* RSF, void* ACT, uint32_t* absmax_slots, int64_t M, int64_t N, int64_t KQ, int64_t KE,
                                      int variant, float alpha_host, const float* alpha_dev, const void* bias, const int16_t* act_scatter_index,
                                      void* stream) {
  const char* who = "arcq_linear_rmsnorm_silu_repacked";
  const int rc = fused_common_checks(who, X, reorder_index, RW, RSF, ACT, M, N, KQ, KE, variant, ARCQ_OUT_BF16);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  if (N % 4) return fail(ARCQ_ERR_SHAPE, "%s: N %% 4 != 0 (interleaved gate|up rows)", who);
  if (!Wn || !absmax_slots) return fail(ARCQ_ERR_NULL, "%s: NULL norm weight / absmax_slots", who);
  if ((bits(Wn) & 15) || (bits(absmax_slots) & 3)) return fail(ARCQ_ERR_SHAPE, "%s: misaligned norm weight / absmax_slots", who);
  if (bits(act_scatter_index) & 3) return fail(ARCQ_ERR_SHAPE, "%s: misaligned act_scatter_index", who);
  if (bits(bias) & 7) return fail(ARCQ_ERR_SHAPE, "%s: bias must be 8-byte aligned", who);
  FusedArgs f{};
  f.act_scatter = act_scatter_index;
  f.kind = ARCQ_SRC_RMSNORM; f.silu_act = 1; f.X = (const uint16_t*)X; f.Wn = (const uint16_t*)Wn; f.eps = eps; f.idx = reorder_index;
  f.RW = RW; f.RSF = RSF; f.D = ACT; f.out_slots = absmax_slots; f.M = (int)M; f.N = (int)N; f.KQ = (int)KQ; f.KE = (int)KE; f.variant = variant;
  f.alpha_host = alpha_host; f.alpha_dev = alpha_dev; f.bias = (const uint16_t*)bias; f.out_dtype = ARCQ_OUT_BF16;
  return gemm_fused(f, (hipStream_t)stream);
}

int arcq_linear_dynamic_repacked(const void* X, const int16_t* reorder_index, const uint8_t* RW, const uint8_t* RSF, void* D, float* scale_out,
                                 const uint32_t* absmax_slots, int64_t nslots, int64_t M, int64_t N, int64_t KQ, int64_t KE, int variant,
                                 float alpha_host, const void* bias, const void* residual, int out_dtype, void* stream) {
  const char* who = "arcq_linear_dynamic_repacked";
  const int rc = fused_common_checks(who, X, reorder_index, RW, RSF, D, M, N, KQ, KE, variant, out_dtype);
  if (rc != ARCQ_OK) return rc < 0 ? rc : ARCQ_OK;
  if (absmax_slots && (nslots <= 0 || nslots > INT32_MAX || (bits(absmax_slots) & 3)))
    return fail(ARCQ_ERR_SHAPE, "%s: absmax_slots given but nslots = %lld, or misaligned", who, (long long)nslots);
  if (const int e = check_epi_align(who, bias, residual, repacked_epi_align(N))) return e;
  FusedArgs f{};
  f.kind = ARCQ_SRC_DYNAMIC; f.X = (const uint16_t*)X; f.idx = reorder_index; f.in_slots = absmax_slots; f.n_in_slots = absmax_slots ? (int)nslots : 0;
  f.scale_out = scale_out; f.RW = RW; f.RSF = RSF; f.D = D; f.M = (int)M; f.N = (int)N; f.KQ = (int)KQ; f.KE = (int)KE; f.variant = variant;
  f.alpha_host = alpha_host; f.bias = (const uint16_t*)bias; f.residual = (const uint16_t*)residual; f.out_dtype = out_dtype;
  return gemm_fused(f, (hipStream_t)stream);
}

int arcq_silu_mul_quantize_x_dyn_slots(const void* GU, const int16_t* reorder_index, uint8_t* QX, uint8_t* SFX, float* scale_out,
                                       const uint32_t* absmax_slots, int64_t nslots, int64_t M, int64_t KQ, int64_t KE, int variant,
                                       int layout, void* stream) {
  return silu_mul_quantize_x_dyn_slots(GU, reorder_index, QX, SFX, scale_out, absmax_slots, nslots, M, KQ, KE, variant, layout, (hipStream_t)stream);
}

}  // extern "C"
