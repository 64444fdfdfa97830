// Internal declarations shared by the translation units of libarcq_hip.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/arcq.h"

namespace arcq {

// Records a formatted message for arcq_last_error() (thread-local) and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// A tuning knob: the integer value of environment variable `name`, or `dflt` when it is unset.  Callers keep the result in a
// function-local static, so each knob is read once per process.
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// Opt-in to more than 48 KB of dynamic LDS for `kernel` on the CURRENT device (returns at once for less).  The attribute is per
// device and per kernel, and the driver call costs host time, so launch_kernel keeps one LdsOptIn per kernel instantiation: a
// small per-device table of the largest size already granted (relaxed atomics: two threads racing both make the same,
// idempotent driver call).  Returns ARCQ_OK or ARCQ_ERR_LAUNCH (message recorded).
constexpr int kMaxDevices = 64;
struct LdsOptIn {
  int granted[kMaxDevices];     // zero-initialised (static storage)
};
int ensure_dynamic_lds(const void* kernel, LdsOptIn& cache, int bytes, const char* who);

// Dynamic LDS of a launch.  `optin` is what the kernel is opted in for: the launch's own size, or the largest size the
// instantiation can ever need (one driver call per device, ever).
struct LdsBytes {
  int launch, optin;
  LdsBytes(int bytes) : launch(bytes), optin(bytes) {}
  LdsBytes(int bytes, int most) : launch(bytes), optin(most) {}
};

// The one way a kernel of this library is launched: LDS opt-in, launch, error check.  The kernel is a template argument, so the
// opt-in record is per kernel instantiation by construction.  Returns ARCQ_OK or ARCQ_ERR_LAUNCH ("<who>: launch failed: ...").
template <auto Kernel, typename... Args>
int launch_kernel(dim3 grid, dim3 block, LdsBytes lds, hipStream_t stream, const char* who, const Args&... args) {
  static LdsOptIn opted;
  if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(Kernel), opted, lds.optin, who)) return rc;
  hipLaunchKernelGGL(Kernel, grid, block, lds.launch, stream, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ARCQ_ERR_LAUNCH, "%s: launch failed: %s", who, hipGetErrorString(e));
  return ARCQ_OK;
}

// c_api.hip: the argument checks of a GEMM-shaped entry point (host only), parameterised by what differs between entry points.
struct GemmRule {
  const char* who;
  int k_mult = 64, n_mult = 1;          // K % k_mult == 0 and N % n_mult == 0
  int64_t max_m = INT32_MAX / 2;        // with M * N <= 2^40; 0: the kernel's `supported` predicate bounds M later
  const char *b = "B", *sfb = "SFB", *d = "D";   // operand names in the alignment messages
  bool slots = false;                   // takes absmax_slots (non-NULL, 4-byte aligned)
  int epi_align = 1;                    // bias and residual alignment in bytes
  const char* prefill_only = nullptr;   // set: M <= 16 is ARCQ_ERR_UNSUPPORTED with this text, reported before a NULL pointer
  bool no_a = false;                    // the fused linears: the activation operand is the quantiser's, A / SFA are neither required nor named
};
// In the order every entry point reports them: divisibility, out_dtype, empty shape (returns 1: nothing to do), prefill_only, NULL, size
// limits, 16-byte operands, 4-byte operands, bias / residual.  Returns ARCQ_OK to go on or the recorded failure; no HIP call.
int gemm_checks(const GemmRule& r, const void* A, const void* B, const void* SFA, const void* SFB, const void* D, const void* absmax_slots, int64_t M,
                int64_t N, int64_t K, const void* bias, const void* residual, int out_dtype);

// c_api.hip: the argument checks of a quantiser entry point (host only), parameterised by what differs between entry points.
// `family` selects the pinned texts, the output alignments and where the KQ range is reported:
//   kQuantNv       NVFP4 rows: variant checked; KQ > 32767 and a KQ outside [kq_min, kq_max] are ARCQ_ERR_UNSUPPORTED, after the variant;
//                  X / reorder_index 16-byte, then QX 8-byte and SFX 4-byte, in two messages
//   kQuantNvContig arcq_quantize_x_dyn_slots with reorder_index == NULL: no index; the KQ range is part of the shape fault
//   kQuantMx       MXFP4 rows: no variant; the range is part of the shape fault; X, reorder_index, QX 16-byte, SFX unaligned
//   kQuantMxFused  MXFP4 fused sources: as kQuantMx, the range spelled out in the text, `extra` among the 16-byte inputs
//   kQuantMxLinear the prologue of the MXFP4 fused linears: kQuantMxFused with `extra`, kQuantMx without; no outputs (Q / SF are neither
//                  required nor named)
enum : int { kQuantNv = 0, kQuantNvContig = 1, kQuantMx = 2, kQuantMxFused = 3, kQuantMxLinear = 4 };
enum : int { kQuantStatic = 0, kQuantState = 1, kQuantSlots = 2 };
struct QuantRule {
  const char* who;
  int family = kQuantNv;
  int64_t kq_min = 64, kq_max = 32767;  // (kQuantNv: the RMSNorm range when narrower)
  bool extra = false;                   // takes a further 16-byte input, the norm weight
  int dyn = kQuantStatic;               // kQuantState: scale_out and state required; kQuantSlots: scale_out, absmax_slots and 0 < nslots <= INT32_MAX
  bool layout = false;                  // takes a gate|up layout
  const char* x_alone = nullptr;        // the three dynamic entries that once validated through a rows = 0 call of the static one, pinned:
                                        // the shape fault says rows=0, M < 0 is empty, and X (under this name) is reported alone ahead of
                                        // the row limit
};
struct QuantArgs {
  const void *X, *extra, *idx, *Q, *SF;
  int64_t rows, KQ, KE;
  int variant = ARCQ_VARIANT_G16, layout = ARCQ_GU_HALVES;
  const void *scale_out = nullptr, *dyn = nullptr;   // dyn: state or absmax_slots
  int64_t nslots = 0;
};
// In the order every entry point reports them: layout, scale_out / state / slots, (kQuantNv) misaligned norm weight, shape, variant,
// KQ limits, empty input (returns 1: nothing to do), NULL, x_alone, row limit, alignment.  Returns ARCQ_OK to go on or the recorded
// failure; no HIP call.
int quant_checks(const QuantRule& r, const QuantArgs& a);

// The grid of every row quantiser: grid.x = one workgroup per row (grid-strided beyond kMaxQuantBlocks = 256 CUs x 8 resident workgroups);
// few rows (decode): each row is also split over up to 16 workgroups (grid.y) of >= 32 units -- 16-element groups or 32-element blocks --
// so that the chip is not idle
constexpr int kMaxQuantBlocks = 2048;
inline dim3 quant_grid(int64_t rows, int64_t units) {
  const int g = (int)(rows < kMaxQuantBlocks ? rows : kMaxQuantBlocks);
  int s = 1;
  while (g * s < 256 && s < 16 && units / (s * 2) >= 32) s *= 2;
  return dim3(g, s);
}

// quantize.hip
int quantize_x(const void* X, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE, int variant,
               hipStream_t stream);
int quantize_w(const void* W, const int16_t* idx, uint8_t* QW, uint8_t* SFW, int64_t N, int64_t KQ, int64_t KE, int variant,
               hipStream_t stream);
int rmsnorm_quantize_x(const void* X, const void* Wn, float eps, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M,
                       int64_t KQ, int64_t KE, int variant, hipStream_t stream);
int absmax_scale(const void* X, int64_t n, float* scale_out, hipStream_t stream);
int quantize_x_dyn(const void* X, const int16_t* idx, uint8_t* QX, uint8_t* SFX, float* scale_out, void* state, int64_t M,
                   int64_t KQ, int64_t KE, int variant, hipStream_t stream);
int quantize_x_dyn_slots(const void* X, const int16_t* idx, uint8_t* QX, uint8_t* SFX, float* scale_out, const uint32_t* slots,
                         int64_t nslots, int64_t M, int64_t KQ, int64_t KE, int variant, hipStream_t stream);
int silu_mul_quantize_x_dyn_slots(const void* GU, const int16_t* idx, uint8_t* QX, uint8_t* SFX, float* scale_out, const uint32_t* slots,
                                  int64_t nslots, int64_t M, int64_t KQ, int64_t KE, int variant, int layout, hipStream_t stream);
int silu_mul_quantize_x_dyn(const void* GU, const int16_t* idx, uint8_t* QX, uint8_t* SFX, float* scale_out, void* state, int64_t M,
                            int64_t KQ, int64_t KE, int variant, int layout, hipStream_t stream);

// quantize_mx.hip / gemm_mx.hip: the MXFP4 path (arcq.h "MXFP4"); K of gemm_mx is the padded K of the operands
int mx_quantize_x(const void* X, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE, hipStream_t stream);
int mx_quantize_w(const void* W, const int16_t* idx, uint8_t* QW, uint8_t* SFW, int64_t N, int64_t KQ, int64_t KE, hipStream_t stream);
int gemm_mx(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* D, int64_t M, int64_t N, int64_t Kp,
            float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, hipStream_t stream);
int mx_rmsnorm_quantize_x(const void* X, const void* Wn, float eps, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ,
                          int64_t KE, hipStream_t stream);
int mx_silu_mul_quantize_x(const void* GU, const int16_t* idx, uint8_t* QX, uint8_t* SFX, int64_t M, int64_t KQ, int64_t KE, int layout,
                           hipStream_t stream);
int gemm_mx_silu_mul(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, void* ACT, int64_t M, int64_t N, int64_t Kp,
                     float alpha_host, const float* alpha_dev, const void* bias, hipStream_t stream);
int gemm_mx_silu_mul_quantize(const uint8_t* A, const uint8_t* B, const uint8_t* SFA, const uint8_t* SFB, uint8_t* QACT, uint8_t* SFACT, int64_t M,
                              int64_t N, int64_t Kp, float alpha_host, const float* alpha_dev, const void* bias, int64_t KE, hipStream_t stream);
// gemm_mx_rw.hip: M <= 64 over the MXFP4 repacked weight (arcq.h "MXFP4 repacked weight"); the sums are gemm_mx's, bit for bit
int64_t gemm_mx_repacked_w_bytes(int64_t N, int64_t Kp);
int64_t gemm_mx_repacked_sf_bytes(int64_t N, int64_t Kp);
int gemm_mx_repacked_supported(int64_t M, int64_t N, int64_t Kp);
int gemm_mx_repacked(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t Kp,
                     float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, hipStream_t stream);
int gemm_mx_repacked_silu_mul(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* ACT, int64_t M, int64_t N,
                              int64_t Kp, float alpha_host, const float* alpha_dev, const void* bias, hipStream_t stream);
// gemm_mx_linear_rw.hip: the MXFP4 fused decode linear (arcq.h "MXFP4 fused decode linear"); kind = ARCQ_SRC_RMSNORM | ARCQ_SRC_PLAIN
int64_t gemm_mx_linear_lds_bytes(int kind, int64_t KQ, int64_t KE);
int gemm_mx_linear_supported(int kind, int64_t M, int64_t N, int64_t KQ, int64_t KE);
int64_t gemm_mx_linear_workgroups(int kind, int64_t N, int64_t KQ, int64_t KE);
int gemm_mx_linear(int kind, bool silu, const void* X, const void* Wn, float eps, const int16_t* idx, const uint8_t* MRW, const uint8_t* MRSF, void* D,
                   int64_t M, int64_t N, int64_t KQ, int64_t KE, float alpha_host, const float* alpha_dev, const void* bias, const void* residual,
                   int out_dtype, const char* who, hipStream_t stream);
// gemm_mx_tile_rw.hip (M > 64, the tile kernel over MRW / MRSF) and gemm_mx_slice_rw.hip (the quantising kernel for M <= 64): every
// M >= 1 over the repacked weight alone; the results are gemm_mx's, gemm_mx_silu_mul's and gemm_mx_silu_mul_quantize's, bit for bit
int gemm_mx_rw_route(int64_t M, int64_t N, int64_t Kp);   // 1: the decode kernels, 2: the tile kernel, 0: no such shape
int gemm_mx_rw(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* D, int64_t M, int64_t N, int64_t Kp,
               float alpha_host, const float* alpha_dev, const void* bias, const void* residual, int out_dtype, hipStream_t stream);
int gemm_mx_rw_silu_mul(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, void* ACT, int64_t M, int64_t N, int64_t Kp,
                        float alpha_host, const float* alpha_dev, const void* bias, hipStream_t stream);
int gemm_mx_rw_silu_mul_quantize(const uint8_t* A, const uint8_t* MRW, const uint8_t* SFA, const uint8_t* MRSF, uint8_t* QACT, uint8_t* SFACT,
                                 int64_t M, int64_t N, int64_t Kp, float alpha_host, const float* alpha_dev, const void* bias, int64_t KE,
                                 hipStream_t stream);

// gemm_skinny.hip / gemm_tile.hip
struct GemmArgs {
  const uint8_t* A;     // [M, K/2]
  const uint8_t* B;     // [N, K/2]
  const uint8_t* SFA;   // swizzled ue4m3
  const uint8_t* SFB;
  void* D;              // [M, N] bf16 or fp32
  int M, N, K;
  float alpha_host;
  const float* alpha_dev;   // optional device scalar multiplied into alpha
  const uint16_t* bias;     // optional bf16 [N]
  const uint16_t* residual; // optional bf16 [M, N], added after the bf16 rounding of alpha*acc (+bias)
  int out_dtype;
  void* workspace;
  int64_t workspace_bytes;
  int epilogue = 0;                  // kEpiPlain, or kEpiSiluMul: D = bf16 [M, N/2] silu(gate)*up of interleaved weight rows
  unsigned int* absmax_slots = nullptr;   // kEpiSiluMul: one max|D| word per workgroup / tile (see gemm_silu_slots)
  int b_layout = 0;                  // kBRef: B / SFB in the reference layout; kBRepacked: B / SFB = RW / RSF of arcq.h (tile, regtile)
};
// The GemmArgs fields that every GEMM kernel's parameter block carries under the same names.  The weight operand stays with the
// caller: B / SFB in some blocks, RW / RSF in others.
template <typename Params>
void copy_gemm_fields(Params& p, const GemmArgs& a) {
  p.A = a.A; p.SFA = a.SFA; p.D = a.D;
  p.alpha_dev = a.alpha_dev; p.bias = a.bias; p.residual = a.residual;
  p.M = a.M; p.N = a.N; p.K = a.K; p.alpha_host = a.alpha_host; p.out_dtype = a.out_dtype;
}
enum : int { kEpiPlain = 0, kEpiSiluMul = 1 };
enum : int { kBRef = 0, kBRepacked = 1 };
int64_t gemm_silu_slots(int64_t M, int64_t N, int64_t K);   // slots the silu-mul epilogue of this shape writes
// gemm_stream.hip: persistent decode GEMM over a weight repacked into MFMA-operand-order tiles (see arcq.h), optionally with
// the activation quantiser as its prologue
int64_t gemm_repacked_w_bytes(int64_t N, int64_t K);
int64_t gemm_repacked_sf_bytes(int64_t N, int64_t K);
int gemm_repacked_supported(int64_t M, int64_t N, int64_t K);
int gemm_repacked(const GemmArgs& a, const uint8_t* RW, const uint8_t* RSF, hipStream_t stream);          // gemm_rowblock.hip (M <= 16), gemm_rowmid.hip above
int gemm_repacked_mid_supported(int64_t M, int64_t N, int64_t K);                                          // gemm_rowmid.hip: 16 < M <= 64
int gemm_repacked_mid(const GemmArgs& a, const uint8_t* RW, const uint8_t* RSF, hipStream_t stream);
int gemm_repacked_stream(const GemmArgs& a, const uint8_t* RW, const uint8_t* RSF, hipStream_t stream);   // gemm_stream.hip (A-B)
// The M <= 16 repacked kernels (gemm_rowblock.hip, gemm_stream.hip) address D and the residual with the 32-bit ELEMENT offset
// m * N + n (finish4<uint32_t>, gemm_common.hpp): the last one, M * N - 1, must fit.  The predicates say no beyond it and the
// launchers refuse by name.
inline bool repacked_out_fits(int64_t M, int64_t N) { return M * N <= ((int64_t)1 << 32); }
inline int repacked_out_refused(const char* who, int64_t M, int64_t N) {
  return fail(ARCQ_ERR_UNSUPPORTED, "%s: M * N = %lld elements exceed the decode kernels' 32-bit output offsets", who, (long long)(M * N));
}
// kEpiSiluMul on the M <= 16 repacked kernels (D stays gate|up, absmax_slots gets max |silu(g) * u| per row block): 0, or the error set
inline int repacked_silu_args_check(const GemmArgs& a) {
  if (a.epilogue == kEpiSiluMul && (!a.absmax_slots || (a.N % 4) || a.bias || a.residual || a.out_dtype != ARCQ_OUT_BF16))
    return fail(ARCQ_ERR_SHAPE, "arcq_gemm_nvfp4_repacked_silu_absmax: needs absmax_slots, N %% 4 == 0, bf16 output, no bias / residual");
  return 0;
}
struct FusedArgs {
  int kind;                   // ARCQ_SRC_RMSNORM | ARCQ_SRC_DYNAMIC
  int silu_act;               // ARCQ_SRC_RMSNORM only: D = bf16 silu(gate) * up [M, N/2] of interleaved gate|up rows + out_slots
  const uint16_t* X;          // bf16 [M, KQ]
  const uint16_t* Wn;         // rmsnorm weight bf16 [KQ]
  float eps;
  const int16_t* idx;
  const uint32_t* in_slots;   // ARCQ_SRC_DYNAMIC: abs-max words of X or NULL
  int n_in_slots;
  float* scale_out;           // ARCQ_SRC_DYNAMIC: max|X| / 2688
  const uint8_t* RW;
  const uint8_t* RSF;
  void* D;
  uint32_t* out_slots;
  const int16_t* act_scatter; // silu_act: ACT[m][act_scatter[j]] = activation j (NULL: ACT[m][j]); a permutation of 0 .. N/2-1
  int M, N, KQ, KE, variant;
  float alpha_host;
  const float* alpha_dev;
  const uint16_t* bias;
  const uint16_t* residual;
  int out_dtype;
};
int gemm_fused_supported(int kind, int64_t M, int64_t N, int64_t KQ, int64_t KE);
int gemm_fused(const FusedArgs& f, hipStream_t stream);
int64_t gemm_skinny_workspace_bytes(int64_t M, int64_t N, int64_t K);
int64_t gemm_tile_workspace_bytes(int64_t M, int64_t N, int64_t K);
int64_t gemm_tile_silu_slots(int64_t M, int64_t N, int64_t K);
int64_t gemm_decode_silu_slots(int64_t M, int64_t N, int64_t K);
// D = epilogue(sum_s partial[s]) over the `splitk` fp32 planes [M, N] at a.workspace, summed in a fixed order
int gemm_splitk_finish(const GemmArgs& a, int splitk, hipStream_t stream);
int gemm_skinny(const GemmArgs& a, hipStream_t stream);   // M <= 16, few tiles: weight-streaming MFMA GEMV, 16-row tiles
int64_t gemm_decode_workspace_bytes(int64_t M, int64_t N, int64_t K);
int gemm_decode(const GemmArgs& a, hipStream_t stream);   // M <= 16, many tiles: 32-row tiles, two units per thread and item
int gemm_tile(const GemmArgs& a, hipStream_t stream);     // general M: LDS-tiled MFMA GEMM (either B layout)
int gemm_tile_repacked(const GemmArgs& a, hipStream_t stream);   // gemm_tile_rw.hip: its B = RW / RSF instantiations (called by gemm_tile)
// gemm_tile_ot.hip: the value of arcq_debug_set_tile_overlap_tail (0 never, 1 by launch_tile's rule, 2 whenever legal).  Under 2 a shape
// made of whole 256 x 256 tiles takes the LDS-tiled kernel's 256 x 256 8-wave tile whatever the routes and heuristics say (tests)
int tile_overlap_tail_mode();
inline bool tile_overlap_tail_forced(int64_t M, int64_t N) { return tile_overlap_tail_mode() == 2 && M % 256 == 0 && N % 256 == 0; }
// gemm_tile_pl.hip: the value of arcq_debug_set_tile_pair_loads (1, the default: a launch that is eligible for the overlapped tail with
// the plain epilogue takes the paired-load sibling; 0: it takes gemm_tile_ot_kernel)
int tile_pair_loads_mode();
// gemm_tile_ql.hip: the value of arcq_debug_set_tile_quad_loads (1, the default: a launch that takes the paired-load sibling over the
// reference B layout takes the quad-load sibling instead; 0: it keeps gemm_tile_pl_kernel)
int tile_quad_loads_mode();
// gemm_regtile.hip: 16 < M <~ 1024, grids the tiled kernel cannot fill: operand fragments straight into registers, K split over waves
int gemm_regtile_cfg(int64_t M, int64_t N, int64_t K, int epilogue);   // 0 = not this kernel, else its configuration
int gemm_regtile(const GemmArgs& a, int cfg, hipStream_t stream);        // either B layout
int gemm_regtile_fits(int64_t M, int64_t N, int64_t K, int b_layout);   // every operand addressable with the kernel's 32-bit offsets

// kv_cache.hip: the paged KV cache of include/arcq_kv.h (arguments validated by c_api_kv.hip)
struct KvWriteArgs {
  void* kv_data;
  void* kv_param;
  const int32_t *kv_indptr, *kv_indices, *last_page_offset;
  const void *k, *v, *k_param, *v_param;   // quantize: k, v are 16-bit [ntok, N, 128] and the parameters are computed
  const int32_t* seqlen_indptr;            // NULL: append (ntok == B, token b is sequence b's last position)
  int64_t ntok, B, L, layer, N, P;
  int format, dtype;
  bool quantize;
};
int kv_write(const KvWriteArgs& a, hipStream_t stream);
struct KvDecodeArgs {
  void* o;
  const void *q, *kv_data, *kv_param;
  const int32_t *kv_indptr, *kv_indices, *last_page_offset;
  int64_t B, Nq, L, layer, N, P, nnz;
  int format, dtype;
  void* workspace;
};
int kv_decode_splits(int64_t B, int64_t Nq, int64_t N, int64_t nnz, int64_t P);   // slices per sequence; > 1 needs the workspace
int kv_decode(const KvDecodeArgs& a, hipStream_t stream);
struct KvStepArgs {                        // what the decode step takes beside KvDecodeArgs (whose q is then strided too)
  const void *k, *v;                       // 16-bit [B, N, 128], tokens kv_stride elements apart
  int64_t q_stride, kv_stride;
  void* state;                             // int32 [B * N * kv_decode_chunks], zero between launches
};
int64_t kv_decode_chunks(int64_t Nq, int64_t N);   // workgroups per (sequence, kv head): ceil(g / min(g, 4))
int kv_decode_step(const KvDecodeArgs& a, const KvStepArgs& st, hipStream_t stream);

// kv_prefill.hip: causal prefill attention over the int4 pages (arguments validated by c_api_kv.hip)
struct KvPrefillArgs {
  void* o;
  const void* q;
  const int32_t* qo_indptr;                // int32 [B + 1]: the query tokens of sequence b are rows qo_indptr[b] .. qo_indptr[b+1] of q / o
  const void *kv_data, *kv_param;
  const int32_t *kv_indptr, *kv_indices, *last_page_offset;
  int64_t ntok, B, Nq, L, layer, N, P;
  int dtype;
};
int kv_prefill(const KvPrefillArgs& a, hipStream_t stream);

// kv_rope.hip: rotary position embedding in front of the quantising writers, and alone (arguments validated by c_api_kv.hip)
struct KvRopeArgs {
  KvWriteArgs w;                           // quantize = true; k, v: 16-bit rows [ntok, N, 128], tokens kv_stride elements apart
  void* q_out;                             // 16-bit [ntok, Nq, 128], contiguous
  const void* q;                           // 16-bit [ntok, Nq, 128], tokens q_stride elements apart
  const void *cos, *sin;                   // 16-bit [rope_len, 128]
  int64_t q_stride, kv_stride, Nq;
  const char* who;
};
int kv_rope_write(const KvRopeArgs& a, hipStream_t stream);
struct RopeQkArgs {
  void *q, *k;                             // rotated in place; k may be NULL when N == 0
  const int32_t* positions;                // int32 [n_pos]: token i takes positions[i % n_pos]
  const void *cos, *sin;
  int64_t q_stride, k_stride, ntok, n_pos, Nq, N;
  int dtype;
};
int kv_rope_qk(const RopeQkArgs& a, hipStream_t stream);

}  // namespace arcq
