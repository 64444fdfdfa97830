/*
 * arcq.h -- C-ABI of the MI355X-native (gfx950) ARC-NVFP4 hot path.
 *
 * This is the drop-in boundary: every entry point takes plain device pointers, sizes and a HIP
 * stream, allocates nothing and returns an int status.  The library holds no caller-visible state: scratch
 * is caller-owned; internally it only remembers, per device, which kernels already have their large-LDS
 * opt-in (thread-safe, any number of devices per process) and the calling thread's last error text.  It replaces what the
 * reference's pybind11 module `agemm` (kernels/src/bindings.cpp:551-575) reaches through
 * libtorch + CUTLASS.  Allocation of outputs stays in the host shim (arcquant_amd/agemm.py), with
 * the reference's sizes (bindings.cpp:83-95,110,133-134,181-182).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in _host
 *   - bf16 tensors are passed as `const void*` (16-bit patterns), row-major, contiguous
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream, which is what
 *     the reference launches on: reorder.cu:344, rmsnorm.cu:272)
 *   - every launch is asynchronous; nothing here synchronises the device
 *   - status: 0 = ok, negative = error (see ARCQ_ERR_*); arcq_last_error() gives the text of the
 *     calling thread's last failure
 *
 * Layout contract (bit-exact with the reference):
 *   packed operand   [rows, K/2] u8, byte j = code[2j] | code[2j+1] << 4   (reorder.cu:28-31,161-164)
 *   scale factors    ue4m3 bytes in the CUTLASS Sm1xx block-scaled layout:
 *                    off(r,p) = (r/128)*(K/64)*512 + (p/4)*512 + (r%32)*16 + ((r/32)%4)*4 + p%4
 *                    (reorder.cuh:118-123, reorder.cu:139-143)
 *   augmented K      K = KQ + KE; group g of the reordered row goes to position
 *                    G16: g + max(0, g-P), residual/duplicate at +1          (reorder.cu:139,175)
 *                    G32: pos1 = 2t + max(0, 2t-P) (+g&1), residual at +2    (reorder.cu:451-452,510)
 *                    with P = (KQ-KE)/16, t = g/2.
 */
#ifndef ARCQ_H_
#define ARCQ_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARCQ_ABI_VERSION 1

#define ARCQ_OK 0
#define ARCQ_ERR_SHAPE (-1)       /* a dimension violates the contract (K % 64, KE % 16, KE > KQ, ...) */
#define ARCQ_ERR_UNSUPPORTED (-2) /* valid but not implemented (e.g. rows that do not fit in LDS)        */
#define ARCQ_ERR_LAUNCH (-3)      /* hipLaunchKernel / hipGetLastError reported a failure               */
#define ARCQ_ERR_NULL (-4)        /* a required pointer is NULL                                          */
#define ARCQ_ERR_WORKSPACE (-5)   /* workspace missing or too small (see arcq_gemm_workspace_bytes)     */

/* Augmented-K layout variants.  The reference picks one by KQ in a closed switch
 * (bindings.cpp:141-160): G32 for {3584, 18944, 27648, 28672}, G16 for its other sizes. */
#define ARCQ_VARIANT_G16 0 /* reorder.cu:68-330, rmsnorm.cu:68-255 */
#define ARCQ_VARIANT_G32 1 /* reorder.cu:380-696, down.cu:71-361   */

#define ARCQ_OUT_BF16 0 /* D is bf16 [M,N]  (the reference's only output type, nvfp4.cu:20-23) */
#define ARCQ_OUT_F32 1  /* D is fp32 [M,N]  (un-rounded alpha*acc: row-parallel partials, tests) */

int arcq_abi_version(void);
const char *arcq_last_error(void);

/* ---- host-side layout helpers (pure integer arithmetic, no GPU) ------------------------------------ */

/* replaces the KQ switch of bindings.cpp:141-160,189-207: KQ-generic rule with the same answers on the
 * reference's closed list. */
int arcq_variant_for_kq(int64_t KQ);
/* bindings.cpp:83-95 get_sf{a,b}_buffer_size_in_bytes: (rows/128 + 1) * 128 * K / 16 */
int64_t arcq_sf_alloc_bytes(int64_t rows, int64_t K);
/* bytes of that buffer a kernel may touch: ceil(rows/128) * 128 * K / 16 */
int64_t arcq_sf_used_bytes(int64_t rows, int64_t K);
int64_t arcq_sf_offset(int64_t row, int64_t pos, int64_t K);
int64_t arcq_primary_pos(int64_t g, int64_t KQ, int64_t KE, int variant);
int64_t arcq_residual_pos(int64_t g, int64_t KQ, int64_t KE, int variant); /* -1 if none */

/* ---- quantisers ------------------------------------------------------------------------------------ */

/* agemm.reorder_quantize_x (bindings.cpp:122-163; kernels reorder.cu:68-203, 380-555, down.cu:71-233).
 *   X [M,KQ] bf16, reorder_index [KQ] int16 (a permutation of 0..KQ-1), QX [M,(KQ+KE)/2] u8,
 *   SFX >= arcq_sf_alloc_bytes(M, KQ+KE) bytes (only the offsets of rows < M are written).
 *   KQ % 64 == 0, KE % 64 == 0, 0 <= KE <= KQ <= 32767 (whole 64-element scale-factor atoms: every size the
 *   reference dispatches and every select_num it produces).  X / reorder_index 16-byte, QX 8-byte, SFX 4-byte aligned. */
int arcq_quantize_x(const void *X, const int16_t *reorder_index, uint8_t *QX, uint8_t *SFX, int64_t M, int64_t KQ,
                    int64_t KE, int variant, void *stream);

/* agemm.reorder_quantize_w (bindings.cpp:170-210; kernels reorder.cu:210-330, 562-696, down.cu:240-361):
 * as above, but the residual slots are copies of the primary codes and scale. */
int arcq_quantize_w(const void *W, const int16_t *reorder_index, uint8_t *QW, uint8_t *SFW, int64_t N, int64_t KQ,
                    int64_t KE, int variant, void *stream);

/* agemm.rmsnorm_quantize_x (bindings.cpp:216-254; kernel rmsnorm.cu:68-255):
 *   xn = bf16(float(x) * float(w) * rsqrt(sum(x^2)/KQ + eps)) gathered by reorder_index, then as
 *   arcq_quantize_x.  2048 <= KQ <= 8192 (the reference's range).  PARITY UNPINNED against the CUDA binary: the
 *   reference's rsqrtf is a <= 2-ulp approximation, this kernel (and the oracle) use the correctly rounded
 *   1/sqrt; the sum-of-squares association order and the fused residual multiply-add are restated from the kernel
 *   text.  Byte-exact to that restatement (oracle/arcq_oracle.c), not provably to the reference's output.  The reference always uses the G16
 *   layout here; pass the variant the weights were quantised with (deviation D1). */
int arcq_rmsnorm_quantize_x(const void *X, const void *W, float eps, const int16_t *reorder_index, uint8_t *QX,
                            uint8_t *SFX, int64_t M, int64_t KQ, int64_t KE, int variant, void *stream);

/* ---- GEMM ------------------------------------------------------------------------------------------ */

/* Bytes of scratch arcq_gemm_nvfp4 needs for this shape (0 when none). */
int64_t arcq_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);

/* agemm.matmul (bindings.cpp:99-120 -> matmul_host_nvfp4_bf16, nvfp4.cu:35-132):
 *   D[m,n] = alpha * sum_g sfa[m,g]*sfb[n,g] * sum_{k in g} a[m,k]*b[n,k]      (fp32 accumulate, beta = 0)
 *   A [M,K/2], B [N,K/2] packed e2m1; SFA/SFB swizzled ue4m3; K % 64 == 0.
 *   alpha = alpha_host * (alpha_dev ? *alpha_dev : 1): the reference takes a host float
 *   (bindings.cpp:104); alpha_dev lets callers keep the per-tensor scale on the device (no sync).
 *   bias (optional, bf16 [N]) and residual (optional, bf16 [M,N], may alias D) are each added to the ROUNDED bf16 result,
 *   rounding again -- exactly the reference's separate torch ops `y = matmul(...); y = y + bias` (qLinearLayer.py:74-76)
 *   and the caller's `x + linear(...)`.  out_dtype: ARCQ_OUT_* (fp32 output adds both in fp32, one result).
 *   workspace / workspace_bytes: scratch of at least arcq_gemm_workspace_bytes(M,N,K) (may be NULL if 0). */
int arcq_gemm_nvfp4(const uint8_t *A, const uint8_t *B, const uint8_t *SFA, const uint8_t *SFB, void *D, int64_t M,
                    int64_t N, int64_t K, float alpha_host, const float *alpha_dev, const void *bias, const void *residual,
                    int out_dtype,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* ---- f1 extension: per-tensor scale on the device (replaces torch.max(x.abs())/2688 + x/scale,
 *      model/qLlamaLayer.py:73-77, with no host sync) ------------------------------------------------- */

/* scale_out[0] = max|x| / (448*6) as fp32; x is bf16 [n]. */
int arcq_absmax_scale(const void *X, int64_t n, float *scale_out, void *stream);

/* NVFP4_reorder_quantize_x (model/qLlamaLayer.py:73-77) in two launches instead of five:
 *   scale = max|X| / 2688 (fp32, written to scale_out[0]);  (QX, SFX) = arcq_quantize_x(bf16(X / scale), ...).
 * `state` is ARCQ_DYN_STATE_BYTES of device scratch owned by the caller (one abs-max word per workgroup of the
 * abs-max pass; plain stores, fully rewritten by every call, so it needs no initialisation and no reset; it must not
 * be shared by calls that may run concurrently on different streams).  Inputs <= 256 KB take a single launch and do
 * not touch it. */
#define ARCQ_DYN_STATE_BYTES 1024
int arcq_quantize_x_dyn(const void *X, const int16_t *reorder_index, uint8_t *QX, uint8_t *SFX, float *scale_out,
                        void *state, int64_t M, int64_t KQ, int64_t KE, int variant, void *stream);

/* Extension: the MLP's `act_fn(gate) * up` (model/qLlamaLayer.py:417, SiLU) folded into the dynamic quantiser.
 * GU = [M, 2*KQ] bf16, the output of a fused gate_up projection, in one of two layouts: ARCQ_GU_HALVES = gate in
 * columns [0, KQ) and up in [KQ, 2*KQ); ARCQ_GU_PAIRS = (g0, u0, g1, u1, ...), the layout of a weight whose gate and
 * up rows interleave (what arcq_gemm_nvfp4_silu_mul consumes).  Equals arcq_quantize_x_dyn on the bf16 tensor torch
 * computes as silu(gate) * up, which is never materialised.  `state` as above. */
#define ARCQ_GU_HALVES 0
#define ARCQ_GU_PAIRS 1
int arcq_silu_mul_quantize_x_dyn(const void *GU, const int16_t *reorder_index, uint8_t *QX, uint8_t *SFX, float *scale_out,
                                 void *state, int64_t M, int64_t KQ, int64_t KE, int variant, int layout, void *stream);

/* ---- f3 extension: the MLP's `act_fn(gate) * up` (SiLU, model/qLlamaLayer.py:417) in the GEMM epilogue -------------
 * B holds the gate and up projections with their ROWS INTERLEAVED (g0, u0, g1, u1, ...: quantise the interleaved
 * weight with arcq_quantize_w as usual), N = 2 * intermediate, N % 8 == 0.  ACT = bf16 [M, N/2] receives
 * silu(bf16(alpha * gate)) * bf16(alpha * up) with torch's roundings (the value `act_fn(gate) * up` has after two
 * separate GEMMs), and absmax_slots[0 .. arcq_gemm_silu_mul_slots(M,N,K)) one max|ACT| word each (bf16 magnitude
 * bits; plain stores, no initialisation needed).  arcq_quantize_x_dyn_slots then quantises ACT with its per-tensor
 * dynamic scale in ONE launch: together two launches replace GEMM + silu + mul + abs-max + quantise. */
int64_t arcq_gemm_silu_mul_slots(int64_t M, int64_t N, int64_t K);
int arcq_gemm_nvfp4_silu_mul(const uint8_t *A, const uint8_t *B, const uint8_t *SFA, const uint8_t *SFB, void *ACT,
                             uint32_t *absmax_slots, int64_t M, int64_t N, int64_t K, float alpha_host,
                             const float *alpha_dev, const void *bias, void *stream);   /* bias: optional bf16 [N], rows interleaved as B's */
/* arcq_quantize_x_dyn with max|X| taken from `nslots` precomputed words instead of an abs-max pass.
 * reorder_index == NULL: X is already in reordered channel order (identity permutation; see act_scatter_index of
 * arcq_linear_rmsnorm_silu_repacked) -- no gather, same bytes. */
int arcq_quantize_x_dyn_slots(const void *X, const int16_t *reorder_index, uint8_t *QX, uint8_t *SFX, float *scale_out,
                              const uint32_t *absmax_slots, int64_t nslots, int64_t M, int64_t KQ, int64_t KE,
                              int variant, void *stream);

/* ---- decode GEMM over a REPACKED weight (optional fast path for M <= 128) ---------------------------------------
 * A static weight can be laid out for the hardware once: RW = tiles of 16 rows x 128 K elements (1 KB) in MFMA operand
 * order (lane 16*q + r of a wave holds the 16 bytes of row r, K elements [32q, 32q+32) of the tile; the tiles of a row
 * block are consecutive), RSF = per pair of tiles 256 bytes, lane l holding the ue4m3 bytes of its two groups in the
 * first and in the second tile; K padded to a multiple of 256 and N to a multiple of 16 with zero scales.  Sizes from
 * arcq_repacked_{w,sf}_bytes; arcquant_amd/agemm.py:repack_w builds both from the reference layout (pure data movement,
 * nothing is re-quantised).  A / SFA stay in the reference layout.  arcq_gemm_repacked_supported tells whether a shape
 * can take this path -- M <= 16, M * N <= 2^32 (32-bit output offsets) and the fp16 image of the activations fits LDS, or a decode batch 16 < M <= 128 on a
 * weight where reading it once beats the tiled GEMM (activations fetched per tile pair or kept packed in LDS; gemm_rowmid.hip) --;
 * results equal arcq_gemm_nvfp4's up to fp32 accumulation order. */
int64_t arcq_repacked_w_bytes(int64_t N, int64_t K);
int64_t arcq_repacked_sf_bytes(int64_t N, int64_t K);
int arcq_gemm_repacked_supported(int64_t M, int64_t N, int64_t K);
int arcq_gemm_nvfp4_repacked(const uint8_t *A, const uint8_t *RW, const uint8_t *SFA, const uint8_t *RSF, void *D,
                             int64_t M, int64_t N, int64_t K, float alpha_host, const float *alpha_dev,
                             const void *bias, const void *residual, int out_dtype, void *stream);

/* The same contraction through the kernel of the fused decode linears below (arcq_linear_*): identical arguments and
 * result up to fp32 accumulation order.  arcq_gemm_nvfp4_repacked picks the faster kernel for plain packed activations; this
 * entry point exists so that a fused linear can be checked BIT FOR BIT against its two-call equivalent
 * (quantiser + this GEMM): same kernel body, same summation order. */
int arcq_gemm_nvfp4_repacked_stream(const uint8_t *A, const uint8_t *RW, const uint8_t *SFA, const uint8_t *RSF, void *D,
                                    int64_t M, int64_t N, int64_t K, float alpha_host, const float *alpha_dev,
                                    const void *bias, const void *residual, int out_dtype, void *stream);

/* The gate|up projection of a decode step on the repacked path, for weights whose ROWS INTERLEAVE gate and up (g0, u0, g1,
 * u1, ...): D = bf16 [M, N] as arcq_gemm_nvfp4_repacked writes it, and absmax_slots[i], i < ceil(N / 16), = max |silu(g) * u|
 * (bf16 bits, computed from the stored values with the quantiser's own rounding) over the outputs of row block i.
 * arcq_silu_mul_quantize_x_dyn_slots then quantises act = silu(gate) * up (model/qLlamaLayer.py:417 -> :73-77) from D in ONE
 * launch: the abs-max pass of arcq_silu_mul_quantize_x_dyn disappears, the bytes are identical.  N % 4 == 0. */
int arcq_gemm_nvfp4_repacked_silu_absmax(const uint8_t *A, const uint8_t *RW, const uint8_t *SFA, const uint8_t *RSF, void *D,
                                         uint32_t *absmax_slots, int64_t M, int64_t N, int64_t K, float alpha_host,
                                         const float *alpha_dev, void *stream);
int arcq_silu_mul_quantize_x_dyn_slots(const void *GU, const int16_t *reorder_index, uint8_t *QX, uint8_t *SFX,
                                       float *scale_out, const uint32_t *absmax_slots, int64_t nslots, int64_t M,
                                       int64_t KQ, int64_t KE, int variant, int layout, void *stream);

/* ---- every M over the REPACKED weight: one weight copy per layer -------------------------------------------------------------
 * arcq_gemm_nvfp4's contract (same A / SFA, alpha, bias, residual -- may alias D --, out_dtype, workspace) with B given as (RW, RSF)
 * from arcq_repacked_{w,sf}_bytes / agemm.repack_w, for EVERY M: a layer that keeps only the repacked weight needs no second copy
 * in the reference layout.  arcq_gemm_rw_route(M, N, K) says which kernels a call with 8-byte aligned bias / residual takes (pure, no GPU):
 *   1  arcq_gemm_repacked_supported(M, N, K): the repacked decode kernels -- the call IS arcq_gemm_nvfp4_repacked;
 *   2  the register-tiled kernel over RW in the configuration arcq_gemm_nvfp4 would use: bit-identical to arcq_gemm_nvfp4 on the
 *      reference-layout weight.  Where arcq_gemm_nvfp4 takes an LDS-transposing decode kernel instead (M <= 16 on very long K or
 *      very wide N, here called the G' shapes) its 16 x 16 configuration: equal up to fp32 summation order only;
 *   3  the LDS-tiled kernel over RW, same configuration and split-K as arcq_gemm_nvfp4: bit-identical to it;
 *   0  unsupported: an invalid shape, or a register-tiled route whose RW exceeds the kernel's 32-bit offsets (< 2 GiB).
 * A bias / residual view that is not 8-byte aligned skips route 1 (the decode kernels reject it) and takes 2 or 3.
 * Workspace: arcq_gemm_rw_workspace_bytes (= arcq_gemm_workspace_bytes on route 3; also sized for the route a route-1 shape
 * takes with a misaligned view; 0 on route 2).  Validation as arcq_gemm_nvfp4:
 * ARCQ_ERR_SHAPE for K % 64 / a bad out_dtype / misaligned A, RW, D (16 B) or SFA, RSF (4 B), ARCQ_ERR_NULL for a NULL operand,
 * M == 0 or N == 0 returns ARCQ_OK, all before any HIP call. */
int     arcq_gemm_rw_route(int64_t M, int64_t N, int64_t K);
int64_t arcq_gemm_rw_workspace_bytes(int64_t M, int64_t N, int64_t K);
int     arcq_gemm_nvfp4_rw(const uint8_t *A, const uint8_t *RW, const uint8_t *SFA, const uint8_t *RSF, void *D,
                           int64_t M, int64_t N, int64_t K, float alpha_host, const float *alpha_dev,
                           const void *bias, const void *residual, int out_dtype,
                           void *workspace, int64_t workspace_bytes, void *stream);
/* arcq_gemm_nvfp4_silu_mul over RW (rows interleaving gate and up, N % 8 == 0; the LDS-tiled kernel, bit-identical to it) for M > 16.
 * M <= 16 returns ARCQ_ERR_UNSUPPORTED (before the pointer checks): decode has arcq_gemm_nvfp4_repacked_silu_absmax and
 * arcq_linear_rmsnorm_silu_repacked.  absmax_slots: arcq_gemm_rw_silu_mul_slots(M, N, K) words (0 for M <= 16). */
int64_t arcq_gemm_rw_silu_mul_slots(int64_t M, int64_t N, int64_t K);
int     arcq_gemm_nvfp4_rw_silu_mul(const uint8_t *A, const uint8_t *RW, const uint8_t *SFA, const uint8_t *RSF,
                                    void *ACT, uint32_t *absmax_slots, int64_t M, int64_t N, int64_t K,
                                    float alpha_host, const float *alpha_dev, const void *bias, void *stream);

/* ---- fused decode linear: the activation quantiser runs as the prologue of the repacked GEMM ------------------------------
 * One launch replaces  [rmsnorm_quantize_x | abs-max + x/scale + reorder_quantize_x]  ->  matmul (+ bias) (+ residual)
 * of a decode step (model/qLlamaLayer.py:73-77 + qLinearLayer.py:62-78; benchmarks/modeling_arc.py:211-228,279-310).  Every
 * workgroup quantises the M <= 16 token rows itself with the quantisers' own group arithmetic, so the result is BIT-IDENTICAL
 * to arcq_rmsnorm_quantize_x / arcq_quantize_x_dyn followed by arcq_gemm_nvfp4_repacked on the same repacked weight.
 * arcq_linear_fused_supported(kind, M, N, KQ, KE) tells whether a shape fits (M <= 16, LDS); callers fall back to the two
 * calls otherwise.  It is a capability, not a recommendation: every CU repeats the quantisation of all M * KQ elements, which beats
 * the separate quantiser launch (~3 us of launch + cold start) while M * KQ is about 16 K elements or less (measured on MI355X:
 * M = 4, KQ = 3584 / 4096: 1-2 us faster per linear; M = 16, KQ = 4096 or M = 4, KQ = 18944: 2-3x slower). */
#define ARCQ_SRC_RMSNORM 1
#define ARCQ_SRC_DYNAMIC 2
int arcq_linear_fused_supported(int kind, int64_t M, int64_t N, int64_t KQ, int64_t KE);

/* D = alpha * matmul(rmsnorm_quantize_x(X, Wn, eps, reorder_index, KE), W) (+ bias) (+ residual); arguments as in
 * arcq_rmsnorm_quantize_x and arcq_gemm_nvfp4_repacked (K = KQ + KE), alpha = alpha_host * (alpha_dev ? *alpha_dev : 1). */
int arcq_linear_rmsnorm_repacked(const void *X, const void *Wn, float eps, const int16_t *reorder_index, const uint8_t *RW,
                                 const uint8_t *RSF, void *D, int64_t M, int64_t N, int64_t KQ, int64_t KE, int variant,
                                 float alpha_host, const float *alpha_dev, const void *bias, const void *residual, int out_dtype,
                                 void *stream);
/* The gate|up projection of the MLP: as above for a weight whose ROWS INTERLEAVE gate and up (g0, u0, g1, u1, ...); ACT = bf16
 * [M, N/2] receives silu(bf16(alpha*gate)) * bf16(alpha*up) with torch's roundings (what `act_fn(gate) * up`,
 * model/qLlamaLayer.py:417, has after two GEMMs) and absmax_slots[i], i < ceil(N/16), max |ACT| over row block i (bf16 bits):
 * arcq_linear_dynamic_repacked then quantises ACT without an abs-max pass.  N % 4 == 0. */
int arcq_linear_rmsnorm_silu_repacked(const void *X, const void *Wn, float eps, const int16_t *reorder_index, const uint8_t *RW,
                                      const uint8_t *RSF, void *ACT, uint32_t *absmax_slots, int64_t M, int64_t N, int64_t KQ,
                                      int64_t KE, int variant, float alpha_host, const float *alpha_dev, const void *bias,
                                      const int16_t *act_scatter_index, void *stream);
/* bias: optional bf16 [N], interleaved (g0, u0, g1, u1, ...) like the rows.
 * act_scatter_index: optional int16 [N/2], a permutation (not checked): activation j is stored at ACT[m][act_scatter_index[j]].
 * With act_scatter_index = the inverse of the consumer's reorder_index, ACT is already in reordered channel order and
 * arcq_quantize_x_dyn_slots(ACT, reorder_index = NULL, ...) yields the same bytes as quantising the natural-order
 * activation with that reorder_index. */
/* scale = max|X| / 2688 (from absmax_slots[0..nslots) when given, else computed from X; written to scale_out[0] if not NULL);
 * D = alpha_host * scale * matmul(quantize_x(bf16(X / scale), reorder_index, KE), W) (+ bias) (+ residual): the reference's
 * NVFP4_reorder_quantize_x + QLinearLayer.forward with alpha_host = the weight's per-tensor scale. */
int arcq_linear_dynamic_repacked(const void *X, const int16_t *reorder_index, const uint8_t *RW, const uint8_t *RSF, void *D,
                                 float *scale_out, const uint32_t *absmax_slots, int64_t nslots, int64_t M, int64_t N, int64_t KQ,
                                 int64_t KE, int variant, float alpha_host, const void *bias, const void *residual, int out_dtype,
                                 void *stream);

/* ---- MXFP4 (quant_type='MXFP4' of the reference, model/quantize.py:94-122,219-268) ----------------------------------------
 * MXFP4-ARC, the packed form of the reference's fake MXFP4 path (DESIGN.md "MXFP4"):
 *   shape      KQ % 64 == 0, KE % 64 == 0, 0 <= KE <= KQ <= 32767, reorder_index an int16 permutation of 0..KQ-1;
 *              K = KQ + KE, Kp = arcq_mx_k_padded(K) = round_up(K, 128) (every K step of the scaled MFMA is full)
 *   augmented K concatenation: [0, KQ) the reordered row xr[c] = X[row, idx[c]]; [KQ, K) for activations the residual of
 *              reordered channels [KQ-KE, KQ), for weights a copy of those channels' codes and scales; [K, Kp) padding,
 *              code 0 and scale byte 127
 *   codes      [rows, Kp/2] u8, low nibble = even element
 *   scales     [rows, Kp/32] u8 E8M0, row-major: byte b means 2^(b-127); 255 is never written.  No swizzle, no per-tensor scale
 *   block      32 elements v (bf16 widened to fp32), amax = max|v|: e = clamp(ceil(log2(amax/6)), -127, 127) computed exactly
 *              (the smallest integer with amax <= 6 * 2^e; 0 for an all-zero block); code = e2m1_RNE(v * 2^-e), ties to the
 *              even code, sign of zero kept, never saturating
 *   residual   res = v - deq(code) * 2^e, exact in bf16; its blocks are quantised like any other block */
int64_t arcq_mx_k_padded(int64_t K);                /* round_up(K, 128) (0 for K <= 0) */
int64_t arcq_mx_sf_bytes(int64_t rows, int64_t K);  /* rows * arcq_mx_k_padded(K) / 32 */

/* X [M,KQ] bf16, reorder_index [KQ] int16, QX [M, Kp/2] u8, SFX [M, Kp/32] u8.  X, reorder_index and QX 16-byte aligned.
 * Status: ARCQ_ERR_SHAPE for a shape outside the contract or a misaligned pointer, ARCQ_ERR_NULL for a NULL pointer (M > 0). */
int arcq_mx_quantize_x(const void *X, const int16_t *reorder_index, uint8_t *QX, uint8_t *SFX, int64_t M, int64_t KQ, int64_t KE,
                       void *stream);
/* as above; the slots [KQ, K) are copies of the codes and scales of reordered channels [KQ-KE, KQ) */
int arcq_mx_quantize_w(const void *W, const int16_t *reorder_index, uint8_t *QW, uint8_t *SFW, int64_t N, int64_t KQ, int64_t KE,
                       void *stream);

/* D[m,n] = alpha * sum_{k<K} deq(A[m,k]) * deq(B[n,k]), fp32 accumulation, on the block-scaled fp4 MFMA.
 *   A [M, K/2], B [N, K/2] codes and SFA [M, K/32], SFB [N, K/32] scales as written by the quantisers; K = Kp (K % 128 == 0);
 *   any M >= 0; N % 16 == 0.  alpha, bias, residual (may alias D) and out_dtype: arcq_gemm_nvfp4's contract and roundings.
 *   workspace / workspace_bytes: unused (no configuration needs scratch), may be NULL / 0.
 *   Status: ARCQ_ERR_SHAPE for K % 128, N % 16, a bad out_dtype or a misaligned pointer (A, B, D 16 bytes; SFA, SFB 4 bytes;
 *   bias, residual 2 bytes), ARCQ_ERR_NULL for a NULL operand; M == 0 or N == 0 returns ARCQ_OK; all before any HIP call. */
int arcq_gemm_mxfp4(const uint8_t *A, const uint8_t *B, const uint8_t *SFA, const uint8_t *SFB, void *D, int64_t M, int64_t N,
                    int64_t K, float alpha_host, const float *alpha_dev, const void *bias, const void *residual, int out_dtype,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* ---- MXFP4 decoder-layer operators: the fused quantisers and the SiLU*up GEMM epilogue ------------------------------------------
 * MXFP4 has no per-tensor scale, so none of them needs an abs-max pass, a `state` buffer or abs-max slots: each is ONE launch.
 *
 * arcq_mx_rmsnorm_quantize_x: (QX, SFX) = arcq_mx_quantize_x(xn, ...) of the normalised row arcq_rmsnorm_quantize_x forms,
 *   xn[c] = bf16(float(X[m, i]) * float(Wn[i]) * rstd), i = reorder_index[c], the product left to right in fp32,
 *   rstd = (float)(1 / sqrt((double)(sumsq / (float)KQ + eps))), sumsq in that entry's association order: the two quant types
 *   normalise identically.  2048 <= KQ <= 8192 (the range of the reduction tree), KQ % 64 == 0, KE % 64 == 0, 0 <= KE <= KQ;
 *   X, Wn, reorder_index and QX 16-byte aligned.  Status as arcq_mx_quantize_x (M == 0 returns ARCQ_OK), before any HIP call. */
int arcq_mx_rmsnorm_quantize_x(const void *X, const void *Wn, float eps, const int16_t *reorder_index, uint8_t *QX, uint8_t *SFX,
                               int64_t M, int64_t KQ, int64_t KE, void *stream);
/* arcq_mx_silu_mul_quantize_x: GU = bf16 [M, 2*KQ] in layout ARCQ_GU_HALVES or ARCQ_GU_PAIRS; (QX, SFX) = arcq_mx_quantize_x of the
 *   bf16 tensor torch computes as silu(gate) * up (two roundings), which is never materialised.  KQ as arcq_mx_quantize_x; GU,
 *   reorder_index and QX 16-byte aligned; ARCQ_ERR_SHAPE for a layout outside {0, 1}. */
int arcq_mx_silu_mul_quantize_x(const void *GU, const int16_t *reorder_index, uint8_t *QX, uint8_t *SFX, int64_t M, int64_t KQ,
                                int64_t KE, int layout, void *stream);
/* arcq_gemm_mxfp4_silu_mul: arcq_gemm_mxfp4 for a weight whose ROWS INTERLEAVE gate and up (g0, u0, g1, u1, ...) with the MLP's
 *   act_fn(gate) * up in its epilogue: ACT = bf16 [M, N/2], ACT[m, j] = silu(y[m, 2j]) * y[m, 2j+1] with torch's roundings, y being
 *   the bf16 value arcq_gemm_mxfp4 would store (bf16(alpha * acc), then + bias -> bf16; same kernels, same accumulation order); y
 *   is never written.  K % 128 == 0, N % 16 == 0; A, B, ACT 16-byte, SFA, SFB 4-byte, bias (optional bf16 [N], interleaved as the
 *   rows) 2-byte aligned.  Status as arcq_gemm_mxfp4; M == 0 or N == 0 returns ARCQ_OK; all before any HIP call. */
int arcq_gemm_mxfp4_silu_mul(const uint8_t *A, const uint8_t *B, const uint8_t *SFA, const uint8_t *SFB, void *ACT, int64_t M,
                             int64_t N, int64_t K, float alpha_host, const float *alpha_dev, const void *bias, void *stream);
/* arcq_gemm_mxfp4_silu_mul_quantize: the gate|up GEMM that writes the down projection's quantised input.  A, B, SFA, SFB, K, alpha and
 *   bias exactly as arcq_gemm_mxfp4_silu_mul; with KQ2 = N / 2 (the activation width), K2 = KQ2 + KE and Kp2 = arcq_mx_k_padded(K2),
 *   QACT u8 [M, Kp2/2] and SFACT u8 [M, Kp2/32] receive, byte for byte, what arcq_mx_quantize_x(ACT, identity, QACT, SFACT, M, KQ2, KE)
 *   writes for the ACT of arcq_gemm_mxfp4_silu_mul and identity = 0 .. KQ2-1: the residual blocks of the last KE channels, the padding
 *   blocks and the sign of zero included (same kernels' accumulation order, same roundings).  ACT is never written: a block of 32
 *   activations is 64 adjacent output columns, which one workgroup holds, and an MXFP4 block needs nothing beyond its own 32 values.
 *   CHANNEL ORDER IS THE CALLER'S: there is no reorder_index here, activation j is channel j of the quantised operand.  A consumer
 *   whose quantiser would gather with a non-identity reorder_index stores the gate|up weight rows (and the bias) in that order at
 *   deployment time -- pair j = (gate row, up row) of channel reorder_index[j] -- which is exact, the weight being quantised per row.
 *   K % 128 == 0; KQ2 % 64 == 0 (so N % 128 == 0), KE % 64 == 0, 0 <= KE <= KQ2 <= 32767; A, B, QACT 16-byte, SFA, SFB 4-byte, bias
 *   2-byte aligned.  Status as arcq_gemm_mxfp4_silu_mul (ARCQ_ERR_SHAPE / ARCQ_ERR_NULL); M == 0 returns ARCQ_OK; all before any HIP
 *   call. */
int arcq_gemm_mxfp4_silu_mul_quantize(const uint8_t *A, const uint8_t *B, const uint8_t *SFA, const uint8_t *SFB, uint8_t *QACT,
                                      uint8_t *SFACT, int64_t M, int64_t N, int64_t K, float alpha_host, const float *alpha_dev,
                                      const void *bias, int64_t KE, void *stream);

/* ---- MXFP4 repacked weight: decode GEMMs (1 <= M <= 64) over a weight laid out in MFMA operand order --------------------------------
 * A static MXFP4 weight (QW [N, K/2], SFW [N, K/32] of arcq_mx_quantize_w, K = Kp) can be laid out for the hardware once;
 * arcquant_amd/agemm.py:mx_repack_w builds both arrays (pure data movement, the same codes and E8M0 bytes), mx_unrepack_w inverts it.
 * N % 16 == 0, K % 128 == 0.  With row block b = n / 16, r = n % 16, step t = k / 128, q = (k % 128) / 32:
 *   MRW   [N/16][K/128][64 lanes][16 bytes], no padding, N * K / 2 bytes:
 *           MRW[((b * (K/128) + t) * 64 + 16*q + r) * 16 + j] = QW[n][64*t + 16*q + j],  j = 0 .. 15
 *         lane 16*q + r of tile (b, t) holds row 16*b + r, K elements [128*t + 32*q, +32): the B operand of one scaled 16x16x128 MFMA.
 *   MRSF  [N/16][R][8][64 lanes][4 bytes], R = ceil((K/128) / 32) rounds of 32 steps, (N/16) * R * 2048 bytes:
 *           MRSF[(((b * R + t/32) * 8 + t%8) * 64 + 16*q + r) * 4 + (t/8)%4] = SFW[n][4*t + q]
 *         the aligned dword of (round, wave = t % 8, lane) holds that lane's scale byte in the four steps 32*round + 8*u + wave, u = 0 .. 3.
 *         Bytes of steps t >= K/128 (a partial last round) are PADDING: mx_repack_w writes 127 (E8M0 2^0); no result depends on them
 *         (a step past K/128 issues no MFMA), they exist so that every dword the kernel fetches lies inside the array.
 * A / SFA stay in the row-major form the quantisers write.  For every output the sum is arcq_gemm_mxfp4's at M <= 64 (K steps s = w mod 8
 * accumulated in ascending order per w, the eight partial sums added w = 0 .. 7, then the same epilogue), so the results are BIT FOR BIT
 * those of arcq_gemm_mxfp4 / arcq_gemm_mxfp4_silu_mul on (QW, SFW).  The weight is read once whatever M is. */
int64_t arcq_mx_repacked_w_bytes(int64_t N, int64_t K);    /* N * K / 2; 0 unless N % 16 == 0 and K % 128 == 0 (both positive) */
int64_t arcq_mx_repacked_sf_bytes(int64_t N, int64_t K);   /* (N/16) * ceil(K/4096) * 2048; 0 likewise */
int arcq_gemm_mxfp4_repacked_supported(int64_t M, int64_t N, int64_t K);   /* 1 <= M <= 64, N % 16 == 0, K % 128 == 0 */
/* arcq_gemm_mxfp4's contract (alpha, bias, residual -- may alias D --, out_dtype) with B given as (MRW, MRSF); no workspace.
 *   Status, all before any HIP call and in this order: ARCQ_ERR_SHAPE for M or N < 0, K % 128 or N % 16; ARCQ_ERR_SHAPE for M > 64;
 *   ARCQ_ERR_SHAPE for a bad out_dtype; M == 0 or N == 0 returns ARCQ_OK; ARCQ_ERR_NULL for a NULL operand; ARCQ_ERR_SHAPE for a
 *   misaligned pointer (A, MRW, D 16 bytes; SFA, MRSF 4 bytes; bias, residual 2 bytes). */
int arcq_gemm_mxfp4_repacked(const uint8_t *A, const uint8_t *MRW, const uint8_t *SFA, const uint8_t *MRSF, void *D, int64_t M,
                             int64_t N, int64_t K, float alpha_host, const float *alpha_dev, const void *bias, const void *residual,
                             int out_dtype, void *stream);
/* arcq_gemm_mxfp4_silu_mul over (MRW, MRSF) of a weight whose rows interleave gate and up: ACT = bf16 [M, N/2].  Status as above. */
int arcq_gemm_mxfp4_repacked_silu_mul(const uint8_t *A, const uint8_t *MRW, const uint8_t *SFA, const uint8_t *MRSF, void *ACT,
                                      int64_t M, int64_t N, int64_t K, float alpha_host, const float *alpha_dev, const void *bias,
                                      void *stream);

/* ---- MXFP4 repacked weight, every batch size: one weight copy per layer ----------------------------------------------------------
 * The three GEMMs of the MXFP4 path over (MRW, MRSF) alone, for ANY M >= 0, so that a layer need not keep (QW, SFW) beside them.
 * M <= 64 runs the decode kernels above (arcq_gemm_mxfp4_rw at such an M IS arcq_gemm_mxfp4_repacked; the quantising form has a decode
 * kernel of its own: four row blocks = one 32-block of activations per workgroup, the same K split and sum order).  M > 64 runs the
 * 128 x 128 tile kernel of arcq_gemm_mxfp4 with its B operand staged from (MRW, MRSF): a wave fetches whole 1 KB spans of MRW, the four
 * scale bytes of a row and step are gathered from their four MRSF dwords, and what the MFMAs read from LDS is byte for byte what the
 * reference-layout kernel stages.  Results are BIT FOR BIT those of arcq_gemm_mxfp4, arcq_gemm_mxfp4_silu_mul and
 * arcq_gemm_mxfp4_silu_mul_quantize on (QW, SFW), at every M.  No result depends on MRSF's padding bytes.  No workspace.
 *   Status, all before any HIP call and in the order of the reference-layout namesake: ARCQ_ERR_SHAPE for M or N < 0, K % 128, N % 16
 *   (N % 128 and the KE rule for the quantising form); ARCQ_ERR_SHAPE for a bad out_dtype; M == 0 or N == 0 returns ARCQ_OK; ARCQ_ERR_NULL
 *   for a NULL operand; ARCQ_ERR_UNSUPPORTED for M beyond arcq_gemm_mxfp4's limit; ARCQ_ERR_SHAPE for a misaligned pointer (A, MRW, D /
 *   ACT / QACT 16 bytes; SFA, MRSF 4 bytes; bias, residual 2 bytes). */
int arcq_gemm_mxfp4_rw_route(int64_t M, int64_t N, int64_t K);   /* 1: the decode kernels (the call IS arcq_gemm_mxfp4_repacked), 2: the tile kernel over MRW, 0: invalid shape */
int arcq_gemm_mxfp4_rw(const uint8_t *A, const uint8_t *MRW, const uint8_t *SFA, const uint8_t *MRSF, void *D, int64_t M, int64_t N,
                       int64_t K, float alpha_host, const float *alpha_dev, const void *bias, const void *residual, int out_dtype,
                       void *stream);
int arcq_gemm_mxfp4_rw_silu_mul(const uint8_t *A, const uint8_t *MRW, const uint8_t *SFA, const uint8_t *MRSF, void *ACT, int64_t M,
                                int64_t N, int64_t K, float alpha_host, const float *alpha_dev, const void *bias, void *stream);
int arcq_gemm_mxfp4_rw_silu_mul_quantize(const uint8_t *A, const uint8_t *MRW, const uint8_t *SFA, const uint8_t *MRSF, uint8_t *QACT,
                                         uint8_t *SFACT, int64_t M, int64_t N, int64_t K, float alpha_host, const float *alpha_dev,
                                         const void *bias, int64_t KE, void *stream);

/* ---- MXFP4 fused decode linear: the activation quantiser runs as the prologue of the repacked decode GEMM -------------------------
 * One launch replaces  [arcq_mx_rmsnorm_quantize_x | arcq_mx_quantize_x]  ->  arcq_gemm_mxfp4_repacked (+ bias) (+ residual) or
 * arcq_gemm_mxfp4_repacked_silu_mul of a decode step.  (MRW, MRSF) are those of the repacked weight for (N, Kp), Kp =
 * arcq_mx_k_padded(KQ + KE).  Every workgroup quantises the M <= 16 token rows itself, with the quantisers' own statements (the
 * RMSNorm row, the MXFP4 block rule, residual and padding blocks) into an image in LDS, and multiplies every row block it owns from
 * that image in the decode kernel's sum order: the result is BIT FOR BIT that of the two calls.  Nothing quantised is written to
 * global memory; no workspace, no host synchronisation, capturable in a HIP graph.
 *   kind       ARCQ_SRC_RMSNORM (the row is bf16(x * wn * rstd)) or ARCQ_SRC_PLAIN (the row is X); ARCQ_SRC_DYNAMIC has no MXFP4
 *              meaning: there is no per-tensor scale.
 *   shape      KQ % 64 == 0, KE % 64 == 0, 0 <= KE <= KQ <= 32767; 2048 <= KQ <= 8192 for ARCQ_SRC_RMSNORM; N % 16 == 0.
 *   supported  arcq_mx_linear_fused_supported(kind, M, N, KQ, KE) is 1 when the shape is valid, 1 <= M <= 16 and the kernel's LDS fits two
 *              workgroups per CU with at least one row staged:   steps * 1088 + 32 + max(16384, (R + w) * row) <= 81920 bytes   for
 *              R = 1, where steps = Kp / 128 (1 KB of codes and 64 scale bytes per K step of the image), row = KQ * 9 / 4 (a padded
 *              row of the quantisers' staging), w = 1 for ARCQ_SRC_RMSNORM (the norm weight) and 0 for ARCQ_SRC_PLAIN.  A launch
 *              stages R = the largest of 8, 4, 2, 1 rows per pass that satisfies it (arcq_mx_linear_fused_lds_bytes returns the left
 *              side for that R).  Callers fall back to the two calls otherwise.
 *   grid       arcq_mx_linear_fused_workgroups(kind, N, KQ, KE): min(N / 16, 512) workgroups, each of which takes the row blocks g,
 *              g + grid, ... (0 for an unsupported shape; pure host arithmetic).
 *   Status, all before any HIP call, in this order: ARCQ_ERR_SHAPE for a shape outside the rules above (the quantiser's rules first,
 *   then M or N < 0 and N % 16); ARCQ_ERR_SHAPE for a bad out_dtype; M == 0 or N == 0 returns ARCQ_OK; ARCQ_ERR_NULL for a NULL operand
 *   (X, the norm weight, reorder_index; then MRW, MRSF, D / ACT); ARCQ_ERR_UNSUPPORTED for a valid shape that
 *   arcq_mx_linear_fused_supported refuses; ARCQ_ERR_SHAPE for a misaligned pointer (X, the norm weight, reorder_index, MRW, D / ACT 16
 *   bytes; MRSF 4 bytes; bias, residual 2 bytes).
 * It is a capability, not a recommendation: every workgroup repeats the quantisation of all M * KQ elements (see DESIGN.md 3.6 "the
 * prologue-fused linear" for what was measured on MI355X, the losses included). */
#define ARCQ_SRC_PLAIN 3     /* beside ARCQ_SRC_RMSNORM */
int arcq_mx_linear_fused_supported(int kind, int64_t M, int64_t N, int64_t KQ, int64_t KE);
int64_t arcq_mx_linear_fused_workgroups(int kind, int64_t N, int64_t KQ, int64_t KE);
int64_t arcq_mx_linear_fused_lds_bytes(int kind, int64_t KQ, int64_t KE);   /* the left side of the budget above */
/* D = alpha * matmul(mx_rmsnorm_quantize_x(X, Wn, eps, reorder_index, KE), W) (+ bias) (+ residual, which may alias D); arguments as in
 * arcq_mx_rmsnorm_quantize_x and arcq_gemm_mxfp4_repacked, alpha = alpha_host * (alpha_dev ? *alpha_dev : 1). */
int arcq_mx_linear_rmsnorm_repacked(const void *X, const void *Wn, float eps, const int16_t *reorder_index, const uint8_t *MRW,
                                    const uint8_t *MRSF, void *D, int64_t M, int64_t N, int64_t KQ, int64_t KE, float alpha_host,
                                    const float *alpha_dev, const void *bias, const void *residual, int out_dtype, void *stream);
/* The gate|up projection: the weight's rows interleave gate and up; ACT = bf16 [M, N/2] as arcq_gemm_mxfp4_repacked_silu_mul writes it. */
int arcq_mx_linear_rmsnorm_silu_repacked(const void *X, const void *Wn, float eps, const int16_t *reorder_index, const uint8_t *MRW,
                                         const uint8_t *MRSF, void *ACT, int64_t M, int64_t N, int64_t KQ, int64_t KE, float alpha_host,
                                         const float *alpha_dev, const void *bias, void *stream);
/* D = alpha * matmul(mx_quantize_x(X, reorder_index, KE), W) (+ bias) (+ residual, which may alias D). */
int arcq_mx_linear_quantize_repacked(const void *X, const int16_t *reorder_index, const uint8_t *MRW, const uint8_t *MRSF, void *D,
                                     int64_t M, int64_t N, int64_t KQ, int64_t KE, float alpha_host, const float *alpha_dev,
                                     const void *bias, const void *residual, int out_dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ARCQ_H_ */
