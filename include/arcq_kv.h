/*
 * arcq_kv.h -- the KV-cache half of the reference's operator module on gfx950: the paged cache writers and the decode attention
 * behind `init_kv_*`, `append_kv_*` and `batch_decode_*` (kernels/src/bindings.cpp:287-581, kernels/src/flashinfer.cu,
 * model/kv_cache.py).  Python mirror: arcquant_amd/kvcache.py.  Status codes and arcq_last_error() are those of arcq.h.
 *
 * FORMAT (the reference's, include/flashinfer/page.cuh:76-103), head dimension 128 only:
 *   kv_data   ARCQ_KV_INT4: uint8 [pages, L, 2, N, P, 64]; byte j of a row holds element 2j in its low nibble and 2j+1 in its high one
 *             ARCQ_KV_16BIT: 16-bit values [pages, L, 2, N, P, 128] (fp16 or bf16, see `dtype`)
 *   kv_param  fp16 [pages, L, 2, N, P, 2] = (scale, zero); an int4 value is float(code) * float(scale) - float(zero) in fp32.
 *             ARCQ_KV_16BIT stores the parameters and decode does not apply them (vec_dtypes.cuh:67-68).
 *   index 2 is K then V, N kv heads, P entries per page (any P >= 1).
 *   kv_indptr int32 [B + 1], kv_indices int32 [nnz], last_page_offset int32 [B]: sequence b owns the pages
 *             kv_indices[kv_indptr[b] .. kv_indptr[b+1]) in order and holds
 *             (kv_indptr[b+1] - kv_indptr[b] - 1) * P + last_page_offset[b] positions, the ones init / append write INCLUDED.
 *             A sequence WITHOUT POSITIONS is one for which that count is <= 0.  Two spellings are supported and mean the same: no pages
 *             (kv_indptr[b+1] == kv_indptr[b]) with last_page_offset[b] = 0, where the formula gives -P, and one page with
 *             last_page_offset[b] = 0, where it gives 0.  Neither has a page entry read or written.
 *
 * THE CONTENTS OF THE INDEX TENSORS ARE THE CALLER'S CONTRACT, as in the reference: kv_indptr non-decreasing from 0 with
 * kv_indptr[B] <= nnz, every kv_indices entry a page of kv_data, 1 <= last_page_offset[b] <= P for a non-empty sequence,
 * seqlen_indptr non-decreasing from 0 with seqlen_indptr[B] <= ntok and no sequence appended to beyond its length.  They live on the
 * device and are not read on the host; a call that breaks the contract reads or writes wherever the tables point.
 *
 * Every shape, NULL and alignment check runs before any HIP call.  B == 0 (and ntok == 0 for the init pair) returns ARCQ_OK.
 * Alignment: kv_data, k, v, q, o 16 bytes; kv_param, k_param, v_param, the index tensors, the workspace and the state 4 bytes.
 * No entry point reads a byte of kv_data / kv_param outside the valid positions of the pages the tables name in layer `layer_idx`,
 * and the writers change the rows they are asked to write and nothing else.
 */
#ifndef ARCQ_KV_H_
#define ARCQ_KV_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARCQ_KV_INT4 0  /* cache format: 4-bit codes + (scale, zero) */
#define ARCQ_KV_16BIT 1 /* cache format: 16-bit values (the reference's `_f16` trio) */
#define ARCQ_KV_F16 0   /* element dtype of q / o / k / v (and of an ARCQ_KV_16BIT cache): float16, the reference's */
#define ARCQ_KV_BF16 1  /* bfloat16, the harness's */

/* Prefill write (AppendPagedKVCachePrefillKernel): k, v = rows [ntok, N, 64 bytes | 128 x 16 bit], k_param, v_param = fp16 [ntok, N, 2].
 * Tokens seqlen_indptr[b] .. seqlen_indptr[b+1] become the LAST positions of sequence b, in order. */
int arcq_kv_init(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset,
                 const void *k, const void *v, const void *k_param, const void *v_param, const int32_t *seqlen_indptr, int64_t ntok,
                 int64_t B, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int format, void *stream);

/* Decode write (AppendPagedKVCacheDecodeKernel): one token per sequence, k, v = rows [B, N, .], written at position seq_len - 1. */
int arcq_kv_append(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset,
                   const void *k, const void *v, const void *k_param, const void *v_param, int64_t B, int64_t L, int64_t layer_idx,
                   int64_t N, int64_t P, int format, void *stream);

/* arcq_kv_append with the quantiser in front, ONE launch (the reference: five torch launches per tensor, kv_cache.py:22-33, then
 * append_kv_i4): k, v = `dtype` [B, N, 128].  Each (token, head) row is quantised as torch eager computes
 *     scale = (amax - amin).clamp(min=1e-5) / 15;  zero = -amin;  code = clamp(round((x + zero) / scale), 0, 15)
 * on a CPU tensor of `dtype` (every operation rounded to `dtype`, round half to even), parameters then converted to fp16; codes and
 * parameters go straight into the page.  ARCQ_KV_INT4 only (ARCQ_KV_16BIT: ARCQ_ERR_UNSUPPORTED).  Inputs are finite. */
int arcq_kv_append_quantize(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                            const int32_t *last_page_offset, const void *k, const void *v, int64_t B, int64_t L, int64_t layer_idx, int64_t N,
                            int64_t P, int format, int dtype, void *stream);

/* arcq_kv_init with the same quantiser in front: k, v = `dtype` [ntok, N, 128]. */
int arcq_kv_init_quantize(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset,
                          const void *k, const void *v, const int32_t *seqlen_indptr, int64_t ntok, int64_t B, int64_t L, int64_t layer_idx,
                          int64_t N, int64_t P, int format, int dtype, void *stream);

/* Bytes of fp32 scratch arcq_kv_batch_decode needs for this call (0: none, the workspace may be NULL).  nnz = entries of kv_indices. */
int64_t arcq_kv_decode_workspace_bytes(int64_t B, int64_t Nq, int64_t N, int64_t nnz, int64_t P);

/* Decode attention: o, q = `dtype` [B, Nq, 128], Nq = g * N; query head h reads kv head h / g (g == 1 is the reference's contract),
 * and the g query heads of a kv head share one pass over its rows.
 *     o[b, h] = softmax_t(q[b, h] . K[t] / sqrt(128)) V[t]   over the positions of sequence b, no RoPE (flashinfer.cu:26-31; a model
 * that rotates does so when it writes: arcq_kv_rope_append_quantize / arcq_kv_rope_init_quantize / arcq_rope_qk below), fp32 accumulation, rounded once to `dtype`.  A sequence without positions gives zeros.  nnz = entries of kv_indices: it sizes the
 * slices, so pass what arcq_kv_decode_workspace_bytes was asked with; workspace_bytes >= that query's answer (0: workspace may be NULL). */
int arcq_kv_batch_decode(void *o, const void *q, const void *kv_data, const void *kv_param, const int32_t *kv_indptr,
                         const int32_t *kv_indices, const int32_t *last_page_offset, int64_t B, int64_t Nq, int64_t L, int64_t layer_idx,
                         int64_t N, int64_t P, int64_t nnz, int format, int dtype, void *workspace, int64_t workspace_bytes, void *stream);

/* Causal prefill attention over the pages: several query tokens per sequence, each attending over everything the cache holds up to and
 * including its own position.  o, q = `dtype` [ntok, Nq, 128], contiguous, Nq = g * N.  qo_indptr = int32 [B + 1] on the device,
 * non-decreasing from 0 with qo_indptr[B] <= ntok (the caller's contract, like the other tables): sequence b has
 * n_b = qo_indptr[b+1] - qo_indptr[b] query tokens, rows qo_indptr[b] .. of q and o.  T_b is what the tables say, as everywhere in
 * this header, and INCLUDES those n_b tokens: the caller has written them with arcq_kv_init* already, as decode reads the row
 * arcq_kv_append just wrote.  The contract requires n_b <= T_b.  Query i of sequence b sits at position T_b - n_b + i and attends over
 * positions 0 .. T_b - n_b + i; query head h reads kv head h / g:
 *     o[qo_indptr[b] + i, h] = softmax_{t <= T_b - n_b + i}(q[qo_indptr[b] + i, h] . K[t] / sqrt(128)) V[t],   no RoPE,
 * scores on the exact 4-bit codes (K is never rounded to 16 bit), softmax in fp32, the weights p_t s_t rounded once to `dtype` for the
 * matrix cores (fp16: a weight below 2^-14 is rounded on the subnormal grid, 2^-25 absolute), one rounding of the result to `dtype`.
 * n_b = 1 for every b is arcq_kv_batch_decode's contract; n_b = 0 writes nothing for that sequence; rows of o at or beyond qo_indptr[B]
 * are not written, and nothing else is.  B == 0 or ntok == 0 returns ARCQ_OK without a launch.  ARCQ_KV_INT4 only (ARCQ_KV_16BIT:
 * ARCQ_ERR_UNSUPPORTED).  No workspace, no state, no host read of a device table: the call can be captured into a HIP graph.
 * nnz = entries of kv_indices (range-checked only).
 * KNOWN LIMIT: the kv range of a sequence is not split over workgroups.  A launch has one workgroup per (sequence, kv head, 128 / g query
 * tokens), so a few query tokens over a very long cache (speculative verification at batch size 1) run on B * N workgroups. */
int arcq_kv_batch_prefill(void *o, const void *q, const int32_t *qo_indptr, const void *kv_data, const void *kv_param,
                          const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset, int64_t ntok, int64_t B,
                          int64_t Nq, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int64_t nnz, int format, int dtype, void *stream);

/* Bytes of the decode step's state: one int32 arrival counter per (sequence, kv head, chunk of <= 4 of its g = Nq / N query heads). */
int64_t arcq_kv_decode_step_state_bytes(int64_t B, int64_t Nq, int64_t N);

/* The whole decode step of an ARCQ_KV_INT4 cache in ONE launch: arcq_kv_append_quantize of k, v followed by arcq_kv_batch_decode of q,
 * bit for bit (pages, parameters and o), without the launches in between.  q = `dtype` rows [B, Nq, 128] and k, v = rows [B, N, 128] whose
 * heads are contiguous and whose tokens lie q_stride / kv_stride ELEMENTS apart (>= Nq * 128 / N * 128, multiples of 8): the three may be
 * slices of one [B, (Nq + 2 N) * 128] projection output.  o = `dtype` [B, Nq, 128], contiguous.  The tables describe the sequences
 * INCLUDING the position being written, as for arcq_kv_append; that position is taken from k, v and the result does not depend on what
 * the page held there.  An empty sequence writes nothing and gives zeros.  ARCQ_KV_16BIT: ARCQ_ERR_UNSUPPORTED.
 * workspace: arcq_kv_decode_workspace_bytes(B, Nq, N, nnz, P) bytes of scratch, contents don't-care.
 * state: arcq_kv_decode_step_state_bytes(B, Nq, N) bytes, 4-byte aligned.  The caller zero-fills it ONCE after allocation; every call
 * whose kernel completes leaves it all zero, so it is reused without clearing.  Calls that share a state (or a workspace) are
 * stream-ordered.  When the workspace query answers 0 neither is touched and both may be NULL.  No workgroup waits for another. */
int arcq_kv_decode_step(void *o, const void *q, const void *k, const void *v, int64_t q_stride, int64_t kv_stride, void *kv_data,
                        void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices, const int32_t *last_page_offset, int64_t B,
                        int64_t Nq, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int64_t nnz, int format, int dtype, void *workspace,
                        int64_t workspace_bytes, void *state, int64_t state_bytes, void *stream);

/* ---- Rotary position embedding (RoPE) on the KV path.  The attention entry points above apply none ("no RoPE"): the rotation is done
 * at WRITE time, as the reference's model path does (apply_rotary_pos_emb, then past_key_value.update): the cache holds rotated keys and
 * attention reads them as they are.  Head dimension 128, full rotation, rotate-half pairing.
 *   cos, sin  `dtype` [rope_len, 128], contiguous, 16-byte aligned: the Hugging Face tables (emb = cat(freqs, freqs); emb.cos().to(dtype)).
 *             Element i of a row at position p reads cos[p, i] and sin[p, i]; the two halves of a table row are not assumed equal and
 *             no trigonometry is computed here (NTK / YaRN / Llama-3.1 scaling live in the caller's table).
 *   result    rot(x)[i] = -x[i + 64] for i < 64, x[i - 64] otherwise, and
 *                 out[i] = dtype(dtype(x[i] * cos[p, i]) + dtype(rot(x)[i] * sin[p, i]))
 *             with the products and the sum in fp32: THREE roundings, bit for bit what torch eager gives on a CPU tensor of `dtype` for
 *             x * cos + rotate_half(x) * sin.  Inputs and results are finite.
 * Every position used is < rope_len: the caller's contract, like the index tables; it is not read on the host.
 * No workspace, no state, no host read of a device table: the three calls can be captured into a HIP graph. */

/* The rotation alone, IN PLACE: q = `dtype` rows [ntok, Nq, 128] and k = rows [ntok, N, 128] whose heads are contiguous and whose tokens lie
 * q_stride / k_stride ELEMENTS apart (>= Nq * 128 / N * 128, multiples of 8), as for arcq_kv_decode_step.  Token i is rotated to
 * positions[i % n_pos]; positions = int32 [n_pos] on the device, n_pos >= 1 divides ntok (n_pos = ntok: the general case; n_pos = q_len:
 * a batch of equal-length sequences; n_pos = 1: a decode step).  N == 0: k is not touched and may be NULL; otherwise Nq % N == 0.
 * ntok == 0 returns ARCQ_OK without a launch.  No two rows may overlap. */
int arcq_rope_qk(void *q, void *k, int64_t q_stride, int64_t k_stride, const int32_t *positions, int64_t n_pos, const void *cos,
                 const void *sin, int64_t rope_len, int64_t ntok, int64_t Nq, int64_t N, int dtype, void *stream);

/* arcq_kv_append_quantize with the rotation in front, and the query's rotation with it, ONE launch: token b is written at position
 * seq_len(b) - 1 and that is the position its q and k rows are rotated to (no position tensor).  q = rows [B, Nq, 128], k, v = rows
 * [B, N, 128] with token strides q_stride / kv_stride as above (the three may be slices of one [B, (Nq + 2 N) * 128] projection output);
 * q_out = `dtype` [B, Nq, 128], contiguous: the rotated q.  It may be exactly q when q is contiguous; otherwise it must not overlap q
 * (nor k, v).  k is rotated and then quantised, v is quantised as it is.  A sequence without positions writes nothing, its q_out rows
 * included.  GUARANTEED: pages, parameters and q_out equal, byte for byte, arcq_rope_qk (positions = seq_len - 1) followed by
 * arcq_kv_append_quantize and a copy of q.  ARCQ_KV_16BIT: ARCQ_ERR_UNSUPPORTED.  B == 0 returns ARCQ_OK without a launch. */
int arcq_kv_rope_append_quantize(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                                 const int32_t *last_page_offset, void *q_out, const void *q, const void *k, const void *v, int64_t q_stride,
                                 int64_t kv_stride, const void *cos, const void *sin, int64_t rope_len, int64_t B, int64_t Nq, int64_t L,
                                 int64_t layer_idx, int64_t N, int64_t P, int format, int dtype, void *stream);

/* The same in front of arcq_kv_init_quantize: tokens seqlen_indptr[b] .. seqlen_indptr[b+1] become the last positions of sequence b and
 * are rotated to them.  Rows of q_out at or beyond seqlen_indptr[B] are not written.  B == 0 or ntok == 0 returns ARCQ_OK without a launch. */
int arcq_kv_rope_init_quantize(void *kv_data, void *kv_param, const int32_t *kv_indptr, const int32_t *kv_indices,
                               const int32_t *last_page_offset, void *q_out, const void *q, const void *k, const void *v, int64_t q_stride,
                               int64_t kv_stride, const void *cos, const void *sin, int64_t rope_len, const int32_t *seqlen_indptr, int64_t ntok,
                               int64_t B, int64_t Nq, int64_t L, int64_t layer_idx, int64_t N, int64_t P, int format, int dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ARCQ_KV_H_ */
