// How the quantising M <= kMxSmallM kernels end (mx_slice_quant_kernel in gemm_mx.hip, mx_slice_rw_quant_kernel in gemm_mx_slice_rw.hip),
// included as statements once the K loop has left each wave's partial sums of the workgroup's four 16-column fragments in acc[0 .. 3].
// In scope: p, part, act, acc, tid, lane, wave, r16, q, n0, m0.  The eight partial sums are added w = 0 .. 7; waves 0 .. 3 each finish
// one fragment and put its activations into LDS; 16 threads then quantise one row's block each (mx_quantize_act_block).
#pragma unroll
  for (int j = 0; j < kMxSliceFrags; ++j) *reinterpret_cast<f32x4*>(part[wave][j][lane]) = acc[j];
  __syncthreads();
  if (wave < kMxSliceFrags) {                                  // wave j: fragment j, y-columns [16 j, 16 j + 16) of the slice
    const float alpha = p.alpha_host * (p.alpha_dev ? *p.alpha_dev : 1.0f);
    f32x4 t = *reinterpret_cast<const f32x4*>(part[0][wave][lane]);
#pragma unroll
    for (int w = 1; w < kMxSmallWaves; ++w) {
      const f32x4 o = *reinterpret_cast<const f32x4*>(part[w][wave][lane]);
#pragma unroll
      for (int r = 0; r < 4; ++r) t[r] += o[r];
    }
    const bool odd = lane & 1;
    const int nl = wave * 16 + r16;
    const float bias = p.bias ? bf16_bits_to_f32(p.bias[n0 + nl]) : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const uint32_t pk = mx_silu_pair(mx_y_bits(alpha, t[r], p.bias, bias), mx_y_bits(alpha, t[r + 1], p.bias, bias), odd);
      const int ml = 4 * q + r + (odd ? 1 : 0);
      if (!(lane & 2)) *reinterpret_cast<uint32_t*>(act + ml * kMxSliceActRowBytes + (nl >> 1) * 2) = pk;
    }
  }
  __syncthreads();
  if (tid < 16 && m0 + tid < p.M) mx_quantize_act_block(p, act + tid * kMxSliceActRowBytes, m0 + tid, (int)blockIdx.x);
