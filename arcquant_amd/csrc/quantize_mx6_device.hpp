// The MXFP6 block rule (include/arcq.h "MXFP6-ARC"), stated once: the e3m2 element, the block exponent for a maximum of 28 and the
// packing of 32 six-bit codes into six dwords.  Integer and exact fp32 arithmetic only, and every function is __host__ __device__: the
// same text can be run on the CPU against tests/mx6_reference.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace arcq {

#define ARCQ_HD __host__ __device__ __forceinline__

// Smallest e with amax <= 28 * 2^e, clamped to [-127, 127]; 0 for amax == 0.  Exact, from the fp32 bits of amax (a widened bf16):
// amax = m * 2^E with m in [1, 2) -> 28 * 2^e = 1.75 * 2^(e+4) >= m * 2^E  <=>  e >= E - 4 when m <= 1.75, else E - 3.
// Subnormal amax (< 2^-126) always lands on the clamp.
ARCQ_HD int mx6_block_exponent(float amax) {
  const uint32_t u = __builtin_bit_cast(uint32_t, amax);
  const int ef = (int)(u >> 23);
  if (u == 0) return 0;
  if (ef == 0) return -127;
  const int E = ef - 127;
  const int e = (u & 0x7fffffu) <= 0x600000u ? E - 4 : E - 3;
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// |y| <= 28 -> e3m2 code (bit 5 sign, bits 4:2 exponent with bias 3, bits 1:0 mantissa), round to nearest, ties to the even code, sign
// of zero kept.  The magnitude codes 0 .. 31 are monotone in the value and the subnormals 0.0625 * {0..3} run into the normals without
// a gap (code 4 = 0.25), so: below 0.25 the code is RNE(|y| * 16) (4 when it rounds up to 0.25); from 0.25 on it is the fp32 exponent
// and the top two mantissa bits re-biased (127 - 3 = 124), rounded on the 21 bits below with the carry running into the exponent.
ARCQ_HD uint32_t f32_to_e3m2(float y) {
  const uint32_t u = __builtin_bit_cast(uint32_t, y), a = u & 0x7fffffffu;
  const uint32_t t = a - (124u << 23);
  const uint32_t normal = (t + 0xfffffu + ((t >> 21) & 1u)) >> 21;
  const uint32_t sub = (uint32_t)__builtin_rintf(__builtin_bit_cast(float, a) * 16.0f);
  return (a < (125u << 23) ? sub : normal) | ((u >> 31) << 5);
}

ARCQ_HD float e3m2_to_f32(uint32_t c) {
  const uint32_t m = c & 31u;
  const float a = m < 4u ? (float)m * 0.0625f : __builtin_bit_cast(float, (m << 21) + (124u << 23));
  return (c & 32u) ? -a : a;
}

struct Mx6Block {
  uint32_t w[6];  // 32 codes: element i in bits [6 i, 6 i + 6) of the 192-bit little-endian string
  uint32_t s8;    // E8M0 byte = e + 127
};

// 32 values -> codes.  v * 2^-e is exact (ldexp) and |v * 2^-e| <= 28: no code saturates.  kResid: v[] is overwritten with the
// residual v - deq(code) * 2^e, exact in bf16 (formed at half scale, as mx_quantize_block does and for its reason).
template <bool kResid>
ARCQ_HD Mx6Block mx6_quantize_block(float (&v)[32]) {
  float amax = 0.0f;
#pragma unroll
  for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(v[i]));
  const int e = mx6_block_exponent(amax);
  Mx6Block b;
#pragma unroll
  for (int d = 0; d < 6; ++d) b.w[d] = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const uint32_t c = f32_to_e3m2(__builtin_ldexpf(v[i], -e));
    const int d = (6 * i) >> 5, sh = (6 * i) & 31;                 // (compile-time after unrolling)
    b.w[d] |= c << sh;
    if (sh > 26) b.w[d + 1] |= c >> (32 - sh);
    if (kResid) v[i] = 2.0f * (0.5f * v[i] - __builtin_ldexpf(e3m2_to_f32(c), e - 1));
  }
  b.s8 = (uint32_t)(e + 127);
  return b;
}

// One e3m2 operand fragment (six dwords, element i in bits [6 i, 6 i + 6)) -> the codes of magnitude >= 2 (exponent field >= 4, i.e. bit 4
// of the code) in `hi` and the others in `lo`, the rest of each +0: hi + lo = the fragment, value for value.  gemm_mx6.hip multiplies the
// two against an e3m2 weight separately (the reason is in its header).  Bit 4 of every field is isolated (mx6_bit4_mask), and ORed with itself
// shifted by +1 .. -4 across the dword borders it covers exactly its own field: fields do not overlap.
ARCQ_HD constexpr uint32_t mx6_bit4_mask(int d) {
  uint32_t m = 0;
  for (int i = 0; i < 32; ++i)
    if ((6 * i + 4) >> 5 == d) m |= 1u << ((6 * i + 4) & 31);
  return m;
}
ARCQ_HD uint32_t mx6_shr(uint32_t up, uint32_t cur, int s) { return (uint32_t)((((uint64_t)up << 32) | cur) >> s); }   // v_alignbit_b32
ARCQ_HD void mx6_split_fragment(const uint32_t (&w)[6], uint32_t (&hi)[6], uint32_t (&lo)[6]) {
  uint32_t t[8];
  t[0] = t[7] = 0;
#pragma unroll
  for (int d = 0; d < 6; ++d) t[d + 1] = w[d] & mx6_bit4_mask(d);
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    const uint32_t dn = t[d], cur = t[d + 1], up = t[d + 2];
    const uint32_t f = cur | mx6_shr(cur, dn, 31) | mx6_shr(up, cur, 1) | mx6_shr(up, cur, 2) | mx6_shr(up, cur, 3) | mx6_shr(up, cur, 4);
    hi[d] = w[d] & f;
    lo[d] = w[d] & ~f;
  }
}

}  // namespace arcq
