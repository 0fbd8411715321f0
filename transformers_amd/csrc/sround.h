// sround.h -- stochastic rounding fp32 -> bf16 with counter-based random bits (optim.hip: TamdAdamW(stochastic_rounding=True),
// tamd_sr_round).
//
// Why: an AdamW step at lr = 2e-5 moves a weight of magnitude 0.02 by a sixth of a bf16 ulp (2^-13 in [2^-6, 2^-5)); rounded to
// nearest, the stored weight never moves.  Rounded up or down with probability equal to its position between the two bf16
// neighbours, the expected stored value IS the fp32 value, and sub-ulp updates accumulate as a random walk with the right drift
// -- without a second (fp32) copy of the parameters.
//
// Rounding rule, sr_bf16(x, r16), r16 in [0, 65535]:
//     exponent field of x == 0xFF (inf / NaN):  f32_to_bf16_bits(x), the round-to-nearest conversion
//     otherwise:                                (bits(x) + r16) >> 16
// The addition works on the sign-magnitude pattern: x moves AWAY from zero with probability (low 16 bits of x) / 65536, the same
// for x and -x; a value that is already a bf16 (low 16 bits zero) never moves.  A finite x within the last bf16 ulp below the
// largest bf16 (|x| > 0x7F7F0000) rounds to +-inf with the probability the rule gives it -- the carry runs into the exponent,
// as for every other binade.
//
// Random bits, sr_bits(key, step, i): a pure function of
//     key   64-bit word of the TENSOR.  The optimizer's is attn_seed_mix(seed + ordinal) mod 2^64 (dropout.h: splitmix64's
//           finaliser), seed = its 63-bit seed, ordinal = the parameter's position across all param_groups (state_dict()'s
//           numbering); the host computes it and hands it over in the table (transformers_amd/ops.py `sr_key`, the one
//           definition) -- the kernels only ever see the key
//     step  the optimizer step count of that tensor
//     i     the element's index inside the tensor (64-bit)
// and of nothing else -- not of the workgroup, chunk, table slot or vector / scalar path that handles the element:
//     s = key + step * 0x9E3779B97F4A7C15                          (mod 2^64: one Weyl step per optimizer step)
//     w = dropout_hash(lo32(s), hi32(s), lo32(i >> 1), hi32(i >> 1))   (dropout.h; three 32-bit multiplies per element PAIR)
//     r16 = (i & 1) ? w >> 16 : w & 0xffff
// The host evaluates the same functions (tamd_sr_bits), so a test can restate a kernel's output bit for bit.
#pragma once
#include <tamd_types.h>

#include "dropout.h"

namespace tamd {

// the per-(tensor, step) stream word
__host__ __device__ __forceinline__ unsigned long long sr_stream(unsigned long long key, unsigned long long step) {
  return key + step * 0x9E3779B97F4A7C15ull;
}
// the 32 bits of element pair `pair` = i >> 1: low half for the even element, high half for the odd one
__host__ __device__ __forceinline__ unsigned sr_pair_word(unsigned long long stream, unsigned long long pair) {
  return dropout_hash((unsigned)stream, (unsigned)(stream >> 32), (unsigned)pair, (unsigned)(pair >> 32));
}
// r16 of element i of the stream's tensor
__host__ __device__ __forceinline__ unsigned sr_elem_bits(unsigned long long stream, unsigned long long i) {
  const unsigned w = sr_pair_word(stream, i >> 1);
  return (i & 1) ? (w >> 16) : (w & 0xffffu);
}
__host__ __device__ __forceinline__ unsigned sr_bits(unsigned long long key, unsigned long long step, unsigned long long i) {
  return sr_elem_bits(sr_stream(key, step), i);
}

__host__ __device__ __forceinline__ unsigned short sr_bf16(float x, unsigned r16) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  if ((u & 0x7f800000u) == 0x7f800000u) return f32_to_bf16_bits(x);
  return (unsigned short)((u + r16) >> 16);
}
// two neighbouring elements (even, odd) with the pair's word, packed as they are stored
__host__ __device__ __forceinline__ unsigned sr_pack2_bf16(float even, float odd, unsigned w) {
  return (unsigned)sr_bf16(even, w & 0xffffu) | ((unsigned)sr_bf16(odd, w >> 16) << 16);
}

}  // namespace tamd
