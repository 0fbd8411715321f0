// moe_gate.inc -- the gate product of the sigmoid routers, with an fp32 result (included at the end of elementwise.hip, behind
// moe_router.inc).
//
// Replaces `F.linear(hidden_states.type(torch.float32), self.weight.type(torch.float32))` of DeepseekV3TopkRouter.forward
// (models/deepseek_v3/modeling_deepseek_v3.py:145-147): two casts -- the whole gate weight on every call -- and an fp32 GEMM.
//   tamd_moe_gate_f32   logits[t, e] = sum_h f32(x[t, h]) * f32(w[e, h]), the fp32 accumulators stored unrounded
// A 16-bit x 16-bit product is exact in fp32, so the result differs from the reference's fp32 F.linear in the order of the
// summation alone.  That order is fixed: v_mfma_f32_16x16x32 over 32-element steps of hidden, the NW waves of a workgroup each
// own a contiguous run of steps ([steps * w / NW, steps * (w + 1) / NW)) and wave 0 adds the partial sums of waves 1 .. NW - 1
// in ascending order out of LDS.  No atomics.
// Tokens are the A operand (rows m), experts the B operand (columns n): lane l loads 16 contiguous bytes of
// x[t0 + (l & 15)][k + 8 (l >> 4) ..] and of w[e0 + (l & 15)][the same k]; accumulator register r of lane l is
// logits[t0 + 4 (l >> 4) + r][e0 + (l & 15)], so a store instruction writes 16 consecutive floats per token.
// Rows past the last token / expert are loaded from the last valid row (always inside the operands) and never stored.
//   tokens <= 16:  one 16-token block against 8 expert rows per workgroup (lanes with (l & 15) >= 8 repeat rows 0 .. 7 and store
//                  nothing), 16 waves over hidden: experts / 8 workgroups x 16 waves stream w once (gemv.hip's header: with 16
//                  rows per workgroup only experts / 16 <= 16 CUs would pull on HBM)
//   above:         32 tokens x 64 experts per workgroup, 8 waves over hidden; w (<= 3.7 MB) stays in L2

namespace tamd {

template <typename T, int MT, int NT, int NW, bool HALF>
__global__ __launch_bounds__(NW * 64) void moe_gate_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                            float* __restrict__ logits, int64_t tokens, int E, int H, int64_t ldx,
                                                            int64_t lde) {
  static_assert(!HALF || NT == 1, "the 8-row block is one column block");
  __shared__ float red[NW - 1][MT * NT][64][4];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int l15 = lane & 15, g4 = lane >> 4;
  const int64_t t0 = (int64_t)blockIdx.x * (MT * 16);
  const int e0 = (int)blockIdx.y * (HALF ? 8 : NT * 16);
  const T* xp[MT];
  const T* wp[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int64_t t = t0 + i * 16 + l15 < tokens ? t0 + i * 16 + l15 : tokens - 1;
    xp[i] = x + t * ldx + g4 * 8;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int e = HALF ? e0 + (l15 & 7) : (e0 + j * 16 + l15 < E ? e0 + j * 16 + l15 : E - 1);
    wp[j] = w + (int64_t)e * H + g4 * 8;
  }
  const int steps = H / 32;
  const int s0 = (int)((int64_t)steps * wave / NW), s1 = (int)((int64_t)steps * (wave + 1) / NW);
  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // U steps per round, every load of the round issued before its first MFMA; a step past s1 multiplies zeros
  constexpr int U = (MT + NT) <= 2 ? 8 : 2;
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int st = s0; st < s1; st += U) {
    u32x4 a[MT][U], b[NT][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in = st + u < s1;
      const int k = (st + u) * 32;
#pragma unroll
      for (int i = 0; i < MT; ++i) a[i][u] = in ? ld16(xp[i] + k) : z;
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j][u] = in ? ld16(wp[j] + k) : z;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = mfma16<T>(a[i][u], b[j][u], acc[i][j]);
  }
  if (wave != 0) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave - 1][i * NT + j][lane][r] = acc[i][j][r];
  }
  block_sync();
  if (wave != 0) return;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int e = e0 + j * 16 + l15;
      const bool ecol = HALF ? l15 < 8 : e < E;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r];
        for (int ww = 1; ww < NW; ++ww) v = v + red[ww - 1][i * NT + j][lane][r];  // waves ascending
        const int64_t t = t0 + i * 16 + 4 * g4 + r;
        if (ecol && t < tokens) logits[t * lde + e] = v;
      }
    }
}

}  // namespace tamd

using namespace tamd;

extern "C" {

int tamd_moe_gate_f32(const void* x, const void* w, float* logits, int64_t tokens, int64_t experts, int64_t hidden,
                      int64_t ldx, int64_t lde, int dtype, tamd_stream_t stream) {
  if (!x || !w || !logits) return TAMD_E_NULL;
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  if (tokens <= 0 || tokens >= ((int64_t)1 << 31) || experts <= 0 || experts > kMoeMaxExperts || experts % 8 != 0) return TAMD_E_SHAPE;
  if (hidden <= 0 || hidden % 64 != 0 || hidden >= ((int64_t)1 << 22) || ldx < hidden || lde < experts) return TAMD_E_SHAPE;
  if ((reinterpret_cast<uintptr_t>(x) & 15u) || (reinterpret_cast<uintptr_t>(w) & 15u) || (ldx & 7) ||
      (reinterpret_cast<uintptr_t>(logits) & 3u))
    return TAMD_E_ALIGN;
  const int E = (int)experts, H = (int)hidden;
  TAMD_DISPATCH_HALF(dtype, {
    if (tokens <= 16) {
      const dim3 grid(1, (unsigned)(E / 8)), block(16 * 64);
      hipLaunchKernelGGL((moe_gate_kernel<T, 1, 1, 16, true>), grid, block, 0, TAMD_STREAM(stream), (const T*)x, (const T*)w,
                         logits, tokens, E, H, ldx, lde);
    } else {
      const dim3 grid((unsigned)((tokens + 31) / 32), (unsigned)((E + 63) / 64)), block(8 * 64);
      hipLaunchKernelGGL((moe_gate_kernel<T, 2, 4, 8, false>), grid, block, 0, TAMD_STREAM(stream), (const T*)x, (const T*)w,
                         logits, tokens, E, H, ldx, lde);
    }
  });
  return launch_status();
}

}  // extern "C"
