// moe_router.inc -- the router of a sparse mixture-of-experts block (included at the end of elementwise.hip, behind moe_route.inc).
//
// Replaces the chain of small ATen ops behind the gate product of the reference's routers (MixtralTopKRouter.forward,
// models/mixtral/modeling_mixtral.py; Qwen2MoeTopKRouter / Qwen3MoeTopKRouter / OlmoeTopKRouter: softmax(dtype=float), topk,
// sum, div, .to()):
//   tamd_moe_router_fwd   logits [T, E] -> w [T, k], idx [T, k]: softmax over the experts, the k largest, optional renormalisation
//   tamd_moe_router_bwd   logits, idx, dw [T, k] -> dlogits [T, E]; m, x, Z, p are recomputed exactly as the forward computes them
// One wave per token, four tokens per 256-thread workgroup.  Lane L holds experts L, 64 + L, 128 + L, 192 + L in registers
// (NR = 1, 2 or 4 of them), so an expert's id is r * 64 + lane: a lane's experts are NOT contiguous, and the arg-max is reduced
// on the pair (logit descending, id ascending), never on the lane.  Reductions are the xor butterflies of wave_max / wave_sum.
// No LDS, no atomics, no host synchronisation; every launch parameter is a function of (T, E, k).

namespace tamd {

constexpr int kRouterMaxTopK = 16;
constexpr float kRouterNoId = 1.0e9f;  // the id of "nothing": loses every tie against a real expert (ids are exact in fp32)

// One token's softmax pieces: l (fp32 logits, -inf past E), m = max, x = exp(l - m) (0 past E), Z = sum x
// (every lane sums its registers r ascending, then the butterfly of wave_sum: a fixed order).
template <typename T, int NR>
__device__ __forceinline__ void router_softmax(const T* __restrict__ row, int E, int lane, float* l, float* x, float& m, float& Z) {
  using raw = typename elem<T>::raw;
  float lm = -INFINITY;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int e = r * 64 + lane;
    l[r] = e < E ? elem<T>::to_f32(reinterpret_cast<const raw*>(row)[e]) : -INFINITY;
    lm = fmaxf(lm, l[r]);
  }
  m = wave_max(lm);
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    x[r] = (r * 64 + lane) < E ? expf(l[r] - m) : 0.f;
    s = s + x[r];
  }
  Z = wave_sum(s);
}

// w[t, j], idx[t, j]: the chain of include/tamd.h (tamd_moe_router_fwd)
template <typename T, int NR, bool WF32>
__global__ __launch_bounds__(kMoeThreads) void moe_router_fwd_kernel(const T* __restrict__ logits, void* __restrict__ w,
                                                                      int64_t* __restrict__ idx, int64_t tokens, int E, int k,
                                                                      int64_t lde, int norm) {
  const int lane = lane_id();
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave_id_uniform(); t < tokens; t += (int64_t)gridDim.x * 4) {
    float l[NR], x[NR], m, Z;
    router_softmax<T, NR>(logits + t * lde, E, lane, l, x, m, Z);
    // the selection runs on the logits (a NaN counts as -inf, so a row of anything still yields k distinct ids)
    float sel[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) sel[r] = l[r] != l[r] ? -INFINITY : l[r];
    unsigned taken = 0u;
    float my_p = 0.f, my_id = 0.f, s = 0.f;
    for (int j = 0; j < k; ++j) {
      float bv = -INFINITY, bi = kRouterNoId;
#pragma unroll
      for (int r = 0; r < NR; ++r) {  // r ascending and a strict >: the lowest id among this lane's equals
        const int e = r * 64 + lane;
        if (e < E && !((taken >> r) & 1u) && (bi == kRouterNoId || sel[r] > bv)) {
          bv = sel[r];
          bi = (float)e;
        }
      }
#pragma unroll
      for (int msk = 32; msk >= 1; msk >>= 1) {  // (logit descending, id ascending): a total order, every lane ends with the same pair
        const float ov = shfl_xor_f32(bv, msk), oi = shfl_xor_f32(bi, msk);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      const int wid = (int)bi;
      if ((wid & 63) == lane) taken |= 1u << (wid >> 6);
      // the winner's probability from its logit: the same expression on the same operands as the owner's x / Z
      const float pj = expf(bv - m) / Z;
      s = s + pj;  // j ascending
      if (lane == j) {
        my_p = pj;
        my_id = bi;
      }
    }
    if (lane < k) {
      const float wj = norm ? my_p / s : my_p;
      if (WF32)
        reinterpret_cast<float*>(w)[t * k + lane] = wj;
      else
        reinterpret_cast<typename elem<T>::raw*>(w)[t * k + lane] = elem<T>::from_f32(wj);
      idx[t * k + lane] = (int64_t)my_id;
    }
  }
}

// dlogits[t, e]: the chain of include/tamd.h (tamd_moe_router_bwd).  idx and dw are read uniformly (every lane the same
// address); an id outside [0, E) is skipped.
template <typename T, int NR, bool WF32>
__global__ __launch_bounds__(kMoeThreads) void moe_router_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ idx,
                                                                      const void* __restrict__ dw, T* __restrict__ dlogits,
                                                                      int64_t tokens, int E, int k, int64_t lde, int norm) {
  using raw = typename elem<T>::raw;
  const int lane = lane_id();
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave_id_uniform(); t < tokens; t += (int64_t)gridDim.x * 4) {
    const T* row = logits + t * lde;
    float l[NR], x[NR], m, Z;
    router_softmax<T, NR>(row, E, lane, l, x, m, Z);
    float gsel[NR];    // g_j of the slot that selected this lane's expert r
    unsigned mine = 0u;  // bit r: expert r * 64 + lane is selected
#pragma unroll
    for (int r = 0; r < NR; ++r) gsel[r] = 0.f;
    float pj[kRouterMaxTopK], gj[kRouterMaxTopK];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kRouterMaxTopK; ++j) {
      pj[j] = 0.f;
      gj[j] = 0.f;
      if (j < k) {
        const int64_t id = idx[t * k + j];
        if (id >= 0 && id < E) {
          const float g = WF32 ? reinterpret_cast<const float*>(dw)[t * k + j]
                               : elem<T>::to_f32(reinterpret_cast<const raw*>(dw)[t * k + j]);
          float lj = elem<T>::to_f32(reinterpret_cast<const raw*>(row)[id]);
          pj[j] = expf(lj - m) / Z;  // the forward's p_{e_j}, bit for bit
          gj[j] = g;
          s = s + pj[j];  // j ascending
          if (((int)id & 63) == lane) {
#pragma unroll
            for (int r = 0; r < NR; ++r)
              if (((int)id >> 6) == r) {
                gsel[r] = g;
                mine |= 1u << r;
              }
          }
        }
      }
    }
    float c = 0.f;  // norm: sum_j g_j w_j;  no norm: sum_j p_j g_j  (j ascending, fp32 multiply then fp32 add)
#pragma unroll
    for (int j = 0; j < kRouterMaxTopK; ++j)
      if (j < k) {
        const float wj = norm ? pj[j] / s : pj[j];
        const float prod = gj[j] * wj;
        c = c + prod;
      }
    T* out = dlogits + t * lde;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int e = r * 64 + lane;
      if (e < E) {
        const float p = x[r] / Z;
        const bool on = (mine >> r) & 1u;
        float dl;
        if (norm)
          dl = on ? (p / s) * (gsel[r] - c) : 0.f;
        else
          dl = p * ((on ? gsel[r] : 0.f) - c);
        reinterpret_cast<raw*>(out)[e] = elem<T>::from_f32(dl);
      }
    }
    for (int64_t e = (int64_t)E + lane; e < lde; e += 64) reinterpret_cast<raw*>(out)[e] = elem<T>::from_f32(0.f);
  }
}

static int moe_router_check(int64_t tokens, int64_t experts, int64_t top_k, int64_t lde) {
  if (tokens <= 0 || experts <= 0 || top_k <= 0) return TAMD_E_SHAPE;
  if (experts > kMoeMaxExperts || top_k > kRouterMaxTopK || top_k > experts || lde < experts) return TAMD_E_SHAPE;
  if (tokens >= ((int64_t)1 << 31)) return TAMD_E_SHAPE;
  return TAMD_OK;
}

}  // namespace tamd

using namespace tamd;

#define TAMD_ROUTER_LAUNCH(KERNEL, ...)                                                                                   \
  do {                                                                                                                    \
    const dim3 grid(moe_pair_blocks(tokens)), block(kMoeThreads);                                                         \
    TAMD_DISPATCH_HALF(dtype, {                                                                                           \
      if (experts <= 64) {                                                                                                \
        if (w_dtype == TAMD_F32)                                                                                          \
          hipLaunchKernelGGL((KERNEL<T, 1, true>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);                     \
        else                                                                                                              \
          hipLaunchKernelGGL((KERNEL<T, 1, false>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);                    \
      } else if (experts <= 128) {                                                                                        \
        if (w_dtype == TAMD_F32)                                                                                          \
          hipLaunchKernelGGL((KERNEL<T, 2, true>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);                     \
        else                                                                                                              \
          hipLaunchKernelGGL((KERNEL<T, 2, false>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);                    \
      } else {                                                                                                            \
        if (w_dtype == TAMD_F32)                                                                                          \
          hipLaunchKernelGGL((KERNEL<T, 4, true>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);                     \
        else                                                                                                              \
          hipLaunchKernelGGL((KERNEL<T, 4, false>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);                    \
      }                                                                                                                   \
    });                                                                                                                   \
  } while (0)

extern "C" {

int tamd_moe_router_fwd(const void* logits, void* w, int64_t* top_k_index, int64_t tokens, int64_t experts, int64_t top_k,
                        int64_t lde, int norm, int w_dtype, int dtype, tamd_stream_t stream) {
  if (!logits || !w || !top_k_index) return TAMD_E_NULL;
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  if (w_dtype != TAMD_F32 && w_dtype != dtype) return TAMD_E_DTYPE;
  const int st = moe_router_check(tokens, experts, top_k, lde);
  if (st != TAMD_OK) return st;
  if ((reinterpret_cast<uintptr_t>(logits) & 1u) || (reinterpret_cast<uintptr_t>(top_k_index) & 7u) ||
      (reinterpret_cast<uintptr_t>(w) & (w_dtype == TAMD_F32 ? 3u : 1u)))
    return TAMD_E_ALIGN;
  TAMD_ROUTER_LAUNCH(moe_router_fwd_kernel, (const T*)logits, w, top_k_index, tokens, (int)experts, (int)top_k, lde, norm);
  return launch_status();
}

int tamd_moe_router_bwd(const void* logits, const int64_t* top_k_index, const void* dw, void* dlogits, int64_t tokens,
                        int64_t experts, int64_t top_k, int64_t lde, int norm, int w_dtype, int dtype, tamd_stream_t stream) {
  if (!logits || !top_k_index || !dw || !dlogits) return TAMD_E_NULL;
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  if (w_dtype != TAMD_F32 && w_dtype != dtype) return TAMD_E_DTYPE;
  const int st = moe_router_check(tokens, experts, top_k, lde);
  if (st != TAMD_OK) return st;
  if ((reinterpret_cast<uintptr_t>(logits) & 1u) || (reinterpret_cast<uintptr_t>(dlogits) & 1u) ||
      (reinterpret_cast<uintptr_t>(top_k_index) & 7u) || (reinterpret_cast<uintptr_t>(dw) & (w_dtype == TAMD_F32 ? 3u : 1u)))
    return TAMD_E_ALIGN;
  TAMD_ROUTER_LAUNCH(moe_router_bwd_kernel, (const T*)logits, top_k_index, dw, (T*)dlogits, tokens, (int)experts, (int)top_k, lde,
                     norm);
  return launch_status();
}

}  // extern "C"

#undef TAMD_ROUTER_LAUNCH
