// moe_router_group.inc -- the sigmoid, group-limited router (included at the end of elementwise.hip, behind moe_gate.inc).
//
// Replaces the chain behind the gate product of DeepseekV3TopkRouter.forward (models/deepseek_v3/modeling_deepseek_v3.py:
// 149-169; Glm4MoeTopkRouter.forward is the same text): sigmoid, add, view, topk(2), sum, topk, zeros_like, scatter_, expand /
// reshape, bool, masked_fill, topk, gather, sum, div_, mul.
//   tamd_moe_router_group_fwd   logits fp32 [T, E], bias [E] -> w fp32 [T, k], idx [T, k]
//   tamd_moe_router_group_bwd   logits, idx, dw [T, k] -> dlogits fp32 [T, E]; s and d recomputed exactly as the forward does
// The layout of moe_router.inc: one wave per token, four tokens per 256-thread workgroup, lane L holds experts L, 64 + L, 128 + L,
// 192 + L (NR = 1, 2 or 4 registers), every arg-max is the xor butterfly on the pair (value descending, id ascending).  A
// group is G consecutive experts, so it lies across lanes and registers: its two largest c come from a butterfly on the sorted
// pair (first, second) over the lanes' own two largest of that group -- one butterfly per group, the sum kept by lane g.
// No LDS, no atomics, no host synchronisation; every launch parameter is a function of (T, E).

namespace tamd {

// s = 1 / (1 + exp(-l)): expf, one addition, one IEEE division.  l = -200: exp = inf, s = 0; l = 200: exp = 0, s = 1.
__device__ __forceinline__ float router_sigmoid(float l) { return 1.f / (1.f + expf(-l)); }

// the larger two of {a1 >= a2} and {b1 >= b2}, as a sorted pair
__device__ __forceinline__ void top2_merge(float& a1, float& a2, float b1, float b2) {
  const float lo = fminf(a1, b1), hi = fmaxf(a1, b1);
  a2 = fmaxf(lo, fmaxf(a2, b2));
  a1 = hi;
}

template <int NR>
__global__ __launch_bounds__(kMoeThreads) void moe_router_group_fwd_kernel(const float* __restrict__ logits,
                                                                            const float* __restrict__ bias, float* __restrict__ w,
                                                                            int64_t* __restrict__ idx, int64_t tokens, int E, int k,
                                                                            int n_group, int topk_group, int64_t lde, int norm,
                                                                            float scale) {
  const int lane = lane_id();
  const int G = E / n_group;
  float b[NR];
  int grp[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int e = r * 64 + lane;
    b[r] = (bias != nullptr && e < E) ? bias[e] : 0.f;
    grp[r] = e < E ? e / G : -1;
  }
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave_id_uniform(); t < tokens; t += (int64_t)gridDim.x * 4) {
    const float* row = logits + t * lde;
    float s[NR], c[NR];  // c: what the choices run on (NaN -> -inf; -inf past E)
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int e = r * 64 + lane;
      s[r] = e < E ? router_sigmoid(row[e]) : 0.f;
      const float cr = s[r] + b[r];
      c[r] = (e < E && cr == cr) ? cr : -INFINITY;
    }
    unsigned taken = 0u;  // bit r: expert r * 64 + lane cannot be chosen (any more)
    if (n_group > 1) {
      float my_gs = -INFINITY;  // lane g < n_group: the score of group g
      for (int g = 0; g < n_group; ++g) {
        float t1 = -INFINITY, t2 = -INFINITY;
#pragma unroll
        for (int r = 0; r < NR; ++r)
          if (grp[r] == g) top2_merge(t1, t2, c[r], -INFINITY);
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
          const float o1 = shfl_xor_f32(t1, msk), o2 = shfl_xor_f32(t2, msk);
          top2_merge(t1, t2, o1, o2);
        }
        const float gs = t1 + t2;
        if (lane == g) my_gs = gs == gs ? gs : -INFINITY;
      }
      unsigned long long chosen = 0ull;  // bit g: group g is one of the topk_group
      bool gone = lane >= n_group;
      for (int j = 0; j < topk_group; ++j) {
        float bv = gone ? -INFINITY : my_gs, bi = gone ? kRouterNoId : (float)lane;
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {  // (score descending, group ascending)
          const float ov = shfl_xor_f32(bv, msk), oi = shfl_xor_f32(bi, msk);
          if (oi != kRouterNoId && (bi == kRouterNoId || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
          }
        }
        const int wg = (int)bi;
        chosen |= 1ull << wg;
        if (wg == lane) gone = true;
      }
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (grp[r] < 0 || !((chosen >> grp[r]) & 1ull)) taken |= 1u << r;
    } else {
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (grp[r] < 0) taken |= 1u << r;
    }
    float my_s = 0.f, my_id = 0.f, d = 0.f;
    for (int j = 0; j < k; ++j) {
      float bv = -INFINITY, bi = kRouterNoId, bs = 0.f;
#pragma unroll
      for (int r = 0; r < NR; ++r) {  // r ascending and a strict >: the lowest id among this lane's equals
        if (!((taken >> r) & 1u) && (bi == kRouterNoId || c[r] > bv)) {
          bv = c[r];
          bi = (float)(r * 64 + lane);
          bs = s[r];
        }
      }
#pragma unroll
      for (int msk = 32; msk >= 1; msk >>= 1) {  // (c descending, id ascending): a total order, every lane ends with the same triple
        const float ov = shfl_xor_f32(bv, msk), oi = shfl_xor_f32(bi, msk), os = shfl_xor_f32(bs, msk);
        if (oi != kRouterNoId && (bi == kRouterNoId || ov > bv || (ov == bv && oi < bi))) {
          bv = ov;
          bi = oi;
          bs = os;
        }
      }
      const int wid = (int)bi;
      if ((wid & 63) == lane) taken |= 1u << (wid >> 6);
      d = d + bs;  // j ascending
      if (lane == j) {
        my_s = bs;
        my_id = bi;
      }
    }
    if (lane < k) {
      float wj;
      if (norm) {
        const float q = my_s / (d + 1e-20f);
        wj = q * scale;
      } else {
        wj = my_s * scale;
      }
      w[t * k + lane] = wj;
      idx[t * k + lane] = (int64_t)my_id;
    }
  }
}

// idx and dw are read uniformly (every lane the same address); an id outside [0, E) is skipped
template <int NR>
__global__ __launch_bounds__(kMoeThreads) void moe_router_group_bwd_kernel(const float* __restrict__ logits,
                                                                            const int64_t* __restrict__ idx,
                                                                            const float* __restrict__ dw, float* __restrict__ dlogits,
                                                                            int64_t tokens, int E, int k, int64_t lde, int norm,
                                                                            float scale) {
  const int lane = lane_id();
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave_id_uniform(); t < tokens; t += (int64_t)gridDim.x * 4) {
    const float* row = logits + t * lde;
    float gsel[NR];      // g_j of the slot that selected this lane's expert r
    unsigned mine = 0u;  // bit r: expert r * 64 + lane is selected
#pragma unroll
    for (int r = 0; r < NR; ++r) gsel[r] = 0.f;
    float sj[kRouterMaxTopK], gj[kRouterMaxTopK];
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < kRouterMaxTopK; ++j) {
      sj[j] = 0.f;
      gj[j] = 0.f;
      if (j < k) {
        const int64_t id = idx[t * k + j];
        if (id >= 0 && id < E) {
          const float g = dw[t * k + j];
          sj[j] = router_sigmoid(row[id]);  // the forward's s_{e_j}, bit for bit
          gj[j] = g;
          d = d + sj[j];  // j ascending
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
    d = d + 1e-20f;
    float q = 0.f;
    if (norm) {
#pragma unroll
      for (int j = 0; j < kRouterMaxTopK; ++j)
        if (j < k) {
          const float wj = sj[j] / d;
          const float prod = gj[j] * wj;
          q = q + prod;
        }
    }
    const float f = norm ? scale / d : scale;
    float* out = dlogits + t * lde;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int e = r * 64 + lane;
      if (e < E) {
        float dl = 0.f;
        if ((mine >> r) & 1u) {
          const float se = router_sigmoid(row[e]);
          const float ds = f * (norm ? gsel[r] - q : gsel[r]);
          dl = (ds * se) * (1.f - se);
        }
        out[e] = dl;
      }
    }
    for (int64_t e = (int64_t)E + lane; e < lde; e += 64) out[e] = 0.f;
  }
}

static int moe_router_group_check(int64_t tokens, int64_t experts, int64_t top_k, int64_t n_group, int64_t topk_group, int64_t lde) {
  if (tokens <= 0 || tokens >= ((int64_t)1 << 31) || experts <= 0 || experts > kMoeMaxExperts || lde < experts) return TAMD_E_SHAPE;
  if (n_group < 1 || n_group > 64 || experts % n_group != 0 || topk_group < 1 || topk_group > n_group) return TAMD_E_SHAPE;
  const int64_t G = experts / n_group;
  if (n_group > 1 && G < 2) return TAMD_E_SHAPE;
  if (top_k < 1 || top_k > kRouterMaxTopK || top_k > topk_group * G) return TAMD_E_SHAPE;
  return TAMD_OK;
}

}  // namespace tamd

using namespace tamd;

#define TAMD_ROUTER_GROUP_LAUNCH(KERNEL, ...)                                                     \
  do {                                                                                            \
    const dim3 grid(moe_pair_blocks(tokens)), block(kMoeThreads);                                 \
    if (experts <= 64)                                                                            \
      hipLaunchKernelGGL((KERNEL<1>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);          \
    else if (experts <= 128)                                                                      \
      hipLaunchKernelGGL((KERNEL<2>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);          \
    else                                                                                          \
      hipLaunchKernelGGL((KERNEL<4>), grid, block, 0, TAMD_STREAM(stream), __VA_ARGS__);          \
  } while (0)

extern "C" {

int tamd_moe_router_group_fwd(const float* logits, const float* bias, float* w, int64_t* top_k_index, int64_t tokens,
                              int64_t experts, int64_t top_k, int64_t n_group, int64_t topk_group, int64_t lde, int norm,
                              float scale, tamd_stream_t stream) {
  if (!logits || !w || !top_k_index) return TAMD_E_NULL;
  const int st = moe_router_group_check(tokens, experts, top_k, n_group, topk_group, lde);
  if (st != TAMD_OK) return st;
  if ((reinterpret_cast<uintptr_t>(logits) & 3u) || (reinterpret_cast<uintptr_t>(bias) & 3u) || (reinterpret_cast<uintptr_t>(w) & 3u) ||
      (reinterpret_cast<uintptr_t>(top_k_index) & 7u))
    return TAMD_E_ALIGN;
  TAMD_ROUTER_GROUP_LAUNCH(moe_router_group_fwd_kernel, logits, bias, w, top_k_index, tokens, (int)experts, (int)top_k, (int)n_group,
                           (int)topk_group, lde, norm, scale);
  return launch_status();
}

int tamd_moe_router_group_bwd(const float* logits, const int64_t* top_k_index, const float* dw, float* dlogits, int64_t tokens,
                              int64_t experts, int64_t top_k, int64_t n_group, int64_t topk_group, int64_t lde, int norm,
                              float scale, tamd_stream_t stream) {
  if (!logits || !top_k_index || !dw || !dlogits) return TAMD_E_NULL;
  const int st = moe_router_group_check(tokens, experts, top_k, n_group, topk_group, lde);
  if (st != TAMD_OK) return st;
  if ((reinterpret_cast<uintptr_t>(logits) & 3u) || (reinterpret_cast<uintptr_t>(dlogits) & 3u) ||
      (reinterpret_cast<uintptr_t>(dw) & 3u) || (reinterpret_cast<uintptr_t>(top_k_index) & 7u))
    return TAMD_E_ALIGN;
  TAMD_ROUTER_GROUP_LAUNCH(moe_router_group_bwd_kernel, logits, top_k_index, dw, dlogits, tokens, (int)experts, (int)top_k, lde, norm,
                           scale);
  return launch_status();
}

}  // extern "C"

#undef TAMD_ROUTER_GROUP_LAUNCH
