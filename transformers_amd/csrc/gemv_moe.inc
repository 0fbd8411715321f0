// gemv_moe.inc -- the experts of a gated-SiLU mixture-of-experts block for a cached decode step (included at the end of gemv.hip).
//
// Replaces, for a handful of tokens and no gradient, the routed path of tamd_moe_route / _gather / tamd_gemm_routed / _combine
// (integrations/moe.py: grouped_mm_experts_forward; MixtralExperts.forward's per-expert loop): with one row per expert a
// 256-row tile is empty, the gather writes megabytes of zeros, and 32 workgroups stream the down projection.  Here the weights
// of the experts that were chosen are streamed once, as gemv_kernel / gemv_swiglu_kernel stream a dense projection, and
// nothing else of size moves: no plan, no sorted buffers, no padding.
//
// THREE launches per call (tamd_moe_gemv_swiglu: 1; tamd_moe_gemv_down: 2), S = tokens * top_k pairs, pair p = t * top_k + j,
// buffers PAIR-MAJOR (row p belongs to pair p):
//   1. act[p, i] = rT(rT(silu(rT(g))) * rT(u)),  g = x[t] . Wgu[e, i, :],  u = x[t] . Wgu[e, I + i, :]     (gemv_swiglu_kernel's way out)
//   2. ys[p, h]  = rT(act[p, :] . Wd[e, h, :])
//   3. out[t]    = rT(sum_j r32(w[t, j] * f32(ys[t k + j])))          j ascending, sentinel pairs skipped (tamd_moe_combine's chain)
// Launches 1 and 2 run on a grid over (feature block, expert): every wave of a workgroup finds the pairs of ITS expert with
// ballots over top_k_index (S <= kMoeGemvMaxPairs ids: four loads per lane) -- a wave-uniform bit mask, no LDS, no barrier --
// and returns before it loads a weight when there is none.  It takes the pairs in ascending p in chunks of up to
// kGemvValuRows rows, so an expert chosen by several tokens has its weights streamed once per chunk (the later chunks out of
// L2); a wave owns R = 2 features, its 64 lanes walk K in 16-byte pieces with fp32 accumulators and wave_sum joins them.
// An id outside [0, E) (moe.py's expert-parallel sentinel) matches no workgroup's expert: it never indexes memory, its act /
// ys rows are not written, and launch 3 skips it.  No atomics, no host synchronisation, plain vector stores.
// HBM traffic = the algorithmic bytes: (distinct chosen experts) * 3 H I * 2 (+ S (H + 2 I) * 2 of activations).

namespace tamd {

constexpr int kMoeGemvMaxTokens = TAMD_MOE_GEMV_MAX_TOKENS;
constexpr int kMoeGemvMaxPairs = TAMD_MOE_GEMV_MAX_PAIRS;
constexpr int kMoeGemvWords = kMoeGemvMaxPairs / 64;  // 64-pair ballots
constexpr int kMoeGemvMaxExperts = 256;
static_assert(kMoeGemvMaxTokens <= kGemvMaxRows && kMoeGemvMaxPairs % 64 == 0, "decode-sized calls only");

struct MoeGemvArgs {
  const void* X;        // [tokens, K] (SWIGLU: row of pair p = p / xdiv) or [S, ldx] (row p; xdiv = 1)
  const int64_t* ids;   // [S]
  const void* W;        // [E, N (SWIGLU: 2 N), K]
  void* Y;              // [S, ldy]
  int64_t npairs, xdiv, N, K, ldx, ldy;
};

// one chunk: MB pairs pr[0 .. MB) (slots from `live` on repeat the last live pair: read again, not stored) against the R
// features (SWIGLU: gate row i and up row N + i) of this wave
template <typename T, int MB, int R, bool SWIGLU>
__device__ __forceinline__ void moe_gemv_chunk(const MoeGemvArgs& g, const T* __restrict__ We, int64_t n0, const int* pr, int live,
                                               int lane) {
  typedef typename elem<T>::raw raw;
  constexpr int NR = SWIGLU ? 2 * R : R;
  const T* __restrict__ X = reinterpret_cast<const T*>(g.X);
  const T* wrow[NR];
  const T* xrow[MB];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t n = n0 + r < g.N ? n0 + r : g.N - 1;  // (rows past N: re-read the last one)
    wrow[r] = We + n * g.K;
    if (SWIGLU) wrow[R + r] = We + (g.N + n) * g.K;
  }
#pragma unroll
  for (int m = 0; m < MB; ++m) xrow[m] = X + ((int64_t)pr[m] / g.xdiv) * g.ldx;
  float acc[MB][NR];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[m][r] = 0.f;
#pragma unroll 2
  for (int64_t k = (int64_t)lane * 8; k < g.K; k += 512) {
    u32x4 wq[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) wq[r] = ld16(wrow[r] + k);
    float xv[MB][8];
#pragma unroll
    for (int m = 0; m < MB; ++m) unpack16<T>(ld16(xrow[m] + k), xv[m]);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      float wv[8];
      unpack16<T>(wq[r], wv);
#pragma unroll
      for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[m][r] = fmaf(wv[e], xv[m][e], acc[m][r]);
    }
  }
  // every lane ends up with every total; lane m * R + r stores output (pair pr[m], feature n0 + r)
  float first = 0.f, second = 0.f;
  int row = -1;
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float t0 = wave_sum(acc[m][r]);
      const float t1 = SWIGLU ? wave_sum(acc[m][R + r]) : 0.f;
      if (lane == m * R + r) first = t0, second = t1, row = m < live ? pr[m] : -1;
    }
  const int64_t n = n0 + lane % R;
  if (row < 0 || n >= g.N) return;
  float v = first;
  if (SWIGLU) {
    const float gr = round_through<T>(first), ur = round_through<T>(second);
    const float sg = fast_sigmoid(gr);  // = silu_f of elementwise.hip
    v = round_through<T>(gr * sg) * ur;
  }
  reinterpret_cast<raw*>(g.Y)[(int64_t)row * g.ldy + n] = elem<T>::from_f32(v);
}

// the lowest pair left in the masks (cleared there), -1 when none is
__device__ __forceinline__ int moe_gemv_pop(unsigned long long (&mask)[kMoeGemvWords]) {
  int p = -1;
#pragma unroll
  for (int w = 0; w < kMoeGemvWords; ++w) {
    const unsigned long long m = mask[w];
    if (p < 0 && m != 0ull) {
      p = w * 64 + __builtin_ctzll(m);
      mask[w] = m & (m - 1ull);
    }
  }
  return p;
}

// grid (ceil(N / 4 R), E), 4 waves: blockIdx.y = the expert whose weights this workgroup streams.  MAXMB (1, 2 or
// kGemvValuRows) = rows per chunk, the host's choice by the token count: a one-token step compiles no four-row chunk in and
// runs at the one-row kernel's registers (98 against 196: five waves per SIMD against two)
template <typename T, int R, bool SWIGLU, int MAXMB>
__global__ __launch_bounds__(256) void moe_gemv_kernel(MoeGemvArgs g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * R;
  if (n0 >= g.N) return;
  const int64_t expert = (int64_t)blockIdx.y;
  unsigned long long mask[kMoeGemvWords];
  bool any = false;
#pragma unroll
  for (int w = 0; w < kMoeGemvWords; ++w) {
    const int64_t p = (int64_t)w * 64 + lane;
    mask[w] = 0ull;
    if ((int64_t)w * 64 < g.npairs) mask[w] = ballot64(p < g.npairs && g.ids[p < g.npairs ? p : 0] == expert);
    any = any || mask[w] != 0ull;
  }
  if (!any) return;  // nobody chose this expert: none of its weights is read
  const T* __restrict__ We = reinterpret_cast<const T*>(g.W) + expert * (SWIGLU ? 2 : 1) * g.N * g.K;
  for (;;) {
    int pr[MAXMB];
    int live = 0;
#pragma unroll
    for (int m = 0; m < MAXMB; ++m) {
      const int p = moe_gemv_pop(mask);
      if (p >= 0) live = m + 1;
      pr[m] = p >= 0 ? p : (m > 0 ? pr[m - 1] : 0);
    }
    if (live == 0) return;
    if (MAXMB == 1 || live == 1)
      moe_gemv_chunk<T, 1, R, SWIGLU>(g, We, n0, pr, live, lane);
    else if (MAXMB == 2 || live == 2)
      moe_gemv_chunk<T, 2, R, SWIGLU>(g, We, n0, pr, live, lane);
    else
      moe_gemv_chunk<T, MAXMB, R, SWIGLU>(g, We, n0, pr, live, lane);
    if (live < MAXMB) return;
  }
}

template <typename T, bool WF32>
__device__ __forceinline__ float moe_gemv_weight(const void* w, int64_t p) {
  if (WF32) return reinterpret_cast<const float*>(w)[p];
  return elem<T>::to_f32(reinterpret_cast<const typename elem<T>::raw*>(w)[p]);
}

// out[t] = rT(sum_j r32(w[t, j] * f32(ys[t k + j]))) over the pair-major rows: moe_combine_kernel's chain (moe_route.inc) with
// pos[p] = p, or -1 where the id is outside [0, E); one wave per token
template <typename T, bool WF32>
__global__ __launch_bounds__(256) void moe_gemv_combine_kernel(const T* __restrict__ ys, const int64_t* __restrict__ ids,
                                                                const void* __restrict__ w, T* __restrict__ out, int64_t tokens,
                                                                int k, int E, int H) {
  const int lane = threadIdx.x & 63, chunks = H / 8;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  for (int i = lane; i < chunks; i += 64) {
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
    for (int j = 0; j < k; ++j) {
      const int64_t p = t * k + j, id = ids[p];
      if (id < 0 || id >= E) continue;
      const float wj = moe_gemv_weight<T, WF32>(w, p);
      float y[8];
      unpack16<T>(ld16(ys + p * H + (int64_t)i * 8), y);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float prod = wj * y[q];
        acc[q] = acc[q] + prod;
      }
    }
    st16(out + t * H + (int64_t)i * 8, pack16<T>(acc));
  }
}

static int moe_gemv_check(int64_t tokens, int64_t top_k, int64_t experts, int64_t hidden, int64_t inter, int64_t ldact, int dtype) {
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  if (tokens < 1 || tokens > kMoeGemvMaxTokens || top_k < 1 || tokens * top_k > kMoeGemvMaxPairs) return TAMD_E_SHAPE;
  if (experts < 1 || experts > kMoeGemvMaxExperts || hidden < 64 || (hidden % 64) != 0 || inter < 8 || (inter % 8) != 0)
    return TAMD_E_SHAPE;
  if (ldact < inter || (ldact % 8) != 0) return TAMD_E_SHAPE;
  if (hidden >= ((int64_t)1 << 31) || inter >= ((int64_t)1 << 30)) return TAMD_E_SHAPE;
  return TAMD_OK;
}

template <typename T, bool SWIGLU>
static int moe_gemv_launch(const MoeGemvArgs& g, int64_t tokens, int64_t experts, hipStream_t s) {
  // R = 2 as gemv_launch_rows below 16384 weight rows: a live expert alone gives every CU several waves (Mixtral's down
  // projection: 512 workgroups per expert), and the workgroups of the experts nobody chose leave at once
  constexpr int R = 2;
  dim3 grid((unsigned)ceil_div(g.N, 4 * R), (unsigned)experts), block(256);
  if (tokens <= 1)
    hipLaunchKernelGGL((moe_gemv_kernel<T, R, SWIGLU, 1>), grid, block, 0, s, g);
  else if (tokens <= 2)
    hipLaunchKernelGGL((moe_gemv_kernel<T, R, SWIGLU, 2>), grid, block, 0, s, g);
  else
    hipLaunchKernelGGL((moe_gemv_kernel<T, R, SWIGLU, kGemvValuRows>), grid, block, 0, s, g);
  return launch_status();
}

}  // namespace tamd

using namespace tamd;

extern "C" {

int tamd_moe_gemv_swiglu(const void* x, const int64_t* top_k_index, const void* gate_up, void* act, int64_t tokens,
                         int64_t top_k, int64_t experts, int64_t hidden, int64_t inter, int64_t ldact, int dtype,
                         tamd_stream_t stream) {
  if (!x || !top_k_index || !gate_up || !act) return TAMD_E_NULL;
  const int st = moe_gemv_check(tokens, top_k, experts, hidden, inter, ldact, dtype);
  if (st != TAMD_OK) return st;
  if (!aligned16(x) || !aligned16(gate_up) || !aligned16(act) || (reinterpret_cast<uintptr_t>(top_k_index) & 7u))
    return TAMD_E_ALIGN;
  const MoeGemvArgs g = {x, top_k_index, gate_up, act, tokens * top_k, top_k, inter, hidden, hidden, ldact};
  TAMD_DISPATCH_HALF(dtype, return (moe_gemv_launch<T, true>(g, tokens, experts, TAMD_STREAM(stream))));
  return TAMD_E_DTYPE;
}

int tamd_moe_gemv_down(const void* act, const int64_t* top_k_index, const void* down, const void* w, void* ys, void* out,
                       int64_t tokens, int64_t top_k, int64_t experts, int64_t hidden, int64_t inter, int64_t ldact,
                       int w_dtype, int dtype, tamd_stream_t stream) {
  if (!act || !top_k_index || !down || !w || !ys || !out) return TAMD_E_NULL;
  const int st = moe_gemv_check(tokens, top_k, experts, hidden, inter, ldact, dtype);
  if (st != TAMD_OK) return st;
  if (w_dtype != TAMD_F32 && w_dtype != dtype) return TAMD_E_DTYPE;
  if (!aligned16(act) || !aligned16(down) || !aligned16(ys) || !aligned16(out) || (reinterpret_cast<uintptr_t>(top_k_index) & 7u) ||
      (reinterpret_cast<uintptr_t>(w) & (w_dtype == TAMD_F32 ? 3u : 1u)))
    return TAMD_E_ALIGN;
  hipStream_t s = TAMD_STREAM(stream);
  const MoeGemvArgs g = {act, top_k_index, down, ys, tokens * top_k, 1, hidden, inter, ldact, hidden};
  const dim3 cgrid((unsigned)ceil_div(tokens, 4)), block(256);
  TAMD_DISPATCH_HALF(dtype, {
    const int st2 = moe_gemv_launch<T, false>(g, tokens, experts, s);
    if (st2 != TAMD_OK) return st2;
    if (w_dtype == TAMD_F32)
      hipLaunchKernelGGL((moe_gemv_combine_kernel<T, true>), cgrid, block, 0, s, (const T*)ys, top_k_index, w, (T*)out, tokens,
                         (int)top_k, (int)experts, (int)hidden);
    else
      hipLaunchKernelGGL((moe_gemv_combine_kernel<T, false>), cgrid, block, 0, s, (const T*)ys, top_k_index, w, (T*)out, tokens,
                         (int)top_k, (int)experts, (int)hidden);
  });
  return launch_status();
}

}  // extern "C"
