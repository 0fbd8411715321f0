// gemv_fp8.inc -- linear layers whose weights are OCP e4m3 bytes with one fp32 scale per 128 x 128 block: the dense projections
// of the DeepSeek-V3 / R1, Qwen3-FP8 and GLM-FP8 checkpoints (integrations/finegrained_fp8.py: FP8Linear, `weight_scale_inv`).
// Included at the end of gemv.hip.  W8A16: the activations stay bf16 / fp16 and are never quantised; no FP8 MFMA.
//
//   M <= 16  gemv_fp8w_kernel   Y[m, n] = rT( sum_k X[m, k] * (f32(W8[n, k]) * S[n / 128, k / 128]) [+ bias[n]] )     fp32 throughout
//   M  > 16  dequant_fp8w_kernel + tamd_gemm per row chunk:  Wd = rT(r32(f32(W8) * S)), Y = the GEMM kernels' X . Wd^T
//
// gemv_fp8w_kernel keeps gemv_kernel's split -- one wave owns R consecutive weight rows, four waves per workgroup, no LDS, no
// MFMA, a reduction over the lanes at the end -- on a data path of its own:
//   * a lane's 16-byte load is 16 weights, a step of the wave covers 1024 values of k, and a lane's 16 values lie inside ONE
//     128-wide scale block: the lane forms the UNSCALED sum of its 16 products and applies the scale with one fma into the
//     accumulator (acc = fma(s, partial, acc)) -- one scale multiply per 16 products;
//   * n0 = R * (wave index) with R | 128: the R rows of a wave share one row of S (rows past a ragged N re-read row N - 1, which
//     lies in the same block as n0);
//   * e4m3 -> fp32 two at a time (v_cvt_pk_f32_fp8: OCP e4m3fn on gfx950), products as packed pairs (v_pk_fma_f32): the even
//     and the odd elements of a lane's 16 run as two chains that meet before the scale;
//   * the weights and the scale of step i + 1 are loaded before the arithmetic of step i starts;
//   * X is 32 bytes per row and lane per step: the M rows are walked in groups of four (64 unpacked values beside the
//     accumulators), the decoded weights of a row are rebuilt per group from the 16 bytes in registers;
//   * the MB * R totals are not summed by MB * R butterflies: at every halving step a lane keeps one half of its values and
//     sends the other half to its partner, so MB * R - 1 exchanges (+ plain butterfly steps once one value is left) leave
//     total j in the lanes whose upper log2(MB R) bits are j.
// HBM traffic = the algorithmic bytes: N*K + 4*ceil(N/128)*ceil(K/128) + M*(K + N)*sizeof(T).
// Registers and scratch of every instantiation: profiles/fp8_linear_isa.md (no scratch anywhere).

namespace tamd {

constexpr int kFp8Block = 128;                             // the scale block (rows and columns)
constexpr size_t kFp8ChunkBytes = (size_t)64 << 20;        // default cap of the dequantised chunk (M > 16)

struct GemvFp8Args {
  const void* X;
  const unsigned char* W;  // [N, ldw] e4m3fn bytes
  const float* S;          // [ceil(N / 128), lds]
  void* Y;
  const void* bias;
  const void* R;
  int64_t M, N, K, ldx, ldw, lds, ldy, ldr;
};

// one e4m3fn byte in plain C++ (bias 7, subnormals man * 2^-9, no infinities): what the CPU execution model runs
__device__ __forceinline__ float e4m3_bits_to_f32(unsigned int b) {
  const unsigned int sign = (b & 0x80u) << 24, em = b & 0x7fu;
  if (em < 8u) return u32_as_f32(sign | f32_as_u32((float)em * 0.001953125f));
  return u32_as_f32(sign | ((em << 20) + (120u << 23)));
}
// the two e4m3fn bytes of the low (HI = false) or high half of a register as fp32
template <bool HI>
__device__ __forceinline__ f32x2 fp8x2_to_f32(unsigned int w) {
#ifdef __HIP__
  return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
#else
  const unsigned int h = HI ? w >> 16 : w;
  return f32x2{e4m3_bits_to_f32(h & 0xffu), e4m3_bits_to_f32((h >> 8) & 0xffu)};
#endif
}
// 16 weights -> 8 pairs (pair e = elements 2e, 2e + 1)
__device__ __forceinline__ void fp8x16_to_f32(u32x4 q, f32x2* out) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned int w = q[j];
    out[2 * j] = fp8x2_to_f32<false>(w);
    out[2 * j + 1] = fp8x2_to_f32<true>(w);
  }
}
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// V = 2^j values per lane -> lane l holds the wave's total of value l >> (6 - j) (every lane with those upper bits does)
template <int V>
__device__ __forceinline__ float wave_sum_scatter(float* v, int lane) {
  static_assert(V >= 1 && V <= 64 && (V & (V - 1)) == 0, "a power of two up to the wave");
  int mask = 32;
#pragma unroll
  for (int n = V; n > 1; n >>= 1, mask >>= 1) {
    const bool hi = (lane & mask) != 0;
#pragma unroll
    for (int i = 0; i < n / 2; ++i) {
      const float keep = hi ? v[i + n / 2] : v[i], send = hi ? v[i] : v[i + n / 2];
      v[i] = keep + shfl_xor_f32(send, mask);
    }
  }
#pragma unroll
  for (; mask >= 1; mask >>= 1) v[0] += shfl_xor_f32(v[0], mask);
  return v[0];
}

template <typename T, int MB, int R, int EPI>
__global__ __launch_bounds__(256) void gemv_fp8w_kernel(GemvFp8Args g) {
  typedef typename elem<T>::raw raw;
  constexpr int MG = MB < 4 ? MB : 4;  // rows of X unpacked at a time
  constexpr int V = MB * R;
  static_assert(kFp8Block % R == 0, "the rows of a wave share one row of scales");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * R;
  if (n0 >= g.N) return;
  const T* __restrict__ X = reinterpret_cast<const T*>(g.X);
  const unsigned char* wrow[R];
#pragma unroll
  for (int r = 0; r < R; ++r) wrow[r] = g.W + (n0 + r < g.N ? n0 + r : g.N - 1) * g.ldw;  // (rows past N: re-read the last one)
  const float* __restrict__ srow = g.S + (n0 / kFp8Block) * g.lds;
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.f;
  const u32x4 z = {0u, 0u, 0u, 0u};
  int64_t k = (int64_t)lane * 16;  // (K % 16 == 0: a lane's 16 values are inside or outside together)
  u32x4 wq[R];
  float s = 0.f;
  if (k < g.K) {
#pragma unroll
    for (int r = 0; r < R; ++r) wq[r] = ld16(wrow[r] + k);
    s = srow[k / kFp8Block];
  }
  for (; k < g.K; k += 1024) {
    const int64_t kn = k + 1024;
    const bool more = kn < g.K;
    u32x4 wn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) wn[r] = more ? ld16(wrow[r] + kn) : z;
    const float sn = more ? srow[kn / kFp8Block] : 0.f;
#pragma unroll
    for (int m0 = 0; m0 < MB; m0 += MG) {
      if (m0 > 0 && m0 >= g.M) break;  // (wave-uniform)
      f32x2 xv[MG][8];
#pragma unroll
      for (int i = 0; i < MG; ++i) {
        const T* xp = X + (m0 + i < g.M ? m0 + i : g.M - 1) * g.ldx + k;
        const u32x4 a = ld16(xp), b = ld16(xp + 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float lo, hi;
          unpack2<T>(a[e], lo, hi);
          xv[i][e] = f32x2{lo, hi};
          unpack2<T>(b[e], lo, hi);
          xv[i][4 + e] = f32x2{lo, hi};
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        f32x2 wv[8];
        fp8x16_to_f32(wq[r], wv);
#pragma unroll
        for (int i = 0; i < MG; ++i) {
          f32x2 p = wv[0] * xv[i][0];
#pragma unroll
          for (int e = 1; e < 8; ++e) p = pk_fma(wv[e], xv[i][e], p);
          acc[(m0 + i) * R + r] = fmaf(s, p[0] + p[1], acc[(m0 + i) * R + r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) wq[r] = wn[r];
    s = sn;
  }
  // lane (m R + r) * (64 / V) stores output (m, n0 + r)
  float v = wave_sum_scatter<V>(acc, lane);
  constexpr int LPV = 64 / V;
  const int idx = lane / LPV, m = idx / R, r = idx % R;
  const int64_t n = n0 + r;
  if (lane % LPV == 0 && m < g.M && n < g.N) {
    if ((EPI == TAMD_EPI_BIAS || EPI == TAMD_EPI_RESIDUAL) && g.bias != nullptr)
      v += elem<T>::to_f32(reinterpret_cast<const raw*>(g.bias)[n]);
    if (EPI == TAMD_EPI_RESIDUAL)
      v = round_through<T>(v) + elem<T>::to_f32(reinterpret_cast<const raw*>(g.R)[m * g.ldr + n]);
    reinterpret_cast<raw*>(g.Y)[m * g.ldy + n] = elem<T>::from_f32(v);
  }
}

template <typename T, int MB, int R>
static int gemv_fp8w_launch_epi(const GemvFp8Args& g, int epilogue, hipStream_t s) {
  dim3 grid((unsigned)ceil_div(g.N, 4 * R)), block(256);
  switch (epilogue) {
    case TAMD_EPI_NONE: hipLaunchKernelGGL((gemv_fp8w_kernel<T, MB, R, TAMD_EPI_NONE>), grid, block, 0, s, g); break;
    case TAMD_EPI_BIAS: hipLaunchKernelGGL((gemv_fp8w_kernel<T, MB, R, TAMD_EPI_BIAS>), grid, block, 0, s, g); break;
    case TAMD_EPI_RESIDUAL: hipLaunchKernelGGL((gemv_fp8w_kernel<T, MB, R, TAMD_EPI_RESIDUAL>), grid, block, 0, s, g); break;
    default: return TAMD_E_ARG;
  }
  return launch_status();
}
template <typename T, int MB>
static int gemv_fp8w_launch_rows(const GemvFp8Args& g, int epilogue, hipStream_t s) {
  // as gemv_launch_rows: 2 rows per wave below 16384 weight rows, so that every CU holds several waves.  8 and 16 rows of X
  // keep 2 everywhere: 64 accumulators beside the unpacked X and the weights in flight do not fit the register file (the
  // <16, 4> instantiation spilled 272 bytes per lane and is not built)
  if constexpr (MB <= 4) {
    if (g.N >= 16384) return gemv_fp8w_launch_epi<T, MB, 4>(g, epilogue, s);
  }
  return gemv_fp8w_launch_epi<T, MB, 2>(g, epilogue, s);
}
template <typename T>
static int gemv_fp8w_launch(const GemvFp8Args& g, int epilogue, hipStream_t s) {
  if (g.M <= 1) return gemv_fp8w_launch_rows<T, 1>(g, epilogue, s);
  if (g.M <= 2) return gemv_fp8w_launch_rows<T, 2>(g, epilogue, s);
  if (g.M <= 4) return gemv_fp8w_launch_rows<T, 4>(g, epilogue, s);
  if (g.M <= 8) return gemv_fp8w_launch_rows<T, 8>(g, epilogue, s);
  return gemv_fp8w_launch_rows<T, 16>(g, epilogue, s);
}

// D[row, k] = rT(r32(f32(W8[n_lo + row, k]) * S[(n_lo + row) / 128, k / 128])) for `rows` rows: a thread turns one 16-byte load
// into two 16-byte stores; the scale index follows the element, so ragged last blocks in N and in K need nothing of their own
template <typename T>
__global__ __launch_bounds__(256) void dequant_fp8w_kernel(const unsigned char* __restrict__ W, const float* __restrict__ S,
                                                            T* __restrict__ D, int64_t n_lo, int64_t rows, int64_t K, int64_t ldw,
                                                            int64_t lds, int64_t ldd) {
  const int64_t pieces = K / 16, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * pieces) return;
  const int64_t row = i / pieces, k = (i % pieces) * 16, n = n_lo + row;
  const float s = S[(n / kFp8Block) * lds + k / kFp8Block];
  f32x2 wv[8];
  fp8x16_to_f32(ld16(W + n * ldw + k), wv);
  float f[16];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f[2 * e] = wv[e][0] * s;
    f[2 * e + 1] = wv[e][1] * s;
  }
  st16(D + row * ldd + k, pack16<T>(f));
  st16(D + row * ldd + k + 8, pack16<T>(f + 8));
}

template <typename T>
static int dequant_fp8w_launch(const unsigned char* W, const float* S, void* D, int64_t n_lo, int64_t rows, int64_t K, int64_t ldw,
                               int64_t lds, int64_t ldd, hipStream_t s) {
  const int64_t blocks = ceil_div(rows * (K / 16), 256);
  if (blocks >= ((int64_t)1 << 31)) return TAMD_E_SHAPE;
  hipLaunchKernelGGL((dequant_fp8w_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, W, S, reinterpret_cast<T*>(D), n_lo, rows, K,
                     ldw, lds, ldd);
  return launch_status();
}

// weight rows dequantised at a time (M > 16): whole scale rows, as many as the cap holds, at least one
static int64_t fp8w_chunk_rows(int64_t N, int64_t K, size_t chunk_bytes) {
  const size_t cap = chunk_bytes ? chunk_bytes : kFp8ChunkBytes;
  int64_t rows = (int64_t)(cap / ((size_t)K * 2)) / kFp8Block * kFp8Block;
  if (rows < kFp8Block) rows = kFp8Block;
  return rows < N ? rows : N;
}

}  // namespace tamd

using namespace tamd;

extern "C" {

size_t tamd_gemm_fp8w_workspace_bytes(int64_t M, int64_t N, int64_t K, size_t chunk_bytes) {
  if (M <= kGemvMaxRows || N <= 0 || K <= 0) return 0;
  return (size_t)fp8w_chunk_rows(N, K, chunk_bytes) * (size_t)K * 2;
}

int tamd_dequant_fp8w(const void* W8, const float* S, void* Wd, int64_t N, int64_t K, int64_t ldw, int64_t lds, int64_t ldd,
                      int dtype, tamd_stream_t stream) {
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  if (N <= 0 || K <= 0 || (K % 16) != 0 || ldw < K || ldd < K || lds < ceil_div(K, kFp8Block)) return TAMD_E_SHAPE;
  if (!W8 || !S || !Wd || !aligned16(W8) || !aligned16(Wd) || (ldw % 16) != 0 || (ldd % 8) != 0 ||
      (reinterpret_cast<uintptr_t>(S) & 3u))
    return TAMD_E_ARG;
  TAMD_DISPATCH_HALF(dtype, return (dequant_fp8w_launch<T>(reinterpret_cast<const unsigned char*>(W8), S, Wd, 0, N, K, ldw, lds, ldd,
                                                           TAMD_STREAM(stream))));
  return TAMD_E_DTYPE;
}

int tamd_gemm_fp8w(const void* X, const void* W8, const float* S, void* Y, const void* bias, const void* R, int64_t M, int64_t N,
                   int64_t K, int64_t ldx, int64_t ldw, int64_t lds, int64_t ldy, int64_t ldr, int epilogue, int dtype,
                   void* workspace, size_t workspace_bytes, size_t chunk_bytes, tamd_stream_t stream) {
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  if (M <= 0 || N <= 0 || K <= 0 || (K % 16) != 0) return TAMD_E_SHAPE;
  if (ldx < K || ldw < K || ldy < N || lds < ceil_div(K, kFp8Block) || (epilogue == TAMD_EPI_RESIDUAL && ldr < N)) return TAMD_E_SHAPE;
  const bool gemm = M > kGemvMaxRows;
  if (gemm && ((N % 8) != 0 || (ldy % 8) != 0)) return TAMD_E_SHAPE;  // (the GEMM kernels' 16-byte rows of Y)
  if (epilogue != TAMD_EPI_NONE && epilogue != TAMD_EPI_BIAS && epilogue != TAMD_EPI_RESIDUAL) return TAMD_E_ARG;
  if (!X || !W8 || !S || !Y || (epilogue == TAMD_EPI_BIAS && !bias) || (epilogue == TAMD_EPI_RESIDUAL && !R)) return TAMD_E_ARG;
  if (!aligned16(X) || !aligned16(W8) || (ldx % 8) != 0 || (ldw % 16) != 0 || (reinterpret_cast<uintptr_t>(S) & 3u) ||
      (reinterpret_cast<uintptr_t>(Y) & (gemm ? 15u : 1u)) || (reinterpret_cast<uintptr_t>(bias) & (gemm ? 7u : 1u)) ||
      (reinterpret_cast<uintptr_t>(R) & (gemm ? 15u : 1u)) || (gemm && R && (ldr % 8) != 0))
    return TAMD_E_ARG;
  hipStream_t s = TAMD_STREAM(stream);
  const unsigned char* W = reinterpret_cast<const unsigned char*>(W8);
  if (!gemm) {
    const GemvFp8Args g{X, W, S, Y, bias, R, M, N, K, ldx, ldw, lds, ldy, ldr};
    TAMD_DISPATCH_HALF(dtype, return (gemv_fp8w_launch<T>(g, epilogue, s)));
    return TAMD_E_DTYPE;
  }
  const int64_t chunk = fp8w_chunk_rows(N, K, chunk_bytes);
  if (!workspace || !aligned16(workspace) || workspace_bytes < (size_t)chunk * (size_t)K * 2) return TAMD_E_ARG;
  for (int64_t n_lo = 0; n_lo < N; n_lo += chunk) {  // (chunk % 128 == 0: every chunk starts a scale row and a 16-byte column of Y)
    const int64_t rows = N - n_lo < chunk ? N - n_lo : chunk;
    TAMD_DISPATCH_HALF(dtype, {
      const int st = dequant_fp8w_launch<T>(W, S, workspace, n_lo, rows, K, ldw, lds, K, s);
      if (st != TAMD_OK) return st;
    });
    const char* b = bias ? reinterpret_cast<const char*>(bias) + n_lo * 2 : nullptr;
    const char* r = R ? reinterpret_cast<const char*>(R) + n_lo * 2 : nullptr;
    const int st = tamd_gemm(X, workspace, reinterpret_cast<char*>(Y) + n_lo * 2, b, r, M, rows, K, ldx, K, ldy, ldr, 0, epilogue,
                             TAMD_ACT_NONE, dtype, stream);
    if (st != TAMD_OK) return st;
  }
  return TAMD_OK;
}

}  // extern "C"
