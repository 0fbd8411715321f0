// gemv_fp8.inc -- linear layers whose weights are OCP e4m3 bytes with one fp32 scale per 128 x 128 block: the dense projections
// of the DeepSeek-V3 / R1, Qwen3-FP8 and GLM-FP8 checkpoints (integrations/finegrained_fp8.py: FP8Linear, `weight_scale_inv`).
// Included at the end of gemv.hip.  W8A16: the activations stay bf16 / fp16 and are never quantised; no FP8 MFMA.
//
//   M <= 16  Y[m, n] = rT( sum_k X[m, k] * (f32(W8[n, k]) * S[n / 128, k / 128]) [+ bias[n]] )     fp32 throughout:
//            gemv_fp8w_kernel (VALU) at one row, at two, and at 3 .. 4 rows below 4096 weight rows; gemv_fp8w_mfma_kernel<ROUNDW =
//            false> for the rest (fp8w_use_mfma records the measurement behind the rule)
//   M  > 16  Wd = rT(r32(f32(W8) * S)), Y = X . Wd^T with the GEMM kernels' roundings:
//            17 .. 64 rows: gemv_fp8w_mfma_kernel<ROUNDW = true> builds Wd in registers, one launch, the workspace is not written;
//            65 .. 1024 rows: gemm_fp8w_kernel (gemm_fp8w.inc), the same in 128-row W tiles with X in LDS: one launch, no workspace
//            write; above (fp8w_use_tile holds the measurements): dequant_fp8w_kernel + tamd_gemm per row chunk, which is also the
//            diagnostic "before" arm
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
// HBM traffic = the algorithmic bytes: N*K + 4*ceil(N/128)*ceil(K/128) + M*(K + N)*sizeof(T), for both streaming kernels.
// Registers and scratch of every instantiation: profiles/fp8_linear_isa.md (no scratch anywhere).

namespace tamd {

constexpr int kFp8Block = 128;                             // the scale block (rows and columns)
constexpr size_t kFp8ChunkBytes = (size_t)64 << 20;        // default cap of the dequantised chunk (M > 16)
constexpr int kFp8MfmaMaxRows = 64;                        // rows of X up to which gemv_fp8w_mfma_kernel runs

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

// ---- 2 .. 64 rows: the same stream through the matrix pipe, on gemv_mfma_kernel's split.  A workgroup owns 16 * RB weight rows
// (16 RB | 128 and n0 a multiple of it: one row of S); its four waves split K in whole 128-wide scale blocks, interleaved (wave w
// takes blocks w, w + 4, ...: a round of the workgroup reads contiguous bytes of every row), and meet in LDS in a fixed order.
// Lane l loads the 16 bytes W[row0 + (l & 15)][k0 + 16 (l >> 4) .. + 15] -- 64 contiguous bytes per row and instruction, a scale
// block is two such loads -- and the 32 bytes X[16 t + (l & 15)][the same 16 k].  The lane's bytes 0 .. 7 and 8 .. 15 become the A
// operands of two v_mfma_f32_16x16x32 against the two halves of its X: A and B carry the same permutation of k.  A weight is
// converted once (e4m3 is exact in T) and shared by the MT row tiles of X; the RB row blocks share every X fragment.  Every load
// of a round of U blocks, W and X and the scales, is issued before the round's first MFMA.
//   ROUNDW = false (M <= 16, MT = 1): the MFMAs run on the UNSCALED weights; the four MFMAs of a scale block start from zero and
//     the partial enters the accumulator as fma(s, partial, acc): 4 RB fmas per 128 x 16 weights, and no weight is ever rounded.
//   ROUNDW = true (17 <= M <= 64, MT = ceil(M / 16)): the A operand is rT(r32(f32(W8) * s)), dequant_fp8w_kernel's Wd bit for
//     bit, accumulated straight across K; the epilogue chain is tamd_gemm's.  Wd never reaches memory.
// Accumulator rb * MT + t, register r of lane l is y[m = 16 t + (l & 15)][n = n0 + 16 rb + 4 (l >> 4) + r].
template <int MT, int RB, bool ROUNDW>
struct Fp8MfmaRound {  // scale blocks per wave and round: 8 (RB + 2 MT) registers of loads each
  static constexpr int U = !ROUNDW ? 4 : (MT * RB >= 8 ? 1 : 2);
};

template <typename T, int MT, int RB, bool ROUNDW, int EPI>
__global__ __launch_bounds__(256) void gemv_fp8w_mfma_kernel(GemvFp8Args g) {
  typedef typename elem<T>::raw raw;
  constexpr int NA = MT * RB, U = Fp8MfmaRound<MT, RB, ROUNDW>::U;
  static_assert(kFp8Block % (16 * RB) == 0, "the rows of a workgroup share one row of scales");
  static_assert(NA <= 8, "the reduction buffer is 4 KiB per accumulator");
  __shared__ float red[4][NA][64][4];
  const int lane = threadIdx.x & 63, wave = wave_id_uniform();
  const int l15 = lane & 15, g4 = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * 16 * RB;
  const unsigned char* wp[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int64_t row = n0 + rb * 16 + l15 < g.N ? n0 + rb * 16 + l15 : g.N - 1;  // (rows past N: re-read the last one)
    wp[rb] = g.W + row * g.ldw + g4 * 16;
  }
  const T* xp[MT];
  bool xlive[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    xlive[t] = 16 * t + l15 < g.M;
    xp[t] = reinterpret_cast<const T*>(g.X) + (xlive[t] ? 16 * t + l15 : 0) * g.ldx + g4 * 16;
  }
  const float* __restrict__ srow = g.S + (n0 / kFp8Block) * g.lds;
  const int64_t nkb = (g.K + kFp8Block - 1) / kFp8Block;
  f32x4 acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 z = {0u, 0u, 0u, 0u};
  for (int64_t kb0 = wave; kb0 < nkb; kb0 += 4 * U) {
    u32x4 wq[U][2][RB], xq[U][2][MT][2];
    float sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t kb = kb0 + 4 * u;
      sc[u] = kb < nkb ? srow[kb] : 0.f;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t k = kb * kFp8Block + 64 * h;
        const bool in = k + g4 * 16 < g.K;  // (K % 16 == 0: a lane's 16 values are inside or outside together)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) wq[u][h][rb] = in ? ld16(wp[rb] + k) : z;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          xq[u][h][t][0] = (in && xlive[t]) ? ld16(xp[t] + k) : z;
          xq[u][h][t][1] = (in && xlive[t]) ? ld16(xp[t] + k + 8) : z;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f32x4 part[NA];
#pragma unroll
      for (int i = 0; i < NA; ++i) part[i] = ROUNDW ? acc[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // (ROUNDW: a lane past K multiplies its zeros by zero, whatever the scale of the ragged block is)
        const float s = (kb0 + 4 * u) * kFp8Block + 64 * h + g4 * 16 < g.K ? sc[u] : 0.f;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          f32x2 wv[8];
          fp8x16_to_f32(wq[u][h][rb], wv);
          if (ROUNDW) {
#pragma unroll
            for (int e = 0; e < 8; ++e) wv[e] = wv[e] * f32x2{s, s};
          }
          const u32x4 a0 = {pack2<T>(wv[0][0], wv[0][1]), pack2<T>(wv[1][0], wv[1][1]), pack2<T>(wv[2][0], wv[2][1]),
                            pack2<T>(wv[3][0], wv[3][1])};
          const u32x4 a1 = {pack2<T>(wv[4][0], wv[4][1]), pack2<T>(wv[5][0], wv[5][1]), pack2<T>(wv[6][0], wv[6][1]),
                            pack2<T>(wv[7][0], wv[7][1])};
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            part[rb * MT + t] = mfma16<T>(a0, xq[u][h][t][0], part[rb * MT + t]);
            part[rb * MT + t] = mfma16<T>(a1, xq[u][h][t][1], part[rb * MT + t]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        if (ROUNDW) {
          acc[i] = part[i];
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][r] = fmaf(sc[u], part[i][r], acc[i][r]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][i][lane][r] = acc[i][r];
  block_sync();
  // accumulator i is summed and stored by wave i % 4
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    if ((i & 3) != wave) continue;
    const int rb = i / MT, t = i % MT;
    const int64_t m = 16 * t + l15;
    if (m >= g.M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = n0 + rb * 16 + 4 * g4 + r;
      if (n >= g.N) continue;
      float v = ((red[0][i][lane][r] + red[1][i][lane][r]) + red[2][i][lane][r]) + red[3][i][lane][r];
      if ((EPI == TAMD_EPI_BIAS || EPI == TAMD_EPI_RESIDUAL) && g.bias != nullptr)
        v += elem<T>::to_f32(reinterpret_cast<const raw*>(g.bias)[n]);
      if (EPI == TAMD_EPI_RESIDUAL)
        v = round_through<T>(v) + elem<T>::to_f32(reinterpret_cast<const raw*>(g.R)[m * g.ldr + n]);
      reinterpret_cast<raw*>(g.Y)[m * g.ldy + n] = elem<T>::from_f32(v);
    }
  }
}

template <typename T, int MT, int RB, bool ROUNDW>
static int gemv_fp8w_mfma_launch_epi(const GemvFp8Args& g, int epilogue, hipStream_t s) {
  dim3 grid((unsigned)ceil_div(g.N, 16 * RB)), block(256);
  switch (epilogue) {
    case TAMD_EPI_NONE: hipLaunchKernelGGL((gemv_fp8w_mfma_kernel<T, MT, RB, ROUNDW, TAMD_EPI_NONE>), grid, block, 0, s, g); break;
    case TAMD_EPI_BIAS: hipLaunchKernelGGL((gemv_fp8w_mfma_kernel<T, MT, RB, ROUNDW, TAMD_EPI_BIAS>), grid, block, 0, s, g); break;
    case TAMD_EPI_RESIDUAL:
      hipLaunchKernelGGL((gemv_fp8w_mfma_kernel<T, MT, RB, ROUNDW, TAMD_EPI_RESIDUAL>), grid, block, 0, s, g);
      break;
    default: return TAMD_E_ARG;
  }
  return launch_status();
}
template <typename T, int MT, bool ROUNDW>
static int gemv_fp8w_mfma_launch_rb(const GemvFp8Args& g, int epilogue, hipStream_t s) {
  // two row blocks per workgroup where that leaves >= 512 workgroups (gemv_mfma_launch's rule).  Four are not built: they would
  // start at 32768 weight rows, above every FP8Linear of the supported checkpoints (their lm_head is not quantised)
  if (ceil_div(g.N, 16) >= 2 * 512) return gemv_fp8w_mfma_launch_epi<T, MT, 2, ROUNDW>(g, epilogue, s);
  return gemv_fp8w_mfma_launch_epi<T, MT, 1, ROUNDW>(g, epilogue, s);
}
template <typename T>
static int gemv_fp8w_mfma_launch(const GemvFp8Args& g, int epilogue, hipStream_t s) {
  if (g.M <= 16) return gemv_fp8w_mfma_launch_rb<T, 1, false>(g, epilogue, s);
  if (g.M <= 32) return gemv_fp8w_mfma_launch_rb<T, 2, true>(g, epilogue, s);
  if (g.M <= 48) return gemv_fp8w_mfma_launch_rb<T, 3, true>(g, epilogue, s);
  return gemv_fp8w_mfma_launch_rb<T, 4, true>(g, epilogue, s);
}

// 0: every M as before gemv_fp8w_mfma_kernel (the streaming kernel up to 16 rows, dequantise + GEMM above); 2: that kernel for
// every M in 2 .. 64; anything else: the rule below.  libtamd_diag.so only (TAMD_FP8W_MFMA in the environment, read at every call
// so that tools/fp8_linear_bench.py can alternate the arms inside one process); the product library has the rule alone.
static int fp8w_mfma_mode() {
#ifdef TAMD_DIAG
  const char* e = getenv("TAMD_FP8W_MFMA");
  return e && (e[0] == '0' || e[0] == '2') ? e[0] - '0' : 1;
#else
  return 1;
#endif
}
// Which kernel for M <= 64 (true: gemv_fp8w_mfma_kernel): medians of old against new in one process, cold weights, us per call
// (profiles/fp8_linear_ab.jsonl, the arms fp8w_before / fp8w_mfma; K -> N).  One row: the streaming kernel (never measured against).
// 2 rows: the streaming kernel everywhere -- 7168 -> 1536 7.5 vs 10.6, 7168 -> 576 5.9 vs 9.5, 16384 -> 7168 28.5 vs 32.1, 7168 ->
// 18432 29.9 vs 37.0, 18432 -> 7168 32.5 vs 34.7; it loses one shape, 1536 -> 24576 at 12.2 vs 11.5.  3 and 4 rows (its 4-row
// form): the streaming kernel below 4096 weight rows (7168 -> 1536 9.4 vs 11.2, 7168 -> 576 8.0 vs 10.1: 96 and 36 workgroups of
// the MFMA kernel), the MFMA kernel from there on (1536 -> 24576 21.8 vs 11.9, 16384 -> 7168 42.0 vs 34.0, 7168 -> 18432 41.4 vs 38.5,
// 18432 -> 7168 48.3 vs 37.8); nothing was measured between 1536 and 7168 rows.  5 .. 64 rows: the MFMA kernel, faster at every
// shape measured (8 rows 0.32 .. 0.84 of the old time, 16 rows 0.13 .. 0.53, 32 rows 0.12 .. 0.30, 64 rows 0.20 .. 0.45).
static bool fp8w_use_mfma(int64_t m, int64_t n) {
  if (m < 2 || m > kFp8MfmaMaxRows) return false;
  const int mode = fp8w_mfma_mode();
  if (mode != 1) return mode == 2;
  return m > 4 || (m > 2 && n >= 4096);
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

#include "gemm_fp8w.inc"

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
  const GemvFp8Args g{X, W, S, Y, bias, R, M, N, K, ldx, ldw, lds, ldy, ldr};
  const bool mfma = fp8w_use_mfma(M, N);
  if (!gemm) {
    if (mfma) {
      TAMD_DISPATCH_HALF(dtype, return (gemv_fp8w_mfma_launch<T>(g, epilogue, s)));
    }
    TAMD_DISPATCH_HALF(dtype, return (gemv_fp8w_launch<T>(g, epilogue, s)));
    return TAMD_E_DTYPE;
  }
  const int64_t chunk = fp8w_chunk_rows(N, K, chunk_bytes);
  if (!workspace || !aligned16(workspace) || workspace_bytes < (size_t)chunk * (size_t)K * 2) return TAMD_E_ARG;
  if (fp8w_use_tile(M, ldx)) {  // 65 .. 1024 rows: Wd in registers in front of the tile kernel's MFMAs; the workspace is not touched
    TAMD_DISPATCH_HALF(dtype, return (gemm_fp8w_launch<T>(g, epilogue, s)));
    return TAMD_E_DTYPE;
  }
  if (mfma) {  // 17 .. 64 rows: the same Wd in registers, one launch; the workspace is validated and not touched
    TAMD_DISPATCH_HALF(dtype, return (gemv_fp8w_mfma_launch<T>(g, epilogue, s)));
    return TAMD_E_DTYPE;
  }
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
