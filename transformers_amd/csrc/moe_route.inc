// moe_route.inc -- routing of a sparse mixture-of-experts block (included at the end of elementwise.hip).
//
// Replaces the index bookkeeping of the reference's expert dispatch (integrations/moe.py: grouped_mm_experts_forward's
// argsort / histc / index_select / index_add, and the eager per-expert loop's one_hot / where / index_add_):
//   tamd_moe_route        the plan: per-expert counts, 64-row padded segment offsets, the row of every (token, slot) pair in the
//                         expert-sorted buffer, and the row-tile table of tamd_gemm_routed
//   tamd_moe_gather       Xs[pos[t, j]] = X[t]                      (padding rows zero)
//   tamd_moe_combine      out[t] = round(sum_j w[t, j] * Ys[pos[t, j]])
//   tamd_moe_combine_bwd  dYs[pos[t, j]] = round(w[t, j] * dOut[t]),  dw[t, j] = dOut[t] . Ys[pos[t, j]]
// No atomics anywhere: the rank of a pair inside its expert comes from wave ballots (pairs of one 64-pair granule), a serial
// prefix over the 16 granules of a 1024-pair chunk in LDS, and one scan workgroup over the chunks -- a stable counting sort,
// so the order of an expert's rows (ascending token, then slot: the summation order of the weight gradients) is a function
// of top_k_index alone.  An id outside [0, E) (the reference's expert-parallel sentinel) gets pos = -1: counted nowhere,
// never used as an index, contributes zero everywhere.

namespace tamd {

constexpr int kMoeThreads = 256;
constexpr int kMoeGranules = 16;                 // 64-pair granules per chunk: 4 per wave
constexpr int kMoeChunk = kMoeGranules * 64;     // pairs per workgroup of the count / rank kernels
constexpr int kMoeMaxExperts = 256;              // one scan thread per expert, 8 ballots per id
constexpr int kMoeSegRows = 64;                  // segments are whole K stages of the full-line GEMM (dW sums over them)
constexpr int kMoeTileRows = 256;                // row tile of the routed GEMM (gemm.hip kBM)
constexpr int kMoeTailBlocks = 64;               // workgroups that zero the rows behind the last segment

// the lanes of this wave whose pair names the same expert as this lane's (`e` < 0: an invalid pair, matches nobody)
__device__ __forceinline__ unsigned long long moe_match(int e) {
  unsigned long long m = ballot64(e >= 0);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const unsigned long long set = ballot64(e >= 0 && ((e >> b) & 1));
    m &= ((e >> b) & 1) ? set : ~set;
  }
  return e >= 0 ? m : 0ull;
}

// wcnt[granule][expert] of chunk `c` (LDS, kMoeGranules x E ints) and this lane's expert / match mask per granule of its wave
__device__ __forceinline__ void moe_chunk_counts(const int64_t* __restrict__ ids, int64_t npairs, int E, int64_t c, int* wcnt,
                                                 int* my_e, unsigned long long* my_m) {
  const int lane = lane_id(), wave = wave_id_uniform();
  for (int i = threadIdx.x; i < kMoeGranules * E; i += kMoeThreads) wcnt[i] = 0;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kMoeGranules / 4; ++i) {
    const int gi = wave * (kMoeGranules / 4) + i;
    const int64_t p = c * kMoeChunk + gi * 64 + lane;
    int e = -1;
    if (p < npairs) {
      const int64_t id = ids[p];
      e = (id >= 0 && id < E) ? (int)id : -1;
    }
    const unsigned long long m = moe_match(e);
    my_e[i] = e;
    my_m[i] = m;
    // one writer per (granule, expert): the lowest lane of the match group
    if (e >= 0 && (m & ((1ull << lane) - 1ull)) == 0ull) wcnt[gi * E + e] = __builtin_popcountll(m);
  }
  __syncthreads();
}

// pass 1: pairs per (chunk, expert)
__global__ __launch_bounds__(kMoeThreads) void moe_count_kernel(const int64_t* __restrict__ ids, int64_t npairs, int E,
                                                                 int* __restrict__ chunk_cnt) {
  __shared__ int wcnt[kMoeGranules * kMoeMaxExperts];
  int my_e[kMoeGranules / 4];
  unsigned long long my_m[kMoeGranules / 4];
  moe_chunk_counts(ids, npairs, E, (int64_t)blockIdx.x, wcnt, my_e, my_m);
  const int e = threadIdx.x;
  if (e < E) {
    int s = 0;
#pragma unroll
    for (int g = 0; g < kMoeGranules; ++g) s += wcnt[g * E + e];
    chunk_cnt[(int64_t)blockIdx.x * E + e] = s;
  }
}

// pass 2 (one workgroup): chunk_cnt -> exclusive prefix over the chunks (in place), count, offset, the row-tile table
//   tiles[0 .. E]        first row tile of expert e (tiles[E] = row tiles in use)
//   tiles[E+1 + j]       expert of row tile j, -1 from tiles[E] on                         (j < max_tiles)
__global__ __launch_bounds__(kMoeThreads) void moe_scan_kernel(int* __restrict__ chunk_cnt, int nchunks, int E,
                                                                int* __restrict__ count, int* __restrict__ offset,
                                                                int* __restrict__ tiles, int max_tiles) {
  __shared__ int s_cnt[kMoeMaxExperts], s_first[kMoeMaxExperts + 1];
  const int e = threadIdx.x;
  if (e < E) {
    int run = 0;
    for (int c = 0; c < nchunks; ++c) {
      const int v = chunk_cnt[(int64_t)c * E + e];
      chunk_cnt[(int64_t)c * E + e] = run;
      run += v;
    }
    s_cnt[e] = run;
    count[e] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int off = 0, first = 0;
    for (int i = 0; i < E; ++i) {
      const int padded = (s_cnt[i] + kMoeSegRows - 1) / kMoeSegRows * kMoeSegRows;
      offset[i] = off;
      s_first[i] = first;
      off += padded;
      first += (padded + kMoeTileRows - 1) / kMoeTileRows;
    }
    offset[E] = off;
    s_first[E] = first;
  }
  __syncthreads();
  if (e <= E) tiles[e] = s_first[e];
  if (e < E)
    for (int j = s_first[e]; j < s_first[e + 1] && j < max_tiles; ++j) tiles[E + 1 + j] = e;
  for (int j = s_first[E] + (int)threadIdx.x; j < max_tiles; j += kMoeThreads) tiles[E + 1 + j] = -1;
}

// pass 3: pos = offset[e] + pairs of e in earlier chunks + in earlier granules of this chunk + in lower lanes of this granule
__global__ __launch_bounds__(kMoeThreads) void moe_rank_kernel(const int64_t* __restrict__ ids, int64_t npairs, int E,
                                                                const int* __restrict__ chunk_base,
                                                                const int* __restrict__ offset, int* __restrict__ pos) {
  __shared__ int wcnt[kMoeGranules * kMoeMaxExperts];
  int my_e[kMoeGranules / 4];
  unsigned long long my_m[kMoeGranules / 4];
  moe_chunk_counts(ids, npairs, E, (int64_t)blockIdx.x, wcnt, my_e, my_m);
  const int e = threadIdx.x;
  if (e < E) {
    int run = offset[e] + chunk_base[(int64_t)blockIdx.x * E + e];
#pragma unroll
    for (int g = 0; g < kMoeGranules; ++g) {
      const int v = wcnt[g * E + e];
      wcnt[g * E + e] = run;
      run += v;
    }
  }
  __syncthreads();
  const int lane = lane_id(), wave = wave_id_uniform();
#pragma unroll
  for (int i = 0; i < kMoeGranules / 4; ++i) {
    const int gi = wave * (kMoeGranules / 4) + i;
    const int64_t p = (int64_t)blockIdx.x * kMoeChunk + gi * 64 + lane;
    if (p < npairs)
      pos[p] = my_e[i] >= 0 ? wcnt[gi * E + my_e[i]] + __builtin_popcountll(my_m[i] & ((1ull << lane) - 1ull)) : -1;
  }
}

// the rows no pair owns: workgroup b < E zeroes rows [offset[b] + count[b], offset[b + 1]) (at most 63), the kMoeTailBlocks
// workgroups behind them the rows [offset[E], rows_pad)
template <typename T>
__device__ __forceinline__ void moe_zero_padding(T* __restrict__ dst, const int* __restrict__ count,
                                                 const int* __restrict__ offset, int E, int64_t rows_pad, int H, int b) {
  const int chunks = H / 8;
  int64_t r0, r1, step = 1;
  if (b < E) {
    r0 = (int64_t)offset[b] + count[b];
    r1 = offset[b + 1];
  } else {
    r0 = (int64_t)offset[E] + (b - E);
    r1 = rows_pad;
    step = kMoeTailBlocks;
  }
  for (int64_t r = r0; r < r1; r += step)
    for (int i = threadIdx.x; i < chunks; i += kMoeThreads) st16(dst + r * H + (int64_t)i * 8, u32x4{0u, 0u, 0u, 0u});
}

// Xs[pos[p]] = X[p / k] in 16-byte pieces, one wave per pair; workgroups >= pair_blocks zero the padding rows
template <typename T>
__global__ __launch_bounds__(kMoeThreads) void moe_gather_kernel(const T* __restrict__ X, const int* __restrict__ pos,
                                                                  const int* __restrict__ count,
                                                                  const int* __restrict__ offset, T* __restrict__ Xs,
                                                                  int64_t npairs, int k, int E, int H, int64_t rows_pad,
                                                                  int pair_blocks) {
  if ((int)blockIdx.x >= pair_blocks) {
    moe_zero_padding<T>(Xs, count, offset, E, rows_pad, H, (int)blockIdx.x - pair_blocks);
    return;
  }
  const int lane = lane_id(), chunks = H / 8;
  for (int64_t p = (int64_t)blockIdx.x * 4 + wave_id_uniform(); p < npairs; p += (int64_t)pair_blocks * 4) {
    const int row = pos[p];
    if (row < 0) continue;
    const T* src = X + (p / k) * H;
    T* dst = Xs + (int64_t)row * H;
    for (int i = lane; i < chunks; i += 64) st16(dst + (int64_t)i * 8, ld16(src + (int64_t)i * 8));
  }
}

template <typename T, bool WF32>
__device__ __forceinline__ float moe_weight(const void* w, int64_t p) {
  if (w == nullptr) return 1.f;
  if (WF32) return reinterpret_cast<const float*>(w)[p];
  return elem<T>::to_f32(reinterpret_cast<const typename elem<T>::raw*>(w)[p]);
}

// out[t] = rT(sum_j r32(w[t, j] * f32(Ys[pos[t, j]]))): j ascending, fp32 multiply then fp32 add, one rounding at the end;
// one wave per token.  w == nullptr: unit weights (the gradient of the gather)
template <typename T, bool WF32>
__global__ __launch_bounds__(kMoeThreads) void moe_combine_kernel(const T* __restrict__ Ys, const int* __restrict__ pos,
                                                                   const void* __restrict__ w, T* __restrict__ out,
                                                                   int64_t tokens, int k, int H) {
  const int lane = lane_id(), chunks = H / 8;
  for (int64_t t = (int64_t)blockIdx.x * 4 + wave_id_uniform(); t < tokens; t += (int64_t)gridDim.x * 4) {
    for (int i = lane; i < chunks; i += 64) {
      float acc[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = 0.f;
      for (int j = 0; j < k; ++j) {
        const int row = pos[t * k + j];
        if (row < 0) continue;
        const float wj = moe_weight<T, WF32>(w, t * k + j);
        float y[8];
        unpack16<T>(ld16(Ys + (int64_t)row * H + (int64_t)i * 8), y);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float prod = wj * y[q];
          acc[q] = acc[q] + prod;
        }
      }
      st16(out + t * H + (int64_t)i * 8, pack16<T>(acc));
    }
  }
}

// dYs[pos[p]] = rT(w[p] * f32(dOut[p / k])) and dw[p] = sum_h f32(dOut[p / k, h]) * f32(Ys[pos[p], h]) (fp32: every lane sums
// its 16-byte pieces in ascending order, element 0..7 inside a piece, then the 64 lanes are joined by the xor butterfly of
// wave_sum -- a fixed order); one wave per pair, padding rows of dYs zeroed as in the gather.  pos = -1: dw = 0, no row
template <typename T, bool WF32>
__global__ __launch_bounds__(kMoeThreads) void moe_combine_bwd_kernel(const T* __restrict__ dOut, const T* __restrict__ Ys,
                                                                       const int* __restrict__ pos,
                                                                       const void* __restrict__ w,
                                                                       const int* __restrict__ count,
                                                                       const int* __restrict__ offset, T* __restrict__ dYs,
                                                                       void* __restrict__ dw, int64_t npairs, int k, int E,
                                                                       int H, int64_t rows_pad, int pair_blocks) {
  if ((int)blockIdx.x >= pair_blocks) {
    moe_zero_padding<T>(dYs, count, offset, E, rows_pad, H, (int)blockIdx.x - pair_blocks);
    return;
  }
  const int lane = lane_id(), chunks = H / 8;
  for (int64_t p = (int64_t)blockIdx.x * 4 + wave_id_uniform(); p < npairs; p += (int64_t)pair_blocks * 4) {
    const int row = pos[p];
    float dot = 0.f;
    if (row >= 0) {
      const float wp = moe_weight<T, WF32>(w, p);
      const T* g = dOut + (p / k) * H;
      const T* y = Ys + (int64_t)row * H;
      T* d = dYs + (int64_t)row * H;
      for (int i = lane; i < chunks; i += 64) {
        float gv[8], yv[8], o[8];
        unpack16<T>(ld16(g + (int64_t)i * 8), gv);
        unpack16<T>(ld16(y + (int64_t)i * 8), yv);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          o[q] = wp * gv[q];
          const float prod = gv[q] * yv[q];
          dot = dot + prod;
        }
        st16(d + (int64_t)i * 8, pack16<T>(o));
      }
    }
    dot = wave_sum(dot);
    if (lane == 0 && dw != nullptr) {
      if (WF32)
        reinterpret_cast<float*>(dw)[p] = dot;
      else
        reinterpret_cast<typename elem<T>::raw*>(dw)[p] = elem<T>::from_f32(dot);
    }
  }
}

static int64_t moe_chunks(int64_t npairs) { return ceil_div(npairs > 0 ? npairs : 1, kMoeChunk); }
// row tiles of the routed GEMM: sum_e ceil(pad64(count_e) / 256) <= (rows_pad + 192 E) / 256
static int64_t moe_max_tiles(int64_t rows_pad, int64_t E) { return ceil_div(rows_pad + 192 * E, kMoeTileRows); }
static unsigned moe_pair_blocks(int64_t n) {
  int64_t b = ceil_div(n, 4);
  if (b > 256 * 8) b = 256 * 8;
  return (unsigned)(b < 1 ? 1 : b);
}
// rows of the expert-sorted buffers: S + 63 E rounded up to whole segments -- known to the host without reading the device
static int64_t moe_rows_pad_min(int64_t tokens, int64_t top_k, int64_t experts) {
  return ceil_div(tokens * top_k + (kMoeSegRows - 1) * experts, kMoeSegRows) * kMoeSegRows;
}
static int moe_check_shape(int64_t tokens, int64_t top_k, int64_t experts, int64_t hidden, int64_t rows_pad) {
  if (tokens <= 0 || top_k <= 0 || experts <= 0 || hidden <= 0) return TAMD_E_SHAPE;
  if (experts > kMoeMaxExperts || (hidden % 8) != 0) return TAMD_E_SHAPE;
  if (tokens * top_k >= ((int64_t)1 << 31) - 64 * (kMoeMaxExperts + 1)) return TAMD_E_SHAPE;  // rows are 32-bit
  if (rows_pad >= 0 && ((rows_pad % kMoeSegRows) != 0 || rows_pad < moe_rows_pad_min(tokens, top_k, experts)))
    return TAMD_E_SHAPE;
  return TAMD_OK;
}

}  // namespace tamd

using namespace tamd;

extern "C" {

size_t tamd_moe_route_workspace_bytes(int64_t tokens, int64_t top_k, int64_t experts) {
  if (tokens <= 0 || top_k <= 0 || experts <= 0 || experts > kMoeMaxExperts) return 0;
  return (size_t)moe_chunks(tokens * top_k) * (size_t)experts * sizeof(int);
}

int tamd_moe_route(const int64_t* top_k_index, int32_t* count, int32_t* offset, int32_t* pos, int32_t* tiles,
                   void* workspace, size_t workspace_bytes, int64_t tokens, int64_t top_k, int64_t experts,
                   int64_t rows_pad, tamd_stream_t stream) {
  if (!top_k_index || !count || !offset || !pos || !tiles || !workspace) return TAMD_E_NULL;
  const int st = moe_check_shape(tokens, top_k, experts, 8, rows_pad);
  if (st != TAMD_OK) return st;
  if ((reinterpret_cast<uintptr_t>(top_k_index) & 7u) || (reinterpret_cast<uintptr_t>(count) & 3u) ||
      (reinterpret_cast<uintptr_t>(offset) & 3u) || (reinterpret_cast<uintptr_t>(pos) & 3u) ||
      (reinterpret_cast<uintptr_t>(tiles) & 3u) || (reinterpret_cast<uintptr_t>(workspace) & 3u))
    return TAMD_E_ALIGN;
  if (workspace_bytes < tamd_moe_route_workspace_bytes(tokens, top_k, experts)) return TAMD_E_WORKSPACE;
  const int64_t npairs = tokens * top_k, nchunks = moe_chunks(npairs);
  hipStream_t s = TAMD_STREAM(stream);
  int* cc = reinterpret_cast<int*>(workspace);
  hipLaunchKernelGGL(moe_count_kernel, dim3((unsigned)nchunks), dim3(kMoeThreads), 0, s, top_k_index, npairs, (int)experts, cc);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(kMoeThreads), 0, s, cc, (int)nchunks, (int)experts, count, offset, tiles,
                     (int)moe_max_tiles(rows_pad, experts));
  hipLaunchKernelGGL(moe_rank_kernel, dim3((unsigned)nchunks), dim3(kMoeThreads), 0, s, top_k_index, npairs, (int)experts,
                     (const int*)cc, (const int*)offset, pos);
  return launch_status();
}

int tamd_moe_gather(const void* x, const int32_t* pos, const int32_t* count, const int32_t* offset, void* xs, int64_t tokens,
                    int64_t top_k, int64_t experts, int64_t hidden, int64_t rows_pad, int dtype, tamd_stream_t stream) {
  if (!x || !pos || !count || !offset || !xs) return TAMD_E_NULL;
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  const int st = moe_check_shape(tokens, top_k, experts, hidden, rows_pad);
  if (st != TAMD_OK) return st;
  if (!aligned16(x) || !aligned16(xs)) return TAMD_E_ALIGN;
  const unsigned pb = moe_pair_blocks(tokens * top_k);
  TAMD_DISPATCH_HALF(dtype, {
    hipLaunchKernelGGL((moe_gather_kernel<T>), dim3(pb + (unsigned)experts + kMoeTailBlocks), dim3(kMoeThreads), 0,
                       TAMD_STREAM(stream), (const T*)x, pos, count, offset, (T*)xs, tokens * top_k, (int)top_k, (int)experts,
                       (int)hidden, rows_pad, (int)pb);
  });
  return launch_status();
}

int tamd_moe_combine(const void* ys, const int32_t* pos, const void* w, void* out, int64_t tokens, int64_t top_k,
                     int64_t hidden, int w_dtype, int dtype, tamd_stream_t stream) {
  if (!ys || !pos || !out) return TAMD_E_NULL;
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  if (w && w_dtype != TAMD_F32 && w_dtype != dtype) return TAMD_E_DTYPE;
  const int st = moe_check_shape(tokens, top_k, 1, hidden, -1);
  if (st != TAMD_OK) return st;
  if (!aligned16(ys) || !aligned16(out)) return TAMD_E_ALIGN;
  if (w && (reinterpret_cast<uintptr_t>(w) & (w_dtype == TAMD_F32 ? 3u : 1u))) return TAMD_E_ALIGN;
  const dim3 grid(moe_pair_blocks(tokens)), block(kMoeThreads);
  TAMD_DISPATCH_HALF(dtype, {
    if (w && w_dtype == TAMD_F32)
      hipLaunchKernelGGL((moe_combine_kernel<T, true>), grid, block, 0, TAMD_STREAM(stream), (const T*)ys, pos, w, (T*)out,
                         tokens, (int)top_k, (int)hidden);
    else
      hipLaunchKernelGGL((moe_combine_kernel<T, false>), grid, block, 0, TAMD_STREAM(stream), (const T*)ys, pos, w, (T*)out,
                         tokens, (int)top_k, (int)hidden);
  });
  return launch_status();
}

int tamd_moe_combine_bwd(const void* dout, const void* ys, const int32_t* pos, const void* w, const int32_t* count,
                         const int32_t* offset, void* dys, void* dw, int64_t tokens, int64_t top_k, int64_t experts,
                         int64_t hidden, int64_t rows_pad, int w_dtype, int dtype, tamd_stream_t stream) {
  if (!dout || !ys || !pos || !w || !count || !offset || !dys || !dw) return TAMD_E_NULL;
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  if (w_dtype != TAMD_F32 && w_dtype != dtype) return TAMD_E_DTYPE;
  const int st = moe_check_shape(tokens, top_k, experts, hidden, rows_pad);
  if (st != TAMD_OK) return st;
  if (!aligned16(dout) || !aligned16(ys) || !aligned16(dys)) return TAMD_E_ALIGN;
  const unsigned wmask = w_dtype == TAMD_F32 ? 3u : 1u;
  if ((reinterpret_cast<uintptr_t>(w) & wmask) || (reinterpret_cast<uintptr_t>(dw) & wmask)) return TAMD_E_ALIGN;
  const unsigned pb = moe_pair_blocks(tokens * top_k);
  const dim3 grid(pb + (unsigned)experts + kMoeTailBlocks), block(kMoeThreads);
  TAMD_DISPATCH_HALF(dtype, {
    if (w_dtype == TAMD_F32)
      hipLaunchKernelGGL((moe_combine_bwd_kernel<T, true>), grid, block, 0, TAMD_STREAM(stream), (const T*)dout, (const T*)ys,
                         pos, w, count, offset, (T*)dys, dw, tokens * top_k, (int)top_k, (int)experts, (int)hidden, rows_pad,
                         (int)pb);
    else
      hipLaunchKernelGGL((moe_combine_bwd_kernel<T, false>), grid, block, 0, TAMD_STREAM(stream), (const T*)dout, (const T*)ys,
                         pos, w, count, offset, (T*)dys, dw, tokens * top_k, (int)top_k, (int)experts, (int)hidden, rows_pad,
                         (int)pb);
  });
  return launch_status();
}

}  // extern "C"
