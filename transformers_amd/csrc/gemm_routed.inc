// gemm_routed.inc -- the full-line kernel body (gemm_fl_body, gemm.hip) behind problem sizes that live in DEVICE memory:
// the experts of a sparse mixture-of-experts block (integrations/moe.py: grouped_mm_experts_forward / the eager per-expert
// loop of `MixtralExperts.forward`, models/mixtral/modeling_mixtral.py) as ONE launch per product, without the host ever
// reading a count.  Included at the end of gemm.hip; gemm_fl_body and everything it calls are used as they are.
//
// The rows of every expert are one segment [offset[e], offset[e + 1]) of the expert-sorted buffers (tamd_moe_route: segments
// are whole multiples of 64 rows, padding rows hold zeros).  Every workgroup reads its entry of the plan with workgroup-uniform
// (scalar) loads, builds the GemmArgs of its expert's product in registers and runs the body with its index inside that product
// -- what gemm_fl_group_kernel does with grp.p[i].
//   rows routed (forward, dX; plain or SwiGLU way out)
//       grid (tiles_n, max row tiles): blockIdx.y = a 256-row tile j of the sorted buffer, tiles[E + 1 + j] its expert (-1:
//       surplus, the workgroup exits), tiles[e] the expert's first row tile.
//         A = Xs + offset[e] lda, M = offset[e+1] - offset[e], B = W + e b_stride, C = Ys + offset[e] ldc
//       index inside the product = (j - tiles[e]) tiles_n + blockIdx.x.  No division anywhere.  The first workgroup of a
//       product is NOT padded to a multiple of 8 as gemm_group_launch does: gemm_tile_of_block reads `index & 7` as a label
//       of the workgroups that share an XCD, and with dispatch order = linear block id, (linear - start) & 7 is a rotation of
//       linear & 7 -- workgroups with equal labels still share an XCD, and labels 0 .. nwg % 8 - 1 still carry the extra tile
//       because the indices run 0 .. nwg - 1.  Padding would change nothing but the number of idle workgroups.
//   K routed (weight gradients dW_e = dYs_e^T . Xs_e, both operands k-major)
//       grid (tiles, E): blockIdx.y = the expert, K = offset[e+1] - offset[e] (whole 64-deep stages), C = dW + e c_stride.
//       An expert WITHOUT rows: gemm_fl_body has never run with zero stages (its prologue requests stages 0 and 1
//       unconditionally), so the wrapper stores the tile's zeros itself and returns before the body.

namespace tamd {

struct GemmRoutedArgs {
  GemmArgs g;          // expert 0's product; M (rows routed) / K (K routed) are filled in per workgroup
  const int* offset;   // [E + 1] segment starts (rows)
  const int* tiles;    // rows routed: [E + 1] first row tile per expert, then the expert of every row tile
  int64_t b_stride;    // rows routed: elements between the experts' weights
  int64_t c_stride;    // K routed: elements between the experts' gradients
  int experts;
};

template <typename T, bool A_KM, bool B_KN, int EPI>
__global__ __launch_bounds__(kFlThreads, 1) void gemm_fl_routed_kernel(GemmRoutedArgs r) {
  GemmArgs g = r.g;
  int local;
  if constexpr (A_KM) {
    const int e = (int)blockIdx.y;
    const int o0 = r.offset[e], o1 = r.offset[e + 1];
    g.A = reinterpret_cast<const T*>(g.A) + (int64_t)o0 * g.lda;
    g.B = reinterpret_cast<const T*>(g.B) + (int64_t)o0 * g.ldb;
    g.C = reinterpret_cast<T*>(g.C) + (int64_t)e * r.c_stride;
    g.K = o1 - o0;
    local = (int)blockIdx.x;
    if (o1 <= o0) {  // no rows: the gradient is zero
      int tile_m, tile_n;
      gemm_tile_of_block(g, local, &tile_m, &tile_n);
      const int64_t n = (int64_t)tile_n * kBN + (threadIdx.x & 31) * 8;
      T* C = reinterpret_cast<T*>(g.C);
      for (int row = (int)threadIdx.x >> 5; row < kBM; row += kFlThreads / 32) {
        const int64_t m = (int64_t)tile_m * kBM + row;
        if (m < g.M && n < g.N) st16(C + m * g.ldc + n, u32x4{0u, 0u, 0u, 0u});
      }
      return;
    }
  } else {
    const int j = (int)blockIdx.y;
    const int e = r.tiles[r.experts + 1 + j];
    if (e < 0) return;
    const int o0 = r.offset[e], o1 = r.offset[e + 1];
    g.A = reinterpret_cast<const T*>(g.A) + (int64_t)o0 * g.lda;
    g.B = reinterpret_cast<const T*>(g.B) + (int64_t)e * r.b_stride;
    if (g.C != nullptr) g.C = reinterpret_cast<T*>(g.C) + (int64_t)o0 * g.ldc;
    if (EPI == kEpiSwiGLU) g.C2 = reinterpret_cast<T*>(g.C2) + (int64_t)o0 * g.ldc2;
    g.M = o1 - o0;
    g.tiles_m = (o1 - o0 + kBM - 1) / kBM;
    local = (j - r.tiles[e]) * g.tiles_n + (int)blockIdx.x;
  }
  gemm_fl_body<T, A_KM, B_KN, EPI, TAMD_ACT_NONE, kSchedAuto>(g, local);
}

}  // namespace tamd

#ifndef TAMD_GEMM_KERNELS_ONLY

// The products of the experts of a mixture-of-experts block over the expert-sorted buffers of tamd_moe_route (include/tamd.h).
extern "C" int tamd_gemm_routed(const void* A, const void* B, void* C, void* C2, const int32_t* offset, const int32_t* tiles,
                                int64_t rows_pad, int64_t experts, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                int64_t ldc, int64_t ldc2, int64_t b_stride, int flags, int epilogue, int dtype,
                                tamd_stream_t stream) {
  if (flags & ~(TAMD_GEMM_A_KM | TAMD_GEMM_B_KN)) return TAMD_E_ARG;
  const bool akm = flags & TAMD_GEMM_A_KM, bkn = flags & TAMD_GEMM_B_KN;
  if (akm && !bkn) return TAMD_E_ARG;
  if (epilogue != TAMD_EPI_NONE && epilogue != TAMD_EPI_SWIGLU) return TAMD_E_ARG;
  if (epilogue == TAMD_EPI_SWIGLU && flags != 0) return TAMD_E_ARG;
  if (dtype != TAMD_BF16 && dtype != TAMD_F16) return TAMD_E_DTYPE;
  const bool swiglu = epilogue == TAMD_EPI_SWIGLU;
  if (!A || !B || !offset || (!swiglu && !C) || (swiglu && !C2) || (!akm && !tiles)) return TAMD_E_NULL;
  if (experts <= 0 || experts > 256 || rows_pad <= 0 || (rows_pad % 64) || N <= 0) return TAMD_E_SHAPE;
  if ((N % 8) || (lda % 8) || (ldb % 8) || (C && (ldc % 8))) return TAMD_E_SHAPE;
  if (akm ? (M <= 0 || (M % 8)) : (K <= 0 || (K % kXK) || b_stride <= 0 || (b_stride % 8))) return TAMD_E_SHAPE;
  if (swiglu && ((N % 16) || (ldc2 % 8) || (int64_t)N * ldb * 2 >= ((int64_t)1 << 31))) return TAMD_E_SHAPE;  // (tamd_gemm_swiglu's limit)
  if (rows_pad >= ((int64_t)1 << 31)) return TAMD_E_SHAPE;
  if (!aligned16(A) || !aligned16(B) || (C && !aligned16(C)) || (swiglu && !aligned16(C2))) return TAMD_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(offset) & 3u) || (tiles && (reinterpret_cast<uintptr_t>(tiles) & 3u))) return TAMD_E_ALIGN;
  GemmRoutedArgs r;
  // (M of the rows-routed product and K of the K-routed one are placeholders: every workgroup fills in its expert's)
  gemm_fill_args(&r.g, A, B, C, nullptr, nullptr, akm ? M : kBM, N, akm ? kXK : K, lda, ldb, ldc, 0);
  r.g.trace = nullptr;
  r.g.timeline = nullptr;
  r.offset = offset;
  r.tiles = tiles;
  r.b_stride = b_stride;
  r.c_stride = M * ldc;
  r.experts = (int)experts;
  dim3 grid, block(kFlThreads);
  if (akm) {
    grid = dim3((unsigned)(r.g.tiles_m * r.g.tiles_n), (unsigned)experts);
  } else {
    if (swiglu) {
      r.g.tiles_n = (int)ceil_div(N / 2, kBN / 2);  // 128 features (gate + up columns) per 256-wide tile
      r.g.C2 = C2;
      r.g.ldc2 = ldc2;
      r.g.n_half = N / 2;
    }
    const int64_t max_tiles = ceil_div(rows_pad + 192 * experts, kBM);  // (moe_route.inc moe_max_tiles)
    if (max_tiles > 65535) return TAMD_E_SHAPE;
    grid = dim3((unsigned)r.g.tiles_n, (unsigned)max_tiles);
  }
  hipStream_t s = TAMD_STREAM(stream);
  TAMD_DISPATCH_HALF(dtype, {
    if (akm)
      hipLaunchKernelGGL((gemm_fl_routed_kernel<T, true, true, TAMD_EPI_NONE>), grid, block, (size_t)kXSmem, s, r);
    else if (swiglu)
      hipLaunchKernelGGL((gemm_fl_routed_kernel<T, false, false, kEpiSwiGLU>), grid, block, (size_t)kXSmem, s, r);
    else if (bkn)
      hipLaunchKernelGGL((gemm_fl_routed_kernel<T, false, true, TAMD_EPI_NONE>), grid, block, (size_t)kXSmem, s, r);
    else
      hipLaunchKernelGGL((gemm_fl_routed_kernel<T, false, false, TAMD_EPI_NONE>), grid, block, (size_t)kXSmem, s, r);
    return launch_status();
  });
  return TAMD_E_DTYPE;
}

#endif  // TAMD_GEMM_KERNELS_ONLY
