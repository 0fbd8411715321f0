// gemm_fp8w.inc -- tamd_gemm_fp8w from 65 to 1024 rows of X (fp8w_use_tile): ONE fused tile kernel.  Included by gemv_fp8.inc in
// front of the C entry points (it uses GemvFp8Args, fp8x16_to_f32 and kFp8Block from there).
//
//   Wd = rT(r32(f32(W8) * S))   built in registers in front of the MFMAs, bit for bit what dequant_fp8w_kernel writes
//   Y  = X . Wd^T               fp32 accumulation, tamd_gemm's epilogue chain (NONE / BIAS / RESIDUAL)
//
// What it replaces is dequant_fp8w_kernel into a workspace + tamd_gemm per row chunk: Wd written to HBM and read back (the weight
// bytes move three times) and two launches per chunk.  Here Wd never reaches memory, the workspace is not written, and the call is
// one launch.  Only the fp32 summation order differs from that path.
//
// Tile and K step.  A workgroup of four waves owns 128 weight rows starting at a multiple of 128 -- exactly one row of S -- against
// BM rows of X, and steps K by 128, one scale block: a K step has ONE scale for the whole workgroup.  Its address is wave-uniform,
// so it is a scalar load, issued one step ahead.
//
// W never touches LDS: each byte is needed by exactly one wave.  Wave w owns weight rows 32 w .. 32 w + 31 as two 16-row blocks and
// loads them global -> registers in gemv_fp8w_mfma_kernel's lane layout: lane l takes the 16 bytes W[row0 + (l & 15)][k0 + 64 h +
// 16 (l >> 4) .. + 15], h = 0, 1 -- 64 contiguous bytes per row and instruction.  It converts them once per step (fp8x16_to_f32,
// times the scale, pack2<T>); the two 8-element halves are the A operands of two v_mfma_f32_16x16x32, shared by the BM / 16 row
// tiles of X.  Rows past a ragged N re-read row N - 1 (same scale row; their accumulators are never stored); lanes past a ragged K
// load zeros and take the scale 0.  The bytes of step i + 1 are requested before the arithmetic of step i.
//
// X goes through LDS once per workgroup and K step: BM x 128 elements of T (256 bytes per row), double-buffered, by range-checked
// LDS-DMA (glds16_buf_rng): the buffer is the M tile's live rows, so rows past M arrive as zeros, and a lane whose 8 columns lie
// past K asks for an offset outside every buffer and gets zeros too -- no branch, no zero page.  A lane reads its B operand with
// the SAME k permutation as its A operand: the 32 bytes X[16 t + (l & 15)][64 h + 16 (l >> 4) ..], two 16-byte reads.
//   Swizzle.  With rows 256 bytes apart those reads would hit one 16-byte bank group 16 ways.  The 16-byte piece c (0 .. 15) of row
//   r is kept at piece c ^ (r & 15) of the row.  ds_read_b128 serves 16 lanes at a time: 8 rows of one lane group and 8 rows of
//   the next (pieces c and c + 2, c even); c ^ {0 .. 3, 12 .. 15} and (c + 2) ^ {4 .. 11} are the 16 distinct pieces, i.e. all 64
//   banks once: conflict-free, and so is the second read (pieces c + 1, c + 3).  The DMA's destination is fixed at lane x 16 bytes,
//   so the swizzle is applied to the SOURCE address: lane l of the piece that fills rows 4 q .. 4 q + 3 fetches row 4 q + (l >> 4),
//   piece (l & 15) ^ (row & 15).
//   Order.  Step i requests X and W of step i + 1, runs its MFMAs, then waits for everything it requested (vmcnt(0)) and meets the
//   other waves at ONE barrier: the data of step i + 1 is complete and buffer i & 1 is free for the request of step i + 2.  The
//   look-ahead is one K step, so a single workgroup does not cover HBM latency on its own: two (BM = 128) or more (BM = 64)
//   workgroups per CU do.
//
// Accumulator (rb, t) of a wave, register r of lane l, is y[m0 + 16 t + (l & 15)][n0 + 32 w + 16 rb + 4 (l >> 4) + r], as in
// gemv_fp8w_mfma_kernel: each wave holds its 32 weight rows against all BM rows, there is no reduction across waves, and the four
// consecutive n of a lane leave as one 8-byte store, predicated on m < M and n < N (N % 8 == 0 and ldy % 8 == 0 hold in this form).
//
// Instantiations: BM = 64 (32 accumulator registers, 32 KiB of LDS) and BM = 128 (64 registers, 64 KiB: two workgroups per CU, which
// is what __launch_bounds__(256, 2) asks the register allocator to keep possible).  BM = 256 is not built: 128 KiB of LDS would
// leave one workgroup per CU with a one-step look-ahead.  Registers and scratch: profiles/fp8_linear_isa.md (no scratch).
//
// Grid: ceil(N / 128) x ceil(M / BM) tiles on a one-dimensional grid.  Consecutive workgroup ids go round the eight XCDs, so id b
// runs on XCD b % 8 as that XCD's workgroup number b / 8.  W tile nt belongs to XCD nt % 8, and an XCD walks the M tiles of one
// W tile before it starts the next: the workgroups that share 128 x K weight bytes run back to back on ONE L2, which fetches them
// from HBM once, while X (read by every W tile) comes from L2 / the last-level cache.  The grid is padded to whole rounds of eight
// W tiles; the padding workgroups leave at once.

namespace tamd {

constexpr int kFp8TileN = 128;  // weight rows per workgroup: one row of S

// S[idx] at a WAVE-UNIFORM address through the constant address space: a scalar load, the value arrives in an SGPR (through the
// global address space the compiler issues one vector load per lane for it)
__device__ __forceinline__ float uniform_f32(const float* table, int64_t idx) {
#ifdef __HIP__
  typedef const __attribute__((address_space(4))) float* cptr32;
  return ((cptr32)(table))[idx];
#else
  return table[idx];
#endif
}

template <typename T, int BM, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_fp8w_kernel(GemvFp8Args g, int mtiles) {
  typedef typename elem<T>::raw raw;
  static_assert(BM % 64 == 0, "every wave requests BM / 16 whole pieces of four rows");
  constexpr int MT = BM / 16;          // 16-row tiles of X
  constexpr int NI = BM / 16;          // 1 KiB pieces (four rows of X) per wave and K step
  constexpr unsigned BUFB = BM * 256u;  // one X buffer
  TAMD_DYN_SMEM(smem);
  const int lane = threadIdx.x & 63, wave = wave_id_uniform();
  const int l15 = lane & 15, g4 = lane >> 4;
  const int64_t wg = (int64_t)blockIdx.x >> 3;
  const int64_t n0 = ((wg / mtiles) * 8 + (blockIdx.x & 7)) * kFp8TileN, m0 = (wg % mtiles) * BM;
  if (n0 >= g.N) return;  // (padding of the last round of eight W tiles; the whole workgroup)

  // X: the M tile's live rows as one buffer; piece i of this wave fills rows 4 (wave NI + i) .. + 3 of the tile
  const T* __restrict__ xb = reinterpret_cast<const T*>(g.X) + m0 * g.ldx;
  const int64_t live = g.M - m0 < BM ? g.M - m0 : BM;
  const unsigned xbytes = (unsigned)(((live - 1) * g.ldx + g.K) * 2);  // (host: BM * ldx * 2 < 2^31)
  unsigned xoff[NI];
  int xcol[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = 4 * (wave * NI + i) + g4, c = l15 ^ (row & 15);
    xoff[i] = (unsigned)row * (unsigned)g.ldx * 2u + (unsigned)c * 16u;
    xcol[i] = 8 * c;
  }
  auto request_x = [&](int buf, int64_t k0) {
#pragma unroll
    for (int i = 0; i < NI; ++i)  // (K % 16 == 0: a lane's 8 columns are inside or outside together)
      glds16_buf_rng(xb, xbytes, k0 + xcol[i] < g.K ? xoff[i] + (unsigned)k0 * 2u : 0x80000000u, smem,
                     (unsigned)buf * BUFB + (unsigned)(wave * NI + i) * 1024u);
  };
  // ... and where the lane reads its B operands: row l15 of a 16-row tile, pieces 8 h + 2 g4 + j, swizzled
  unsigned roff[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) roff[h][j] = (unsigned)l15 * 256u + (unsigned)((8 * h + 2 * g4 + j) ^ l15) * 16u;

  const unsigned char* wp[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int64_t row = n0 + 32 * wave + 16 * rb + l15;
    wp[rb] = g.W + (row < g.N ? row : g.N - 1) * g.ldw + g4 * 16;  // (rows past N: re-read the last one)
  }
  const u32x4 z = {0u, 0u, 0u, 0u};
  auto request_w = [&](u32x4 (&q)[2][2], int64_t k0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool in = k0 + 64 * h + 16 * g4 < g.K;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) q[h][rb] = in ? ld16(wp[rb] + k0 + 64 * h) : z;
    }
  };
  const float* __restrict__ srow = g.S + (n0 / kFp8Block) * g.lds;
  const int64_t nkb = (g.K + kFp8Block - 1) / kFp8Block;

  f32x4 acc[2 * MT];
#pragma unroll
  for (int i = 0; i < 2 * MT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 wq[2][2];
  request_x(0, 0);
  request_w(wq, 0);
  float s = uniform_f32(srow, 0);
  wait_vmcnt0();
  block_sync();
  for (int64_t kb = 0; kb < nkb; ++kb) {
    const int64_t k0 = kb * kFp8Block;
    const unsigned buf = (unsigned)(kb & 1) * BUFB;
    u32x4 wn[2][2] = {{z, z}, {z, z}};
    float sn = 0.f;
    if (kb + 1 < nkb) {  // (uniform) step kb + 1: X into the buffer that step kb - 1 read, W and the scale into registers
      request_x((int)((kb + 1) & 1), k0 + kFp8Block);
      request_w(wn, k0 + kFp8Block);
      sn = uniform_f32(srow, kb + 1);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float sh = k0 + 64 * h + 16 * g4 < g.K ? s : 0.f;  // (a lane past K multiplies its zeros by zero, whatever the scale is)
      u32x4 a[2][2];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        f32x2 wv[8];
        fp8x16_to_f32(wq[h][rb], wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = wv[e] * f32x2{sh, sh};
        a[rb][0] = u32x4{pack2<T>(wv[0][0], wv[0][1]), pack2<T>(wv[1][0], wv[1][1]), pack2<T>(wv[2][0], wv[2][1]),
                         pack2<T>(wv[3][0], wv[3][1])};
        a[rb][1] = u32x4{pack2<T>(wv[4][0], wv[4][1]), pack2<T>(wv[5][0], wv[5][1]), pack2<T>(wv[6][0], wv[6][1]),
                         pack2<T>(wv[7][0], wv[7][1])};
      }
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const u32x4 b0 = lds_read16(smem, buf + (unsigned)t * 4096u + roff[h][0]);
        const u32x4 b1 = lds_read16(smem, buf + (unsigned)t * 4096u + roff[h][1]);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[rb * MT + t] = mfma16<T>(a[rb][0], b0, acc[rb * MT + t]);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[rb * MT + t] = mfma16<T>(a[rb][1], b1, acc[rb * MT + t]);
      }
    }
    wait_vmcnt0();
    block_sync();
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) wq[h][rb] = wn[h][rb];
    s = sn;
  }

  // the way out: tamd_gemm's chain on the lane's four consecutive n, one 8-byte store
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int64_t n = n0 + 32 * wave + 16 * rb + 4 * g4;
    if (n >= g.N) continue;  // (N % 8 == 0: the four are inside or outside together)
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if ((EPI == TAMD_EPI_BIAS || EPI == TAMD_EPI_RESIDUAL) && g.bias != nullptr) {
      const u32x2 b = ld8(reinterpret_cast<const raw*>(g.bias) + n);
      unpack2<T>(b[0], bv[0], bv[1]);
      unpack2<T>(b[1], bv[2], bv[3]);
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int64_t m = m0 + 16 * t + l15;
      if (m >= g.M) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[rb * MT + t][r] + bv[r];
      if (EPI == TAMD_EPI_RESIDUAL) {
        const u32x2 q = ld8(reinterpret_cast<const raw*>(g.R) + m * g.ldr + n);
        float rv[4];
        unpack2<T>(q[0], rv[0], rv[1]);
        unpack2<T>(q[1], rv[2], rv[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = round_through<T>(v[r]) + rv[r];
      }
      st8(reinterpret_cast<raw*>(g.Y) + m * g.ldy + n, u32x2{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3])});
    }
  }
}

template <typename T, int BM, int EPI>
static void gemm_fp8w_launch_one(const GemvFp8Args& g, hipStream_t s) {
  constexpr size_t smem = 2 * (size_t)BM * 256;
  const int64_t mtiles = ceil_div(g.M, BM), rounds = ceil_div(ceil_div(g.N, kFp8TileN), 8);
  hipLaunchKernelGGL((gemm_fp8w_kernel<T, BM, EPI>), dim3((unsigned)(rounds * 8 * mtiles)), dim3(256), smem, s, g, (int)mtiles);
}
template <typename T, int BM>
static int gemm_fp8w_launch_epi(const GemvFp8Args& g, int epilogue, hipStream_t s) {
  switch (epilogue) {
    case TAMD_EPI_NONE: gemm_fp8w_launch_one<T, BM, TAMD_EPI_NONE>(g, s); break;
    case TAMD_EPI_BIAS: gemm_fp8w_launch_one<T, BM, TAMD_EPI_BIAS>(g, s); break;
    case TAMD_EPI_RESIDUAL: gemm_fp8w_launch_one<T, BM, TAMD_EPI_RESIDUAL>(g, s); break;
    default: return TAMD_E_ARG;
  }
  return launch_status();
}

// Rows of X per workgroup: 128 above 512 rows of X where there are at least 4096 weight rows, 64 otherwise.  Medians, us per call,
// BM = 64 against BM = 128 with the kernel forced (profiles/fp8_linear_ab.jsonl, the arms fp8w_tile64 / fp8w_tile128; K -> N):
//   128 rows   7168 -> 1536 70.3 / 80.5, 7168 -> 576 62.1 / 74.2, 1536 -> 24576 24.3 / 23.1, 16384 -> 7168 154.4 / 178.4,
//              7168 -> 18432 91.3 / 84.1, 18432 -> 7168 176.5 / 202.3
//   256 rows   69.6 / 81.9, 60.7 / 76.3, 34.6 / 31.4, 153.8 / 177.8, 129.5 / 116.1, 174.7 / 200.1
//   512 rows   68.5 / 80.9, 64.1 / 77.4, 59.4 / 51.7, 179.0 / 176.2, 202.3 / 210.1, 208.0 / 198.5
//   1024 rows  70.2 / 81.1, 66.2 / 78.3, 116.4 / 94.9, 362.4 / 264.4, 381.7 / 316.3, 414.2 / 301.9
// Up to 512 rows BM = 64 is the faster one at three or four shapes of six, and the only one that beats the parent's path at every
// shape (BM = 128 loses 7168 -> 1536 at 256 and 512 rows, 81.9 against 81.4 and 80.9 against 78.1); at 1024 rows BM = 128 is 17 ..
// 27 % faster at the four shapes of 7168 weight rows and more and 15 .. 18 % slower at the two small ones.  Nothing was measured between
// 1536 and 7168 weight rows: 4096 is a guess inside that gap.  libtamd_diag.so: TAMD_FP8W_TILE_BM = 64 / 128 overrides the choice,
// read at every call (that is how the arms above were run).
static int fp8w_tile_rows(int64_t m, int64_t n) {
#ifdef TAMD_DIAG
  const char* e = getenv("TAMD_FP8W_TILE_BM");
  if (e && (atoi(e) == 64 || atoi(e) == 128)) return atoi(e);
#endif
  return m > 512 && n >= 4096 ? 128 : 64;
}
template <typename T>
static int gemm_fp8w_launch(const GemvFp8Args& g, int epilogue, hipStream_t s) {
  if (fp8w_tile_rows(g.M, g.N) == 64) return gemm_fp8w_launch_epi<T, 64>(g, epilogue, s);
  return gemm_fp8w_launch_epi<T, 128>(g, epilogue, s);
}

// 0: every M > 16 as before gemm_fp8w_kernel (gemv_fp8w_mfma_kernel up to 64 rows by its own rule, dequantise + GEMM above);
// 2: that kernel for every M > 16; anything else: the rule below.  libtamd_diag.so only (TAMD_FP8W_TILE in the environment, read at
// every call so that tools/fp8_linear_bench.py can alternate the arms inside one process); the product library has the rule alone.
static int fp8w_tile_mode() {
#ifdef TAMD_DIAG
  const char* e = getenv("TAMD_FP8W_TILE");
  return e && (e[0] == '0' || e[0] == '2') ? e[0] - '0' : 1;
#else
  return 1;
#endif
}
// Which M take gemm_fp8w_kernel (M > kGemvMaxRows only): a function of M alone, so small N and short K stay on it -- one launch
// against the two or more of dequantise + GEMM (7168 -> 576: 62.0 us against 80.4 at 128 rows, 64.1 against 78.6 at 512).  The one
// thing the kernel cannot address is a 128-row tile of X of 2 GiB or more (32-bit buffer offsets): such a row stride goes the old way.
// Medians of this kernel forced against the parent's path in one process, cold weights, us per call (profiles/fp8_linear_ab.jsonl,
// the arms fp8w_tile / fp8w_tile64 / fp8w_tile128 against fp8w_before; K -> N in the order 7168 -> 1536, 7168 -> 576, 1536 -> 24576,
// 16384 -> 7168, 7168 -> 18432, 18432 -> 7168).  The spread between the five rounds of one arm, (max - min) / median, was at most
// 2.5 % at any point (a bf16 arm; 2.1 % for an fp8 arm) and below 1 % at most points; every difference the rule rests on is larger than the spread of its two arms.
//   32 rows    71.4 / 20.0, 62.5 / 19.1, 18.8 / 19.0, 156.1 / 74.7, 74.1 / 66.0, 180.6 / 84.7: gemv_fp8w_mfma_kernel stays
//   48 rows    71.7 / 26.4, 62.8 / 25.5, 19.2 / 24.2, 156.6 / 102.2, 74.4 / 84.7, 181.1 / 116.1: wins two shapes, loses four -- stays
//   64 rows    71.9 / 32.5, 63.3 / 31.6, 19.6 / 28.5, 157.5 / 129.9, 74.9 / 102.6, 181.3 / 147.1: the same
//   128 rows   70.3 / 86.2, 62.1 / 80.4, 24.3 / 67.6, 154.4 / 658.9, 91.3 / 364.0, 176.5 / 807.7 (BM = 64): taken
//   256 rows   69.6 / 81.4, 60.7 / 76.9, 34.6 / 74.2, 153.8 / 655.7, 129.5 / 356.3, 174.7 / 774.8 (BM = 64): taken
//   512 rows   68.5 / 78.1, 64.1 / 78.6, 59.4 / 78.8, 179.0 / 658.1, 202.3 / 355.3, 208.0 / 755.0 (BM = 64): taken
//   1024 rows  70.2 / 78.1, 66.2 / 78.2 (BM = 64), 94.9 / 114.5, 264.4 / 668.8, 316.3 / 491.5, 301.9 / 762.2 (BM = 128): taken
//   2048 rows  85.0 / 78.6, 74.2 / 73.2, 191.1 / 168.9, 523.7 / 703.0, 582.1 / 547.5, 594.2 / 792.6 (the better BM): loses four
//   4096 rows  123.8 / 115.6, 82.9 / 73.8, 399.3 / 280.3, 1051.6 / 1076.5, 1177.5 / 1091.9, 1173.4 / 1263.5: loses four
// So 65 .. 1024 rows take the kernel and more rows dequantise + tamd_gemm, whose 256 x 256 tiles read X once per 256 weight rows
// where this kernel reads it once per 128.  Nothing was measured between 64 and 128 rows (the rule starts where
// gemv_fp8w_mfma_kernel ends) or between 1024 and 2048.  The 1024-row point rests on fp8w_tile_rows choosing BM by N.
constexpr int kFp8TileMaxRows = 1024;
static bool fp8w_use_tile(int64_t m, int64_t ldx) {
  if (m <= kGemvMaxRows || 128 * ldx * 2 >= ((int64_t)1 << 31)) return false;
  const int mode = fp8w_tile_mode();
  if (mode != 1) return mode == 2;
  return m > kFp8MfmaMaxRows && m <= kFp8TileMaxRows;
}

}  // namespace tamd
