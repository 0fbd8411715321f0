// attention_d256_kernel.inc -- the forward attention kernel for heads of 256 (every Gemma-1 size, CodeGemma, PaliGemma's
// language model, Gemma-2 2B / 9B, Gemma-3 1B / 4B / 12B): q, k, v, o rows of 256.  Included once from attention.hip; reached
// through tamd_attn_fwd / tamd_attn_decode with head_dim == 256.  Inference only: no backward, no dropout, no q_start planes, no
// key counts in device memory, no window (refused by the entry points).
//
// Why not attn_fwd_kernel<T, 256, ..>: that text holds Q in VGPRs beside its accumulators and runs two or three workgroups per
// CU.  At D = 256 one lane carries (arithmetic, 32-bit registers)
//     O accumulators   8 d-tiles x 16            = 128
//     Q fragments      16 k-steps x 4 (scaled)   =  64
//     S'' of one tile  2 sub-tiles x 16          =  32
//     -m_ref tuple (srcC of every S chain)       =  16
//     P as B operands  4 x 4                     =  16   (dead while S is being produced: shares nothing with it, though)
//     K / V fragment ring  (KA + 1) x 4          =  16
//     LDS offsets 8 + 8, DMA offsets 4 + 4       =  24
//     row state, bounds, addresses               ~  12        -> ~ 308 > 256,
// and a double-buffered stage of a 64-key K tile (32 KB) and V tile (32 KB) is 128 KB of the CU's 160 KB.  Both budgets say: ONE
// workgroup per CU, one wave per SIMD, 512 registers per lane -- the regime of attn_bwd_dkdv_kernel
// (__launch_bounds__(kAttnThreads, 1)).  This translation unit is compiled with the MFMA results in arch VGPRs (build.py: the
// softmax reads every S element with VALU instructions), so the split of the 512 is the dK/dV kernel's: the accumulators (O, S)
// stay in VGPRs and the RESIDENT operand -- the 64 registers of scaled Q fragments, read by MFMAs alone -- lives in AGPRs
// (scale_frag<T, true>).  ~244 VGPRs + 64 AGPRs; profiles/attn_d256_isa.md has what the compiler made of it.
//
// Work split (the product forward's): 128 query rows per workgroup, 4 waves x 32 rows; 64-key tiles, the heaviest causal tiles
// first; K/V-sharing workgroups on one XCD.  SPLIT: the key range is cut into a.kv_splits pieces that leave as normalised fp32
// rows + their log-sum-exp for attn_combine_kernel<T, 256>.
//
// LDS map (dynamic, 128 KB; nothing static):  stage s at s * 64 KB =  K[:, 0:128] | K[:, 128:256] | V[:, 0:128] | V[:, 128:256],
// four [64][128] panels of 16 KB.  A 512-byte row has no conflict-free row_swz: a row is stored as two 256-byte half rows in
// the product's D = 128 layout (TileOffsets<128>, TileFeed<128>), which is conflict-free for the ds_read_b128 row fragments
// and the transposing reads alike.  A tile is 16 LDS-DMA pieces per wave (4 per panel).  The O staging rows (4 x 32 x 528 B =
// 66 KB) lie over stage 0 and the head of stage 1 behind the loop's last barrier.
//
// Tile loop.  No second wave hides latency on a SIMD here, so the loop places its own traffic between the MFMAs:
//   K.Q^T   32 MFMAs (16 k-steps x 2 sub-tiles, alternating accumulators); K fragments through a ring requested KA MFMAs ahead
//           (untracked reads, counted waits); one LDS-DMA piece of the NEXT tile behind each MFMA pair: 16 pairs, 16 pieces;
//   softmax the product's: S'' leaves the matrix pipe as S*scale*log2(e) - m_ref (Q carries the scale, the chain starts from -m
//           through srcC), p = exp2(S''), the O rescale deferred while no row outgrows m_ref by 2^6; the first VA V fragments are
//           requested in front of it and land under it;
//   P.V     32 MFMAs (4 key blocks x 8 d-tiles, consecutive MFMAs on different accumulators), V through the same ring.
// 64 MFMAs of 32x32x16 per tile and wave against the softmax VALU work of D = 128 (which has 32): the loop is expected to sit
// closer to the matrix pipe's rate than the product forward.  DESIGN.md has what was measured.
//
// Masks: causal with the bottom-right offset (k <= s + seq_k - seq_q, any seq_q <= seq_k); an optional [batch, seq_k] key_valid
// plane, tested per tile on 64 ballot bits -- a wave-uniform run-time branch, not a template axis (8 instantiations: T x CAUSAL x
// SPLIT); ragged ends are cut by the loaders' buffer range check.  A row without a visible key: O = 0, lse = +inf.  As in the MLA
// kernel there is no wave-level skip of a tile above the diagonal (it masks to p = 0): the waves meet at a barrier per tile.
constexpr int kD256 = 256;
constexpr int kD256PanelB = kKB * 128 * 2;      // one [64][128] panel: 16 KB
constexpr int kD256StageB = 4 * kD256PanelB;    // K lo | K hi | V lo | V hi: 64 KB
constexpr int kD256Smem = 2 * kD256StageB;      // 128 KB

template <typename T, bool CAUSAL, bool SPLIT>
__global__ __launch_bounds__(kAttnThreads, 1) void attn_d256_kernel(AttnArgs a) {
  constexpr int KS = kD256 / 16;          // 16 QK^T k-steps: 8 per K panel
  constexpr int DT = kD256 / 32;          // 8 output d-tiles: 4 per V panel
  constexpr int PROWB = 128 * 2;          // a panel row
  constexpr int OROWB = kD256 * 2 + 16;   // padded staging row
  static_assert(4 * 32 * OROWB <= kD256Smem, "the O staging rows live in the two stages");
  TAMD_DYN_SMEM(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = wave_id_uniform();
  const int hi = lane >> 5, l31 = lane & 31;

  // ---- work decode: (b, h, query tile); heavy (late) causal tiles first, K/V-sharing blocks on one XCD
  const int group = a.heads_q / a.heads_kv;
  int b, h, qt;
  const int split = SPLIT ? (int)(blockIdx.x % (unsigned)a.kv_splits) : 0;
  {
    const int bid = SPLIT ? (int)(blockIdx.x / (unsigned)a.kv_splits) : (int)blockIdx.x;
    const int per_grp = a.nqt * group;
    int g, within;
    if (a.xcd_map) {
      const int xcd = bid & 7, j = bid >> 3;
      g = (j / per_grp) * 8 + xcd;
      within = j % per_grp;
    } else {
      g = bid / per_grp;
      within = bid % per_grp;
    }
    b = g / a.heads_kv;
    const int hkv0 = g % a.heads_kv;
    h = hkv0 * group + within % group;
    qt = a.nqt - 1 - within / group;
  }
  const int hkv = h / group;
  const int q0 = qt * kQB;
  const int seq_k = a.seq_k;
  const int off = seq_k - a.seq_q;  // causal: key k visible to query s iff k <= s + off
  const T* Q = reinterpret_cast<const T*>(a.q) + (int64_t)b * a.qsb + (int64_t)h * a.qsh;
  const T* K = reinterpret_cast<const T*>(a.k) + (int64_t)b * a.ksb + (int64_t)hkv * a.ksh;
  const T* V = reinterpret_cast<const T*>(a.v) + (int64_t)b * a.vsb + (int64_t)hkv * a.vsh;

  // ---- Q fragments (MFMA B operand): Q[q = qw0 + l31][d = ks*16 + hi*8 .. +7], carrying scale*log2(e); resident in AGPRs
  const int qw0 = q0 + wave * 32;
  const int qrow = qw0 + l31;
  u32x4 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    qf[ks] = scale_frag<T, true>((qrow < a.seq_q) ? ld16(Q + (int64_t)qrow * a.qss + ks * 16 + hi * 8) : u32x4{0, 0, 0, 0},
                                 a.scale_log2);

  f32x16 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;  // running max (log2 domain, scaled) and row sum of this lane's key half
  f32x16 neg_m = splat16(0.f);           // -m_ref: the srcC tuple of the first K.Q^T MFMA of each sub-tile

  int kend = seq_k;
  if (CAUSAL) {
    const int lim = q0 + kQB - 1 + off + 1;  // keys visible to the last query row of the block
    kend = lim < kend ? lim : kend;
    if (kend < 0) kend = 0;
  }
  const int nkt = (kend + kKB - 1) / kKB;

  TileOffsets<128> to;  // the rows of either K panel and the columns of either V panel
  to.init(lane);
  const unsigned lds0 = lds_base_u32(smem);
  constexpr float kDeferThr = 6.f;  // skip the O rescale while the row max grows by < 2^6

  // K/V tiles: buffer-addressed, range-checked LDS-DMA with loop-invariant lane offsets.  Rows a tile does not have arrive as
  // zeros (masked keys; V rows that multiply p = 0), so every tile takes one path.  The high panel is the same loader on a base
  // moved by 128 columns: its range [0, rows * stride) then ends 256 B behind the last row's start, inside that row.
  TileFeed<128> feedk, feedv;
  feedk.init(a.kss, wave, lane);
  feedv.init(a.vss, wave, lane);
  constexpr int NP = TileFeed<128>::NI, NPIECE = 4 * NP;  // 4 pieces per panel and wave, 16 per tile
  auto issue_piece = [&](int t, int rows, int buf, int n) {  // piece n < NPIECE of tile t (`rows` of it exist)
    const int panel = n / NP;                                // 0, 1: K lo / hi; 2, 3: V lo / hi
    const unsigned st = (unsigned)buf * kD256StageB + (unsigned)panel * kD256PanelB;
    if (panel < 2)
      feedk.issue_one_rng(K + (int64_t)t * kKB * a.kss + (panel & 1) * 128, rows, a.kss, smem, st, wave, n % NP);
    else
      feedv.issue_one_rng(V + (int64_t)t * kKB * a.vss + (panel & 1) * 128, rows, a.vss, smem, st, wave, n % NP);
  };
  auto tile_rows = [&](int t) { return seq_k - t * kKB < kKB ? seq_k - t * kKB : kKB; };  // (a scalar min: stays in SGPRs)
  // the key tiles this workgroup visits: [t0, nkt_w) -- all of them, or this split's share
  const int t0 = SPLIT ? split * a.tiles_per_split : 0;
  const int nkt_w = SPLIT ? (nkt < (split + 1) * a.tiles_per_split ? nkt : (split + 1) * a.tiles_per_split) : nkt;
  if (nkt_w > t0) {
#pragma unroll
    for (int n = 0; n < NPIECE; ++n) issue_piece(t0, tile_rows(t0), t0 & 1, n);
  }
  wait_vmcnt0();
  block_sync();

  const bool has_mask = a.key_valid != nullptr;  // (wave-uniform)
  for (int t = t0; t < nkt_w; ++t) {
    const int cur = t & 1;
    // the next tile goes out behind this tile's K.Q^T MFMAs (behind the last tile: nothing to fetch, zeros into the free stage)
    const int tn = t + 1, rows_n = t + 1 < nkt_w ? tile_rows(t + 1) : 0;
    const int kt0 = t * kKB;
    const unsigned kb = lds0 + (unsigned)cur * kD256StageB, vb = kb + 2 * kD256PanelB;
    // ---- S^T tile [64 keys][32 q] = K . Q^T: two 32-key sub-tiles, MFMAs alternate between them; MFMA i = (k-step i >> 1,
    // sub-tile i & 1).  K fragments through a register ring, requested KA MFMAs ahead: untracked reads, counted waits.
    f32x16 s[2] = {neg_m, neg_m};  // S'' = S*scale*log2(e) - m_ref
    {
      constexpr int NM = 2 * KS;  // 32 MFMAs
      constexpr int KA = 3;
      u32x4 kr[KA + 1];
      auto kreq = [&](int i) -> u32x4 {
        const int ks = i >> 1, sub = i & 1;
        return lds_read16_abs(kb + to.row[ks & 7], (ks >> 3) * kD256PanelB + sub * 32 * PROWB);
      };
#pragma unroll
      for (int i = 0; i < KA; ++i) kr[i] = kreq(i);
#pragma unroll
      for (int i = 0; i < NM; ++i) {
        if (i + KA < NM) kr[(i + KA) % (KA + 1)] = kreq(i + KA);
        constexpr_wait_frag<KA>(NM - 1 - i, kr[i % (KA + 1)]);
        s[i & 1] = mfma32<T>(kr[i % (KA + 1)], qf[i >> 1], s[i & 1]);
        if (i & 1) issue_piece(tn, rows_n, cur ^ 1, i >> 1);  // 16 pairs, 16 pieces
      }
    }
    // the first VA V fragments are requested now and land under the softmax arithmetic
    constexpr int NV = DT * 4;  // 32 MFMAs
    constexpr int VA = 3;
    u32x4 vr[VA + 1];
    auto vreq = [&](int i) -> u32x4 {  // step i = (key block i / DT, d-tile i % DT): two transposing reads
      const int dt = i % DT, j = i / DT;
      const int rb = (dt >> 2) * kD256PanelB + ((j >> 1) * 32 + (j & 1) * 16) * PROWB;
      const u32x2 lo = lds_read8_tr16_abs(vb + to.tr[dt & 3][0], rb);
      const u32x2 h2 = lds_read8_tr16_abs(vb + to.tr[dt & 3][1], rb);
      return u32x4{lo[0], lo[1], h2[0], h2[1]};
    };
#pragma unroll
    for (int i = 0; i < VA; ++i) vr[i] = vreq(i);
    // ---- mask (diagonal / ragged / padded tiles only: wave-uniform branches, the common tile has no mask code)
    unsigned long long vmask = ~0ull;
    if (has_mask) {
      const int kp = kt0 + lane;
      vmask = ballot64(kp < seq_k && a.key_valid[(int64_t)b * a.seq_k + kp] != 0);
    }
    const bool need_mask = (vmask != ~0ull) || (kt0 + kKB > seq_k) || (CAUSAL && (kt0 + kKB - 1 > qw0 + off));
    if (need_mask) {
      // element (sub, r) is key kl = c + 4*hi of the tile, c = sub*32 + (r&3) + 8*(r>>2) a constant: visible iff c <= lim and
      // bit c of vm.  lim and vm are made here, per tile, and kept opaque (left transparent, the 32 bounds are hoisted out of
      // the loop into 32 registers)
      int last = seq_k - 1;
      if (CAUSAL) last = qrow + off < last ? qrow + off : last;
      const int lim = opaque_vgpr_i32(last - kt0 - 4 * hi);
      const unsigned long long vm = vmask >> (4 * hi);
      const int vm_lo = opaque_vgpr_i32((int)(unsigned)vm), vm_hi = opaque_vgpr_i32((int)(unsigned)(vm >> 32));
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = (r & 3) + 8 * (r >> 2);
          const bool vis = (sub * 32 + c <= lim) && ((((unsigned)(sub ? vm_hi : vm_lo)) >> c) & 1u);
          s[sub][r] = vis ? s[sub][r] : -INFINITY;
        }
    }
    // ---- online softmax in the exp2 domain: p = exp2(S''), S'' = s*c - m_ref from the MFMAs
    float mx = s[0][0];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[sub][r]);
    mx = fmaxf(mx, swap32_f32(mx));  // the other half-wave holds the other 32 keys of this query
    const float m_old = (m_run == -INFINITY) ? 0.f : m_run;  // the m_ref this tile's S'' refers to
    const float m_tile = mx + m_old;
    if (ballot64(m_tile - m_run > kDeferThr) != 0ull) {  // deferred rescale
      const float m_new = fmaxf(m_run, m_tile);
      const float alpha = (m_new == -INFINITY) ? 1.f : fast_exp2(m_run - m_new);  // m_run = -inf -> 0
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
      // this tile's S'' move to the new reference (row fully masked so far: m_ref stays 0, every p is exp2(-inf) = 0)
      const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
      const float shift = m_ref - m_old;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[sub][r] -= shift;
      neg_m = splat16(-m_ref);
    }
    float psum = 0.f;
    u32x4 pf[4];  // P^T as MFMA B operand: step j covers registers 8*(j&1).. of sub-tile j>>1
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // the reference rounds the probabilities to the storage dtype before P.V; the row sum takes the fp32 values
        p[r] = fast_exp2(s[sub][r]);
        psum += p[r];
      }
      pack_c_to_b<T>(p, &pf[sub * 2]);
    }
    l_run += psum;
    // ---- O^T[d][q] += V^T[d][key] . P^T[key][q]
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (i + VA < NV) vr[(i + VA) % (VA + 1)] = vreq(i + VA);
      constexpr_wait_frag<2 * VA>(2 * (NV - 1 - i), vr[i % (VA + 1)]);
      oacc[i % DT] = mfma32<T>(vr[i % (VA + 1)], pf[i / DT], oacc[i % DT]);  // consecutive MFMAs: different accumulators
    }
    wait_vmcnt0();
    block_sync();
  }

  // ---- finalise: l over both half-waves, normalise, LSE, stage O through LDS, row-wise stores
  l_run += swap32_f32(l_run);
  const float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
  if (SPLIT) {  // this piece's rows, normalised by its own row sums, and their log-sum-exp (-inf: the piece saw no visible key)
    if (qrow < a.seq_q) {
      const int64_t prow = (((int64_t)split * a.batch + b) * a.seq_q + qrow) * a.heads_q + h;
      if (hi == 0)
        a.lse_part[(((int64_t)split * a.batch + b) * a.heads_q + h) * a.seq_q + qrow] =
            (l_run > 0.f) ? (m_run + fast_log2(l_run)) * 0.69314718055994530942f : -INFINITY;
      float* dst = a.o_part + prow * kD256;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
          st16(dst + dt * 32 + 8 * qd + 4 * hi,
               u32x4{f32_as_u32(oacc[dt][qd * 4 + 0] * inv_l), f32_as_u32(oacc[dt][qd * 4 + 1] * inv_l),
                     f32_as_u32(oacc[dt][qd * 4 + 2] * inv_l), f32_as_u32(oacc[dt][qd * 4 + 3] * inv_l)});
    }
    return;
  }
  if (a.lse != nullptr && hi == 0 && qrow < a.seq_q) {
    const float lse = (l_run > 0.f) ? (m_run + fast_log2(l_run)) * 0.69314718055994530942f : INFINITY;
    a.lse[((int64_t)b * a.heads_q + h) * a.seq_q + qrow] = lse;
  }
  // (every wave is behind the loop's last barrier and its own vmcnt(0): nothing reads or lands in either stage any more)
  T* O = reinterpret_cast<T*>(a.o) + (int64_t)b * a.osb + (int64_t)h * a.osh;
  store_rows_via_lds<T, kD256>(oacc, inv_l, smem, (unsigned)wave * (32u * OROWB), O, a.oss, qw0, a.seq_q, lane);
}
