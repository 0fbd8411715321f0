// attention_mla_kernel.inc -- the forward attention kernel for multi-head latent attention as the reference's DeepSeek-V2 / -V3
// family hands it to the attention interface (models/deepseek_v3/modeling_deepseek_v3.py DeepseekV3Attention.forward):
//   q, k [.., 192] = 128 "nope" columns + 64 rotary columns,   v, o [.., 128]
// -- a problem whose QK^T depth differs from its PV width, which attn_fwd_kernel<T, D, ..> (one D for Q, K, V and O) cannot
// express.  Included once from attention.hip; entry points tamd_attn_fwd_mla / tamd_attn_decode_mla.
//
// Work split (the product forward's): 128 query rows per workgroup, 4 waves x 32 rows; 64-key tiles, the heaviest causal tiles
// first; K/V-sharing workgroups on one XCD.  SPLIT: the key range is cut into a.kv_splits pieces that leave as normalised fp32
// rows + their log-sum-exp for attn_combine_kernel<T, 128> (the output is 128 wide: the merge kernel is the product's).
//
// QK^T: S^T = K.Q^T on 32x32x16 MFMAs with Q resident as the B operand -- 12 k-steps per 32-key sub-tile, 12 fragments (48
// registers) carrying scale*log2(e) (scale_frag); every S chain starts from -m through srcC, so the softmax numerator is
// exp2(S'') alone, and the O rescale is deferred while no row outgrows its reference maximum by 2^6.
// PV: O^T += V^T.P^T, 4 x 16 accumulators for the 128 value columns; P rounded to T is the B operand as it stands in the S
// registers, V comes through the transposing LDS reads.
//
// LDS: a 384-byte K row does not fit the power-of-two swizzle of TileOffsets<D>, so a K tile is stored as MLA's own two
// panels -- [64][128] (nope) and [64][64] (rotary) -- each in the layout, and fed by the loaders, of the product kernel
// (TileFeed<128> / TileFeed<64>, TileOffsets<128> / <64>); V is one [64][128] panel.  16 + 8 + 16 = 40 KB per stage, two stages:
// 80 KB per workgroup of dynamic LDS and nothing static, so two workgroups fill a CU's 160 KB exactly; the O staging rows
// (4 x 32 x 272 B) reuse stage 0 behind the loop's last barrier.  A tile is 10 LDS-DMA pieces per wave; they go out one by one
// behind the first 10 of the 12 K.Q^T MFMA pairs.
// Registers: two workgroups per CU leave 256 per lane.  The product kernel's D = 128 text needs ~190 beside its fragment
// rings; 16 more for Q, 4 + 2 for the second panel's offsets leave room for rings of 2 K fragments and 2 V fragments ahead
// (the depth of the product's padding-mask instantiations) -- profiles/attn_mla_isa.md has the figures.
//
// Masks: causal with the bottom-right offset (k <= s + seq_k - seq_q, any seq_q <= seq_k); an optional [batch, seq_k] key_valid
// plane, tested per tile on 64 ballot bits -- a wave-uniform run-time branch, NOT a template axis (8 instantiations in all: T x
// CAUSAL x SPLIT) -- so that only tiles holding an invalid key pay for mask arithmetic; ragged ends are cut by the loaders'
// buffer range check.  A row without a visible key: O = 0, lse = +inf.  No dropout, no q_start planes, no key counts in device
// memory, no window (refused by the entry points).
constexpr int kMlaDqk = 192, kMlaDv = 128;
constexpr int kMlaKaB = kKB * 128 * 2;            // K panel A: the 128 nope columns
constexpr int kMlaKbB = kKB * 64 * 2;             // K panel B: the 64 rotary columns
constexpr int kMlaVB = kKB * kMlaDv * 2;          // V
constexpr int kMlaStageB = kMlaKaB + kMlaKbB + kMlaVB;  // 40 KB
constexpr int kMlaSmem = 2 * kMlaStageB;                // 80 KB

template <typename T, bool CAUSAL, bool SPLIT>
__global__ __launch_bounds__(kAttnThreads, 2) void attn_mla_kernel(AttnArgs a) {
  constexpr int KS = kMlaDqk / 16;        // 12 QK^T k-steps: 8 on panel A, 4 on panel B
  constexpr int DT = kMlaDv / 32;         // 4 output d-tiles
  constexpr int VROWB = kMlaDv * 2;
  constexpr int OROWB = VROWB + 16;       // padded staging row
  static_assert(4 * 32 * OROWB <= kMlaStageB, "the O staging rows live in stage 0");
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

  // ---- Q fragments (MFMA B operand): Q[q = qw0 + l31][d = ks*16 + hi*8 .. +7], carrying scale*log2(e)
  const int qw0 = q0 + wave * 32;
  const int qrow = qw0 + l31;
  u32x4 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    qf[ks] = (qrow < a.seq_q) ? ld16(Q + (int64_t)qrow * a.qss + ks * 16 + hi * 8) : u32x4{0, 0, 0, 0};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = scale_frag<T>(qf[ks], a.scale_log2);

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

  TileOffsets<128> toa;  // panel A rows and the V columns (both [64][128])
  TileOffsets<64> tob;   // panel B rows
  toa.init(lane);
  tob.init(lane);
  const unsigned lds0 = lds_base_u32(smem);
  constexpr float kDeferThr = 6.f;  // skip the O rescale while the row max grows by < 2^6

  // K/V tiles: buffer-addressed, range-checked LDS-DMA with loop-invariant lane offsets.  Rows a tile does not have arrive
  // as zeros (masked keys; V rows that multiply p = 0), so every tile takes one path.  Panel B is the same loader on a base
  // moved by 128 columns: its range [0, rows * stride) then ends 256 B behind the last row's start, inside that row.
  TileFeed<128> feeda, feedv;
  TileFeed<64> feedb;
  feeda.init(a.kss, wave, lane);
  feedb.init(a.kss, wave, lane);
  feedv.init(a.vss, wave, lane);
  constexpr int NPA = TileFeed<128>::NI, NPB = TileFeed<64>::NI, NPIECE = 2 * NPA + NPB;  // 4 + 2 + 4 pieces per wave
  auto issue_piece = [&](int t, int rows, int buf, int n) {  // piece n < NPIECE of tile t (`rows` of it exist)
    const unsigned st = (unsigned)buf * kMlaStageB;
    const T* krow = K + (int64_t)t * kKB * a.kss;
    if (n < NPA)
      feeda.issue_one_rng(krow, rows, a.kss, smem, st, wave, n);
    else if (n < NPA + NPB)
      feedb.issue_one_rng(krow + 128, rows, a.kss, smem, st + kMlaKaB, wave, n - NPA);
    else
      feedv.issue_one_rng(V + (int64_t)t * kKB * a.vss, rows, a.vss, smem, st + kMlaKaB + kMlaKbB, wave, n - NPA - NPB);
  };
  auto tile_rows = [&](int t) { return seq_k - t * kKB < kKB ? seq_k - t * kKB : kKB; };  // (a scalar min: stays in SGPRs)
  auto issue = [&](int t, int rows, int buf) {
#pragma unroll
    for (int n = 0; n < NPIECE; ++n) issue_piece(t, rows, buf, n);
  };
  // the key tiles this workgroup visits: [t0, nkt_w) -- all of them, or this split's share
  const int t0 = SPLIT ? split * a.tiles_per_split : 0;
  const int nkt_w = SPLIT ? (nkt < (split + 1) * a.tiles_per_split ? nkt : (split + 1) * a.tiles_per_split) : nkt;
  if (nkt_w > t0) issue(t0, tile_rows(t0), t0 & 1);
  wait_vmcnt0();
  block_sync();

  const bool has_mask = a.key_valid != nullptr;  // (wave-uniform)
  for (int t = t0; t < nkt_w; ++t) {
    const int cur = t & 1;
    // the next tile goes out behind this tile's K.Q^T MFMAs (behind the last tile: nothing to fetch, zeros into the free stage)
    const int tn = t + 1, rows_n = t + 1 < nkt_w ? tile_rows(t + 1) : 0;
    const int kt0 = t * kKB;
    // (Deviation from the product loop: NO wave-uniform skip of a tile that lies above the diagonal for all 32 rows of a wave.
    // With the second path -- the wave's share of the loads issued in a row -- hipcc spilled 57 .. 63 registers of the causal
    // instantiations, Q fragments among them; without it every instantiation is free of scratch.  Such a tile masks to p = 0
    // like a fully padded one.  The waves meet at a barrier per tile, so the skip never shortened the workgroup's tile: at most
    // the block's last tile, for two of its four waves.)
    {
      const unsigned kb = lds0 + (unsigned)cur * kMlaStageB, vb = kb + kMlaKaB + kMlaKbB;
      // ---- S^T tile [64 keys][32 q] = K . Q^T: two 32-key sub-tiles, MFMAs alternate between them; MFMA i = (k-step i >> 1,
      // sub-tile i & 1).  K fragments through a register ring, requested KA MFMAs ahead: untracked reads, counted waits.
      f32x16 s[2] = {neg_m, neg_m};  // S'' = S*scale*log2(e) - m_ref
      {
        constexpr int NM = 2 * KS;  // 24 MFMAs
        constexpr int KA = 2;
        u32x4 kr[KA + 1];
        auto kreq = [&](int i) -> u32x4 {
          const int ks = i >> 1, sub = i & 1;
          return ks < 8 ? lds_read16_abs(kb + toa.row[ks < 8 ? ks : 0], sub * 32 * 256)
                        : lds_read16_abs(kb + tob.row[ks < 8 ? 0 : ks - 8], kMlaKaB + sub * 32 * 128);
        };
#pragma unroll
        for (int i = 0; i < KA; ++i) kr[i] = kreq(i);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
          if (i + KA < NM) kr[(i + KA) % (KA + 1)] = kreq(i + KA);
          constexpr_wait_frag<KA>(NM - 1 - i, kr[i % (KA + 1)]);
          s[i & 1] = mfma32<T>(kr[i % (KA + 1)], qf[i >> 1], s[i & 1]);
          if ((i & 1) && (i >> 1) < NPIECE) issue_piece(tn, rows_n, cur ^ 1, i >> 1);
        }
      }
      // the first VA V fragments are requested now and land under the softmax arithmetic
      constexpr int NV = DT * 4;  // 16 MFMAs
      constexpr int VA = 2;
      u32x4 vr[VA + 1];
      auto vreq = [&](int i) -> u32x4 {  // step i = (key block i / DT, d-tile i % DT): two transposing reads
        const int dt = i % DT, j = i / DT;
        const int rb = ((j >> 1) * 32 + (j & 1) * 16) * VROWB;
        const u32x2 lo = lds_read8_tr16_abs(vb + toa.tr[dt][0], rb);
        const u32x2 h2 = lds_read8_tr16_abs(vb + toa.tr[dt][1], rb);
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
        // bit c of vm.  lim and vm are made here, per tile, and kept opaque: left transparent, the 32 bounds `row + off - c` are
        // loop-invariant and were hoisted into 32 registers that the loop does not have (scratch)
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
      float* dst = a.o_part + prow * kMlaDv;
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
  // (every wave is behind the loop's last barrier and its own vmcnt(0): nothing reads or lands in stage 0 any more)
  T* O = reinterpret_cast<T*>(a.o) + (int64_t)b * a.osb + (int64_t)h * a.osh;
  store_rows_via_lds<T, kMlaDv>(oacc, inv_l, smem, (unsigned)wave * (32u * OROWB), O, a.oss, qw0, a.seq_q, lane);
}
