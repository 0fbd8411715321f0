// attention_fwd_kernel.inc -- the forward attention kernel (structure: header of attention.hip; included there once).
// (Round 2 also instantiated this text with two query tiles per workgroup -- heaviest causal tile, then lightest -- and
// built a 64-rows-per-wave kernel next to it: bit-identical, 958 and 622 against 961 TFLOP/s on MI355X,
// profiles/r03a_attn_fwd_ab.jsonl; both were removed.  Round 3 then ran this loop with 8 waves per workgroup -- 256 query
// rows, one workgroup per CU, a 4-deep K/V ring requested three tiles ahead, so that the issue / wait / barrier share of
// the phase trace (770 of 3611 cycles per tile) would go -- bit-identical, and 1.14 vs 1.12 ms causal, level bidirectional,
// slower on short prompts (profiles/r03d_attn_fwd8_ab.jsonl, code in r03d_attn_8wave.patch): with two workgroups per CU
// the other workgroup already fills those gaps.)
// SPLIT (tamd_attn_decode): the key range is cut into a.kv_splits pieces, one workgroup each; a piece leaves as normalised
// fp32 rows + their log-sum-exp (a.o_part / a.lse_part) for attn_combine_kernel instead of as O / LSE.
// DEVLEN (SPLIT only; a.seq_k_dev): the number of keys of a batch row comes from device memory (a pre-allocated KV cache): every
// piece of geometry below uses that count, so the tiles behind it are neither loaded nor visited and the pieces that own them
// leave as "saw no key".  (A template argument, not a test of the pointer inside the SPLIT kernels: with the test there the
// calls WITHOUT counts ran 0.4 us slower at every shape and 1.4 us at 8 query rows x 4096 keys, 23.5 against 22.1 -- the same
// loop, another order of the prologue's scalar loads; as it is they run the code they ran before.)
// WINDOW (tamd_attn_fwd_window / tamd_attn_decode_window; a.window): a causal sliding window over a KV cache -- query row s sees
// the keys max(0, s + off - W + 1) .. s + off.  The lower bound takes the place of the packed-sequence plane: computed from the
// row index, no plane read; it does not decrease along the rows, so the wave-uniform bounds are those of the wave's first and
// last live row, and the block's first tile that of its first row.  Everything behind that is the machinery the planes use.
// Without CAUSAL (SPLIT only: one query row, its heads re-strided into the rows of the tile) every row stands at the last key.
// (A template argument for the reason DEVLEN is one: the instantiations without it are the code they were,
// profiles/attn_window_isa.md.)
template <typename T, int D, bool CAUSAL, bool HAS_MASK, bool DROP, bool SPLIT = false, bool DEVLEN = false, bool WINDOW = false>
// (two workgroups per CU where the registers allow it: the dropout variants at D = 128 need more than 256)
// (three at head_dim 64 without padding mask / dropout -- CLIP: the kernel sat at 155 registers before the resident -m tuple)
__global__ __launch_bounds__(kAttnThreads, (DROP && D > 64) ? 1 : ((D == 64 && !HAS_MASK && !DROP) ? 3 : 2)) void attn_fwd_kernel(AttnArgs a) {
  constexpr int ROWB = D * 2;
  constexpr int TILEB = kKB * ROWB;       // one K or V tile
  constexpr int KS = D / 16;              // QK^T k-steps
  constexpr int DT = D / 32;              // output d-tiles
  constexpr int OROWB = ROWB + 16;        // padded staging row
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
    const int hkv = g % a.heads_kv;
    h = hkv * group + within % group;
    qt = a.nqt - 1 - within / group;
  }
  const int hkv = h / group;
  const int q0 = qt * kQB;
  // the keys of this batch row: all of them, or (DEVLEN) the count in device memory, clamped to the allocation.  b is
  // workgroup-uniform: one load, made wave-uniform before anything is derived from it, and two scalar selects (see tile_rows)
  static_assert(!DEVLEN || SPLIT, "key counts in device memory: the split-KV instantiations only");
  int seq_k = a.seq_k;
  if constexpr (SPLIT && DEVLEN) {
    int n = wave_uniform_i32(a.seq_k_dev[b]);
    n = n < a.seq_k ? n : a.seq_k;
    seq_k = n > 0 ? n : 0;
  }
  const int off = seq_k - a.seq_q;  // causal: key k visible to query s iff k <= s + off
  const T* Q = reinterpret_cast<const T*>(a.q) + (int64_t)b * a.qsb + (int64_t)h * a.qsh;
  const T* K = reinterpret_cast<const T*>(a.k) + (int64_t)b * a.ksb + (int64_t)hkv * a.ksh;
  const T* V = reinterpret_cast<const T*>(a.v) + (int64_t)b * a.vsb + (int64_t)hkv * a.vsh;

  // ---- Q fragments (MFMA B operand): Q[q = qw0 + l31][d = ks*16 + hi*8 .. +7]
  const int qw0 = q0 + wave * 32;
  const int qrow = qw0 + l31;
  u32x4 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    qf[ks] = (qrow < a.seq_q) ? ld16(Q + (int64_t)qrow * a.qss + ks * 16 + hi * 8) : u32x4{0, 0, 0, 0};
  // Q carries scale*log2(e), rounded once more to the storage dtype (attention_common.h scale_frag): S leaves the MFMAs
  // in the exp2 domain, and because every S chain STARTS from -m (neg_m below) the softmax numerator is exp2(S'') alone
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = scale_frag<T>(qf[ks], a.scale_log2, !a.q_prescaled);

  // packed sequences: this query's first visible key; wave-uniform bounds for tile skipping / mask-free tiles
  static_assert(!WINDOW || (!DROP && !DEVLEN), "the window instantiations: inference, key counts from the host");
  int klo, klo_max, klo_min;
  if constexpr (WINDOW) {
    // ... a sliding window: the bound follows from the row's position among the keys -- row + off under the causal mask, the
    // last key's for every row without it (one query row whose heads became the rows of the tile: attention.hip decode_plan).
    // Scalars for a wave's first and last live row
    const int last = qw0 + 31 < a.seq_q ? qw0 + 31 : a.seq_q - 1;
    klo_min = window_klo(a, CAUSAL ? qw0 + off : seq_k - 1);
    klo_max = window_klo(a, CAUSAL ? last + off : seq_k - 1);
    klo = CAUSAL ? window_klo(a, qrow + off) : klo_min;  // (without the causal mask: one bound for all rows)
    // the lane's bound is ONE register from here on, as the plane's value is in the other instantiations (left transparent, the
    // mask arithmetic of the 32 elements was rewritten around row + off - W and hoisted out of the tile loop: scratch,
    // profiles/attn_window_isa.md)
    if constexpr (CAUSAL) klo = opaque_vgpr_i32(klo);
  } else {
    klo = packed_klo(a, b, qrow);
    klo_max = (int)wave_max((float)klo), klo_min = -(int)wave_max(-(float)klo);
  }

  f32x16 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;  // running max (log2 domain, scaled) and row sum of this lane's key half
  // -m_ref as 16 equal registers: the srcC tuple of the first K.Q^T MFMA of each sub-tile (m_ref: the running maximum the
  // exponentials refer to, 0 while the row has seen no visible key); rewritten only when the deferred rescale fires
  f32x16 neg_m = splat16(0.f);

  int kend = seq_k;
  if (CAUSAL) {
    const int lim = q0 + kQB - 1 + off + 1;  // keys visible to the last query row of the block
    kend = lim < kend ? lim : kend;
    if (kend < 0) kend = 0;
  }
  const int nkt = (kend + kKB - 1) / kKB;

  TileOffsets<D> toff;
  toff.init(lane);
  const unsigned lds0 = lds_base_u32(smem);
  const AttnDrop drop = attn_drop_ctx(a);
  const unsigned long long drop_base = drop.row_base((unsigned long long)b * a.heads_q + h, (qrow >> 1) <= ((a.seq_q - 1) >> 1) ? qrow : 0);  // (the row PAIR exists: both of its lanes hash for it)
  const unsigned drop_lsh = (qrow & 1) ? 0u : 16u;  // this lane's query row: the high or the low half of each word (dropout.h)
  constexpr float kDeferThr = 6.f;  // skip the O rescale while the row max grows by < 2^6 (cdna guide T13)

  // K/V tiles: buffer-addressed, range-checked LDS-DMA with loop-invariant lane offsets (TileFeed).  The rows a tile does not
  // have -- the ragged end of the key range, or the whole tile behind the last one -- are cut off by the buffer's size and
  // arrive as zeros (what the zero page of the general loader delivered: masked keys, V rows that multiply p = 0), so every
  // tile takes ONE path and the pieces of the next tile go out unconditionally, one by one behind the K.Q^T MFMAs (an LDS-DMA
  // instruction holds its wave for ~90 cycles: 720 per tile when the eight were issued in a row; behind an MFMA the matrix
  // pipe works through that time).  (Rounds 2-4 kept a second, general loader for ragged tiles and tested `next tile is a
  // full one` behind every MFMA pair: eight wave-uniform branches per tile and the spilled lane offsets of the cold path.)
  TileFeed<D> feed, feedv;
  feed.init(a.kss, wave, lane);
  feedv.init(a.vss, wave, lane);
  auto issue_piece = [&](int t, int rows, int buf, int n) {  // piece n < 2 * NI of tile t (`rows` of it exist): K pieces, then V pieces
    constexpr int NI = TileFeed<D>::NI;
    const unsigned k_off = (unsigned)buf * 2u * TILEB, v_off = k_off + TILEB;
    if (n < NI)
      feed.issue_one_rng(K + (int64_t)t * kKB * a.kss, rows, a.kss, smem, k_off, wave, n);
    else
      feedv.issue_one_rng(V + (int64_t)t * kKB * a.vss, rows, a.vss, smem, v_off, wave, n - NI);
  };
  // rows of tile t < ceil(seq_k / 64) (a scalar min, never a two-sided clamp: hipcc makes that a v_med3_i32 -- a VGPR -- and the
  // buffer descriptor built from it a waterfall loop per piece)
  auto tile_rows = [&](int t) { return seq_k - t * kKB < kKB ? seq_k - t * kKB : kKB; };
  auto issue = [&](int t, int rows, int buf) {
#pragma unroll
    for (int n = 0; n < 2 * TileFeed<D>::NI; ++n) issue_piece(t, rows, buf, n);
  };
  // packed sequences: q_start is non-decreasing along a row, so no row of this block sees a key before the first
  // visible key of its first row: whole K/V tiles below it are neither loaded nor visited (buffers alternate from t0)
  // (a sliding window: the same, with the bound of the block's first row)
  const int t0f = (WINDOW ? window_klo(a, CAUSAL ? q0 + off : seq_k - 1) : (q0 < a.seq_q ? packed_klo(a, b, q0) : 0)) / kKB;
  // the key tiles this workgroup visits: [t0, nkt_w) -- all of them, or this split's share
  const int t0 = SPLIT ? (t0f > split * a.tiles_per_split ? t0f : split * a.tiles_per_split) : t0f;
  const int nkt_w = SPLIT ? (nkt < (split + 1) * a.tiles_per_split ? nkt : (split + 1) * a.tiles_per_split) : nkt;
  if (nkt_w > t0) issue(t0, tile_rows(t0), t0 & 1);
  wait_vmcnt0();
  block_sync();

#ifdef TAMD_DIAG
  const bool tr = a.trace != nullptr && blockIdx.x == 0;
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = tr ? device_clock() : 0ull;
#endif
  for (int t = t0; t < nkt_w; ++t) {
    const int cur = t & 1;
    // the next tile goes out behind this tile's K.Q^T MFMAs (behind the last tile: nothing to fetch, zeros into the free buffer)
    const int tn = t + 1, rows_n = t + 1 < nkt_w ? tile_rows(t + 1) : 0;
    TAMD_ATTN_PHASE(0)
    const unsigned k_off = (unsigned)cur * 2u * TILEB, v_off = k_off + TILEB;
    const int kt0 = t * kKB;
    // wave-uniform skip: every key of the tile is above the diagonal for all 32 rows of this wave
    // (packed: ... or below the first visible key of all 32 rows)
    const bool wave_active = (!CAUSAL || (kt0 <= qw0 + 31 + off)) && (kt0 + kKB > klo_min);
    if (wave_active) {
      // ---- S^T tile [64 keys][32 q] = K . Q^T   (two 32-key sub-tiles, MFMAs alternate between them)
      // K fragments through a 5-deep register ring, requested four MFMAs ahead: every read of the loop is issued
      // untracked (the compiler would put vmcnt(0) -- the next tile's LDS-DMA -- in front of the transposing V reads and
      // serialise each K read with its MFMA) and waited for with a counted lgkmcnt tied to the fragment register.
      const unsigned kb = lds0 + k_off, vb = lds0 + v_off;
      f32x16 s[2] = {neg_m, neg_m};  // S'' = S*scale*log2(e) - m_ref
      {
        constexpr int NM = 2 * KS;                 // MFMAs
        constexpr int KA = (DROP || (HAS_MASK && D > 64)) ? 2 : (NM < 8 ? NM : 8);  // K fragments requested ahead (LDS latency under load: several MFMAs)
        u32x4 kr[KA + 1];
#pragma unroll
        for (int i = 0; i < KA; ++i) kr[i] = lds_read16_abs(kb + toff.row[i >> 1], (i & 1) * 32 * ROWB);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
          if (i + KA < NM) kr[(i + KA) % (KA + 1)] = lds_read16_abs(kb + toff.row[(i + KA) >> 1], ((i + KA) & 1) * 32 * ROWB);
          // one counted wait per TWO MFMAs (a wait is an issue slot; the loop is bound by them): behind the pair's second
          // fragment at most KA - 1 requests stay outstanding
          if (KA >= 3) {
            if (!(i & 1)) constexpr_wait_frag2<KA - 1>(NM - 2 - i, kr[i % (KA + 1)], kr[(i + 1) % (KA + 1)]);
          } else {
            constexpr_wait_frag<KA>(NM - 1 - i, kr[i % (KA + 1)]);
          }
          s[i & 1] = mfma32<T>(kr[i % (KA + 1)], qf[i >> 1], s[i & 1]);
          if ((i & 1) && (i >> 1) < 2 * TileFeed<D>::NI) issue_piece(tn, rows_n, cur ^ 1, i >> 1);
        }
      }
      TAMD_ATTN_PHASE(1)
      // the first VA V fragments are requested now and land under the softmax arithmetic; P.V requests the others VA
      // steps ahead (LDS latency under load -- two workgroups' reads and the tile loads -- is several MFMAs)
      constexpr int NV = DT * 4;
      constexpr int VA = (DROP || (HAS_MASK && D > 64)) ? 2 : (NV < 7 ? NV : 7);  // (no registers to spare in the dropout / padding-mask variants)
      u32x4 vr[VA + 1];
      auto vreq = [&](int i) -> u32x4 {  // step i = (key block i / DT, d-tile i % DT): two transposing reads
        const int dt = i % DT, j = i / DT;
        const int rb = ((j >> 1) * 32 + (j & 1) * 16) * ROWB;
        const u32x2 lo = lds_read8_tr16_abs(vb + toff.tr[dt][0], rb);
        const u32x2 h2 = lds_read8_tr16_abs(vb + toff.tr[dt][1], rb);
        return u32x4{lo[0], lo[1], h2[0], h2[1]};
      };
#pragma unroll
      for (int i = 0; i < VA; ++i) vr[i] = vreq(i);
      // ---- mask (diagonal / ragged / padded tiles only: wave-uniform branch, the common tile has no mask code)
      // (a padding mask: the tile's 64 validity bits first -- a batch is padded at one end, most of its tiles have every key
      // valid and take the path without mask code; until round 5 HAS_MASK meant the mask arithmetic, 5 instructions per
      // element, on every tile: the padded Llama-3-8B shape ran 1.54 ms against 1.01 without a mask)
      unsigned long long vmask = ~0ull;
      if (HAS_MASK) {
        const int kp = kt0 + lane;
        vmask = ballot64(kp < seq_k && (a.key_valid == nullptr || a.key_valid[(int64_t)b * a.seq_k + kp] != 0));  // (rows of the plane: the allocation)
      }
      const bool need_mask = (HAS_MASK && vmask != ~0ull) || (kt0 + kKB > seq_k) || (CAUSAL && (kt0 + kKB - 1 > qw0 + off)) ||
                             (kt0 < klo_max);
      if (need_mask) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kl = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;  // key index inside the tile
            const int kp = kt0 + kl;
            bool vis = kp < seq_k && kp >= klo;
            if (CAUSAL) vis = vis && (kp <= qrow + off);
            if (HAS_MASK) vis = vis && ((vmask >> kl) & 1ull);
            s[sub][r] = vis ? s[sub][r] : -INFINITY;
          }
      }
      // ---- online softmax in the exp2 domain: p = exp2(S''), S'' = s*c - m_ref from the MFMAs (c = scale*log2(e) > 0)
      float mx = s[0][0];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[sub][r]);
      mx = fmaxf(mx, swap32_f32(mx));  // the other half-wave holds the other 32 keys of this query
      const float m_old = (m_run == -INFINITY) ? 0.f : m_run;  // the m_ref this tile's S'' refers to
      const float m_tile = mx + m_old;
      // deferred rescale: keep the old reference max while no row of the wave outgrows it by 2^thr
      if (ballot64(m_tile - m_run > kDeferThr) != 0ull) {
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
          // the reference rounds softmax probabilities to the storage dtype before P.V; the row sum uses the
          // unrounded fp32 values like softmax(dtype=float32) does.
          p[r] = fast_exp2(s[sub][r]);
          psum += p[r];
        }
        if (DROP) {  // dropout acts on the probabilities that multiply V, not on the normaliser (softmax, then dropout);
                     // the keep-scale 1 / (1 - p) multiplies the finished row (inv_l below), not every element
          // registers r, r + 1 are keys 2j, 2j + 1: one hash, the two words.  The hash block is 2 x 2 -- this query row and its
          // neighbour (lane ^ 1) need the same 64 bits -- so the pair shares the work (round 6): of the blocks at registers 4i and
          // 4i + 2 (key pairs p and p + 1) the even row's lane hashes the first, the odd row's lane the second, and each word
          // reaches both lanes through a DPP move (pair_even_u32 / pair_odd_u32): 8 hashes of ~17 issue slots per tile and lane
          // instead of 16, in a loop that is bound by instruction issue.
#pragma unroll
          for (int r = 0; r < 16; r += 4) {
            unsigned w0, w1;
            drop.words(drop_base + (unsigned long long)(((kt0 + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) >> 1) + (qrow & 1)), w0, w1);
            p[r] = drop.kept(pair_even_u32(w0), drop_lsh) ? p[r] : 0.f;
            p[r + 1] = drop.kept(pair_even_u32(w1), drop_lsh) ? p[r + 1] : 0.f;
            p[r + 2] = drop.kept(pair_odd_u32(w0), drop_lsh) ? p[r + 2] : 0.f;
            p[r + 3] = drop.kept(pair_odd_u32(w1), drop_lsh) ? p[r + 3] : 0.f;
          }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st)
          pf[sub * 2 + st] = u32x4{pack2<T>(p[8 * st + 0], p[8 * st + 1]), pack2<T>(p[8 * st + 2], p[8 * st + 3]),
                                   pack2<T>(p[8 * st + 4], p[8 * st + 5]), pack2<T>(p[8 * st + 6], p[8 * st + 7])};
      }
      l_run += psum;
      TAMD_ATTN_PHASE(2)
      // ---- O^T[d][q] += V^T[d][key] . P^T[key][q]
      // step (sub, st): P registers r = 8*st + j  <->  key = sub*32 + 16*st + 8*(j>>2) + 4*hi + (j&3)
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (i + VA < NV) vr[(i + VA) % (VA + 1)] = vreq(i + VA);
        if (VA >= 3) {
          if (!(i & 1)) constexpr_wait_frag2<2 * (VA - 1)>(2 * (NV - 2 - i), vr[i % (VA + 1)], vr[(i + 1) % (VA + 1)]);
        } else {
          constexpr_wait_frag<2 * VA>(2 * (NV - 1 - i), vr[i % (VA + 1)]);
        }
        oacc[i % DT] = mfma32<T>(vr[i % (VA + 1)], pf[i / DT], oacc[i % DT]);  // consecutive MFMAs: different accumulators
      }
      TAMD_ATTN_PHASE(3)
    } else {  // this wave skips the tile (all its rows are above the diagonal): its share of the loads still goes out
      issue(tn, rows_n, cur ^ 1);
    }
    wait_vmcnt0();
    TAMD_ATTN_PHASE(4)
    block_sync();
    TAMD_ATTN_PHASE(5)
  }
#ifdef TAMD_DIAG
  if (tr && lane == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) a.trace[wave * 8 + i] = ph[i];
  }
#endif

  // ---- finalise: l over both half-waves, normalise, LSE, stage O through LDS, row-wise stores
  l_run += swap32_f32(l_run);
  const float inv_l = (l_run > 0.f) ? (DROP ? drop.scale : 1.f) / l_run : 0.f;
  if (SPLIT) {  // this piece's rows, normalised by its own row sums, and their log-sum-exp (-inf: the piece saw no visible key)
    if (qrow < a.seq_q) {
      const int64_t prow = (((int64_t)split * a.batch + b) * a.seq_q + qrow) * a.heads_q + h;
      if (hi == 0)
        a.lse_part[(((int64_t)split * a.batch + b) * a.heads_q + h) * a.seq_q + qrow] =
            (l_run > 0.f) ? (m_run + fast_log2(l_run)) * 0.69314718055994530942f : -INFINITY;
      float* dst = a.o_part + prow * D;
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
  const unsigned st_off = (unsigned)wave * (32u * OROWB);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int d0 = dt * 32 + 8 * qd + 4 * hi;
      const u32x2 pk = {pack2<T>(oacc[dt][qd * 4 + 0] * inv_l, oacc[dt][qd * 4 + 1] * inv_l),
                        pack2<T>(oacc[dt][qd * 4 + 2] * inv_l, oacc[dt][qd * 4 + 3] * inv_l)};
      lds_write8(smem, st_off + (unsigned)l31 * OROWB + (unsigned)d0 * 2u, pk);
    }
  wave_lockstep_point();
  T* O = reinterpret_cast<T*>(a.o) + (int64_t)b * a.osb + (int64_t)h * a.osh;
  constexpr int SLOTS = ROWB / 16;      // 16 (D=128) or 8 (D=64) lanes per row
  constexpr int RPI = 64 / SLOTS;       // rows per wave instruction
#pragma unroll
  for (int it = 0; it < 32 / RPI; ++it) {
    const int row = it * RPI + lane / SLOTS, slot = lane % SLOTS;
    const int qr = qw0 + row;
    const u32x4 v = lds_read16(smem, st_off + (unsigned)row * OROWB + (unsigned)slot * 16u);
    if (qr < a.seq_q) st16(O + (int64_t)qr * a.oss + slot * 8, v);
  }
}

// Merge of the split-KV pieces (tamd_attn_decode): one workgroup of 4 waves per (batch, query row, head);
//   lse = log sum_s exp(lse_s),   O = sum_s exp(lse_s - lse) O_s        (a piece that saw no key: lse_s = -inf, weight 0)
// O rounded once to the storage dtype; lse written when the caller asked for it.
// Every wave finds the maximum over ALL pieces with lane-parallel loads, then adds up the pieces s = wave, wave + 4, ...
// (independent loads, unrolled: several in flight); the four partial rows meet in LDS and wave 0 adds them in a fixed order.
// (The first version walked the pieces one by one on ONE wave, two dependent loads each: 32 us per call at one sequence x
// 4096 keys -- 96 pieces -- where the split-KV kernel itself takes 14.5, profiles/r04o_decode_kernel_stats.csv.)
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_combine_kernel(AttnArgs a) {
  __shared__ float part[4][D];
  __shared__ float wpart[4];
  const int wave = wave_id_uniform(), lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x;  // (the grid is the rows)
  const int h = row % a.heads_q, qrow = (row / a.heads_q) % a.seq_q, b = row / (a.heads_q * a.seq_q);
  const int64_t lse_stride = (int64_t)a.batch * a.heads_q * a.seq_q;                       // between pieces
  const float* lse0 = a.lse_part + ((int64_t)b * a.heads_q + h) * a.seq_q + qrow;
  float mx = -INFINITY;
  for (int s = lane; s < a.kv_splits; s += 64) mx = fmaxf(mx, lse0[(int64_t)s * lse_stride]);
  mx = wave_max(mx);
  constexpr int PER = D / 64;  // output elements per lane
  float acc[PER], wsum = 0.f;
#pragma unroll
  for (int e = 0; e < PER; ++e) acc[e] = 0.f;
  const int64_t o_stride = (int64_t)a.batch * a.seq_q * a.heads_q * D;                     // between pieces
  const float* o0 = a.o_part + (((int64_t)b * a.seq_q + qrow) * a.heads_q + h) * D + lane * PER;
#pragma unroll 4
  for (int s = wave; s < a.kv_splits; s += 4) {
    const float ls = lse0[(int64_t)s * lse_stride];
    const float w = (ls == -INFINITY) ? 0.f : __expf(ls - mx);
    wsum += w;
    const float* src = o0 + (int64_t)s * o_stride;
#pragma unroll
    for (int e = 0; e < PER; ++e) acc[e] += w * src[e];
  }
#pragma unroll
  for (int e = 0; e < PER; ++e) part[wave][lane * PER + e] = acc[e];
  if (lane == 0) wpart[wave] = wsum;
  block_sync();
  if (wave != 0) return;
  wsum = ((wpart[0] + wpart[1]) + wpart[2]) + wpart[3];
  const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
  T* O = reinterpret_cast<T*>(a.o) + (int64_t)b * a.osb + (int64_t)qrow * a.oss + (int64_t)h * a.osh + lane * PER;
  typedef typename elem<T>::raw raw;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int c = lane * PER + e;
    reinterpret_cast<raw*>(O)[e] = elem<T>::from_f32((((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]) * inv);
  }
  if (a.lse != nullptr && lane == 0)
    a.lse[((int64_t)b * a.heads_q + h) * a.seq_q + qrow] = wsum > 0.f ? mx + __logf(wsum) : INFINITY;
}
