// vc_gemm_rows_body.h - the body of the decode-step rows GEMM, written once.  NOT a header of declarations: it is the text between the
// braces of rows_gemm_k (vc_gemm.hip: bf16 / fp32 image), rows_gemm_lnq_w8_k (vc_gemm_w8.hip: the FFN up-projection of 2..16
// finished rows on the pair planes of vc_w8.h, block-scaled E4M3 bytes) and rows_gemm_qkvq_w8_k (there: the QKV projection of such rows
// on the pairs of the 12-channel image), in the manner of vc_gemm_fr_body.h / vc_gemm_wds_body.h
// (vc_gemm_fr1_body.h says why this is text and not a function template).  vc_gemm.hip describes the kernel in front of rows_gemm_k.
//
// The kernel supplies, in scope:
//   WT, KTW, PRO, EPI, NTW, NT, R2, NP     rows_gemm_k's template parameters (template or constexpr)
//   a                                       const GemmArgs&
// and the weight source as six hooks (macros, #undef'd at the end of this file), in program order.  They see the body's lane, wave, nt,
// kt0, grp, SPT and wslot:
//   VC_ROWS_EARLY            statements: what the wave requests with n_active, BEFORE the epilogue operands (a wave's loads return in
//                            order) - a packed format's side bytes; empty for an image
//   VC_ROWS_WDECL            statements: the wave's weight addresses and the registers its requests land in
//   VC_ROWS_BURST            statements: every weight request of the wave's first chunk, behind the prologue's first requests
//   VC_ROWS_FRAG(i)          statements right in front of the MFMA of k-tile i of the chunk: a packed format rebuilds the operand here;
//                            empty for an image
//   VC_ROWS_W(i)             lvalue (uint4): the four dwords of that MFMA's A operand
//   VC_ROWS_REFILL(c)        statements: behind chunk c's MFMAs, the requests of chunk c + 1 when there is one (a.nchunk > 1)
  using T = WTr<WT>;
  constexpr bool LNW = PRO == PRO_LNW || PRO == PRO_LNQ;       // finished-row consumers (fp32 rows / the producers' centred copy)
  static_assert(NTW == 1 || LNW, "two tiles per workgroup: finished-row consumers only");
  static_assert(NP == VC_MAX_KSPLIT || PRO == PRO_LN, "slab count: LayerNorm prologue of slab-form passes only");
  static_assert(NP == 0 || NP == 2 || NP == VC_MAX_KSPLIT, "slabs requested per row");
  static_assert(!R2 || NTW == 2, "two rows per wave: the two-tile form");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  VC_KTS_DECL();
  VC_KTS(0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = (NTW == 1) ? wv : (wv & 3);    // K quarter of the tile
  const int tg = (NTW == 1) ? 0 : (wv >> 2);      // which of the workgroup's tiles
  const int nt = (NTW == 1) ? (int)blockIdx.x : (int)blockIdx.x * NTW + tg;
  const int ks = blockIdx.y, grp = blockIdx.z;
  const int n_rows = a.n_rows;                    // >= 1 (host contract)
  const int kt_blk = a.nchunk * 4 * KTW;          // k-tiles this block covers
  const int kt0 = ks * kt_blk;                    // first of them
  const int kblk = kt_blk * T::KW;                // K elements this block covers
  const int k0 = kt0 * T::KW;
  const int xs = kblk * (int)sizeof(WT) + 16;     // LDS row stride in bytes (+16: rotate bank slots)
  char* xl = smem;
  f32x4* red0 = reinterpret_cast<f32x4*>(smem + (size_t)a.r_lds * xs);
  f32x4* red = red0 + tg * 256;
  float* stat = reinterpret_cast<float*>(red0 + 256 * NTW);      // LN prologue: [row][wave][sum, sum of squares] of the centred, rounded row
  float* msum = stat + VC_ROWS * 4 * 2;                   // LN prologue: [row][wave] partial sums of the fp32 row (its mean)

  // Tile height: the QKV projection (N = 3d) uses 12-channel tiles, so that its 3d/12 = d/4 tiles are
  // a multiple of the CU count (512 workgroups of 48 KB at d = 2048 instead of 384 of 64 KB = 1.5 per
  // CU); lanes 12..15 of each fragment row group re-read slot 11 and are zeroed before the MFMA.
  constexpr int TH = (EPI == EPI_QKV) ? VC_TH_QKV : 16;
  constexpr int SPT = 4 * TH;                     // fragment slots per (n_tile, k_tile)
  const int active = *a.n_active;                 // scalar; looked at once the burst is on its way
  VC_ROWS_EARLY
  const int m = lane & 15;
  const int kg = lane >> 4;
  const int n = nt * TH + 4 * kg;
  const bool wvalid = m < TH;                     // this lane's fragment row exists
  const bool nvalid = 4 * kg < TH;                // this lane's 4 output channels exist
  const int wslot = kg * TH + min(m, TH - 1);
  float4 eb;
  int epos, eseq;
  epi_preload<WT, EPI>(a, (m < n_rows) ? m : 0, n, grp, eb, epos, eseq);
  float4 ewg = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (PRO == PRO_LN || LNW) ewg = wg_preload<WT, EPI>(a, n, grp);

  VC_ROWS_WDECL
#define VC_BURST_OUT()                                                                           \
  __builtin_amdgcn_sched_barrier(0);                                                             \
  if (active == 0) return;   /* every sequence finished: the replayed step is a no-op */     \
  VC_KTS(1);

  // prologue: build the rows' X slice [n_rows][kblk] as WT in LDS.  Every load is unconditional and
  // branch-free (out-of-range lanes re-read a valid address, unused split slabs are read and discarded
  // by a select): a load inside a branch makes the compiler drain the whole queue (vmcnt(0)).
  if constexpr (PRO == PRO_LN) {
    // LayerNorm fold (see the top of vc_gemm.hip): hn = h + prev_bias + sum(parts); X = hn - mean(hn), un-scaled; the
    // sum and sum of squares of the ROUNDED centred values the MFMA multiplies are reduced per wave here, in the
    // shadow of the weight stream, and combined in the epilogue (the residual mean of the rounded row and rstd).  The whole block works on one row at a time:
    // thread t owns float4 columns t and t+256.  Rows beyond the first are software-pipelined through two
    // register sets (the next row's loads fly during this row's arithmetic).
    const int d = a.d;
    const int nq = d >> 2;                               // float4 per row (<= 512)
    const bool on0 = tid < nq, on1 = tid + 256 < nq;
    const int c0 = on0 ? tid * 4 : 0, c1 = on1 ? (tid + 256) * 4 : 0;
    constexpr int NPA = NP > 0 ? NP : 1;
    float4 pb0 = make_float4(0.f, 0.f, 0.f, 0.f), pb1 = pb0;
    if constexpr (NP > 0) {
      pb0 = *reinterpret_cast<const float4*>(a.prev_bias + c0);
      pb1 = *reinterpret_cast<const float4*>(a.prev_bias + c1);
    }
    const bool use_pb = NP > 0 && a.has_prev_bias != 0;
    float4 x0A, x1A, p0A[NPA], p1A[NPA];
    float4 x0B, x1B, p0B[NPA], p1B[NPA];
#define VC_LOAD_ROW(S, r, G)   /* G: honour a.gather_rows (single-row launches only, host contract) */ \
    {                                                                                            \
      int sr_ = (r);                                                                             \
      if (G && a.gather_rows) sr_ = a.gather_rows[sr_];                                          \
      const float* hp_ = a.h_in + (long)sr_ * d;                                                 \
      x0##S = *reinterpret_cast<const float4*>(hp_ + c0);                                        \
      x1##S = *reinterpret_cast<const float4*>(hp_ + c1);                                        \
      _Pragma("unroll") for (int s_ = 0; s_ < NP; ++s_) {                                        \
        const float* pp_ = a.parts + ((long)(s_ * a.rows_cap + sr_)) * d;                        \
        p0##S[s_] = *reinterpret_cast<const float4*>(pp_ + c0);                                  \
        p1##S[s_] = *reinterpret_cast<const float4*>(pp_ + c1);                                  \
      }                                                                                          \
    }
#define VC_FINISH_ROW(S, r)                                                                      \
    {                                                                                            \
      float4 x0 = x0##S, x1 = x1##S;                                                             \
      if (use_pb) {                                                                              \
        x0.x += pb0.x; x0.y += pb0.y; x0.z += pb0.z; x0.w += pb0.w;                              \
        x1.x += pb1.x; x1.y += pb1.y; x1.z += pb1.z; x1.w += pb1.w;                              \
      }                                                                                          \
      _Pragma("unroll") for (int s_ = 0; s_ < NP; ++s_) {                                        \
        const bool u_ = s_ < a.n_parts;                                                          \
        x0.x += u_ ? p0##S[s_].x : 0.f; x0.y += u_ ? p0##S[s_].y : 0.f; x0.z += u_ ? p0##S[s_].z : 0.f; x0.w += u_ ? p0##S[s_].w : 0.f; \
        x1.x += u_ ? p1##S[s_].x : 0.f; x1.y += u_ ? p1##S[s_].y : 0.f; x1.z += u_ ? p1##S[s_].z : 0.f; x1.w += u_ ? p1##S[s_].w : 0.f; \
      }                                                                                          \
      const bool writer_ = a.h_out && grp == 0 && (((r) % (int)gridDim.x) == (int)blockIdx.x);   \
      if (writer_ && on0) *reinterpret_cast<float4*>(a.h_out + (long)(r) * d + c0) = x0;         \
      if (writer_ && on1) *reinterpret_cast<float4*>(a.h_out + (long)(r) * d + c1) = x1;         \
      /* the row is CENTRED before it is rounded to the MFMA's input type: a residual stream with a large common   */ \
      /* offset (|mean| >> sigma, usual in trained pre-LN stacks) would otherwise spend its bf16 mantissa on the   */ \
      /* offset and the rounding error would come out of the fold amplified by |mean| / sigma                      */ \
      float t_ = (on0 ? ((x0.x + x0.y) + (x0.z + x0.w)) : 0.f) + (on1 ? ((x1.x + x1.y) + (x1.z + x1.w)) : 0.f);  \
      t_ = wave_sum(t_);                                                                         \
      if (lane == 0) msum[(r) * 4 + wave] = t_;                                                  \
      __syncthreads();                                                                           \
      const float4 ms_ = *reinterpret_cast<const float4*>(msum + (r) * 4);                       \
      const float mu_ = ((ms_.x + ms_.y) + (ms_.z + ms_.w)) * (1.0f / (float)d);                 \
      WT* xr_ = reinterpret_cast<WT*>(xl + (size_t)(r) * xs);                                    \
      float s1_ = 0.f, s2_ = 0.f;                                                                \
      if (on0) {                                                                                 \
        const f32x4 y_ = {x0.x - mu_, x0.y - mu_, x0.z - mu_, x0.w - mu_};                       \
        const f32x4 q_ = store4r(xr_ + c0, y_);                                                  \
        s1_ += (q_[0] + q_[1]) + (q_[2] + q_[3]);                                                \
        s2_ += (q_[0] * q_[0] + q_[1] * q_[1]) + (q_[2] * q_[2] + q_[3] * q_[3]);                \
      }                                                                                          \
      if (on1) {                                                                                 \
        const f32x4 y_ = {x1.x - mu_, x1.y - mu_, x1.z - mu_, x1.w - mu_};                       \
        const f32x4 q_ = store4r(xr_ + c1, y_);                                                  \
        s1_ += (q_[0] + q_[1]) + (q_[2] + q_[3]);                                                \
        s2_ += (q_[0] * q_[0] + q_[1] * q_[1]) + (q_[2] * q_[2] + q_[3] * q_[3]);                \
      }                                                                                          \
      s1_ = wave_sum(s1_);                                                                       \
      s2_ = wave_sum(s2_);                                                                       \
      if (lane == 0) { stat[((r) * 4 + wave) * 2] = s1_; stat[((r) * 4 + wave) * 2 + 1] = s2_; } \
    }
    VC_LOAD_ROW(A, 0, 1);
    VC_ROWS_BURST
    VC_BURST_OUT();
    if (n_rows == 1) {
      VC_FINISH_ROW(A, 0);
    } else {
      int r = 0;
      for (;;) {
        VC_LOAD_ROW(B, min(r + 1, n_rows - 1), 0);
        VC_FINISH_ROW(A, r);
        if (++r >= n_rows) break;
        VC_LOAD_ROW(A, min(r + 1, n_rows - 1), 0);
        VC_FINISH_ROW(B, r);
        if (++r >= n_rows) break;
      }
    }
#undef VC_LOAD_ROW
#undef VC_FINISH_ROW
  } else if constexpr (PRO == PRO_LNW) {
    // LayerNorm fold of 2..8 FINISHED rows (h holds the whole residual, bias included: the finished-row producers,
    // rows_gemm_fr_k): one WAVE per row - wave w takes rows w and w + 4 - so a row's mean and its two statistics are wave
    // reductions, the prologue has no block barrier per row and both rows of a wave are requested ahead of the weight
    // burst.  (PRO_LN walks the rows one after the other with the whole block: one dependent round trip + one barrier per
    // row in every workgroup - 20 us per GEMM at 8 rows - which is why several-row steps used a separate LayerNorm launch.)
    const int d = a.d;
    const int npl = d >> 8;                                 // float4 per lane and row: d / 4 / 64 = 1..8 (d % 256 == 0)
    const int rowA = (NTW == 1) ? wave : wv;                // (two tiles per workgroup: 8 waves, one row each - or two, R2)
    const int rowB = (NTW == 1) ? wave + 4 : wv + 8;
    constexpr bool TWO_ROWS = (NTW == 1) || R2;
    const float* hrA = a.h_in + (long)min(rowA, n_rows - 1) * d;
    const float* hrB = a.h_in + (long)min(rowB, n_rows - 1) * d;
    float4 xa[8], xb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = (min(j, npl - 1) * 64 + lane) * 4;
      xa[j] = *reinterpret_cast<const float4*>(hrA + c);
      if constexpr (TWO_ROWS) xb[j] = *reinterpret_cast<const float4*>(hrB + c);
    }
    VC_ROWS_BURST
    VC_BURST_OUT();
#define VC_LNW_ROW(X, r)                                                                         \
    if ((r) < n_rows) {                                                                          \
      float t_ = 0.f;                                                                            \
      _Pragma("unroll") for (int j = 0; j < 8; ++j)                                              \
        if (j < npl) t_ += (X[j].x + X[j].y) + (X[j].z + X[j].w);                                \
      const float mu_ = wave_sum(t_) * (1.0f / (float)d);                                        \
      WT* xr_ = reinterpret_cast<WT*>(xl + (size_t)(r) * xs);                                    \
      float s1_ = 0.f, s2_ = 0.f;                                                                \
      _Pragma("unroll") for (int j = 0; j < 8; ++j)                                              \
        if (j < npl) {                                                                           \
          const f32x4 y_ = {X[j].x - mu_, X[j].y - mu_, X[j].z - mu_, X[j].w - mu_};             \
          const f32x4 q_ = store4r(xr_ + (j * 64 + lane) * 4, y_);                               \
          s1_ += (q_[0] + q_[1]) + (q_[2] + q_[3]);                                              \
          s2_ += (q_[0] * q_[0] + q_[1] * q_[1]) + (q_[2] * q_[2] + q_[3] * q_[3]);              \
        }                                                                                        \
      s1_ = wave_sum(s1_);                                                                       \
      s2_ = wave_sum(s2_);                                                                       \
      if (lane == 0) {      /* the epilogue sums four per-wave pairs: this row has one */          \
        *reinterpret_cast<float4*>(stat + (r) * 8) = make_float4(s1_, s2_, 0.f, 0.f);            \
        *reinterpret_cast<float4*>(stat + (r) * 8 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);        \
        if (a.row_mu_out && blockIdx.x == 0 && grp == 0) a.row_mu_out[r] = mu_;      /* the next producer centres its copy of the row on it */ \
      }                                                                                          \
    }
    VC_LNW_ROW(xa, rowA);
    if constexpr (TWO_ROWS) { VC_LNW_ROW(xb, rowB); }
#undef VC_LNW_ROW
  } else if constexpr (PRO == PRO_LNQ) {
    // The same fold on the producer's centred copy q = WT(h - c) of the finished rows (c = a.row_mu[row] + a.mu_shift: the mean the PREVIOUS LayerNorm of
    // the row found, plus the mean of the bias the producer's update added): W LN(h) = rstd (W' q - mean(q) rowsum(W')) + cb holds for any c, and
    // |mean(q)| stays far below sigma because the rest of one residual update moves a row's mean by little - the rounding of q keeps its mantissa for the signal, as with the exact mean.  A wave
    // copies its row(s) from HBM / L2 to LDS as they are (16 bytes per lane and request: HALF the bytes of the fp32 rows in bf16 mode, no
    // conversion) and sums the values and their squares on the way.
    const int d = a.d;
    constexpr int E16 = 16 / (int)sizeof(WT);                   // elements per 16-byte unit
    const int npl = (d * (int)sizeof(WT)) >> 10;                // units per lane and row: d sizeof(WT) / 16 / 64 = 1..8
    const int rowA = (NTW == 1) ? wave : wv;
    const int rowB = (NTW == 1) ? wave + 4 : wv + 8;
    constexpr bool TWO_ROWS = (NTW == 1) || R2;
    const char* qA = reinterpret_cast<const char*>(a.x_in) + (long)min(rowA, n_rows - 1) * d * (long)sizeof(WT);
    const char* qB = reinterpret_cast<const char*>(a.x_in) + (long)min(rowB, n_rows - 1) * d * (long)sizeof(WT);
    const float cA = a.row_mu[min(rowA, n_rows - 1)] + a.mu_shift, cB = a.row_mu[min(rowB, n_rows - 1)] + a.mu_shift;
    uint4 xa[8], xb[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int u = (min(j, npl - 1) * 64 + lane) * 16;
      xa[j] = *reinterpret_cast<const uint4*>(qA + u);
      if constexpr (TWO_ROWS) xb[j] = *reinterpret_cast<const uint4*>(qB + u);
    }
    VC_ROWS_BURST
    VC_BURST_OUT();
#define VC_LNQ_ROW(X, r, c_)                                                                     \
    if ((r) < n_rows) {                                                                          \
      char* xr_ = xl + (size_t)(r) * xs;                                                         \
      float s1_ = 0.f, s2_ = 0.f;                                                                \
      _Pragma("unroll") for (int j = 0; j < 8; ++j)                                              \
        if (j < npl) {                                                                           \
          *reinterpret_cast<uint4*>(xr_ + (j * 64 + lane) * 16) = X[j];                          \
          float f_[E16];                                                                         \
          if constexpr (sizeof(WT) == 2) {                                                       \
            f_[0] = __uint_as_float(X[j].x << 16); f_[1] = __uint_as_float(X[j].x & 0xffff0000u); \
            f_[2] = __uint_as_float(X[j].y << 16); f_[3] = __uint_as_float(X[j].y & 0xffff0000u); \
            f_[4] = __uint_as_float(X[j].z << 16); f_[5] = __uint_as_float(X[j].z & 0xffff0000u); \
            f_[6] = __uint_as_float(X[j].w << 16); f_[7] = __uint_as_float(X[j].w & 0xffff0000u); \
          } else {                                                                               \
            f_[0] = __uint_as_float(X[j].x); f_[1] = __uint_as_float(X[j].y);                    \
            f_[2] = __uint_as_float(X[j].z); f_[3] = __uint_as_float(X[j].w);                    \
          }                                                                                      \
          _Pragma("unroll") for (int e_ = 0; e_ < E16; e_ += 4) {                                \
            s1_ += (f_[e_] + f_[e_ + 1]) + (f_[e_ + 2] + f_[e_ + 3]);                            \
            s2_ += (f_[e_] * f_[e_] + f_[e_ + 1] * f_[e_ + 1]) + (f_[e_ + 2] * f_[e_ + 2] + f_[e_ + 3] * f_[e_ + 3]); \
          }                                                                                      \
        }                                                                                        \
      s1_ = wave_sum(s1_);                                                                       \
      s2_ = wave_sum(s2_);                                                                       \
      if (lane == 0) {                                                                           \
        *reinterpret_cast<float4*>(stat + (r) * 8) = make_float4(s1_, s2_, 0.f, 0.f);            \
        *reinterpret_cast<float4*>(stat + (r) * 8 + 4) = make_float4(0.f, 0.f, 0.f, 0.f);        \
        if (a.row_mu_out && blockIdx.x == 0 && grp == 0) a.row_mu_out[r] = (c_) + s1_ * (1.0f / (float)d);   \
      }                                                                                          \
    }
    VC_LNQ_ROW(xa, rowA, cA);
    if constexpr (TWO_ROWS) { VC_LNQ_ROW(xb, rowB, cB); }
#undef VC_LNQ_ROW
  } else if constexpr (PRO == PRO_PLAIN) {
    // X rows copied as 16-byte units, flat index = row * upr + unit.  The first NB*256 units are
    // requested ahead of the weight burst (clamped, unconditional), the rest behind it.
    const int upr = kblk * (int)sizeof(WT) / 16;   // 16-byte units per row
    const int total = n_rows * upr;
    const char* src = reinterpret_cast<const char*>(a.x_in) + ((long)grp * a.x_group_stride + k0) * (long)sizeof(WT);
    const long rstride = (long)a.x_ld * (long)sizeof(WT);
    const int sh = a.x_upr_shift;                  // log2(upr) when upr is a power of two, else -1
#define VC_X_SPLIT(idx_, r_, u_)                                                                 \
    const int r_ = (sh >= 0) ? ((idx_) >> sh) : ((idx_) / upr);                                  \
    const int u_ = (idx_) - r_ * upr;
#define VC_X_LOAD(j, dst)                                                                        \
    {                                                                                            \
      const int i_ = min((j) * 256 + tid, total - 1);                                            \
      VC_X_SPLIT(i_, rr_, uu_)                                                                   \
      dst = *reinterpret_cast<const uint4*>(src + (long)rr_ * rstride + (long)uu_ * 16);         \
    }
#define VC_X_STORE(j, val)                                                                       \
    {                                                                                            \
      const int i_ = (j) * 256 + tid;                                                            \
      if (i_ < total) {                                                                          \
        VC_X_SPLIT(i_, rr_, uu_)                                                                 \
        *reinterpret_cast<uint4*>(xl + (size_t)rr_ * xs + (size_t)uu_ * 16) = val;               \
      }                                                                                          \
    }
    // (explicit scalars: an indexed array here is demoted to scratch memory by the compiler)
#define VC_X_LATE(NB)                                                                            \
      for (int i_ = NB * 256 + tid; i_ < total; i_ += 256) {                                     \
        VC_X_SPLIT(i_, rr_, uu_)                                                                 \
        *reinterpret_cast<uint4*>(xl + (size_t)rr_ * xs + (size_t)uu_ * 16) =                    \
            *reinterpret_cast<const uint4*>(src + (long)rr_ * rstride + (long)uu_ * 16);         \
      }
    if (total <= 4 * 256) {        // one decode row (up to 4 KB x 4 slices)
      uint4 x0, x1, x2, x3;
      VC_X_LOAD(0, x0); VC_X_LOAD(1, x1); VC_X_LOAD(2, x2); VC_X_LOAD(3, x3);
      VC_ROWS_BURST
      VC_BURST_OUT();
      VC_X_STORE(0, x0); VC_X_STORE(1, x1); VC_X_STORE(2, x2); VC_X_STORE(3, x3);
    } else {                       // batched decode / span switch: 16 rows of 4 KB in one round trip
      uint4 x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, x10, x11, x12, x13, x14, x15;
      VC_X_LOAD(0, x0); VC_X_LOAD(1, x1); VC_X_LOAD(2, x2); VC_X_LOAD(3, x3);
      VC_X_LOAD(4, x4); VC_X_LOAD(5, x5); VC_X_LOAD(6, x6); VC_X_LOAD(7, x7);
      VC_X_LOAD(8, x8); VC_X_LOAD(9, x9); VC_X_LOAD(10, x10); VC_X_LOAD(11, x11);
      VC_X_LOAD(12, x12); VC_X_LOAD(13, x13); VC_X_LOAD(14, x14); VC_X_LOAD(15, x15);
      VC_ROWS_BURST
      VC_BURST_OUT();
      VC_X_STORE(0, x0); VC_X_STORE(1, x1); VC_X_STORE(2, x2); VC_X_STORE(3, x3);
      VC_X_STORE(4, x4); VC_X_STORE(5, x5); VC_X_STORE(6, x6); VC_X_STORE(7, x7);
      VC_X_STORE(8, x8); VC_X_STORE(9, x9); VC_X_STORE(10, x10); VC_X_STORE(11, x11);
      VC_X_STORE(12, x12); VC_X_STORE(13, x13); VC_X_STORE(14, x14); VC_X_STORE(15, x15);
      VC_X_LATE(16)
    }
#undef VC_X_LATE
#undef VC_X_LOAD
#undef VC_X_STORE
#undef VC_X_SPLIT
  } else {  // PRO_ATT: merge the split-S partials of the decode attention (softmax denominators)
    // item = (row, 4 columns of one head) with NS partials of (max, sum, acc[4]); a thread carries IB
    // items at a time, NS * IB = 8 (one decode row: 8 splits x 1 item; batched rows: fewer splits, more
    // items).  The first batch is requested before the weight burst, the exp/scale arithmetic runs
    // behind it; further batches are double-buffered.
    const int q4 = kblk >> 2;
    const int n_items = n_rows * q4;
    const int qsh = a.att_q4_shift;                 // log2(q4) when q4 is a power of two, else -1
#define VC_ATT_LOAD(S, NS, IB, base)                                                             \
    _Pragma("unroll") for (int ib_ = 0; ib_ < IB; ++ib_) {                                       \
      const int idx_ = (base) + ib_ * 256 + tid;                                                 \
      on##S[ib_] = idx_ < n_items;                                                               \
      const int ic_ = on##S[ib_] ? idx_ : 0;                                                     \
      r##S[ib_] = (qsh >= 0) ? (ic_ >> qsh) : (ic_ / q4);                                        \
      c##S[ib_] = k0 + (ic_ - r##S[ib_] * q4) * 4;                                               \
      const int h_ = c##S[ib_] >> a.hd_shift, e_ = c##S[ib_] & (a.hd - 1);                      \
      const float2* ml_ = reinterpret_cast<const float2*>(a.att_ml) + (long)(r##S[ib_] * a.H + h_) * a.nsplit; \
      const float* op_ = a.att_o + ((long)(r##S[ib_] * a.H + h_) * a.nsplit) * a.hd + e_;        \
      _Pragma("unroll") for (int s_ = 0; s_ < NS; ++s_) {                                        \
        const int se_ = (s_ < a.nsplit) ? s_ : 0;                                                \
        ml##S[ib_][s_] = ml_[se_];                                                               \
        os##S[ib_][s_] = *reinterpret_cast<const float4*>(op_ + (long)se_ * a.hd);               \
      }                                                                                          \
    }
#define VC_ATT_FINISH(S, NS, IB)                                                                 \
    _Pragma("unroll") for (int ib_ = 0; ib_ < IB; ++ib_) {                                       \
      float M_ = -INFINITY;                                                                      \
      _Pragma("unroll") for (int s_ = 0; s_ < NS; ++s_) {                                        \
        ml##S[ib_][s_].x = (s_ < a.nsplit) ? ml##S[ib_][s_].x : -INFINITY;                       \
        M_ = fmaxf(M_, ml##S[ib_][s_].x);                                                        \
      }                                                                                          \
      float L_ = 0.f;                                                                            \
      f32x4 o_ = {0.f, 0.f, 0.f, 0.f};                                                           \
      _Pragma("unroll") for (int s_ = 0; s_ < NS; ++s_) {                                        \
        const float w_ = (ml##S[ib_][s_].x == -INFINITY) ? 0.f : expf(ml##S[ib_][s_].x - M_);    \
        L_ += w_ * ml##S[ib_][s_].y;                                                             \
        o_[0] += w_ * os##S[ib_][s_].x; o_[1] += w_ * os##S[ib_][s_].y;                          \
        o_[2] += w_ * os##S[ib_][s_].z; o_[3] += w_ * os##S[ib_][s_].w;                          \
      }                                                                                          \
      const float inv_ = (L_ > 0.f) ? 1.0f / L_ : 0.f;                                           \
      o_[0] *= inv_; o_[1] *= inv_; o_[2] *= inv_; o_[3] *= inv_;                                \
      if (on##S[ib_]) store4(reinterpret_cast<WT*>(xl + (size_t)r##S[ib_] * xs) + (c##S[ib_] - k0), o_); \
    }
#define VC_ATT_PATH(NS, IB)                                                                      \
    {                                                                                            \
      float2 mlA[IB][NS], mlB[IB][NS];                                                           \
      float4 osA[IB][NS], osB[IB][NS];                                                           \
      int rA[IB], cA[IB], rB[IB], cB[IB];                                                        \
      bool onA[IB], onB[IB];                                                                     \
      VC_ATT_LOAD(A, NS, IB, 0);                                                                 \
      VC_ROWS_BURST                                                                              \
      VC_BURST_OUT();                                                                            \
      if (n_items <= IB * 256) {                                                                 \
        VC_ATT_FINISH(A, NS, IB);                                                                \
      } else {                                                                                   \
        int base = 0;                                                                            \
        for (;;) {                                                                               \
          VC_ATT_LOAD(B, NS, IB, base + IB * 256);   /* past the end: clamped loads, nothing stored */ \
          VC_ATT_FINISH(A, NS, IB);                                                              \
          if ((base += IB * 256) >= n_items) break;                                              \
          VC_ATT_LOAD(A, NS, IB, base + IB * 256);                                               \
          VC_ATT_FINISH(B, NS, IB);                                                              \
          if ((base += IB * 256) >= n_items) break;                                              \
        }                                                                                        \
      }                                                                                          \
    }
    if (a.nsplit > 4) VC_ATT_PATH(8, 1)
    else if (a.nsplit > 2) VC_ATT_PATH(4, 2)
    else VC_ATT_PATH(2, 4)
#undef VC_ATT_PATH
#undef VC_ATT_LOAD
#undef VC_ATT_FINISH
  }
#undef VC_BURST_OUT
  VC_KTS(2);
  __syncthreads();
  VC_KTS(3);

  // main loop: one ds_read_b128 + one MFMA per 1 KiB weight burst
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int mrow = (m < a.r_lds) ? m : 0;
  const char* xrow = xl + (size_t)mrow * xs + (size_t)(lane >> 4) * 16;
  for (int c = 0; c < a.nchunk; ++c) {
    const int ktl = (c * 4 + wave) * KTW;
#pragma unroll
    for (int i = 0; i < KTW; ++i) {
      const uint4 xf = *reinterpret_cast<const uint4*>(xrow + (size_t)(ktl + i) * 64);
      VC_ROWS_FRAG(i)
      if constexpr (TH < 16) {
        if (!wvalid) VC_ROWS_W(i) = make_uint4(0u, 0u, 0u, 0u);
      }
      acc = mfma_frag(VC_ROWS_W(i), xf, acc, (WT*)nullptr);
    }
    VC_ROWS_REFILL(c)
  }
  VC_KTS(4);

  // 4-way in-block K reduction, then the epilogue on wave 0
  red[wave * 64 + lane] = acc;
  __syncthreads();
  VC_KTS(5);
  if (wave == 0 && m < n_rows && nvalid) {
    {
      const f32x4 a1 = red[64 + lane], a2 = red[128 + lane], a3 = red[192 + lane];
      acc = (acc + a1) + (a2 + a3);
    }
    if constexpr (PRO == PRO_LN || LNW) {   // LayerNorm fold on the centred row xc: y = rstd * (W'xc - mean(xc) * rowsum(W')) [+ cb in the epilogue]
      const float4 sa = *reinterpret_cast<const float4*>(stat + m * 8), sb = *reinterpret_cast<const float4*>(stat + m * 8 + 4);
      const float inv_d = 1.0f / (float)a.d;
      const float mean = ((sa.x + sa.z) + (sb.x + sb.z)) * inv_d;
      const float var = fmaxf(((sa.y + sa.w) + (sb.y + sb.w)) * inv_d - mean * mean, 0.f);
      const float rstd = 1.0f / sqrtf(var + 1e-5f);      // eps 1e-5 (transformer.py:30)
      acc[0] = rstd * (acc[0] - mean * ewg.x); acc[1] = rstd * (acc[1] - mean * ewg.y);
      acc[2] = rstd * (acc[2] - mean * ewg.z); acc[3] = rstd * (acc[3] - mean * ewg.w);
    }
    gemm_epilogue<WT, EPI>(a, acc, m, n, ks, grp, (int)gridDim.z, eb, epos, eseq);
  }
  VC_KTS(6);
  VC_KTS_FLUSH();
#undef VC_ROWS_EARLY
#undef VC_ROWS_WDECL
#undef VC_ROWS_BURST
#undef VC_ROWS_FRAG
#undef VC_ROWS_W
#undef VC_ROWS_REFILL
