// vc_gemm_fr_body.h - the body of the finished-row producer of 2..16-row passes with X in LDS in one piece, written once.  NOT a header
// of declarations: it is the text between the braces of rows_gemm_fr_k (vc_gemm.hip: bf16 / fp32 image, every prologue) and
// rows_gemm_fr_w8_k (vc_gemm_w8.hip: block-scaled E4M3 bytes, plain prologue, 9..16 rows), in the manner of vc_gemm_fr1_body.h (which
// says why this is text and not a function template).  What the kernel computes and why it is laid out this way stands in front of
// rows_gemm_fr_k.
//
// The kernel supplies, in scope:
//   WT, KTW, PRO, NS, P16   weight type, k-tiles per wave and chunk, prologue, partials per item, bf16 partials
//   GROUP                   k-tiles per group of the format (1 for an image, 8 for the E4M3 bytes; a divisor of KTW)
//   CHUNKS                  true: a.nchunk chunks, the registers refilled between them (the image); false: the wave's share is one chunk
//   a                       const GemmArgs&
// and four hooks (macros, #undef'd at the end of this file), in program order.  They see the body's tid, lane, wave, nt, m, kg, wslot,
// NW, TH and SPT:
//   VC_FR_EARLY             statements: what the wave requests with n_active, BEFORE the epilogue operands (a wave's loads return in
//                           order) - a packed format's side words; empty for an image
//   VC_FR_WDECL             statements: the registers of the wave's weights and what addresses them
//   VC_FR_WEIGHTS(c_)       statements: the wave's whole share of chunk c_, everything up front
//   VC_FR_FRAG(J, w)        statements that declare uint4 w = k-tile J (a literal, < GROUP) of the wave's group g, the four dwords of the
//                           MFMA's A operand: lane (m, kg) holds unit kg * TH + m for m < TH; what lanes m >= TH hold only reaches D
//                           rows nobody reads
  static_assert(!P16 || (PRO == PRO_ATT && sizeof(WT) == 2), "bf16 attention partials: the merging out-projection in bf16 mode");
  using T = WTr<WT>;
  constexpr int NW = VC_FR_WAVES, NTHR = 64 * NW, TH = VC_TH_RES, SPT = 4 * TH;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x;
  const int n_rows = a.n_rows;                    // 2..16 as far as rows x K fits LDS and 16 staging units per thread (host contract)
  const int K = a.K;
  const int xs = K * (int)sizeof(WT) + 16;        // LDS row stride (+16: rotate bank slots)
  char* xl = smem;
  f32x4* red = reinterpret_cast<f32x4*>(smem + (size_t)a.r_lds * xs);
  const int active = *a.n_active;
  const int m = lane & 15, kg = lane >> 4;
  VC_FR_EARLY
  const bool nvalid = 4 * kg < TH;
  const int n = nt * TH + (nvalid ? 4 * kg : 0);
  const int wslot = kg * TH + min(m, TH - 1);
  // epilogue operands first (a wave's loads return in order): the residual and the bias of the lane's four channels
  const float4 eres = *reinterpret_cast<const float4*>(a.h_in + (long)((m < n_rows) ? m : 0) * a.d + n);
  const float4 eb = *reinterpret_cast<const float4*>(a.bias + n);
  const float cmu = a.row_mu[(m < n_rows) ? m : 0] + a.mu_shift;         // centring constant of the row's copy in the compute dtype (hq_out)
  VC_FR_WDECL
  if constexpr (PRO == PRO_PLAIN) {
    // X rows as 16-byte units, flat index = row * upr + unit; <= 16 units per thread (rows x K x sizeof <= 128 KB)
    const int upr = K * (int)sizeof(WT) / 16;
    const int total = n_rows * upr;
    const char* src = reinterpret_cast<const char*>(a.x_in);
    const long rstride = (long)a.x_ld * (long)sizeof(WT);
    const int sh = a.x_upr_shift;
    // (explicit scalars: an indexed array is demoted to scratch memory by the compiler)
    uint4 x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, x10, x11, x12, x13, x14, x15;
#define VC_FRX_LOAD(j, dst)                                                                      \
    {                                                                                            \
      const int i_ = min((j) * NTHR + tid, total - 1);                                           \
      const int r_ = (sh >= 0) ? (i_ >> sh) : (i_ / upr);                                        \
      dst = *reinterpret_cast<const uint4*>(src + (long)r_ * rstride + (long)(i_ - r_ * upr) * 16); \
    }
#define VC_FRX_STORE(j, val)                                                                     \
    {                                                                                            \
      const int i_ = (j) * NTHR + tid;                                                           \
      if (i_ < total) {                                                                          \
        const int r_ = (sh >= 0) ? (i_ >> sh) : (i_ / upr);                                      \
        *reinterpret_cast<uint4*>(xl + (size_t)r_ * xs + (size_t)(i_ - r_ * upr) * 16) = val;    \
      }                                                                                          \
    }
    VC_FRX_LOAD(0, x0) VC_FRX_LOAD(1, x1) VC_FRX_LOAD(2, x2) VC_FRX_LOAD(3, x3)
    VC_FRX_LOAD(4, x4) VC_FRX_LOAD(5, x5) VC_FRX_LOAD(6, x6) VC_FRX_LOAD(7, x7)
    VC_FRX_LOAD(8, x8) VC_FRX_LOAD(9, x9) VC_FRX_LOAD(10, x10) VC_FRX_LOAD(11, x11)
    VC_FRX_LOAD(12, x12) VC_FRX_LOAD(13, x13) VC_FRX_LOAD(14, x14) VC_FRX_LOAD(15, x15)
    VC_FR_WEIGHTS(0);
    __builtin_amdgcn_sched_barrier(0);
    if (active == 0) return;
    VC_FRX_STORE(0, x0) VC_FRX_STORE(1, x1) VC_FRX_STORE(2, x2) VC_FRX_STORE(3, x3)
    VC_FRX_STORE(4, x4) VC_FRX_STORE(5, x5) VC_FRX_STORE(6, x6) VC_FRX_STORE(7, x7)
    VC_FRX_STORE(8, x8) VC_FRX_STORE(9, x9) VC_FRX_STORE(10, x10) VC_FRX_STORE(11, x11)
    VC_FRX_STORE(12, x12) VC_FRX_STORE(13, x13) VC_FRX_STORE(14, x14) VC_FRX_STORE(15, x15)
#undef VC_FRX_LOAD
#undef VC_FRX_STORE
  } else if constexpr (P16) {   // PRO_ATT on bf16 partials (round 6): item = (row, EIGHT columns of one head) - one 16-byte load per partial - NI items per thread
    constexpr int NI = 8 / NS;
    const int q8 = K >> 3;
    const int n_items = n_rows * q8;              // <= NI * NTHR (rows x NS <= 16, K <= 2048: host contract)
    const int qsh = a.att_q4_shift - 1;           // log2(K / 8) when K / 4 is a power of two, else < 0
    float2 ml[NI][NS];
    uint4 os[NI][NS];
    int ir[NI], ic[NI];
    bool on[NI];
#pragma unroll
    for (int ib = 0; ib < NI; ++ib) {
      const int idx = ib * NTHR + tid;
      on[ib] = idx < n_items;
      const int i_ = on[ib] ? idx : 0;
      ir[ib] = (a.att_q4_shift >= 1) ? (i_ >> qsh) : (i_ / q8);
      ic[ib] = (i_ - ir[ib] * q8) * 8;
      const int h_ = ic[ib] >> a.hd_shift, e_ = ic[ib] & (a.hd - 1);
      const float2* mp = reinterpret_cast<const float2*>(a.att_ml) + (long)(ir[ib] * a.H + h_) * a.nsplit;
      const uint16_t* op = reinterpret_cast<const uint16_t*>(a.att_o) + ((long)(ir[ib] * a.H + h_) * a.nsplit) * a.hd + e_;
#pragma unroll
      for (int sp = 0; sp < NS; ++sp) {
        const int se = (sp < a.nsplit) ? sp : 0;
        ml[ib][sp] = mp[se];
        os[ib][sp] = *reinterpret_cast<const uint4*>(op + (long)se * a.hd);
      }
    }
    VC_FR_WEIGHTS(0);
    __builtin_amdgcn_sched_barrier(0);
    if (active == 0) return;
#pragma unroll
    for (int ib = 0; ib < NI; ++ib) {
      float M = -INFINITY;
#pragma unroll
      for (int sp = 0; sp < NS; ++sp) {
        ml[ib][sp].x = (sp < a.nsplit) ? ml[ib][sp].x : -INFINITY;
        M = fmaxf(M, ml[ib][sp].x);
      }
      float L = 0.f;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = 0.f;
#pragma unroll
      for (int sp = 0; sp < NS; ++sp) {
        const float w = (ml[ib][sp].x == -INFINITY) ? 0.f : expf(ml[ib][sp].x - M);
        L += w * ml[ib][sp].y;
        const uint4 u = os[ib][sp];
        o[0] += w * __uint_as_float(u.x << 16); o[1] += w * __uint_as_float(u.x & 0xffff0000u);
        o[2] += w * __uint_as_float(u.y << 16); o[3] += w * __uint_as_float(u.y & 0xffff0000u);
        o[4] += w * __uint_as_float(u.z << 16); o[5] += w * __uint_as_float(u.z & 0xffff0000u);
        o[6] += w * __uint_as_float(u.w << 16); o[7] += w * __uint_as_float(u.w & 0xffff0000u);
      }
      const float inv = (L > 0.f) ? 1.0f / L : 0.f;
      uint4 pk;
      pk.x = pack_bf16x2(o[0] * inv, o[1] * inv); pk.y = pack_bf16x2(o[2] * inv, o[3] * inv);
      pk.z = pack_bf16x2(o[4] * inv, o[5] * inv); pk.w = pack_bf16x2(o[6] * inv, o[7] * inv);
      if (on[ib]) *reinterpret_cast<uint4*>(reinterpret_cast<WT*>(xl + (size_t)ir[ib] * xs) + ic[ib]) = pk;
    }
  } else {   // PRO_ATT: item = (row, 4 columns of one head) with a.nsplit <= NS partials of (max, sum, acc[4]); NI items per thread
    constexpr int NI = 16 / NS;
    const int q4 = K >> 2;
    const int n_items = n_rows * q4;              // <= NI * NTHR (rows x NS <= 16, K <= 2048: host contract)
    const int qsh = a.att_q4_shift;
    float2 ml[NI][NS];
    float4 os[NI][NS];
    int ir[NI], ic[NI];
    bool on[NI];
#pragma unroll
    for (int ib = 0; ib < NI; ++ib) {
      const int idx = ib * NTHR + tid;
      on[ib] = idx < n_items;
      const int i_ = on[ib] ? idx : 0;
      ir[ib] = (qsh >= 0) ? (i_ >> qsh) : (i_ / q4);
      ic[ib] = (i_ - ir[ib] * q4) * 4;
      const int h_ = ic[ib] >> a.hd_shift, e_ = ic[ib] & (a.hd - 1);
      const float2* mp = reinterpret_cast<const float2*>(a.att_ml) + (long)(ir[ib] * a.H + h_) * a.nsplit;
      const float* op = a.att_o + ((long)(ir[ib] * a.H + h_) * a.nsplit) * a.hd + e_;
#pragma unroll
      for (int sp = 0; sp < NS; ++sp) {
        const int se = (sp < a.nsplit) ? sp : 0;
        ml[ib][sp] = mp[se];
        os[ib][sp] = *reinterpret_cast<const float4*>(op + (long)se * a.hd);
      }
    }
    VC_FR_WEIGHTS(0);
    __builtin_amdgcn_sched_barrier(0);
    if (active == 0) return;
#pragma unroll
    for (int ib = 0; ib < NI; ++ib) {
      float M = -INFINITY;
#pragma unroll
      for (int sp = 0; sp < NS; ++sp) {
        ml[ib][sp].x = (sp < a.nsplit) ? ml[ib][sp].x : -INFINITY;
        M = fmaxf(M, ml[ib][sp].x);
      }
      float L = 0.f;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int sp = 0; sp < NS; ++sp) {
        const float w = (ml[ib][sp].x == -INFINITY) ? 0.f : expf(ml[ib][sp].x - M);
        L += w * ml[ib][sp].y;
        o[0] += w * os[ib][sp].x; o[1] += w * os[ib][sp].y; o[2] += w * os[ib][sp].z; o[3] += w * os[ib][sp].w;
      }
      const float inv = (L > 0.f) ? 1.0f / L : 0.f;
      o[0] *= inv; o[1] *= inv; o[2] *= inv; o[3] *= inv;
      if (on[ib]) store4(reinterpret_cast<WT*>(xl + (size_t)ir[ib] * xs) + ic[ib], o);
    }
  }
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int mrow = (m < a.r_lds) ? m : 0;
  const char* xrow = xl + (size_t)mrow * xs + (size_t)kg * 16;
  static_assert(KTW % GROUP == 0 && GROUP <= 8, "a wave's k-tiles come in whole groups of at most eight");
  const int nchunk = CHUNKS ? a.nchunk : 1;
  for (int c = 0; c < nchunk; ++c) {
    const int ktl = (c * NW + wave) * KTW;
    // group g of the wave, k-tile J of the group: J is a literal, so that a packed format rebuilds its fragment with compile-time shifts
#pragma unroll
    for (int g = 0; g < KTW / GROUP; ++g) {
#define VC_FR_STEP(J)                                                                                          \
      if constexpr (GROUP > (J)) {                                                                             \
        const uint4 xf = *reinterpret_cast<const uint4*>(xrow + (size_t)(ktl + GROUP * g + (J)) * 64);         \
        VC_FR_FRAG(J, wfrag)                                                                                   \
        acc = mfma_frag(wfrag, xf, acc, (WT*)nullptr);     /* (fragment rows 8..15 only reach D rows nobody reads) */ \
      }
      VC_FR_STEP(0) VC_FR_STEP(1) VC_FR_STEP(2) VC_FR_STEP(3) VC_FR_STEP(4) VC_FR_STEP(5) VC_FR_STEP(6) VC_FR_STEP(7)
#undef VC_FR_STEP
    }
    if (c + 1 < nchunk) VC_FR_WEIGHTS(c + 1);            // exact fp32 mode at d = 2048: the registers hold half of a wave's share
  }
  red[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave == 0 && m < n_rows && nvalid) {
#pragma unroll
    for (int w = 1; w < NW; ++w) acc += red[w * 64 + lane];
    const f32x4 o = {eres.x + eb.x + acc[0], eres.y + eb.y + acc[1], eres.z + eb.z + acc[2], eres.w + eb.w + acc[3]};
    store4(a.h_out + (long)m * a.d + n, o);
    if (a.hq_out) { const f32x4 q = {o[0] - cmu, o[1] - cmu, o[2] - cmu, o[3] - cmu}; store4(reinterpret_cast<WT*>(a.hq_out) + (long)m * a.d + n, q); }
  }
#undef VC_FR_EARLY
#undef VC_FR_WDECL
#undef VC_FR_WEIGHTS
#undef VC_FR_FRAG
