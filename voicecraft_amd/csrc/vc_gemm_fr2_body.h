// vc_gemm_fr2_body.h - the body of the FFN down-projection of 9..16 finished rows with K through LDS in two halves, written once.  NOT a
// header of declarations: it is the text between the braces of rows_gemm_fr2_k (vc_gemm.hip: bf16 / fp32 image) and rows_gemm_fr2_w8_k
// (vc_gemm_w8.hip: block-scaled E4M3 bytes), in the manner of vc_gemm_fr1_body.h (which says why this is text and not a function
// template).  What the kernel computes and why it is laid out this way stands in front of rows_gemm_fr2_k.
//
// The kernel supplies, in scope:
//   WT, KTW                 weight type, k-tiles per wave and half
//   GROUP                   k-tiles per group of the format (1 for an image, 8 for the E4M3 bytes; a divisor of KTW)
//   a                       const GemmArgs&
// and four hooks (macros, #undef'd at the end of this file), in program order.  They see the body's tid, lane, wave, nt, m, kg, wslot,
// NW, TH and SPT:
//   VC_FR2_EARLY            statements: what the wave requests with n_active, BEFORE the epilogue operands (a wave's loads return in
//                           order) - a packed format's side words; empty for an image
//   VC_FR2_WDECL            statements: the registers of the wave's weights of BOTH halves and what addresses them
//   VC_FR2_BURST            statements: the wave's whole share of both halves, everything up front, the first half first
//   VC_FR2_FRAG(h_, J, w)   statements that declare uint4 w = k-tile J (a literal, < GROUP) of the wave's group g of half h_ (a literal),
//                           the four dwords of the MFMA's A operand: lane (m, kg) holds unit kg * TH + m for m < TH; what lanes m >= TH
//                           hold only reaches D rows nobody reads
  using T = WTr<WT>;
  constexpr int NW = VC_FR_WAVES, NTHR = 64 * NW, TH = VC_TH_RES, SPT = 4 * TH;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x;
  const int n_rows = a.n_rows;                    // <= 16 (host contract)
  const int Kh = a.K >> 1;                        // K elements per half = NW * KTW k-tiles
  const int xs = Kh * (int)sizeof(WT) + 16;
  char* xl = smem;
  f32x4* red = reinterpret_cast<f32x4*>(smem + (size_t)a.r_lds * xs);
  const int active = *a.n_active;
  const int m = lane & 15, kg = lane >> 4;
  VC_FR2_EARLY
  const bool nvalid = 4 * kg < TH;
  const int n = nt * TH + (nvalid ? 4 * kg : 0);
  const int wslot = kg * TH + min(m, TH - 1);
  const float4 eres = *reinterpret_cast<const float4*>(a.h_in + (long)((m < n_rows) ? m : 0) * a.d + n);
  const float4 eb = *reinterpret_cast<const float4*>(a.bias + n);
  const float cmu = a.row_mu[(m < n_rows) ? m : 0] + a.mu_shift;
  VC_FR2_WDECL
  const int upr = Kh * (int)sizeof(WT) / 16;       // 16-byte units per row and half; rows x upr <= 16 x 512 (host contract)
  const int total = n_rows * upr;
  const char* src = reinterpret_cast<const char*>(a.x_in);
  const long rstride = (long)a.x_ld * (long)sizeof(WT);
  const long hoff = (long)Kh * (long)sizeof(WT);
  const int sh = a.x_upr_shift;
  uint4 x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, x10, x11, x12, x13, x14, x15;
#define VC_FR2_LOAD(j, dst, off_)                                                                \
    {                                                                                            \
      const int i_ = min((j) * NTHR + tid, total - 1);                                           \
      const int r_ = (sh >= 0) ? (i_ >> sh) : (i_ / upr);                                        \
      dst = *reinterpret_cast<const uint4*>(src + (off_) + (long)r_ * rstride + (long)(i_ - r_ * upr) * 16); \
    }
#define VC_FR2_STORE(j, val)                                                                     \
    {                                                                                            \
      const int i_ = (j) * NTHR + tid;                                                           \
      if (i_ < total) {                                                                          \
        const int r_ = (sh >= 0) ? (i_ >> sh) : (i_ / upr);                                      \
        *reinterpret_cast<uint4*>(xl + (size_t)r_ * xs + (size_t)(i_ - r_ * upr) * 16) = val;    \
      }                                                                                          \
    }
#define VC_FR2_LOAD_ALL(off_)                                                                    \
    VC_FR2_LOAD(0, x0, off_) VC_FR2_LOAD(1, x1, off_) VC_FR2_LOAD(2, x2, off_) VC_FR2_LOAD(3, x3, off_)         \
    VC_FR2_LOAD(4, x4, off_) VC_FR2_LOAD(5, x5, off_) VC_FR2_LOAD(6, x6, off_) VC_FR2_LOAD(7, x7, off_)         \
    VC_FR2_LOAD(8, x8, off_) VC_FR2_LOAD(9, x9, off_) VC_FR2_LOAD(10, x10, off_) VC_FR2_LOAD(11, x11, off_)     \
    VC_FR2_LOAD(12, x12, off_) VC_FR2_LOAD(13, x13, off_) VC_FR2_LOAD(14, x14, off_) VC_FR2_LOAD(15, x15, off_)
#define VC_FR2_STORE_ALL()                                                                       \
    VC_FR2_STORE(0, x0) VC_FR2_STORE(1, x1) VC_FR2_STORE(2, x2) VC_FR2_STORE(3, x3)               \
    VC_FR2_STORE(4, x4) VC_FR2_STORE(5, x5) VC_FR2_STORE(6, x6) VC_FR2_STORE(7, x7)               \
    VC_FR2_STORE(8, x8) VC_FR2_STORE(9, x9) VC_FR2_STORE(10, x10) VC_FR2_STORE(11, x11)           \
    VC_FR2_STORE(12, x12) VC_FR2_STORE(13, x13) VC_FR2_STORE(14, x14) VC_FR2_STORE(15, x15)
  VC_FR2_LOAD_ALL(0L)
  VC_FR2_BURST
  __builtin_amdgcn_sched_barrier(0);
  if (active == 0) return;
  VC_FR2_STORE_ALL()
  __syncthreads();
  VC_FR2_LOAD_ALL(hoff)                           // second half of the rows: on its way during the first half's MFMAs
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int mrow = (m < a.r_lds) ? m : 0;
  const char* xrow = xl + (size_t)mrow * xs + (size_t)kg * 16 + (size_t)(wave * KTW) * 64;
  static_assert(KTW % GROUP == 0 && GROUP <= 8, "a wave's k-tiles come in whole groups of at most eight");
  // group g of the wave, k-tile J of the group: J is a literal, so that a packed format rebuilds its fragment with compile-time shifts
#define VC_FR2_STEP(h_, J)                                                                                     \
    if constexpr (GROUP > (J)) {                                                                               \
      const uint4 xf = *reinterpret_cast<const uint4*>(xrow + (size_t)(GROUP * g + (J)) * 64);                 \
      VC_FR2_FRAG(h_, J, wfrag)                                                                                \
      acc = mfma_frag(wfrag, xf, acc, (WT*)nullptr);                                                           \
    }
#define VC_FR2_HALF(h_)                                                                                        \
  _Pragma("unroll") for (int g = 0; g < KTW / GROUP; ++g) {                                                    \
    VC_FR2_STEP(h_, 0) VC_FR2_STEP(h_, 1) VC_FR2_STEP(h_, 2) VC_FR2_STEP(h_, 3)                                \
    VC_FR2_STEP(h_, 4) VC_FR2_STEP(h_, 5) VC_FR2_STEP(h_, 6) VC_FR2_STEP(h_, 7)                                \
  }
  VC_FR2_HALF(0)
  __syncthreads();                                // every wave has read the first half
  VC_FR2_STORE_ALL()
  __syncthreads();
  VC_FR2_HALF(1)
#undef VC_FR2_STEP
#undef VC_FR2_HALF
#undef VC_FR2_LOAD
#undef VC_FR2_STORE
#undef VC_FR2_LOAD_ALL
#undef VC_FR2_STORE_ALL
  red[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave == 0 && m < n_rows && nvalid) {
#pragma unroll
    for (int w = 1; w < NW; ++w) acc += red[w * 64 + lane];
    const f32x4 o = {eres.x + eb.x + acc[0], eres.y + eb.y + acc[1], eres.z + eb.z + acc[2], eres.w + eb.w + acc[3]};
    store4(a.h_out + (long)m * a.d + n, o);
    if (a.hq_out) { const f32x4 q = {o[0] - cmu, o[1] - cmu, o[2] - cmu, o[3] - cmu}; store4(reinterpret_cast<WT*>(a.hq_out) + (long)m * a.d + n, q); }
  }
#undef VC_FR2_EARLY
#undef VC_FR2_WDECL
#undef VC_FR2_BURST
#undef VC_FR2_FRAG
