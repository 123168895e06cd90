// vc_gemm_frp_body.h - the body of the paired finished-row producer of 2..8-row steps, written once.  NOT a header of declarations: it
// is the text between the braces of rows_gemm_frp_k (vc_gemm.hip: bf16 / fp32 image) and rows_gemm_frp_w8_k (vc_gemm_w8.hip:
// block-scaled E4M3 bytes), in the manner of vc_gemm_fr1_body.h (which says why this is text and not a function template).
//
// The kernel supplies, in scope:
//   WT, NPW, RMAX           weight type, fragment pairs per wave, rows the staging is unrolled for (4 or 8)
//   GROUP                   fragment pairs per group of the format (1 for an image, 4 for the E4M3 bytes; a divisor of NPW)
//   a                       const GemmArgs&
// and three hooks (macros, #undef'd at the end of this file), in program order.  They see the body's tid, lane, wave, nt, m, kg and
// (from VC_FRP_BURST on) wunit, SPT:
//   VC_FRP_EARLY            statements: what the wave requests with n_active, BEFORE the epilogue operands (a wave's loads return in
//                           order) - a packed format's side words; empty for an image
//   VC_FRP_BURST            statements: the wave's whole share of the weights, everything up front, with the format's own sched_barrier
//   VC_FRP_FRAG(F, w)       statements that declare uint4 w = fragment pair F (a literal, < GROUP) of the wave's group g, the four dwords
//                           of the MFMA's A operand
//
// ------------------------------------------------------------------ finished-row producer of 2..8-row steps, paired (round 5)
// The same two-k-tiles-per-fragment trick for up to EIGHT rows: the B operand has 16 columns, so row r takes columns 2r (x over
// k-tile 2p) and 2r + 1 (x over k-tile 2p + 1); D[c][2r] + D[c + 8][2r + 1] is channel c of row r.  rows_gemm_fr_k (vc_gemm.hip) issues one
// 512-byte fragment per wave instruction for the same 8-channel tiles; here every instruction is a full KB - half the vector-memory
// instructions of the FFN down-projection of config 5's per-GPU share (8 rows).  X rows sit in LDS at r K + 16 (r & 3) + 128 (r >> 2)
// bytes, so that the sixteen 16-byte reads of a lane group (8 rows x 2 k-tile parities) fall into sixteen different bank quads.
// RMAX = rows the staging is unrolled for (4 or 8); K x sizeof(WT) / 16 is a power of two (host contract).
  using T = WTr<WT>;
  constexpr int NW = VC_FR_WAVES, NTHR = 64 * NW, TH = VC_TH_RES, SPT = 4 * TH;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x;
  const int n_rows = a.n_rows;                      // 2..RMAX (host contract)
  const int Kb = a.K * (int)sizeof(WT);             // bytes of one X row = NW * NPW * 128
  char* xl = smem;
  f32x4* red = reinterpret_cast<f32x4*>(smem + (size_t)RMAX * Kb + 256);      // [NW][RMAX][4]
  const int active = *a.n_active;
  const int m = lane & 15, kg = lane >> 4;
  VC_FRP_EARLY
  // epilogue operands first: thread t < 2 RMAX finishes channels 4 (t & 1) .. of row t >> 1
  const int frow = min(tid >> 1, n_rows - 1);
  const int nfin = nt * TH + 4 * (tid & 1);
  const float4 eres = *reinterpret_cast<const float4*>(a.h_in + (long)frow * a.d + nfin);
  const float4 eb = *reinterpret_cast<const float4*>(a.bias + nfin);
  const float cmu = a.row_mu[frow] + a.mu_shift;
  // X rows as 16-byte units, flat index = row * upr + unit; RMAX * NPW / 8 units per thread
  constexpr int NXU = RMAX * ((NPW * 8 + 63) / 64);
  const int ush = a.x_upr_shift;                    // log2(units per row)
  const int upr = 1 << ush, total = n_rows * upr;
  const char* src = reinterpret_cast<const char*>(a.x_in);
  const long rstride = (long)a.x_ld * (long)sizeof(WT);
  // (explicit scalars: an indexed array is demoted to scratch memory by the compiler)
  uint4 x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, x10, x11, x12, x13, x14, x15;
  static_assert(NXU <= 16, "staging registers per thread");
#define VC_FRP_LOAD(j, dst)                                                                      \
  if constexpr (NXU > (j)) {                                                                     \
    const int i_ = min(tid + (j) * NTHR, total - 1);                                             \
    const int r_ = i_ >> ush;                                                                    \
    dst = *reinterpret_cast<const uint4*>(src + (long)r_ * rstride + (long)(i_ - (r_ << ush)) * 16); \
  }
#define VC_FRP_PARK(j, val)                                                                      \
  if constexpr (NXU > (j)) {                                                                     \
    const int i_ = tid + (j) * NTHR;                                                             \
    if (i_ < total) {                                                                            \
      const int r_ = i_ >> ush;                                                                  \
      *reinterpret_cast<uint4*>(xl + (size_t)r_ * Kb + 16 * (r_ & 3) + 128 * (r_ >> 2) + (size_t)(i_ - (r_ << ush)) * 16) = val; \
    }                                                                                            \
  }
  VC_FRP_LOAD(0, x0) VC_FRP_LOAD(1, x1) VC_FRP_LOAD(2, x2) VC_FRP_LOAD(3, x3) VC_FRP_LOAD(4, x4) VC_FRP_LOAD(5, x5) VC_FRP_LOAD(6, x6) VC_FRP_LOAD(7, x7)
  VC_FRP_LOAD(8, x8) VC_FRP_LOAD(9, x9) VC_FRP_LOAD(10, x10) VC_FRP_LOAD(11, x11) VC_FRP_LOAD(12, x12) VC_FRP_LOAD(13, x13) VC_FRP_LOAD(14, x14) VC_FRP_LOAD(15, x15)
  const int wunit = (m >> 3) * SPT + kg * TH + (m & 7);
  VC_FRP_BURST
  if (active == 0) return;
  VC_FRP_PARK(0, x0) VC_FRP_PARK(1, x1) VC_FRP_PARK(2, x2) VC_FRP_PARK(3, x3) VC_FRP_PARK(4, x4) VC_FRP_PARK(5, x5) VC_FRP_PARK(6, x6) VC_FRP_PARK(7, x7)
  VC_FRP_PARK(8, x8) VC_FRP_PARK(9, x9) VC_FRP_PARK(10, x10) VC_FRP_PARK(11, x11) VC_FRP_PARK(12, x12) VC_FRP_PARK(13, x13) VC_FRP_PARK(14, x14) VC_FRP_PARK(15, x15)
#undef VC_FRP_LOAD
#undef VC_FRP_PARK
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int rl = min(m >> 1, n_rows - 1);           // (columns of rows the pass does not have repeat the last row: cross terms)
  const char* xcol = xl + (size_t)rl * Kb + 16 * (rl & 3) + 128 * (rl >> 2) + ((size_t)(m & 1) * T::KW + (size_t)kg * T::EPL) * sizeof(WT);
  static_assert(NPW % GROUP == 0 && GROUP <= 4, "a wave's pairs come in whole groups of at most four");
  // group g of the wave, pair F of the group: F is a literal, so that a packed format rebuilds its fragment with compile-time shifts
#pragma unroll
  for (int g = 0; g < NPW / GROUP; ++g) {
    const int gp = NPW * wave + GROUP * g;
#define VC_FRP_STEP(F)                                                                                          \
    if constexpr (GROUP > (F)) {                                                                                \
      const uint4 xf = *reinterpret_cast<const uint4*>(xcol + (size_t)(gp + (F)) * (2 * T::KW * sizeof(WT)));   \
      VC_FRP_FRAG(F, wfrag)                                                                                     \
      acc = mfma_frag(wfrag, xf, acc, (WT*)nullptr);                                                            \
    }
    VC_FRP_STEP(0) VC_FRP_STEP(1) VC_FRP_STEP(2) VC_FRP_STEP(3)
#undef VC_FRP_STEP
  }
  // D[n = 4 kg + r][m]: row m >> 1; even columns hold the even k-tiles' channels 0..7 (kg 0 / 1), odd columns the odd k-tiles' (kg 2 / 3)
  if ((m & 1) == (kg >> 1) && (m >> 1) < n_rows) red[(wave * RMAX + (m >> 1)) * 4 + kg] = acc;
  __syncthreads();
  if (tid < 2 * n_rows) {
    const int r = tid >> 1, half = tid & 1;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < NW; ++w) sum += red[(w * RMAX + r) * 4 + half] + red[(w * RMAX + r) * 4 + half + 2];
    const f32x4 o = {eres.x + eb.x + sum[0], eres.y + eb.y + sum[1], eres.z + eb.z + sum[2], eres.w + eb.w + sum[3]};
    store4(a.h_out + (long)r * a.d + nfin, o);
    if (a.hq_out) { const f32x4 q = {o[0] - cmu, o[1] - cmu, o[2] - cmu, o[3] - cmu}; store4(reinterpret_cast<WT*>(a.hq_out) + (long)r * a.d + nfin, q); }
  }
#undef VC_FRP_EARLY
#undef VC_FRP_BURST
#undef VC_FRP_FRAG
