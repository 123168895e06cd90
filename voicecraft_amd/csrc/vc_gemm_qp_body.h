// vc_gemm_qp_body.h - the body of the paired QKV consumer of 2..8 finished rows, written once.  NOT a header of declarations: it is the
// text between the braces of rows_gemm_qp_k (vc_gemm.hip: bf16 / fp32 image) and rows_gemm_qp_w8_k (vc_gemm_w8.hip: block-scaled E4M3
// bytes), in the manner of vc_gemm_fr1_body.h (which says why this is text and not a function template).  What the kernel computes and
// why it is laid out this way stands in front of rows_gemm_qp_k.
//
// The kernel supplies, in scope:
//   WT, NPW, RMAX           weight type, fragment pairs per wave AND TILE, rows (4 or 8)
//   GROUP                   fragment pairs per group of the format (1 for an image, 4 for the E4M3 bytes; a divisor of NPW)
//   a                       const GemmArgs&
// and three hooks (macros, #undef'd at the end of this file), in program order.  They see the body's tid, lane, wave, m, kg, NTQ and
// (from VC_QP_BURST on) wunit, SPT:
//   VC_QP_EARLY             statements: what the wave requests with n_active, BEFORE the epilogue operands (a wave's loads return in
//                           order) - a packed format's side words; empty for an image
//   VC_QP_BURST             statements: the wave's share of its three tiles, everything up front, tile by tile, with the format's own
//                           sched_barrier
//   VC_QP_FRAG(t, F, w)     statements that declare uint4 w = fragment pair F (a literal, < GROUP) of group g of tile t, the four dwords
//                           of the MFMA's A operand
  using T = WTr<WT>;
  constexpr int NW = VC_FR_WAVES, TH = VC_TH_RES, SPT = 4 * TH, NTQ = 3;
  constexpr int E16 = 16 / (int)sizeof(WT);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_rows = a.n_rows;                      // 2..RMAX (host contract)
  const int Kb = a.K * (int)sizeof(WT);             // bytes of one row = NPW * 1024
  char* xl = smem;
  f32x4* red = reinterpret_cast<f32x4*>(smem + (size_t)RMAX * Kb + 256);      // [NW][RMAX][NTQ][4]
  float* stat = reinterpret_cast<float*>(red + NW * RMAX * NTQ * 4);         // [RMAX][2]: sum and sum of squares of the row's copy
  const int active = *a.n_active;
  const int m = lane & 15, kg = lane >> 4;
  VC_QP_EARLY
  // epilogue operands first (a wave's loads return in order): thread t < 6 n_rows finishes channels 4 (t & 1) .. of tile (t >> 1) % 3 of row t / 6
  const int frow = min(tid / (2 * NTQ), n_rows - 1);
  const int ftile = (tid >> 1) % NTQ;
  const int nfin = ((int)blockIdx.x * NTQ + ftile) * TH + 4 * (tid & 1);
  const float4 eb = *reinterpret_cast<const float4*>(a.bias + nfin);
  const float4 ewg = *reinterpret_cast<const float4*>(a.wg + nfin);
  const int epos = a.row_pos[frow], eseq = a.row_seq[frow];
  // wave r < n_rows: row r of the centred copy, NPW requests of 1 KB
  const int xrow = min(wave, n_rows - 1);
  const char* qsrc = reinterpret_cast<const char*>(a.x_in) + (long)xrow * a.x_ld * (long)sizeof(WT);
  const float cmu = a.row_mu[xrow] + a.mu_shift;
  uint4 xq[NPW];
#pragma unroll
  for (int j = 0; j < NPW; ++j) xq[j] = *reinterpret_cast<const uint4*>(qsrc + (j * 64 + lane) * 16);
  const int wunit = (m >> 3) * SPT + kg * TH + (m & 7);
  VC_QP_BURST
  if (active == 0) return;
  if (wave < n_rows) {
    char* xr = xl + (size_t)wave * Kb + 16 * (wave & 3) + 128 * (wave >> 2);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NPW; ++j) {
      *reinterpret_cast<uint4*>(xr + (j * 64 + lane) * 16) = xq[j];
      float f[E16];
      if constexpr (sizeof(WT) == 2) {
        f[0] = __uint_as_float(xq[j].x << 16); f[1] = __uint_as_float(xq[j].x & 0xffff0000u);
        f[2] = __uint_as_float(xq[j].y << 16); f[3] = __uint_as_float(xq[j].y & 0xffff0000u);
        f[4] = __uint_as_float(xq[j].z << 16); f[5] = __uint_as_float(xq[j].z & 0xffff0000u);
        f[6] = __uint_as_float(xq[j].w << 16); f[7] = __uint_as_float(xq[j].w & 0xffff0000u);
      } else {
        f[0] = __uint_as_float(xq[j].x); f[1] = __uint_as_float(xq[j].y);
        f[2] = __uint_as_float(xq[j].z); f[3] = __uint_as_float(xq[j].w);
      }
#pragma unroll
      for (int e = 0; e < E16; e += 4) {
        s1 += (f[e] + f[e + 1]) + (f[e + 2] + f[e + 3]);
        s2 += (f[e] * f[e] + f[e + 1] * f[e + 1]) + (f[e + 2] * f[e + 2] + f[e + 3] * f[e + 3]);
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
      stat[2 * wave] = s1; stat[2 * wave + 1] = s2;
      if (a.row_mu_out && blockIdx.x == 0) a.row_mu_out[wave] = cmu + s1 * (1.0f / (float)a.K);      // the next producer centres its copy of the row on it
    }
  }
  __syncthreads();
  f32x4 acc[NTQ];
#pragma unroll
  for (int t = 0; t < NTQ; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int rl = min(m >> 1, n_rows - 1);           // (columns of rows the pass does not have repeat the last row: cross terms)
  const char* xcol = xl + (size_t)rl * Kb + 16 * (rl & 3) + 128 * (rl >> 2) + ((size_t)(m & 1) * T::KW + (size_t)kg * T::EPL) * sizeof(WT);
  static_assert(NPW % GROUP == 0 && GROUP <= 4, "a wave's pairs come in whole groups of at most four");
  // group g of the wave, pair F of the group: F is a literal, so that a packed format rebuilds its fragments with compile-time shifts
#pragma unroll
  for (int g = 0; g < NPW / GROUP; ++g) {
    const int gp = NPW * wave + GROUP * g;
#define VC_QP_STEP(F)                                                                                           \
    if constexpr (GROUP > (F)) {                                                                                \
      const uint4 xf = *reinterpret_cast<const uint4*>(xcol + (size_t)(gp + (F)) * (2 * T::KW * sizeof(WT)));   \
      _Pragma("unroll") for (int t = 0; t < NTQ; ++t) {                                                         \
        VC_QP_FRAG(t, F, wfrag)                                                                                 \
        acc[t] = mfma_frag(wfrag, xf, acc[t], (WT*)nullptr);                                                    \
      }                                                                                                         \
    }
    VC_QP_STEP(0) VC_QP_STEP(1) VC_QP_STEP(2) VC_QP_STEP(3)
#undef VC_QP_STEP
  }
  // D[n = 4 kg + r][m]: row m >> 1; even columns hold the even k-tiles' channels 0..7 (kg 0 / 1), odd columns the odd k-tiles' (kg 2 / 3)
  if ((m & 1) == (kg >> 1) && (m >> 1) < n_rows) {
#pragma unroll
    for (int t = 0; t < NTQ; ++t) red[((wave * RMAX + (m >> 1)) * NTQ + t) * 4 + kg] = acc[t];
  }
  __syncthreads();
  if (tid < 2 * NTQ * n_rows) {
    const int half = tid & 1;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < NW; ++w) sum += red[((w * RMAX + frow) * NTQ + ftile) * 4 + half] + red[((w * RMAX + frow) * NTQ + ftile) * 4 + half + 2];
    const float inv_d = 1.0f / (float)a.K;
    const float mean = stat[2 * frow] * inv_d;
    const float var = fmaxf(stat[2 * frow + 1] * inv_d - mean * mean, 0.f);
    const float rstd = 1.0f / sqrtf(var + 1e-5f);      // eps 1e-5 (transformer.py:30)
    sum[0] = rstd * (sum[0] - mean * ewg.x); sum[1] = rstd * (sum[1] - mean * ewg.y);
    sum[2] = rstd * (sum[2] - mean * ewg.z); sum[3] = rstd * (sum[3] - mean * ewg.w);
    gemm_epilogue<WT, EPI_QKV>(a, sum, frow, nfin, 0, 0, 1, eb, epos, eseq);
  }
#undef VC_QP_EARLY
#undef VC_QP_BURST
#undef VC_QP_FRAG
