// vc_gemm_fr1_body.h - the body of the one-row paired GEMM kernels, written once.  NOT a header of declarations: it is the text between
// the braces of row_gemm_fr1_k (vc_gemm.hip: bf16 / fp32 image), row_gemm_fr1_w13_k (vc_gemm_w13.hip: exact 13-bit planes) and
// row_gemm_fr1_w8_k (vc_gemm_w8.hip: block-scaled E4M3 bytes), each of which is
//     { <names>  <three hooks>  #include "vc_gemm_fr1_body.h" }
// Why text and not a __device__ __forceinline__ template with a per-format source object: the inliner works bottom-up, so such a body
// is optimised as a function of its own, behind generic pointers, BEFORE it is inlined, and the kernel is optimised a second time
// around it.  That was built first: 31 of the 56 kernels came out with other code (commuted operands, scalar registers renumbered, a
// branch for a select in the non-EXACT forms, four more VGPRs in two of them).  As text every kernel compiles to its earlier code,
// instruction for instruction (profiles/fr1_body_kernel_body_diff.log), which is the whole proof that results and speed are unchanged.
//
// The kernel supplies, in scope:
//   WT, NPW, NW, PRO, EPI   weight type, fragment pairs per wave, waves per workgroup, the form (below)
//   EXACT                   the matrix has exactly NW * NPW fragment pairs per tile: no clamped addresses, no zeroed fragments
//   GROUP                   fragment pairs per group of the format (1, 2 or 4, a divisor of NPW; 1 for an image, and whenever !EXACT)
//   a                       const GemmArgs&
// and three hooks (macros, #undef'd at the end of this file), in program order.  They see the body's tid, lane, wave, nt, m, kg,
// npairs and (from VC_FR1_BURST on) wunit, SPT:
//   VC_FR1_EARLY            statements: what the wave requests BEFORE the epilogue operands (a wave's loads return in order) - the packed
//                           formats' side words, scalar operands first needed long after the burst is out; empty for an image
//   VC_FR1_BURST            statements: the wave's whole share of the weights, everything up front, with the format's own sched_barrier
//                           placement (and the pins that keep the side words in front of the prologue)
//   VC_FR1_FRAG(F, w)       statements that declare uint4 w = fragment pair F (a literal, < GROUP) of the wave's group g, the four dwords
//                           of the MFMA's A operand; gpr = the group's first pair in the tile, beyond the matrix from npairs on
// A new weight format is such a kernel, a packer with its check, and a vc_packed_kind entry (vc_common.h).
//
// ------------------------------------------------------------------ finished-row producer of ONE-row decode steps (round 5)
// The one-row step kept split-K slabs through round 4: the FFN down-projection left 4 fp32 slabs and every one of the 512
// workgroups of the next launch (the following layer's QKV projection) re-summed h + bias + 4 slabs - 40 KB out of L2 per
// workgroup, requested in front of its own 48 KB weight burst.  rows_gemm_fr_k (vc_gemm.hip) finishes rows for 2..16-row steps, but
// its 8-channel tiles fill only half of every MFMA fragment (lanes 8..15 repeat slot 7): twice the vector-memory instructions per
// weight byte, which a one-row step - nothing but a weight stream - cannot afford.  With ONE row the other 15 columns of the B
// operand are free, so a fragment carries TWO k-tiles: A rows 0..7 = the tile's 8 channels over k-tile 2p, rows 8..15 = the same
// channels over k-tile 2p + 1 (the 8-channel image stores consecutive k-tiles of a tile back to back: one contiguous 1 KB
// burst per wave instruction, every lane's 16 bytes used); B column 0 = x over k-tile 2p, column 1 = x over k-tile 2p + 1.
// D[c][0] + D[c + 8][1] is channel c's partial sum; every other element of D is a cross term nobody reads.  A workgroup owns
// 8 channels over the whole K (d/8 workgroups), its 8 waves stream K/8 each in one burst, the row of X is staged once in LDS,
// and the epilogue adds residual + bias and writes the finished channels: the consumer's LayerNorm prologue reads ONE 8 KB row.
// NPW = fragment pairs per wave (K / KW / 16, rounded up; pairs beyond the matrix are zeroed).
// NW waves per workgroup, each streaming NPW consecutive fragment pairs (KB) in one burst.
// PRO_PLAIN / EPI_RES (the FFN down-projection): X = a.x_in (WT [K]), h_out = h_in + bias + W x.
// PRO_LN / EPI_QKV (the QKV projection behind a FINISHED row, option "qkv_p8"): X = the row of h_in, centred and rounded (LayerNorm
//   fold, rows_gemm_k in vc_gemm.hip), epilogue = rstd / mean correction + folded bias, q to a buffer, K / V into the cache.  The
//   12-channel tiles of rows_gemm_k leave a quarter of every fragment's lanes idle: the QKV launch pays the vector-memory instructions
//   of a 33.6 MB stream for 25.2 MB; here every lane's 16 bytes are weights (3d / 8 workgroups: three per CU at d = 2048).
// (A third form - the FFN up-projection on its ordinary 16-channel tiles with this kernel's lean code, LayerNorm fold of h + bias + two
// slabs - was built at the end of round 5 on the reading that straight-line code in front of the burst is paid in instruction fetch
// at every cold launch start: its first workgroup had the burst out after 2 000 clk instead of 2 756, and the step came out
// +0.84 % +- 0.44 at giga830M, +0.21 % +- 0.06 at giga330M in in-process A/Bs, profiles/r05g_ab_*.log.  Not carried: the FFN-up
// launch is bound by its stream, not by its prologue.)
  using T = WTr<WT>;
  static_assert((PRO == PRO_PLAIN && EPI == EPI_RES) || (PRO == PRO_LN && EPI == EPI_QKV), "one-row paired forms");
  constexpr int NTHR = 64 * NW, TH = VC_TH_RES, SPT = 4 * TH;   // SPT = 16-byte units per (tile, k-tile) = 32
  extern __shared__ __attribute__((aligned(16))) char smem[];
  VC_KTS_DECL();
  VC_KTS(0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x;
  const int K = a.K;
  const int npairs = a.KT >> 1;                    // KT even (host contract)
  char* xl = smem;                                 // the row: K elements of WT
  f32x4* red = reinterpret_cast<f32x4*>(smem + (size_t)K * sizeof(WT));     // [NW][4] partial quads
  float* stat = reinterpret_cast<float*>(red + NW * 4);                     // PRO_LN: [NW] row sums, then [NW][2] statistics of the rounded row
  const int active = *a.n_active;
  const int m = lane & 15, kg = lane >> 4;
  VC_FR1_EARLY
  // epilogue operands first (a wave's loads return in order): for the two finishing threads, channels 4 t .. 4 t + 3 of the tile
  const int nfin = nt * TH + 4 * (tid & 1);
  float4 eres = make_float4(0.f, 0.f, 0.f, 0.f), ewg = eres;
  const float4 eb = *reinterpret_cast<const float4*>(a.bias + nfin);
  int epos = -1, eseq = 0;
  if constexpr (EPI == EPI_RES) eres = *reinterpret_cast<const float4*>(a.h_in + nfin);
  else { ewg = *reinterpret_cast<const float4*>(a.wg + nfin); epos = a.row_pos[0]; eseq = a.row_seq[0]; }
  // the operand row: PLAIN - 16-byte units of X (a fragment pair covers 64 of them); LN - float4 columns of the residual row
  // (a fragment pair = two k-tiles = 128 bytes of WT = 8 units; K = NW * NPW pairs when EXACT)
  constexpr int NXU = (NPW * 8 + 63) / 64;                               // 16-byte units of the WT row per thread
  constexpr int NXQ = ((sizeof(WT) == 2 ? 16 : 8) * NPW + 63) / 64;      // float4 columns of the fp32 row per thread
  static_assert(NXU <= 4 && (PRO != PRO_LN || NXQ <= 4), "the operand row fits four staging registers per thread");
  const int units = K * (int)sizeof(WT) / 16, nq = K >> 2;
  // (explicit scalars: an indexed array is demoted to scratch memory by the compiler)
  uint4 xu0 = make_uint4(0u, 0u, 0u, 0u), xu1 = xu0, xu2 = xu0, xu3 = xu0;
  float4 xq0 = make_float4(0.f, 0.f, 0.f, 0.f), xq1 = xq0, xq2 = xq0, xq3 = xq0;
  if constexpr (PRO == PRO_PLAIN) {
    const char* src = reinterpret_cast<const char*>(a.x_in);
#define VC_FR1_XLOAD(j, dst) if constexpr (NXU > (j)) dst = *reinterpret_cast<const uint4*>(src + (size_t)min(tid + (j) * NTHR, units - 1) * 16);
    VC_FR1_XLOAD(0, xu0) VC_FR1_XLOAD(1, xu1) VC_FR1_XLOAD(2, xu2) VC_FR1_XLOAD(3, xu3)
#undef VC_FR1_XLOAD
  } else {
#define VC_FR1_QLOAD(j, dst) if constexpr (NXQ > (j)) dst = *reinterpret_cast<const float4*>(a.h_in + (size_t)min(tid + (j) * NTHR, nq - 1) * 4);
    VC_FR1_QLOAD(0, xq0) VC_FR1_QLOAD(1, xq1) VC_FR1_QLOAD(2, xq2) VC_FR1_QLOAD(3, xq3)
#undef VC_FR1_QLOAD
  }
  // the wave's whole share of the weights in one burst: pair p of wave w = fragment pair (NPW w + p)
  const int wunit = (m >> 3) * SPT + kg * TH + (m & 7);
  VC_FR1_BURST
  if (active == 0) return;
  VC_KTS(1);
  if constexpr (PRO == PRO_PLAIN) {
#define VC_FR1_XPARK(j, val) if constexpr (NXU > (j)) { if (tid + (j) * NTHR < units) *reinterpret_cast<uint4*>(xl + (size_t)(tid + (j) * NTHR) * 16) = val; }
    VC_FR1_XPARK(0, xu0) VC_FR1_XPARK(1, xu1) VC_FR1_XPARK(2, xu2) VC_FR1_XPARK(3, xu3)
#undef VC_FR1_XPARK
  } else {
    // LayerNorm fold of the finished row (see the top of vc_gemm.hip): centred BEFORE it is rounded, statistics of the rounded values
    float t = 0.f;
#define VC_FR1_QSUM(j, v) if constexpr (NXQ > (j)) { if (tid + (j) * NTHR < nq) t += (v.x + v.y) + (v.z + v.w); }
    VC_FR1_QSUM(0, xq0) VC_FR1_QSUM(1, xq1) VC_FR1_QSUM(2, xq2) VC_FR1_QSUM(3, xq3)
#undef VC_FR1_QSUM
    t = wave_sum(t);
    if (lane == 0) stat[wave] = t;
    __syncthreads();
    float mu = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) mu += stat[w];
    mu *= 1.0f / (float)K;
    float s1 = 0.f, s2 = 0.f;
    WT* xr = reinterpret_cast<WT*>(xl);
#define VC_FR1_QPARK(j, v)                                                                     \
    if constexpr (NXQ > (j)) {                                                                 \
      if (tid + (j) * NTHR < nq) {                                                             \
        const f32x4 y_ = {v.x - mu, v.y - mu, v.z - mu, v.w - mu};                             \
        const f32x4 q_ = store4r(xr + (size_t)(tid + (j) * NTHR) * 4, y_);                     \
        s1 += (q_[0] + q_[1]) + (q_[2] + q_[3]);                                               \
        s2 += (q_[0] * q_[0] + q_[1] * q_[1]) + (q_[2] * q_[2] + q_[3] * q_[3]);               \
      }                                                                                        \
    }
    VC_FR1_QPARK(0, xq0) VC_FR1_QPARK(1, xq1) VC_FR1_QPARK(2, xq2) VC_FR1_QPARK(3, xq3)
#undef VC_FR1_QPARK
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) { stat[NW + 2 * wave] = s1; stat[NW + 2 * wave + 1] = s2; }
  }
  VC_KTS(2);
  __syncthreads();
  VC_KTS(3);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // B operand: column m = 0 reads x over k-tile 2 gp, column 1 over k-tile 2 gp + 1 (the other columns repeat these: cross terms)
  const char* xcol = xl + ((size_t)(m & 1) * T::KW + (size_t)kg * T::EPL) * sizeof(WT);
  static_assert(NPW % GROUP == 0 && GROUP <= 4 && (EXACT || GROUP == 1), "a wave's pairs come in whole groups of at most four");
  // group g of the wave, pair F of the group: F is a literal, so that a packed format rebuilds its fragment with compile-time shifts
#pragma unroll
  for (int g = 0; g < NPW / GROUP; ++g) {
    const int gpr = NPW * wave + GROUP * g;
    const int gp = EXACT ? gpr : min(gpr, npairs - 1);
#define VC_FR1_STEP(F)                                                                                          \
    if constexpr (GROUP > (F)) {                                                                                \
      const uint4 xf = *reinterpret_cast<const uint4*>(xcol + (size_t)(gp + (F)) * (2 * T::KW * sizeof(WT)));   \
      VC_FR1_FRAG(F, wfrag)                                                                                     \
      acc = mfma_frag(wfrag, xf, acc, (WT*)nullptr);                                                            \
    }
    VC_FR1_STEP(0) VC_FR1_STEP(1) VC_FR1_STEP(2) VC_FR1_STEP(3)
#undef VC_FR1_STEP
  }
  // D[n = 4 kg + r][m]: channels 0..3 / 4..7 over the even k-tiles sit in lanes (m = 0, kg = 0 / 1), over the odd ones in lanes
  // (m = 1, kg = 2 / 3): four quads per wave
  VC_KTS(4);
  if (m == (kg >> 1) && m < 2) red[wave * 4 + kg] = acc;
  __syncthreads();
  VC_KTS(5);
  if (tid < 2) {             // thread t finishes channels 4 t .. 4 t + 3: quads t and t + 2 of every wave, in a fixed order
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < NW; ++w) sum += red[w * 4 + tid] + red[w * 4 + tid + 2];
    if constexpr (EPI == EPI_RES) {
      const f32x4 o = {eres.x + eb.x + sum[0], eres.y + eb.y + sum[1], eres.z + eb.z + sum[2], eres.w + eb.w + sum[3]};
      store4(a.h_out + nfin, o);
    } else {
      float q1 = 0.f, q2 = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) { q1 += stat[NW + 2 * w]; q2 += stat[NW + 2 * w + 1]; }
      const float inv_d = 1.0f / (float)K;
      const float mean = q1 * inv_d;
      const float var = fmaxf(q2 * inv_d - mean * mean, 0.f);
      const float rstd = 1.0f / sqrtf(var + 1e-5f);      // eps 1e-5 (transformer.py:30)
      sum[0] = rstd * (sum[0] - mean * ewg.x); sum[1] = rstd * (sum[1] - mean * ewg.y);
      sum[2] = rstd * (sum[2] - mean * ewg.z); sum[3] = rstd * (sum[3] - mean * ewg.w);
      gemm_epilogue<WT, EPI_QKV>(a, sum, 0, nfin, 0, 0, 1, eb, epos, eseq);
    }
  }
  VC_KTS(6);
  VC_KTS_FLUSH();
#undef VC_FR1_EARLY
#undef VC_FR1_BURST
#undef VC_FR1_FRAG
