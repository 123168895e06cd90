// vc_gemm_w13.hip - one-row decode on weights stored as exact 13-bit planes ("w13", vc_w13.h).
//
// A one-row step is a weight stream: every big launch fits t = 2.2 .. 2.5 us + bytes / 6.1 TB/s, and while the stream runs
// the CUs idle.  The planes carry the same bf16 values in 13/16 of the bytes; the kernels below are row_gemm_fr1_k (vc_gemm.hip) with the
// weight burst replaced: per group of four fragments a wave requests two KB of low bytes, one KB of exponent codes and 256 bytes of
// signs, contiguous per request (non-temporal, everything up front), and rebuilds each fragment's four dwords in registers right in
// front of its MFMA.  (The group base is wave-uniform, but only group 0 is addressed from SGPRs in the compiled code: a group is 3 328
// bytes, past the immediate offset field, so groups 1.. carry a 64-bit VGPR address add between their requests - the bf16 twins have none.)
// No data-dependent branch, no dependent load: the side bytes are wave-uniform and on their way with the burst.
// Prologue, epilogue and summation order are the bf16 kernels', the MFMA operands are bit-identical, so every result is.
// Measured at giga830M (one row, 654 steps, in-process A/B of option w13, profiles/w13_ab.log): see DESIGN section 4.6.
// The packer and its check run once per matrix at creation (vc_engine.hip pack_w13): a matrix with a fragment the codes cannot hold,
// or whose planes do not decode to the image bit for bit, keeps its bf16 kernel.
#include "vc_gemm_dev.h"
#include "vc_w13.h"

// ------------------------------------------------------------------ packing (creation time)
// One wave per group: image = consecutive 1 KB fragments (any tile shape), unit u of fragment F at img[64 F + u].
// counts[0] += fragments refused.
__global__ __launch_bounds__(64) void w13_pack_k(const uint4* __restrict__ img, uint4* __restrict__ planes,
                                                  unsigned char* __restrict__ side, unsigned int* __restrict__ counts) {
  const long G = blockIdx.x;
  const int u = threadIdx.x;
  uint32_t w[4][4];
  int base[4], refused = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const uint4 v = img[(G * 4 + f) * 64 + u];
    w[f][0] = v.x; w[f][1] = v.y; w[f][2] = v.z; w[f][3] = v.w;
    int mn, mx, ok;
    vc_w13_minmax(w[f], &mn, &mx);
    mn = wave_min_i(mn);
    mx = -wave_min_i(-mx);
    base[f] = vc_w13_base(mn, mx, &ok);
    refused += ok ? 0 : 1;
  }
  vc_w13_lane L;
  vc_w13_encode(w, base, &L);
  uint4* gp = planes + G * VC_W13_GROUP_U4;
  gp[u] = make_uint4(L.lo[0], L.lo[1], L.lo[2], L.lo[3]);
  gp[64 + u] = make_uint4(L.lo[4], L.lo[5], L.lo[6], L.lo[7]);
  gp[128 + u] = make_uint4(L.nib[0], L.nib[1], L.nib[2], L.nib[3]);
  reinterpret_cast<uint32_t*>(gp + 192)[u] = L.sign;
  if (u < 4) side[G * 4 + u] = (unsigned char)(u == 0 ? base[0] : u == 1 ? base[1] : u == 2 ? base[2] : base[3]);
  if (u == 0 && refused) atomicAdd(counts, (unsigned int)refused);
}
// counts[1] += dwords that do not decode to the image's
__global__ __launch_bounds__(64) void w13_check_k(const uint4* __restrict__ img, const uint4* __restrict__ planes,
                                                   const unsigned char* __restrict__ side, unsigned int* __restrict__ counts) {
  const long G = blockIdx.x;
  const int u = threadIdx.x;
  const uint4* gp = planes + G * VC_W13_GROUP_U4;
  const uint4 la = gp[u], lb = gp[64 + u], nb = gp[128 + u];
  vc_w13_lane L = {{la.x, la.y, la.z, la.w, lb.x, lb.y, lb.z, lb.w}, {nb.x, nb.y, nb.z, nb.w}, reinterpret_cast<const uint32_t*>(gp + 192)[u]};
  int bad = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    uint32_t w[4];
    vc_w13_decode_frag(&L, f, side[G * 4 + f], w);
    const uint4 v = img[(G * 4 + f) * 64 + u];
    bad += (w[0] != v.x) + (w[1] != v.y) + (w[2] != v.z) + (w[3] != v.w);
  }
  bad = wave_sum_i(bad);
  if (u == 0 && bad) atomicAdd(counts + 1, (unsigned int)bad);
}
// Packs `n_frags` fragments (a multiple of four) of a bf16 image and checks the planes against it; counts = two device words, zeroed here.
hipError_t vc_launch_w13_pack(const uint4* img, long n_frags, uint4* planes, unsigned char* side, unsigned int* counts, hipStream_t s) {
  if (n_frags <= 0 || n_frags % VC_W13_GROUP_FRAGS != 0 || n_frags / VC_W13_GROUP_FRAGS > 0x7fffffffL) return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(counts, 0, 2 * sizeof(unsigned int), s);
  if (err != hipSuccess) return err;
  const unsigned int groups = (unsigned int)(n_frags / VC_W13_GROUP_FRAGS);
  hipLaunchKernelGGL(w13_pack_k, dim3(groups), dim3(64), 0, s, img, planes, side, counts);
  hipLaunchKernelGGL(w13_check_k, dim3(groups), dim3(64), 0, s, img, (const uint4*)planes, (const unsigned char*)side, counts);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the one-row paired kernel on the planes
struct W13Args {
  GemmArgs g;
  const uint4* planes;      // groups in image order (VC_W13_GROUP_U4 units each)
  const uint32_t* side;     // one byte per fragment, four per word = one word per group
};

// fragment F of a group from the lane's plane registers
template <int F>
__device__ __forceinline__ uint4 w13_frag(const uint4& la, const uint4& lb, const uint4& nb, uint32_t sg, uint32_t sidew) {
  const uint32_t bm1 = vc_w13_bm1((sidew >> (8 * F)) & 0xffu);
  const uint32_t l0 = F == 0 ? la.x : F == 1 ? la.z : F == 2 ? lb.x : lb.z;
  const uint32_t l1 = F == 0 ? la.y : F == 1 ? la.w : F == 2 ? lb.y : lb.w;
  const uint32_t n = F == 0 ? nb.x : F == 1 ? nb.y : F == 2 ? nb.z : nb.w;
  uint4 w;
  vc_w13_decode_half(l0, n, sg, 2 * F, bm1, &w.x, &w.y);
  vc_w13_decode_half(l1, n, sg, 2 * F + 1, bm1, &w.z, &w.w);
  return w;
}

// row_gemm_fr1_k<bf16_t, 4 NG, EXACT, NW, PRO, EPI> (vc_gemm.hip; see there for the tile and fragment-pair arithmetic) with the wave's
// NG groups of planes in place of its 4 NG fragments.
template <int NG, int NW, int PRO, int EPI>
__global__ __launch_bounds__(64 * NW) void row_gemm_fr1_w13_k(const W13Args wa) {
  using WT = bf16_t;
  using T = WTr<WT>;
  static_assert((PRO == PRO_PLAIN && EPI == EPI_RES) || (PRO == PRO_LN && EPI == EPI_QKV), "one-row paired forms");
  constexpr int NPW = 4 * NG;
  constexpr int NTHR = 64 * NW, TH = VC_TH_RES, SPT = 4 * TH;
  const GemmArgs& a = wa.g;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  VC_KTS_DECL();
  VC_KTS(0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt = blockIdx.x;
  const int K = a.K;
  char* xl = smem;                                 // the row: K elements of WT
  f32x4* red = reinterpret_cast<f32x4*>(smem + (size_t)K * sizeof(WT));     // [NW][4] partial quads
  float* stat = reinterpret_cast<float*>(red + NW * 4);                     // PRO_LN: [NW] row sums, then [NW][2] statistics of the rounded row
  const int active = *a.n_active;
  const int m = lane & 15, kg = lane >> 4;
  // the wave's side bytes: scalar operands, first needed long after the burst is out
  const long G0 = ((long)nt * NW + wave) * NG;     // the matrix has exactly NW * NG groups per tile (host contract)
  uint32_t sb[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) sb[g] = wa.side[G0 + g];
  const int nfin = nt * TH + 4 * (tid & 1);
  float4 eres = make_float4(0.f, 0.f, 0.f, 0.f), ewg = eres;
  const float4 eb = *reinterpret_cast<const float4*>(a.bias + nfin);
  int epos = -1, eseq = 0;
  if constexpr (EPI == EPI_RES) eres = *reinterpret_cast<const float4*>(a.h_in + nfin);
  else { ewg = *reinterpret_cast<const float4*>(a.wg + nfin); epos = a.row_pos[0]; eseq = a.row_seq[0]; }
  constexpr int NXU = (NPW * 8 + 63) / 64;                               // 16-byte units of the WT row per thread
  constexpr int NXQ = (16 * NPW + 63) / 64;                              // float4 columns of the fp32 row per thread
  static_assert(NXU <= 4 && (PRO != PRO_LN || NXQ <= 4), "the operand row fits four staging registers per thread");
  const int units = K * (int)sizeof(WT) / 16, nq = K >> 2;
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
  // the wave's whole share of the planes in one burst, group by group (loads return in order: group g decodes while g + 1.. land)
  const int wunit = (m >> 3) * SPT + kg * TH + (m & 7);
  const uint4* gbase = wa.planes + G0 * VC_W13_GROUP_U4;                 // wave-uniform
  uint4 la[NG], lb[NG], nb[NG];
  uint32_t sg[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const uint4* gp = gbase + g * VC_W13_GROUP_U4;
    la[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + wunit)));
    lb[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + 64 + wunit)));
    nb[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + 128 + wunit)));
    sg[g] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(gp + 192) + wunit);
    __builtin_amdgcn_sched_barrier(0);             // requests in group order: the counted waits below release group g as it lands
  }
#pragma unroll
  for (int g = 0; g < NG; ++g) asm volatile("" : "+s"(sb[g]));      // the side words are on their way with n_active, not behind the prologue
  if (active == 0) return;
  VC_KTS(1);
  if constexpr (PRO == PRO_PLAIN) {
#define VC_FR1_XPARK(j, val) if constexpr (NXU > (j)) { if (tid + (j) * NTHR < units) *reinterpret_cast<uint4*>(xl + (size_t)(tid + (j) * NTHR) * 16) = val; }
    VC_FR1_XPARK(0, xu0) VC_FR1_XPARK(1, xu1) VC_FR1_XPARK(2, xu2) VC_FR1_XPARK(3, xu3)
#undef VC_FR1_XPARK
  } else {
    // LayerNorm fold of the finished row (vc_gemm.hip): centred BEFORE it is rounded, statistics of the rounded values
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
  const char* xcol = xl + ((size_t)(m & 1) * T::KW + (size_t)kg * T::EPL) * sizeof(WT);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const char* xg = xcol + (size_t)(NPW * wave + 4 * g) * (2 * T::KW * sizeof(WT));
#define VC_W13_STEP(F)                                                                                          \
    {                                                                                                           \
      const uint4 xf = *reinterpret_cast<const uint4*>(xg + (size_t)(F) * (2 * T::KW * sizeof(WT)));            \
      acc = mfma_frag(w13_frag<F>(la[g], lb[g], nb[g], sg[g], sb[g]), xf, acc, (WT*)nullptr);                   \
    }
    VC_W13_STEP(0) VC_W13_STEP(1) VC_W13_STEP(2) VC_W13_STEP(3)
#undef VC_W13_STEP
  }
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
      const float rstd = 1.0f / sqrtf(var + 1e-5f);
      sum[0] = rstd * (sum[0] - mean * ewg.x); sum[1] = rstd * (sum[1] - mean * ewg.y);
      sum[2] = rstd * (sum[2] - mean * ewg.z); sum[3] = rstd * (sum[3] - mean * ewg.w);
      gemm_epilogue<WT, EPI_QKV>(a, sum, 0, nfin, 0, 0, 1, eb, epos, eseq);
    }
  }
  VC_KTS(6);
  VC_KTS_FLUSH();
}

// Groups per wave of the planes form for an [N x K] matrix on the one-row paired kernel with `nw` waves, 0 = no form: bf16, the
// kernel's own form (vc_gemm_fr1_ok) with EXACTLY nw x 4 NG fragment pairs per tile.  The engine's packing and the launcher agree on it.
int vc_gemm_w13_fr1_ng(int N, int K, int dtype, int nw) {
  if (dtype != VC_DTYPE_BF16 || !vc_gemm_fr1_ok(N, K, dtype, nw)) return 0;
  const int npairs = K / 64;
  if (npairs % (nw * VC_W13_GROUP_FRAGS) != 0) return 0;
  const int ng = npairs / (nw * VC_W13_GROUP_FRAGS);
  return (ng == 1 || ng == 2 || ng == 4) ? ng : 0;
}

template <int NG, int NW, int PRO, int EPI>
static hipError_t launch_fr1_w13_n(const W13Args& wa, hipStream_t s) {
  const GemmArgs& a = wa.g;
  const size_t lds = (size_t)a.K * sizeof(bf16_t) + (size_t)NW * 4 * sizeof(f32x4) + (size_t)NW * 3 * sizeof(float);
  ++vc_launch_counts[VC_LC_ROW_GEMM_FR1];      // the form its bf16 twin counts in
  ++vc_launch_counts[VC_LC_W13];
  hipLaunchKernelGGL((row_gemm_fr1_w13_k<NG, NW, PRO, EPI>), dim3(a.n_tiles), dim3(64 * NW), lds, s, wa);
  return hipGetLastError();
}
// vc_launch_gemm_fr1 on the planes of a.Wp's image (`planes`, `side` from vc_launch_w13_pack over the whole image).
hipError_t vc_launch_gemm_fr1_w13(const GemmArgs& a0, const uint4* planes, const uint32_t* side, int pro, int epi, hipStream_t s) {
  const bool qkv = pro == PRO_LN && epi == EPI_QKV;
  if (!qkv && !(pro == PRO_PLAIN && epi == EPI_RES)) return hipErrorInvalidValue;
  const int nw = qkv ? 4 : VC_FR_WAVES;
  const int ng = vc_gemm_w13_fr1_ng(a0.N, a0.K, VC_DTYPE_BF16, nw);
  if (!ng || a0.n_rows != 1 || !planes || !side) return hipErrorInvalidValue;
  W13Args wa;
  wa.g = a0;
  wa.g.n_tiles = a0.N / VC_TH_RES;
  wa.g.KT = a0.K / 32;
  wa.planes = planes;
  wa.side = side;
#define VC_W13_CASE(G_) case G_:                                                             \
    return qkv ? launch_fr1_w13_n<G_, 4, PRO_LN, EPI_QKV>(wa, s) : launch_fr1_w13_n<G_, VC_FR_WAVES, PRO_PLAIN, EPI_RES>(wa, s);
  switch (ng) {
    VC_W13_CASE(1) VC_W13_CASE(2) VC_W13_CASE(4)
    default: return hipErrorInvalidValue;
  }
#undef VC_W13_CASE
}

