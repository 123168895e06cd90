// vc_gemm_w8.hip - one-row decode on weights stored as block-scaled E4M3 bytes ("w8", vc_w8.h).
//
// A one-row step is a weight stream: every big launch fits t = 2.2 .. 2.5 us + bytes / 6.1 TB/s.  A checkpoint whose
// matrices lie on the w8 grid (voicecraft_amd/quant.py puts one there) is streamed in half the bytes of its bf16 image: the kernels below
// are row_gemm_fr1_k (vc_gemm.hip) with the weight burst replaced.  Per group of four fragments a wave requests two KB of code bytes,
// 16 bytes per lane and request, contiguous per request (non-temporal, everything up front), and rebuilds each fragment's four dwords
// with four v_cvt_scalef32_pk_bf16_fp8 right in front of its MFMA; the scale is the fragment's side byte shifted into an fp32
// exponent, a wave-uniform scalar.  No data-dependent branch, no dependent load.
// Prologue, epilogue and summation order are the bf16 kernels', the MFMA operands are bit-identical, so every result is.
// The packer and its check run once per matrix at creation (vc_engine.hip pack_w8, on request: vc_request_w8): the check decodes with
// the instruction the kernels use, so a matrix off the grid - or a surprise in the instruction - keeps the bf16 kernel.
#include "vc_gemm_dev.h"
#include "vc_w8.h"

// ------------------------------------------------------------------ packing (creation time)
// One wave per group: image = consecutive 1 KB fragments, unit u of fragment F at img[64 F + u].  counts[0] += fragments refused.
__global__ __launch_bounds__(64) void w8_pack_k(const uint4* __restrict__ img, uint4* __restrict__ planes,
                                                 unsigned char* __restrict__ side, unsigned int* __restrict__ counts) {
  const long G = blockIdx.x;
  const int u = threadIdx.x;
  uint32_t w[4][4];
  int shift[4], refused = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const uint4 v = img[(G * 4 + f) * 64 + u];
    w[f][0] = v.x; w[f][1] = v.y; w[f][2] = v.z; w[f][3] = v.w;
    int mn, mx, ok;
    vc_w8_minmax(w[f], &mn, &mx);
    mn = wave_min_i(mn);
    mx = -wave_min_i(-mx);
    const int top = wave_sum_i(vc_w8_top111(w[f], mx));
    shift[f] = vc_w8_shift(mn, mx, top, &ok);
    refused |= ok ? 0 : 1 << f;
  }
  vc_w8_lane L;
  const int bad = vc_w8_encode(w, shift, &L);
  int nref = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) nref += (wave_sum_i((bad >> f) & 1) > 0 || ((refused >> f) & 1)) ? 1 : 0;
  uint4* gp = planes + G * VC_W8_GROUP_U4;
  gp[u] = make_uint4(L.a[0], L.a[1], L.a[2], L.a[3]);
  gp[64 + u] = make_uint4(L.b[0], L.b[1], L.b[2], L.b[3]);
  if (u < 4) side[G * 4 + u] = (unsigned char)vc_w8_side(u == 0 ? shift[0] : u == 1 ? shift[1] : u == 2 ? shift[2] : shift[3]);
  if (u == 0 && nref) atomicAdd(counts, (unsigned int)nref);
}
// counts[1] += dwords that do not decode to the image's
__global__ __launch_bounds__(64) void w8_check_k(const uint4* __restrict__ img, const uint4* __restrict__ planes,
                                                  const unsigned char* __restrict__ side, unsigned int* __restrict__ counts) {
  const long G = blockIdx.x;
  const int u = threadIdx.x;
  const uint4* gp = planes + G * VC_W8_GROUP_U4;
  const uint4 pa = gp[u], pb = gp[64 + u];
  const vc_w8_lane L = {{pa.x, pa.y, pa.z, pa.w}, {pb.x, pb.y, pb.z, pb.w}};
  int bad = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    uint32_t w[4];
    vc_w8_decode_frag(&L, f, side[G * 4 + f], w);
    const uint4 v = img[(G * 4 + f) * 64 + u];
    bad += (w[0] != v.x) + (w[1] != v.y) + (w[2] != v.z) + (w[3] != v.w);
  }
  bad = wave_sum_i(bad);
  if (u == 0 && bad) atomicAdd(counts + 1, (unsigned int)bad);
}
// Packs `n_frags` fragments (a multiple of four) of a bf16 image and checks the planes against it; counts = two device words, zeroed here.
hipError_t vc_launch_w8_pack(const uint4* img, long n_frags, uint4* planes, unsigned char* side, unsigned int* counts, hipStream_t s) {
  if (n_frags <= 0 || n_frags % VC_W8_GROUP_FRAGS != 0 || n_frags / VC_W8_GROUP_FRAGS > 0x7fffffffL) return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(counts, 0, 2 * sizeof(unsigned int), s);
  if (err != hipSuccess) return err;
  const unsigned int groups = (unsigned int)(n_frags / VC_W8_GROUP_FRAGS);
  hipLaunchKernelGGL(w8_pack_k, dim3(groups), dim3(64), 0, s, img, planes, side, counts);
  hipLaunchKernelGGL(w8_check_k, dim3(groups), dim3(64), 0, s, img, (const uint4*)planes, (const unsigned char*)side, counts);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the one-row paired kernel on the planes
struct W8Args {
  GemmArgs g;
  const uint4* planes;      // groups in image order (VC_W8_GROUP_U4 units each)
  const uint32_t* side;     // one byte per fragment, four per word = one word per group
};

// fragment F of a group from the lane's two pieces; the scale is scalar arithmetic on the group's side word
template <int F>
__device__ __forceinline__ uint4 w8_frag(const uint4& pa, const uint4& pb, uint32_t sidew) {
  const uint32_t sc = vc_w8_scale_bits(sidew >> (8 * F));
  const uint32_t d0 = F == 0 ? pa.x : F == 1 ? pa.z : F == 2 ? pb.x : pb.z;
  const uint32_t d1 = F == 0 ? pa.y : F == 1 ? pa.w : F == 2 ? pb.y : pb.w;
  uint4 w;
  w.x = vc_w8_cvt(d0, 0, sc);
  w.y = vc_w8_cvt(d0, 1, sc);
  w.z = vc_w8_cvt(d1, 0, sc);
  w.w = vc_w8_cvt(d1, 1, sc);
  return w;
}

// row_gemm_fr1_k<bf16_t, 4 NG, EXACT, NW, PRO, EPI> (vc_gemm.hip; see there for the tile and fragment-pair arithmetic) with the wave's
// NG groups of code bytes in place of its 4 NG fragments.  (TWIN of row_gemm_fr1_w13_k, vc_gemm_w13.hip: everything but the burst and
// the fragment decode is that kernel's text.)
template <int NG, int NW, int PRO, int EPI>
__global__ __launch_bounds__(64 * NW) void row_gemm_fr1_w8_k(const W8Args wa) {
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
  // the wave's whole share of the code bytes in one burst, group by group (loads return in order: group g decodes while g + 1.. land)
  const int wunit = (m >> 3) * SPT + kg * TH + (m & 7);
  const uint4* gbase = wa.planes + G0 * VC_W8_GROUP_U4;                  // wave-uniform
  uint4 pa[NG], pb[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const uint4* gp = gbase + g * VC_W8_GROUP_U4;
    pa[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + wunit)));
    pb[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + 64 + wunit)));
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
#define VC_W8_STEP(F)                                                                                           \
    {                                                                                                           \
      const uint4 xf = *reinterpret_cast<const uint4*>(xg + (size_t)(F) * (2 * T::KW * sizeof(WT)));            \
      acc = mfma_frag(w8_frag<F>(pa[g], pb[g], sb[g]), xf, acc, (WT*)nullptr);                                  \
    }
    VC_W8_STEP(0) VC_W8_STEP(1) VC_W8_STEP(2) VC_W8_STEP(3)
#undef VC_W8_STEP
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

// Groups per wave of the w8 form for an [N x K] matrix on the one-row paired kernel with `nw` waves, 0 = no form: the contract of
// vc_gemm_w13_fr1_ng (bf16, the kernel's own form with EXACTLY nw x 4 NG fragment pairs per tile).
int vc_gemm_w8_fr1_ng(int N, int K, int dtype, int nw) {
  if (dtype != VC_DTYPE_BF16 || !vc_gemm_fr1_ok(N, K, dtype, nw)) return 0;
  const int npairs = K / 64;
  if (npairs % (nw * VC_W8_GROUP_FRAGS) != 0) return 0;
  const int ng = npairs / (nw * VC_W8_GROUP_FRAGS);
  return (ng == 1 || ng == 2 || ng == 4) ? ng : 0;
}

template <int NG, int NW, int PRO, int EPI>
static hipError_t launch_fr1_w8_n(const W8Args& wa, hipStream_t s) {
  const GemmArgs& a = wa.g;
  const size_t lds = (size_t)a.K * sizeof(bf16_t) + (size_t)NW * 4 * sizeof(f32x4) + (size_t)NW * 3 * sizeof(float);
  ++vc_launch_counts[VC_LC_ROW_GEMM_FR1];      // the form its bf16 twin counts in
  ++vc_launch_counts[VC_LC_W8];
  hipLaunchKernelGGL((row_gemm_fr1_w8_k<NG, NW, PRO, EPI>), dim3(a.n_tiles), dim3(64 * NW), lds, s, wa);
  return hipGetLastError();
}
// vc_launch_gemm_fr1 on the code bytes of a.Wp's image (`planes`, `side` from vc_launch_w8_pack over the whole image).
hipError_t vc_launch_gemm_fr1_w8(const GemmArgs& a0, const uint4* planes, const uint32_t* side, int pro, int epi, hipStream_t s) {
  const bool qkv = pro == PRO_LN && epi == EPI_QKV;
  if (!qkv && !(pro == PRO_PLAIN && epi == EPI_RES)) return hipErrorInvalidValue;
  const int nw = qkv ? 4 : VC_FR_WAVES;
  const int ng = vc_gemm_w8_fr1_ng(a0.N, a0.K, VC_DTYPE_BF16, nw);
  if (!ng || a0.n_rows != 1 || !planes || !side) return hipErrorInvalidValue;
  W8Args wa;
  wa.g = a0;
  wa.g.n_tiles = a0.N / VC_TH_RES;
  wa.g.KT = a0.K / 32;
  wa.planes = planes;
  wa.side = side;
#define VC_W8_CASE(G_) case G_:                                                              \
    return qkv ? launch_fr1_w8_n<G_, 4, PRO_LN, EPI_QKV>(wa, s) : launch_fr1_w8_n<G_, VC_FR_WAVES, PRO_PLAIN, EPI_RES>(wa, s);
  switch (ng) {
    VC_W8_CASE(1) VC_W8_CASE(2) VC_W8_CASE(4)
    default: return hipErrorInvalidValue;
  }
#undef VC_W8_CASE
}
