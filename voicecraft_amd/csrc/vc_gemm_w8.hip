// vc_gemm_w8.hip - one-row decode on weights stored as block-scaled E4M3 bytes ("w8", vc_w8.h).
//
// A one-row step is a weight stream: every big launch fits t = 2.2 .. 2.5 us + bytes / 6.1 TB/s.  A checkpoint whose
// matrices lie on the w8 grid (voicecraft_amd/quant.py puts one there) is streamed in half the bytes of its bf16 image: the kernels below
// are the one-row paired body (vc_gemm_fr1_body.h, shared with row_gemm_fr1_k of vc_gemm.hip) with their own weight burst.  Per group of four fragments a wave requests two KB of code bytes,
// 16 bytes per lane and request, contiguous per request (non-temporal, everything up front), and rebuilds each fragment's four dwords
// with four v_cvt_scalef32_pk_bf16_fp8 right in front of its MFMA; the scale is the fragment's side byte shifted into an fp32
// exponent, a wave-uniform scalar.  No data-dependent branch, no dependent load.
// Prologue, epilogue and summation order are the bf16 kernels', the MFMA operands are bit-identical, so every result is.
// The packer and its check run once per matrix at creation (vc_engine.hip pack_planes, on request: vc_request_w8): the check decodes with
// the instruction the kernels use, so a matrix off the grid - or a surprise in the instruction - keeps the bf16 kernel.
#include "vc_gemm_fr1.h"
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
hipError_t vc_launch_w8_pack(const uint4* img, long n_frags, uint4* planes, unsigned char* side, unsigned int* counts, hipStream_t s) {
  return vc_fr1_launch_pack(VC_PK_W8, w8_pack_k, w8_check_k, img, n_frags, planes, side, counts, s);
}

// ------------------------------------------------------------------ the one-row paired kernel on the code bytes
struct W8Args : Fr1PackedArgs {};

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

// The shared body (vc_gemm_fr1_body.h) on the code bytes: the wave's NG groups in place of its 4 NG fragments.  The matrix has exactly
// NW * NG groups per tile (host contract).
template <int NG, int NW, int PRO, int EPI>
__global__ __launch_bounds__(64 * NW) void row_gemm_fr1_w8_k(const W8Args wa) {
  using WT = bf16_t;
  constexpr int NPW = 4 * NG, GROUP = 4;
  constexpr bool EXACT = true;
  const GemmArgs& a = wa.g;
  /* the wave's side bytes: scalar operands, first needed long after the burst is out */
#define VC_FR1_EARLY                                                                                                                   \
  const long G0 = ((long)nt * NW + wave) * NG;                                                                                         \
  uint32_t sb[NG];                                                                                                                     \
  _Pragma("unroll") for (int g = 0; g < NG; ++g) sb[g] = wa.side[G0 + g];
  /* the wave's whole share of the code bytes in one burst, group by group (loads return in order: group g decodes while g + 1.. land); */
  /* the sched_barrier keeps the requests in group order: the counted waits of the MFMA steps release group g as it lands; */
  /* the pins: the side words are on their way with n_active, not behind the prologue */
#define VC_FR1_BURST                                                                                                                   \
  const uint4* gbase = wa.planes + G0 * VC_W8_GROUP_U4;                  /* wave-uniform */                                             \
  uint4 pa[NG], pb[NG];                                                                                                                \
  _Pragma("unroll") for (int g = 0; g < NG; ++g) {                                                                                     \
    const uint4* gp = gbase + g * VC_W8_GROUP_U4;                                                                                      \
    pa[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + wunit)));                         \
    pb[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + 64 + wunit)));                    \
    __builtin_amdgcn_sched_barrier(0);                                                                                                 \
  }                                                                                                                                    \
  _Pragma("unroll") for (int g = 0; g < NG; ++g) asm volatile("" : "+s"(sb[g]));
#define VC_FR1_FRAG(F, w) const uint4 w = w8_frag<F>(pa[g], pb[g], sb[g]);
#include "vc_gemm_fr1_body.h"
}

struct W8Kind {
  using Args = W8Args;
  static constexpr int KIND = VC_PK_W8;
  template <int NG, int NW, int PRO, int EPI> static auto kernel() { return &row_gemm_fr1_w8_k<NG, NW, PRO, EPI>; }
};
hipError_t vc_launch_gemm_fr1_w8(const GemmArgs& a, const uint4* planes, const uint32_t* side, int pro, int epi, hipStream_t s) {
  return vc_fr1_launch_packed<W8Kind>(a, planes, side, pro, epi, s);
}
