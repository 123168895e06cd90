// vc_gemm_w13.hip - one-row decode on weights stored as exact 13-bit planes ("w13", vc_w13.h).
//
// A one-row step is a weight stream: every big launch fits t = 2.2 .. 2.5 us + bytes / 6.1 TB/s, and while the stream runs
// the CUs idle.  The planes carry the same bf16 values in 13/16 of the bytes; the kernels below are the one-row paired body
// (vc_gemm_fr1_body.h, shared with row_gemm_fr1_k of vc_gemm.hip) with their own weight burst: per group of four fragments a wave
// requests two KB of low bytes, one KB of exponent codes and 256 bytes of signs, contiguous per request (non-temporal, everything up front), and rebuilds each fragment's four dwords in registers right in
// front of its MFMA.  (The group base is wave-uniform, but only group 0 is addressed from SGPRs in the compiled code: a group is 3 328
// bytes, past the immediate offset field, so groups 1.. carry a 64-bit VGPR address add between their requests - the image kernels have none.)
// No data-dependent branch, no dependent load: the side bytes are wave-uniform and on their way with the burst.
// Prologue, epilogue and summation order are the bf16 kernels', the MFMA operands are bit-identical, so every result is.
// Measured at giga830M (one row, 654 steps, in-process A/B of option w13, profiles/w13_ab.log): see DESIGN section 4.6.
// The packer and its check run once per matrix at creation (vc_engine.hip pack_checked): a matrix with a fragment the codes cannot hold,
// or whose planes do not decode to the image bit for bit, keeps its bf16 kernel.
#include "vc_gemm_fr1.h"
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
hipError_t vc_launch_w13_pack(const uint4* img, long n_frags, uint4* planes, unsigned char* side, unsigned int* counts, hipStream_t s) {
  return vc_fr1_launch_pack(VC_PK_W13, w13_pack_k, w13_check_k, img, n_frags, planes, side, counts, s);
}

// ------------------------------------------------------------------ the one-row paired kernel on the planes
struct W13Args : Fr1PackedArgs {};

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

// The shared body (vc_gemm_fr1_body.h) on the planes: the wave's NG groups in place of its 4 NG fragments.  The matrix has exactly
// NW * NG groups per tile (host contract).
template <int NG, int NW, int PRO, int EPI>
__global__ __launch_bounds__(64 * NW) void row_gemm_fr1_w13_k(const W13Args wa) {
  using WT = bf16_t;
  constexpr int NPW = 4 * NG, GROUP = 4;
  constexpr bool EXACT = true;
  const GemmArgs& a = wa.g;
  /* the wave's side bytes: scalar operands, first needed long after the burst is out */
#define VC_FR1_EARLY                                                                                                                   \
  const long G0 = ((long)nt * NW + wave) * NG;                                                                                         \
  uint32_t sb[NG];                                                                                                                     \
  _Pragma("unroll") for (int g = 0; g < NG; ++g) sb[g] = wa.side[G0 + g];
  /* the wave's whole share of the planes in one burst, group by group (loads return in order: group g decodes while g + 1.. land); */
  /* the sched_barrier keeps the requests in group order: the counted waits of the MFMA steps release group g as it lands; */
  /* the pins: the side words are on their way with n_active, not behind the prologue */
#define VC_FR1_BURST                                                                                                                   \
  const uint4* gbase = wa.planes + G0 * VC_W13_GROUP_U4;                 /* wave-uniform */                                             \
  uint4 la[NG], lb[NG], nb[NG];                                                                                                        \
  uint32_t sg[NG];                                                                                                                     \
  _Pragma("unroll") for (int g = 0; g < NG; ++g) {                                                                                     \
    const uint4* gp = gbase + g * VC_W13_GROUP_U4;                                                                                     \
    la[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + wunit)));                         \
    lb[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + 64 + wunit)));                    \
    nb[g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + 128 + wunit)));                   \
    sg[g] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(gp + 192) + wunit);                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                                 \
  }                                                                                                                                    \
  _Pragma("unroll") for (int g = 0; g < NG; ++g) asm volatile("" : "+s"(sb[g]));
#define VC_FR1_FRAG(F, w) const uint4 w = w13_frag<F>(la[g], lb[g], nb[g], sg[g], sb[g]);
#include "vc_gemm_fr1_body.h"
}

struct W13Kind {
  using Args = W13Args;
  static constexpr int KIND = VC_PK_W13;
  template <int NG, int NW, int PRO, int EPI> static auto kernel() { return &row_gemm_fr1_w13_k<NG, NW, PRO, EPI>; }
};
hipError_t vc_launch_gemm_fr1_w13(const GemmArgs& a, const uint4* planes, const uint32_t* side, int pro, int epi, hipStream_t s) {
  return vc_fr1_launch_packed<W13Kind>(a, planes, side, pro, epi, s);
}
