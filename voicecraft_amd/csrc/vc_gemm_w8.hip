// vc_gemm_w8.hip - one-row decode on weights stored as block-scaled E4M3 bytes ("w8", vc_w8.h).
//
// A one-row step is a weight stream: every big launch fits t = 2.2 .. 2.5 us + bytes / 6.1 TB/s.  A checkpoint whose
// matrices lie on the w8 grid (voicecraft_amd/quant.py puts one there) is streamed in half the bytes of its bf16 image: the kernels below
// are the one-row paired body (vc_gemm_fr1_body.h, shared with row_gemm_fr1_k of vc_gemm.hip) with their own weight burst.  Per group of four fragments a wave requests two KB of code bytes,
// 16 bytes per lane and request, contiguous per request (non-temporal, everything up front), and rebuilds each fragment's four dwords
// with four v_cvt_scalef32_pk_bf16_fp8 right in front of its MFMA; the scale is the fragment's side byte shifted into an fp32
// exponent, a wave-uniform scalar.  No data-dependent branch, no dependent load.
// Prologue, epilogue and summation order are the bf16 kernels', the MFMA operands are bit-identical, so every result is.
// The packer and its check run once per matrix at creation (vc_engine.hip pack_checked, on request: vc_request_w8): the check decodes with
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

// The weight source of the five kernels on the group planes, written once: a wave owns NO_ runs of NG consecutive groups, run o
// starting NW * NG groups behind run o - 1 (NO_ = 1: its share of one tile; NTQ: of the workgroup's tiles; 2: of a tile's two halves of
// K), the first at group G0 = ((TILE_ NO_) NW + wave) NG.  The macros see the body's wave and wunit, the kernel's NG, NW and wa.
// VC_W8_SIDE: the wave's side bytes - scalar operands, first needed long after the burst is out.
#define VC_W8_SIDE(NO_, TILE_)                                                                                                         \
  const long G0 = ((long)(TILE_) * (NO_) * NW + wave) * NG;                                                                            \
  uint32_t sb[NO_][NG];                                                                                                                \
  _Pragma("unroll") for (int o_ = 0; o_ < (NO_); ++o_)                                                                                 \
    _Pragma("unroll") for (int g = 0; g < NG; ++g) sb[o_][g] = wa.side[G0 + o_ * (NW * NG) + g];
// VC_W8_PLANES: the lane's two pieces of every group.  VC_W8_BURST: the wave's whole share of the code bytes in one burst, run by run
// and group by group (loads return in order: group g decodes while g + 1.. land); the sched_barrier keeps the requests in that
// order: the counted waits of the MFMA steps release a group as it lands; the pins: the side words are on their way with n_active, not
// behind the prologue.
#define VC_W8_PLANES(NO_)                                                                                                              \
  const uint4* gbase = wa.planes + G0 * VC_W8_GROUP_U4;                  /* wave-uniform */                                             \
  uint4 pa[NO_][NG], pb[NO_][NG];
#define VC_W8_BURST(NO_)                                                                                                               \
  _Pragma("unroll") for (int o_ = 0; o_ < (NO_); ++o_)                                                                                 \
    _Pragma("unroll") for (int g = 0; g < NG; ++g) {                                                                                   \
      const uint4* gp = gbase + (o_ * (NW * NG) + g) * VC_W8_GROUP_U4;                                                                 \
      pa[o_][g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + wunit)));                   \
      pb[o_][g] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(gp + 64 + wunit)));              \
      __builtin_amdgcn_sched_barrier(0);                                                                                               \
    }                                                                                                                                  \
  _Pragma("unroll") for (int o_ = 0; o_ < (NO_); ++o_)                                                                                 \
    _Pragma("unroll") for (int g = 0; g < NG; ++g) asm volatile("" : "+s"(sb[o_][g]));

// The shared body (vc_gemm_fr1_body.h) on the code bytes: the wave's NG groups in place of its 4 NG fragments.  The matrix has exactly
// NW * NG groups per tile (host contract).
template <int NG, int NW, int PRO, int EPI>
__global__ __launch_bounds__(64 * NW) void row_gemm_fr1_w8_k(const W8Args wa) {
  using WT = bf16_t;
  constexpr int NPW = 4 * NG, GROUP = 4;
  constexpr bool EXACT = true;
  const GemmArgs& a = wa.g;
#define VC_FR1_EARLY VC_W8_SIDE(1, nt)
#define VC_FR1_BURST VC_W8_PLANES(1) VC_W8_BURST(1)
#define VC_FR1_FRAG(F, w) const uint4 w = w8_frag<F>(pa[0][g], pb[0][g], sb[0][g]);
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

// ------------------------------------------------------------------ the paired kernels of 2..8-row steps on the code bytes (option "w8r")
// rows_gemm_frp_k (FFN-down) and rows_gemm_qp_k (QKV of layers 1..) read the images the planes are made from, with the one-row kernel's
// lane mapping: a wave's NPW consecutive fragments of a tile are NG = NPW / 4 whole groups.  The shared bodies (vc_gemm_frp_body.h,
// vc_gemm_qp_body.h) with the burst above in place of the image loads: X staging, B columns, reduction order, row statistics and
// epilogues are the image kernels' text and the MFMA operands are bit-identical, so every result is.  24 / 32 VGPRs of bytes where the
// image kernels hold 48 / 64 of weights.
template <int NG, int RMAX>
__global__ __launch_bounds__(64 * VC_FR_WAVES) void rows_gemm_frp_w8_k(const W8Args wa) {
  using WT = bf16_t;
  constexpr int NPW = 4 * NG, GROUP = 4;
  const GemmArgs& a = wa.g;
#define VC_FRP_EARLY VC_W8_SIDE(1, nt)
#define VC_FRP_BURST VC_W8_PLANES(1) VC_W8_BURST(1)
#define VC_FRP_FRAG(F, w) const uint4 w = w8_frag<F>(pa[0][g], pb[0][g], sb[0][g]);
#include "vc_gemm_frp_body.h"
}
// Three tiles per workgroup: group g of tile t of wave w = (((3 blockIdx.x + t) NW + w) NG + g), requested tile by tile as the image is.
template <int NG, int RMAX>
__global__ __launch_bounds__(64 * VC_FR_WAVES) void rows_gemm_qp_w8_k(const W8Args wa) {
  using WT = bf16_t;
  constexpr int NPW = 4 * NG, GROUP = 4;
  const GemmArgs& a = wa.g;
#define VC_QP_EARLY VC_W8_SIDE(NTQ, blockIdx.x)
#define VC_QP_BURST VC_W8_PLANES(NTQ) VC_W8_BURST(NTQ)
#define VC_QP_FRAG(t, F, w) const uint4 w = w8_frag<F>(pa[t][g], pb[t][g], sb[t][g]);
#include "vc_gemm_qp_body.h"
}

// Groups per wave of the w8 form of the paired producer / consumer for `rows` rows of an [N x K] matrix, 0 = no form: the image
// kernel's own form (vc_gemm_frp_ok / vc_gemm_qp_ok), bf16, and a wave's fragments per tile whole groups.  (QKV at d = 1024 has two
// fragments per wave and tile, half a group: it stays on the image.)
int vc_gemm_frp_w8_ng(int rows, int N, int K, int dtype) {
  if (dtype != VC_DTYPE_BF16 || !vc_gemm_frp_ok(rows, N, K, dtype)) return 0;
  const int npw = K / (64 * VC_FR_WAVES);
  if (npw % VC_W8_GROUP_FRAGS != 0) return 0;
  const int ng = npw / VC_W8_GROUP_FRAGS;
  return (ng == 1 || ng == 2 || ng == 4) ? ng : 0;      // (K = 16384, four rows at the most, stays on the image)
}
int vc_gemm_qp_w8_ng(int rows, int N, int K, int dtype) {
  if (dtype != VC_DTYPE_BF16 || !vc_gemm_qp_ok(rows, N, K, dtype)) return 0;
  return K * 2 / 1024 == VC_W8_GROUP_FRAGS ? 1 : 0;
}
// the launch of one of the two kernels: dynamic LDS beyond 64 KB is granted once per kernel and device
static hipError_t launch_rows_w8(void (*kern)(const W8Args), size_t* granted, const W8Args& wa, int grid, size_t lds, int lc, hipStream_t s) {
  if (hipError_t e = grant_lds(reinterpret_cast<const void*>(kern), granted, lds); e != hipSuccess) return e;
  ++vc_launch_counts[lc];                      // the form the image kernel counts in
  ++vc_launch_counts[VC_LC_W8_ROWS];
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * VC_FR_WAVES), lds, s, wa);
  return hipGetLastError();
}
// vc_launch_gemm_frp on the E4M3 bytes of a.Wp's image (W28)
hipError_t vc_launch_gemm_frp_w8(const GemmArgs& a0, const uint4* planes, const uint32_t* side, hipStream_t s) {
  const int ng = vc_gemm_frp_w8_ng(a0.n_rows, a0.N, a0.K, VC_DTYPE_BF16);
  if (!ng || !planes || !side) return hipErrorInvalidValue;
  W8Args wa;
  wa.g = a0;
  wa.g.n_tiles = a0.N / VC_TH_RES;
  wa.g.KT = a0.K / 32;
  const int upr = a0.K * 2 / 16;
  wa.g.x_upr_shift = 0;
  while ((1 << wa.g.x_upr_shift) < upr) ++wa.g.x_upr_shift;
  wa.planes = planes;
  wa.side = side;
  const int rmax = a0.n_rows <= 4 ? 4 : 8;
  static size_t granted[3][2][16] = {{{0}}};   // per kernel and device
  void (*kern)(const W8Args) = nullptr;
  int slot = 0;
#define VC_FRP_W8_CASE(G_, S_) case G_: kern = rmax == 4 ? rows_gemm_frp_w8_k<G_, 4> : rows_gemm_frp_w8_k<G_, 8>; slot = S_; break;
  switch (ng) {
    VC_FRP_W8_CASE(1, 0) VC_FRP_W8_CASE(2, 1) VC_FRP_W8_CASE(4, 2)
    default: return hipErrorInvalidValue;
  }
#undef VC_FRP_W8_CASE
  const size_t lds = (size_t)rmax * a0.K * sizeof(bf16_t) + 256 + (size_t)VC_FR_WAVES * rmax * 4 * sizeof(f32x4);
  return launch_rows_w8(kern, granted[slot][rmax == 8], wa, wa.g.n_tiles, lds, VC_LC_ROWS_GEMM_FRP, s);
}
// vc_launch_gemm_qp on the E4M3 bytes of a.Wp's image (Wqkv8)
hipError_t vc_launch_gemm_qp_w8(const GemmArgs& a0, const uint4* planes, const uint32_t* side, hipStream_t s) {
  const int ng = vc_gemm_qp_w8_ng(a0.n_rows, a0.N, a0.K, VC_DTYPE_BF16);
  if (ng != 1 || !planes || !side || a0.x_in == nullptr || a0.row_mu == nullptr) return hipErrorInvalidValue;
  W8Args wa;
  wa.g = a0;
  wa.g.n_tiles = a0.N / VC_TH_RES;
  wa.g.KT = a0.K / 32;
  wa.planes = planes;
  wa.side = side;
  const int rmax = a0.n_rows <= 4 ? 4 : 8;
  static size_t granted[2][16] = {{0}};        // per kernel and device
  void (*kern)(const W8Args) = rmax == 4 ? rows_gemm_qp_w8_k<1, 4> : rows_gemm_qp_w8_k<1, 8>;
  const size_t lds = (size_t)rmax * a0.K * sizeof(bf16_t) + 256 + (size_t)VC_FR_WAVES * rmax * 3 * 4 * sizeof(f32x4) + (size_t)rmax * 2 * sizeof(float);
  return launch_rows_w8(kern, granted[rmax == 8], wa, wa.g.n_tiles / 3, lds, VC_LC_ROWS_GEMM_QP, s);
}

// ------------------------------------------------------------------ the finished-row producers of 9..16-row passes on the code bytes (option "w8m")
// rows_gemm_fr_k<.., PRO_PLAIN, ..> and rows_gemm_fr2_k (vc_gemm.hip) read the same image, W28, one 512-byte k-tile per wave instruction:
// lane (m, kg) takes unit kg * 8 + min(m, 7), operand rows 0..7 are the real channels and nvalid masks the outputs of rows 8..15.  A
// decoded w8 fragment is a PAIR in the paired kernels' lane mapping (wunit): lanes m < 8 hold k-tile 2 P, lanes m >= 8 k-tile 2 P + 1,
// unit kg * 8 + (m & 7) each.  One decoded fragment therefore feeds two consecutive MFMAs of the image kernel's loop: k-tile 2 P takes it
// as it is (lanes m >= 8 carry the other k-tile's weights, which only reach output channels 8..15: nobody reads those), k-tile 2 P + 1
// takes the same four dwords with each 16-lane row rotated by eight (one DPP move per dword).  The operand lanes that are read are
// bit-identical to the image's and so is the order of the sums - k-tile after k-tile in one accumulator per wave, the 8-way reduction,
// residual + bias, the centred copy -: the shared bodies (vc_gemm_fr_body.h, vc_gemm_fr2_body.h) with the burst above in place of the
// image loads.  A group is eight k-tiles; the wave's share of a piece is NG whole groups (host contract).
template <int H>
__device__ __forceinline__ uint4 w8_ktile(const uint4& w) {
  if constexpr (H == 0) {
    return w;
  } else {      // row_ror:8 - lane (m, kg) takes lane (m ^ 8, kg)'s dword; every lane is active here
    uint4 r;
    r.x = (uint32_t)__builtin_amdgcn_update_dpp((int)w.x, (int)w.x, 0x128, 0xf, 0xf, false);
    r.y = (uint32_t)__builtin_amdgcn_update_dpp((int)w.y, (int)w.y, 0x128, 0xf, 0xf, false);
    r.z = (uint32_t)__builtin_amdgcn_update_dpp((int)w.z, (int)w.z, 0x128, 0xf, 0xf, false);
    r.w = (uint32_t)__builtin_amdgcn_update_dpp((int)w.w, (int)w.w, 0x128, 0xf, 0xf, false);
    return r;
  }
}
// X in LDS in one piece (d = 512: NG = 1, d = 1024: NG = 2): group g of wave w = ((nt NW + w) NG + g), the wave's share one chunk.
template <int NG>
__global__ __launch_bounds__(64 * VC_FR_WAVES) void rows_gemm_fr_w8_k(const W8Args wa) {
  using WT = bf16_t;
  constexpr int KTW = 8 * NG, GROUP = 8, PRO = PRO_PLAIN, NS = 1;
  constexpr bool P16 = false, CHUNKS = false;
  const GemmArgs& a = wa.g;
#define VC_FR_EARLY VC_W8_SIDE(1, nt)
#define VC_FR_WDECL                                                                                                                    \
  const int wunit = (m >> 3) * SPT + kg * TH + (m & 7);                                                                                \
  VC_W8_PLANES(1)
#define VC_FR_WEIGHTS(c_) { VC_W8_BURST(1) }
#define VC_FR_FRAG(J, w) const uint4 w = w8_ktile<(J) & 1>(w8_frag<((J) >> 1)>(pa[0][g], pb[0][g], sb[0][g]));
#include "vc_gemm_fr_body.h"
}
// K in two halves (d = 2048: NG = 2 per half): a tile has 2 NW NG groups, half h of wave w = groups ((2 nt + h) NW + w) NG + g, both
// halves requested up front in group order.
template <int NG>
__global__ __launch_bounds__(64 * VC_FR_WAVES) void rows_gemm_fr2_w8_k(const W8Args wa) {
  using WT = bf16_t;
  constexpr int KTW = 8 * NG, GROUP = 8;
  const GemmArgs& a = wa.g;
#define VC_FR2_EARLY VC_W8_SIDE(2, nt)
#define VC_FR2_WDECL                                                                                                                   \
  const int wunit = (m >> 3) * SPT + kg * TH + (m & 7);                                                                                \
  VC_W8_PLANES(2)
#define VC_FR2_BURST VC_W8_BURST(2)
#define VC_FR2_FRAG(h_, J, w) const uint4 w = w8_ktile<(J) & 1>(w8_frag<((J) >> 1)>(pa[h_][g], pb[h_][g], sb[h_][g]));
#include "vc_gemm_fr2_body.h"
}

// Groups per wave and piece of the w8 form of the plain finished-row producer for `rows` rows of an [N x K] matrix, 0 = no form: bf16,
// 9..16 rows, the image launcher's own form (vc_gemm_fr_form: 1 = one piece, 2 = two halves) and a wave's k-tiles per piece whole
// groups of eight in ONE chunk - one piece: K = 2048 (1 group) and 4096 (2), two halves: K = 8192 (2 per half).  Other widths keep the image.
int vc_gemm_fr_w8_ng(int rows, int N, int K, int dtype) {
  if (dtype != VC_DTYPE_BF16 || rows <= VC_FR_MAX_ROWS || rows > VC_ROWS) return 0;
  const int form = vc_gemm_fr_form(rows, N, K, dtype, PRO_PLAIN, 1);
  const int KT = K / 32;
  if (form == 1) {
    if (KT % (VC_FR_WAVES * 8) != 0) return 0;
    const int ng = KT / (VC_FR_WAVES * 8);      // (vc_launch_gemm_fr: k-tiles per wave 8 or 16, one chunk)
    return (ng == 1 || ng == 2) ? ng : 0;
  }
  if (form == 2) return KT == 2 * VC_FR_WAVES * 16 ? 2 : 0;
  return 0;
}
// vc_launch_gemm_fr(.., PRO_PLAIN, ..) on the E4M3 bytes of a.Wp's image (W28): the image launch's grid, LDS and arguments
hipError_t vc_launch_gemm_fr_w8(const GemmArgs& a0, const uint4* planes, const uint32_t* side, hipStream_t s) {
  const int ng = vc_gemm_fr_w8_ng(a0.n_rows, a0.N, a0.K, VC_DTYPE_BF16);
  if (!ng || !planes || !side || a0.x_in == nullptr) return hipErrorInvalidValue;
  const int form = vc_gemm_fr_form(a0.n_rows, a0.N, a0.K, VC_DTYPE_BF16, PRO_PLAIN, 1);
  W8Args wa;
  wa.g = a0;
  wa.g.n_tiles = a0.N / VC_TH_RES;
  wa.g.KT = a0.K / 32;
  wa.g.r_lds = a0.n_rows;
  wa.g.nchunk = form == 2 ? 2 : 1;
  const int kp = form == 2 ? a0.K / 2 : a0.K;      // elements of X a piece stages per row
  const int upr = kp * 2 / 16;
  wa.g.x_upr_shift = -1; wa.g.att_q4_shift = -1;
  for (int sft = 0; sft < 20; ++sft) if ((1 << sft) == upr) wa.g.x_upr_shift = sft;
  wa.planes = planes;
  wa.side = side;
  static size_t granted[3][16] = {{0}};        // per kernel and device
  void (*kern)(const W8Args) = nullptr;
  int slot = 0;
  if (form == 2 && ng == 2) { kern = rows_gemm_fr2_w8_k<2>; slot = 2; }
  else if (form == 1 && ng == 2) { kern = rows_gemm_fr_w8_k<2>; slot = 1; }
  else if (form == 1 && ng == 1) { kern = rows_gemm_fr_w8_k<1>; slot = 0; }
  else return hipErrorInvalidValue;
  const size_t lds = vc_gemm_fr_lds_bytes(a0.n_rows, kp, VC_DTYPE_BF16);
  if (hipError_t e = grant_lds(reinterpret_cast<const void*>(kern), granted[slot], lds); e != hipSuccess) return e;
  ++vc_launch_counts[VC_LC_ROWS_GEMM_FR];      // the form the image kernel counts in
  ++vc_launch_counts[VC_LC_W8_MID];
  hipLaunchKernelGGL(kern, dim3(wa.g.n_tiles), dim3(64 * VC_FR_WAVES), lds, s, wa);
  return hipGetLastError();
}

// ------------------------------------------------------------------ wide steps (17..64 rows) on the code bytes (option "w8w")
// rows_gemm_wds_k (vc_gemm_wd.hip) reads 16-channel images: W2 and Wqkv16.  Their planes are PAIRS (vc_w8.h): k-tiles 2j, 2j + 1 of a
// tile = one X chunk's worth of weights = 1 KB of codes, 16 bytes per lane, and two side bytes (channels 0..7, channels 8..15: the two
// 8 x 64 blocks of the quantiser's grid the pair consists of).
// Packer: one wave per pair, image = consecutive 1 KB fragments (pair P = fragments 2 P, 2 P + 1).  counts[0] += pairs refused.
__global__ __launch_bounds__(64) void w8w_pack_k(const uint4* __restrict__ img, uint4* __restrict__ planes,
                                                  unsigned char* __restrict__ side, unsigned int* __restrict__ counts) {
  const long P = blockIdx.x;
  const int u = threadIdx.x;
  const int half = vc_w8w_half(u);
  uint32_t w[2][4];
  int mn = 256, mx = -1;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint4 v = img[(P * 2 + h) * 64 + u];
    w[h][0] = v.x; w[h][1] = v.y; w[h][2] = v.z; w[h][3] = v.w;
    int a, b;
    vc_w8_minmax(w[h], &a, &b);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  int shift[2], refused = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {        // the two halves, each over its 32 lanes
    const int mnq = wave_min_i(half == q ? mn : 256);
    const int mxq = -wave_min_i(half == q ? -mx : 1);
    const int top = wave_sum_i(half == q ? (vc_w8_top111(w[0], mxq) | vc_w8_top111(w[1], mxq)) : 0);
    int ok;
    shift[q] = vc_w8_shift(mnq, mxq, top, &ok);
    refused |= ok ? 0 : 1;
  }
  uint32_t c[4];
  const int bad = vc_w8w_encode_lane(w, half ? shift[1] : shift[0], c);
  refused |= wave_sum_i(bad) > 0 ? 1 : 0;
  planes[P * VC_W8W_PAIR_U4 + u] = make_uint4(c[0], c[1], c[2], c[3]);
  if (u < 2) side[P * 2 + u] = (unsigned char)vc_w8_side(u == 0 ? shift[0] : shift[1]);
  if (u == 0 && refused) atomicAdd(counts, 1u);
}
// counts[1] += dwords that do not decode to the image's (the conversion the GEMM uses)
__global__ __launch_bounds__(64) void w8w_check_k(const uint4* __restrict__ img, const uint4* __restrict__ planes,
                                                   const unsigned char* __restrict__ side, unsigned int* __restrict__ counts) {
  const long P = blockIdx.x;
  const int u = threadIdx.x;
  const uint4 pc = planes[P * VC_W8W_PAIR_U4 + u];
  const uint32_t c[4] = {pc.x, pc.y, pc.z, pc.w};
  uint32_t w[2][4];
  vc_w8w_decode_lane(c, side[P * 2 + vc_w8w_half(u)], w);
  int bad = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint4 v = img[(P * 2 + h) * 64 + u];
    bad += (w[h][0] != v.x) + (w[h][1] != v.y) + (w[h][2] != v.z) + (w[h][3] != v.w);
  }
  bad = wave_sum_i(bad);
  if (u == 0 && bad) atomicAdd(counts + 1, (unsigned int)bad);
}
hipError_t vc_launch_w8w_pack(const uint4* img, long n_pairs, uint4* planes, unsigned char* side, unsigned int* counts, hipStream_t s) {
  if (n_pairs <= 0 || n_pairs > 0x7fffffffL) return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(counts, 0, 2 * sizeof(unsigned int), s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(w8w_pack_k, dim3((unsigned int)n_pairs), dim3(64), 0, s, img, planes, side, counts);
  hipLaunchKernelGGL(w8w_check_k, dim3((unsigned int)n_pairs), dim3(64), 0, s, img, (const uint4*)planes, (const unsigned char*)side, counts);
  return hipGetLastError();
}
// The packer's text on a host buffer (no device): image16 = n_pairs x 2 KB of a 16-channel bf16 image, planes = n_pairs x 1 KB, side =
// n_pairs x 2 bytes; *refused_pairs = pairs with a half off the grid (their bytes decode to something else).
extern "C" int vc_w8w_pack_host(const uint16_t* image16, long n_pairs, uint8_t* planes, uint8_t* side, int32_t* refused_pairs) {
  if (!image16 || !planes || !side || !refused_pairs || n_pairs < 0) return -1;
  int32_t nref = 0;
  for (long P = 0; P < n_pairs; ++P) {
    uint32_t img[512], codes[256];
    memcpy(img, image16 + P * 1024, sizeof img);
    nref += vc_w8w_encode_pair(img, codes, side + P * 2) ? 1 : 0;
    memcpy(planes + P * VC_W8W_PAIR_BYTES, codes, sizeof codes);
  }
  *refused_pairs = nref;
  return 0;
}

// The wave's side bytes, as scalars: KPW bytes at byte offset off = tile * KT + ktb of the side stream (two per pair, KT per tile); KPW
// = 2 is a halfword: the aligned word, shifted down.  Byte 2 c + q = pair c, channels 8 q .. 8 q + 7.
template <int KPW>
struct W8wSide {
  static constexpr int NSW = KPW <= 4 ? 1 : KPW / 4;
  uint32_t w[NSW];
  __device__ __forceinline__ void load(const uint32_t* side, long off) {
#pragma unroll
    for (int i = 0; i < NSW; ++i) w[i] = side[(off >> 2) + i];
    if constexpr (KPW == 2) w[0] >>= 8 * (int)(off & 2);
  }
  template <int C> __device__ __forceinline__ uint32_t scale(int hi) const {      // hi: the lane holds channels 8..15
    const uint32_t sw = w[(2 * C) >> 2] >> (8 * ((2 * C) & 3));
    const uint32_t s0 = vc_w8_scale_bits(sw), s1 = vc_w8_scale_bits(sw >> 8);      // scalar arithmetic; one select per lane
    return hi ? s1 : s0;
  }
  // the same for a pair index that an unrolled loop makes a constant (vc_gemm_rows_body.h walks k-tiles, not pairs)
  __device__ __forceinline__ uint32_t scale_at(int c, int hi) const {
    const uint32_t sw = w[(2 * c) >> 2] >> (8 * ((2 * c) & 3));
    const uint32_t s0 = vc_w8_scale_bits(sw), s1 = vc_w8_scale_bits(sw >> 8);
    return hi ? s1 : s0;
  }
};
// k-tile 2 c + H of a pair from the lane's 16 bytes
template <int H>
__device__ __forceinline__ uint4 w8w_frag(const uint4& pw, uint32_t sc) {
  const uint32_t d0 = H == 0 ? pw.x : pw.z, d1 = H == 0 ? pw.y : pw.w;
  uint4 w;
  w.x = vc_w8_cvt(d0, 0, sc);
  w.y = vc_w8_cvt(d0, 1, sc);
  w.z = vc_w8_cvt(d1, 0, sc);
  w.w = vc_w8_cvt(d1, 1, sc);
  return w;
}

// The shared body (vc_gemm_wds_body.h) on the pair planes: KPW / 2 pairs per tile and wave, all requested up front (half the registers
// of the image's fragments), the side bytes on their way with n_active, each fragment rebuilt right before its MFMAs.  grid.z = 1.
// The hooks and the body are text in vc_gemm_wds_w8_body.h, shared with the FFN up-projection's kernel below.
template <int KPW, int RT, int EPI>
__global__ __launch_bounds__(512) void rows_gemm_wds_w8_k(const W8Args wa) {
#include "vc_gemm_wds_w8_body.h"
}
// The same text with the FFN up-projection's epilogue (bias, ReLU, bf16 store into the activation rows): option "w8u", the pair planes
// of W1.  A kernel of its own name: rows_gemm_wds_w8_k stays the twelve FFN-down / QKV instantiations of option "w8w".
template <int KPW, int RT>
__global__ __launch_bounds__(512) void rows_gemm_wds_w8u_k(const W8Args wa) {
  constexpr int EPI = EPI_RELU;
#include "vc_gemm_wds_w8_body.h"
}

int vc_gemm_wd_w8_ok(int K, int dtype, int ksplit) {
  if (dtype != VC_DTYPE_BF16) return 0;
  const int kpw = vc_gemm_wd_kpw(K, dtype, ksplit);
  return (kpw == 2 || kpw == 4 || kpw == 8) ? 1 : 0;
}

template <int KPW, int RT, int EPI>
static hipError_t launch_wds_w8(const W8Args& wa, int ksplit, hipStream_t s) {
  void (*kern)(const W8Args);
  if constexpr (EPI == EPI_RELU) kern = rows_gemm_wds_w8u_k<KPW, RT>;
  else kern = rows_gemm_wds_w8_k<KPW, RT, EPI>;
  constexpr size_t lds = (size_t)8 * 2 * RT * 64 * sizeof(f32x4) + (size_t)8 * RT * 16 * 128;      // the image kernel's: reduction + X stages
  // (this launcher asks from exactly 64 KB on, as the image launcher does: RT = 2 is 65 536 bytes)
  static size_t granted[16] = {0};           // per instantiation and device
  if (hipError_t e = grant_lds(reinterpret_cast<const void*>(kern), granted, lds, 64 * 1024 - 1); e != hipSuccess) return e;
  ++vc_launch_counts[VC_LC_WD];                // the form the image kernel counts in
  ++vc_launch_counts[EPI == EPI_RELU ? VC_LC_W8_UP : VC_LC_W8_WIDE];      // FFN-up (option "w8u") has a slot of its own
  hipLaunchKernelGGL(kern, dim3((wa.g.n_tiles + 1) / 2, ksplit, 1), dim3(512), lds, s, wa);
  return hipGetLastError();
}
template <int KPW, int RT>
static hipError_t launch_wds_w8_epi(const W8Args& wa, int epi, int ksplit, hipStream_t s) {
  switch (epi) {
    case EPI_QKV16: return launch_wds_w8<KPW, RT, EPI_QKV16>(wa, ksplit, s);
    case EPI_PART: return launch_wds_w8<KPW, RT, EPI_PART>(wa, ksplit, s);
    case EPI_RELU: return ksplit == 1 ? launch_wds_w8<KPW, RT, EPI_RELU>(wa, ksplit, s) : hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
}
template <int KPW>
static hipError_t launch_wds_w8_rt(const W8Args& wa, int epi, int ksplit, hipStream_t s) {
  if (wa.g.n_rows <= 2 * VC_ROWS) return launch_wds_w8_epi<KPW, 2>(wa, epi, ksplit, s);      // row tiles in flight, as vc_launch_gemm_wd
  return launch_wds_w8_epi<KPW, 4>(wa, epi, ksplit, s);
}
// vc_launch_gemm_wd's staged form on the pair planes of a.Wp's 16-channel image (a.n_tiles tiles x a.KT k-tiles, packed whole by
// vc_launch_w8w_pack): the same arguments, grid and LDS.
hipError_t vc_launch_gemm_wd_w8(const GemmArgs& a, const uint4* planes, const uint8_t* side, int epi, int ksplit, hipStream_t s) {
  if (a.n_rows < 1 || a.n_rows > 4 * VC_ROWS || !planes || !side || !a.wd_stage) return hipErrorInvalidValue;
  if (!vc_gemm_wd_w8_ok(a.K, VC_DTYPE_BF16, ksplit) || a.KT * 32 != a.K || a.n_tiles < 1) return hipErrorInvalidValue;
  W8Args wa;
  wa.g = a;
  wa.planes = planes;
  wa.side = reinterpret_cast<const uint32_t*>(side);      // n_tiles x KT bytes, KT a multiple of 16: whole aligned words
  switch (vc_gemm_wd_kpw(a.K, VC_DTYPE_BF16, ksplit)) {
    case 2: return launch_wds_w8_rt<2>(wa, epi, ksplit, s);
    case 4: return launch_wds_w8_rt<4>(wa, epi, ksplit, s);
    case 8: return launch_wds_w8_rt<8>(wa, epi, ksplit, s);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------------ the FFN up-projection of 2..16 finished rows on the pair planes (option "w8ur")
// At these row counts site_ffn_up launches rows_gemm_k<bf16_t, KTW, PRO_LNQ, EPI_RELU, NTW, NT, R2> (vc_gemm.hip) on W1, the 16-channel image
// whose pair planes option "w8u" streams at 17..64 rows.  There TH = 16, so a lane's fragment slot is its lane number, and wave w of a tile
// reads k-tiles kt0 + w KTW .. + KTW - 1, 16 bytes per lane each: KTW / 2 whole, contiguous pairs in this very lane order and KTW contiguous
// side bytes - half the weight bytes, half the fragment registers.  The shared text (vc_gemm_rows_body.h) with the pairs as the weight
// source: all requests of the wave in place of the image burst (non-temporal, always), the side bytes as scalar loads on their way with
// n_active, each fragment rebuilt right in front of its MFMA.  X staging, statistics, row_mu_out, LDS layout, MFMA order, reduction and
// epilogue are the image kernel's text and the operands are bit-identical, so every result is.  K = d in one chunk (host contract).
__device__ __forceinline__ uint4 w8w_frag_at(const uint4& pw, int h, uint32_t sc) {      // h: a constant once the k-tile loop is unrolled
  return h ? w8w_frag<1>(pw, sc) : w8w_frag<0>(pw, sc);
}
template <int KTW, int NTW, bool R2>
__global__ __launch_bounds__(256 * NTW) void rows_gemm_lnq_w8_k(const W8Args wa) {
  constexpr int EPI = EPI_RELU;
#define VC_ROWS_W8_PAIR_U4 VC_W8W_PAIR_U4
#define VC_ROWS_W8_SLOT lane
#define VC_ROWS_W8_HI8 (lane & 8)
#include "vc_gemm_rows_w8_body.h"
}

// ------------------------------------------------------------------ the QKV projection of 2..16 finished rows on the pairs of the 12-channel image (option "w8q")
// Past the row counts the paired consumer takes (rows_gemm_qp_k: 2..8 rows, 2..6 at d = 2048) site_qkv launches
// rows_gemm_k<bf16_t, KTW, PRO_LNQ, EPI_QKV, NTW, NT, R2> on Wqkv, the 12-channel image: 48 slots of 16 bytes per (tile, k-tile).  Its
// planes are the "w8q" pairs of vc_w8.h: k-tiles 2j, 2j + 1 of a tile = 768 B of codes, 16 bytes per slot, and two side bytes, one per
// PART (the tile's channels on either side of the quantiser's 8-channel block boundary).
// Packer: one wave per pair, lanes 48..63 idle (they take part in the reductions with neutral values and store nothing); image =
// consecutive 768 B fragments (pair P = fragments 2 P, 2 P + 1), the tile of pair P is P / (KT / 2).  counts[0] += pairs refused.
__global__ __launch_bounds__(64) void w8q_pack_k(const uint4* __restrict__ img, uint4* __restrict__ planes, unsigned char* __restrict__ side,
                                                  int pairs_per_tile, unsigned int* __restrict__ counts) {
  const long P = blockIdx.x;
  const int u = threadIdx.x;
  const bool on = u < VC_W8Q_SLOTS;
  const int odd = (int)((P / pairs_per_tile) & 1);
  const int part = vc_w8q_part(u % 12, odd);
  uint32_t w[2][4];
  int mn = 256, mx = -1;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint4 v = on ? img[(P * 2 + h) * VC_W8Q_SLOTS + u] : make_uint4(0u, 0u, 0u, 0u);
    w[h][0] = v.x; w[h][1] = v.y; w[h][2] = v.z; w[h][3] = v.w;
    int a, b;
    vc_w8_minmax(w[h], &a, &b);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  int shift[2], refused = 0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {        // the two parts, each over its own lanes
    const bool mine = on && part == q;
    const int mnq = wave_min_i(mine ? mn : 256);
    const int mxq = -wave_min_i(mine ? -mx : 1);
    const int top = wave_sum_i(mine ? (vc_w8_top111(w[0], mxq) | vc_w8_top111(w[1], mxq)) : 0);
    int ok;
    shift[q] = vc_w8_shift(mnq, mxq, top, &ok);
    refused |= ok ? 0 : 1;
  }
  uint32_t c[4];
  const int bad = vc_w8w_encode_lane(w, part ? shift[1] : shift[0], c);
  refused |= wave_sum_i(on ? bad : 0) > 0 ? 1 : 0;
  if (on) planes[P * VC_W8Q_PAIR_U4 + u] = make_uint4(c[0], c[1], c[2], c[3]);
  if (u < 2) side[P * 2 + u] = (unsigned char)vc_w8_side(u == 0 ? shift[0] : shift[1]);
  if (u == 0 && refused) atomicAdd(counts, 1u);
}
// counts[1] += dwords that do not decode to the image's (the conversion the GEMM uses)
__global__ __launch_bounds__(64) void w8q_check_k(const uint4* __restrict__ img, const uint4* __restrict__ planes,
                                                   const unsigned char* __restrict__ side, int pairs_per_tile, unsigned int* __restrict__ counts) {
  const long P = blockIdx.x;
  const int u = threadIdx.x;
  const bool on = u < VC_W8Q_SLOTS;
  const int us = on ? u : 0;      // idle lanes re-read slot 0 and count nothing
  const int odd = (int)((P / pairs_per_tile) & 1);
  const uint4 pc = planes[P * VC_W8Q_PAIR_U4 + us];
  const uint32_t c[4] = {pc.x, pc.y, pc.z, pc.w};
  uint32_t w[2][4];
  vc_w8w_decode_lane(c, side[P * 2 + vc_w8q_part(us % 12, odd)], w);
  int bad = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint4 v = img[(P * 2 + h) * VC_W8Q_SLOTS + us];
    bad += (w[h][0] != v.x) + (w[h][1] != v.y) + (w[h][2] != v.z) + (w[h][3] != v.w);
  }
  bad = wave_sum_i(on ? bad : 0);
  if (u == 0 && bad) atomicAdd(counts + 1, (unsigned int)bad);
}
// pair planes of a 12-channel bf16 image of KT k-tiles per tile (n_pairs = tiles x KT / 2)
hipError_t vc_launch_w8q_pack(const uint4* img, long n_pairs, int KT, uint4* planes, unsigned char* side, unsigned int* counts, hipStream_t s) {
  if (n_pairs <= 0 || n_pairs > 0x7fffffffL || KT < 2 || KT % 2 != 0 || n_pairs % (KT / 2) != 0) return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(counts, 0, 2 * sizeof(unsigned int), s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(w8q_pack_k, dim3((unsigned int)n_pairs), dim3(64), 0, s, img, planes, side, KT / 2, counts);
  hipLaunchKernelGGL(w8q_check_k, dim3((unsigned int)n_pairs), dim3(64), 0, s, img, (const uint4*)planes, (const unsigned char*)side, KT / 2, counts);
  return hipGetLastError();
}
// The packer's text on a host buffer (no device): image12 = n_pairs x 1536 B of a 12-channel bf16 image of KT k-tiles per tile (pair P
// belongs to tile P / (KT / 2)), planes = n_pairs x 768 B, side = n_pairs x 2 bytes; *refused_pairs = pairs with a part off the grid.
extern "C" int vc_w8q_pack_host(const uint16_t* image12, long n_pairs, uint8_t* planes, uint8_t* side, int KT, int32_t* refused_pairs) {
  if (!image12 || !planes || !side || !refused_pairs || n_pairs < 0 || KT < 2 || KT % 2 != 0 || n_pairs % (KT / 2) != 0) return -1;
  int32_t nref = 0;
  for (long P = 0; P < n_pairs; ++P) {
    uint32_t img[2 * VC_W8Q_SLOTS * 4], codes[VC_W8Q_SLOTS * 4];
    memcpy(img, image12 + P * (2 * VC_W8Q_SLOTS * 8), sizeof img);
    nref += vc_w8q_encode_pair(img, (int)((P / (KT / 2)) & 1), codes, side + P * 2) ? 1 : 0;
    memcpy(planes + P * VC_W8Q_PAIR_BYTES, codes, sizeof codes);
  }
  *refused_pairs = nref;
  return 0;
}

// The kernel: the shared text (vc_gemm_rows_body.h) with TH = 12 and the pairs as the weight source, in the manner of rows_gemm_lnq_w8_k.
// Wave w of a tile reads k-tiles kt0 + w KTW .. + KTW - 1: KTW / 2 whole, contiguous pairs and KTW contiguous side bytes.  A lane's slot
// is the body's wslot = kg * 12 + min(m, 11): lanes with m >= 12 re-read slot 11 and the body zeroes their operand.  The lane's part
// follows from its channel m and the tile's parity (with two tiles per workgroup the parity is the wave's tile, so it is wave-uniform).
// X staging, statistics, row_mu_out, LDS layout, MFMA order, reduction and gemm_epilogue<EPI_QKV> (q to q_out, K / V straight into the
// cache) are the image kernel's text and the operands are bit-identical, so every result is.  K = d in one chunk (host contract).
// A kernel of its own name: rows_gemm_lnq_w8_k stays the nine FFN-up instantiations of option "w8ur".
template <int KTW, int NTW, bool R2>
__global__ __launch_bounds__(256 * NTW) void rows_gemm_qkvq_w8_k(const W8Args wa) {
  constexpr int EPI = EPI_QKV;
#define VC_ROWS_W8_PAIR_U4 VC_W8Q_PAIR_U4
#define VC_ROWS_W8_SLOT wslot
#define VC_ROWS_W8_HI8 ((nt & 1) ? (m >= 4) : (m >= 8))      /* the lane's part */
#include "vc_gemm_rows_w8_body.h"
}

// ------------------------------------------------------------------ the host side of the two kernels on pairs ("w8ur", "w8q")
// The one statement of "a form exists" for `rows` finished rows of an [N x K] matrix in tiles of `th` channels behind a centred copy:
// bf16, 2..16 rows, whole tiles, make_plan's k-tiles per wave (K / 32 in one slice: the largest of 16, 8, 4, 2 that divides a quarter of
// them) 4, 8 or 16 in ONE chunk - K = 512, 1024, 2048 -, and an even tile count where a workgroup takes two tiles (5 rows and up).
// Returns the k-tiles per wave, 0 = no form.
static int rows_w8_ok(int rows, int N, int K, int dtype, int th) {
  if (dtype != VC_DTYPE_BF16 || rows < 2 || rows > VC_ROWS || N < th || N % th != 0 || K < 32 || K % 32 != 0) return 0;
  const int KT = K / 32;
  int ktw = 16;
  while (ktw > 2 && KT % (4 * ktw) != 0) ktw >>= 1;
  if (KT != 4 * ktw || (ktw != 4 && ktw != 8 && ktw != 16)) return 0;
  if (rows > 4 && (N / th) % 2 != 0) return 0;
  return ktw;
}
int vc_gemm_lnq_w8_ok(int rows, int N, int K, int dtype) { return rows_w8_ok(rows, N, K, dtype, 16); }              // FFN-up: the 16-channel image W1
int vc_gemm_qkvq_w8_ok(int rows, int N, int K, int dtype) { return rows_w8_ok(rows, N, K, dtype, VC_TH_QKV); }      // QKV: the 12-channel image Wqkv

// What differs between the two launches: the kernel, its census slot, the image's tile height, the outputs its epilogue writes.
struct LnqW8Kind {
  static constexpr int TH = 16, LC = VC_LC_W8_UP_ROWS;
  template <int KTW, int NTW, bool R2> static auto kernel() { return &rows_gemm_lnq_w8_k<KTW, NTW, R2>; }
  static bool outputs_ok(const GemmArgs&) { return true; }      // (a.out: as for the image launch, the site's)
};
struct QkvqW8Kind {
  static constexpr int TH = VC_TH_QKV, LC = VC_LC_W8_QKV_ROWS;
  template <int KTW, int NTW, bool R2> static auto kernel() { return &rows_gemm_qkvq_w8_k<KTW, NTW, R2>; }
  static bool outputs_ok(const GemmArgs& a) { return a.q_out && a.kcache && a.vcache; }
};

template <class Kind, int KTW, int NTW, bool R2>
static hipError_t launch_rows_pairs(const W8Args& wa, hipStream_t s) {
  void (*kern)(const W8Args) = Kind::template kernel<KTW, NTW, R2>();
  // the image launch's (launch_dec_nt, vc_gemm.hip): X rows, the reduction area per tile, statistics
  const size_t lds = vc_gemm_lds_bytes(wa.g, VC_DTYPE_BF16, 1) + (size_t)(NTW - 1) * 4 * 64 * sizeof(f32x4);
  static size_t granted[16] = {0};   // per instantiation and device
  if (hipError_t e = grant_lds(reinterpret_cast<const void*>(kern), granted, lds); e != hipSuccess) return e;
  ++vc_launch_counts[VC_LC_ROWS_GEMM];         // the form the image kernel counts in
  ++vc_launch_counts[Kind::LC];
  hipLaunchKernelGGL(kern, dim3(wa.g.n_tiles / NTW, 1, 1), dim3(256 * NTW), lds, s, wa);
  return hipGetLastError();
}
template <class Kind, int KTW>
static hipError_t launch_rows_pairs_form(const W8Args& wa, hipStream_t s) {
  if (wa.g.mt == 4) return launch_rows_pairs<Kind, KTW, 2, true>(wa, s);       // 9..16 rows: two tiles per workgroup, two rows per wave
  if (wa.g.mt == 3) return launch_rows_pairs<Kind, KTW, 2, false>(wa, s);      // 5..8 rows: two tiles per workgroup
  return launch_rows_pairs<Kind, KTW, 1, false>(wa, s);                        // 2..4 rows
}
// vc_launch_gemm(a, bf16, PRO_LNQ, the kind's epilogue, 1, 1) on the pairs of a.Wp's image (a.n_tiles tiles x a.KT k-tiles, packed whole
// by the kind's packer): the same arguments, grid and LDS; a.mt picks the form as it does there.
template <class Kind>
static hipError_t launch_gemm_rows_pairs(const GemmArgs& a, const uint4* planes, const uint8_t* side, hipStream_t s) {
  const int ktw = rows_w8_ok(a.n_rows, a.N, a.K, VC_DTYPE_BF16, Kind::TH);
  if (!ktw || !planes || !side || a.x_in == nullptr || a.row_mu == nullptr || !Kind::outputs_ok(a)) return hipErrorInvalidValue;
  if (a.KT != 4 * ktw || a.nchunk != 1 || a.n_tiles != a.N / Kind::TH || a.r_lds < a.n_rows || a.r_lds > VC_ROWS) return hipErrorInvalidValue;
  if (a.mt != (a.n_rows > VC_FR_MAX_ROWS ? 4 : a.n_rows >= 5 ? 3 : 0)) return hipErrorInvalidValue;      // (plan_pass's rule for these rows)
  W8Args wa;
  wa.g = a;
  wa.g.x_upr_shift = -1; wa.g.att_q4_shift = -1;      // (prologues these kernels do not have)
  wa.planes = planes;
  wa.side = reinterpret_cast<const uint32_t*>(side);      // n_tiles x KT bytes, a wave's share whole aligned words
  switch (ktw) {
    case 4: return launch_rows_pairs_form<Kind, 4>(wa, s);
    case 8: return launch_rows_pairs_form<Kind, 8>(wa, s);
    case 16: return launch_rows_pairs_form<Kind, 16>(wa, s);
    default: return hipErrorInvalidValue;
  }
}
// FFN-up on the pair planes of the 16-channel image W1 (vc_launch_w8w_pack), epilogue EPI_RELU
hipError_t vc_launch_gemm_lnq_w8(const GemmArgs& a, const uint4* planes, const uint8_t* side, hipStream_t s) {
  return launch_gemm_rows_pairs<LnqW8Kind>(a, planes, side, s);
}
// QKV on the pairs of the 12-channel image Wqkv (vc_launch_w8q_pack), epilogue EPI_QKV
hipError_t vc_launch_gemm_qkvq_w8(const GemmArgs& a, const uint4* planes, const uint8_t* side, hipStream_t s) {
  return launch_gemm_rows_pairs<QkvqW8Kind>(a, planes, side, s);
}
