// vc_gemm_rows_w8_body.h - the body of the rows-GEMM behind a centred copy on E4M3 PAIRS (vc_w8.h "w8w" / "w8q"), written once: the
// hooks of vc_gemm_rows_body.h for that weight source, then the body itself.  NOT a header of declarations: it is the text between the
// braces of rows_gemm_lnq_w8_k (the FFN up-projection on the pair planes of the 16-channel image W1, option "w8ur") and
// rows_gemm_qkvq_w8_k (the QKV projection on the pairs of the 12-channel image Wqkv, option "w8q") in vc_gemm_w8.hip.  Wave w of a
// tile reads k-tiles kt0 + w KTW .. + KTW - 1: KTW / 2 whole, contiguous pairs and KTW contiguous side bytes.  All requests of the wave
// stand in place of the image burst (non-temporal, always), the side bytes are scalar loads on their way with n_active, each fragment
// is rebuilt right in front of its MFMA.
//
// The kernel supplies, in scope: KTW, NTW, R2, EPI (template or constexpr) and wa (const W8Args); and three macros, #undef'd here:
//   VC_ROWS_W8_PAIR_U4   16-byte units of a pair of the image (its slots per k-tile)
//   VC_ROWS_W8_SLOT      the lane's slot within a pair, from the body's lane / wslot
//   VC_ROWS_W8_HI8       whether the lane's channel takes the pair's second side byte, from the body's lane / m / nt
  using WT = bf16_t;
  constexpr int PRO = PRO_LNQ, NP = VC_MAX_KSPLIT;
  static_assert(KTW == 4 || KTW == 8 || KTW == 16, "pairs per wave and tile: 2, 4 or 8");
  const GemmArgs& a = wa.g;
  /* the wave's side bytes: scalar operands, first needed long after the burst is out */
#define VC_ROWS_EARLY                                                                                                                  \
  W8wSide<KTW> sd8;                                                                                                                    \
  sd8.load(wa.side, (long)nt * a.KT + kt0 + wave * KTW);
#define VC_ROWS_WDECL                                                                                                                  \
  const uint4* pbase = wa.planes + (((long)nt * a.KT + kt0 + wave * KTW) >> 1) * VC_ROWS_W8_PAIR_U4 + VC_ROWS_W8_SLOT;      /* wave-uniform + slot */ \
  const int hi8 = VC_ROWS_W8_HI8;                                                                                                      \
  uint4 pw[KTW / 2];
#define VC_ROWS_BURST                                                                                                                  \
  _Pragma("unroll") for (int j = 0; j < KTW / 2; ++j)                                                                                  \
    pw[j] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pbase + (size_t)j * VC_ROWS_W8_PAIR_U4))); \
  /* the pins: the side words are on their way with n_active, not behind the `active == 0` exit */                                    \
  _Pragma("unroll") for (int i = 0; i < W8wSide<KTW>::NSW; ++i) asm volatile("" : "+s"(sd8.w[i]));
#define VC_ROWS_FRAG(i_) uint4 wfi = w8w_frag_at(pw[(i_) >> 1], (i_) & 1, sd8.scale_at((i_) >> 1, hi8));
#define VC_ROWS_W(i_) wfi
#define VC_ROWS_REFILL(c_)
#include "vc_gemm_rows_body.h"
#undef VC_ROWS_W8_PAIR_U4
#undef VC_ROWS_W8_SLOT
#undef VC_ROWS_W8_HI8
