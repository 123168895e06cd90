// vc_gemm_wds_w8_body.h - the body of the staged wide-decode GEMM on the E4M3 PAIR planes (vc_w8.h "w8w"), written once: the hooks of
// vc_gemm_wds_body.h for that weight source, then the body itself.  NOT a header of declarations: it is the text between the braces
// of rows_gemm_wds_w8_k (FFN-down and QKV, option "w8w") and rows_gemm_wds_w8u_k (the FFN up-projection, option "w8u") in
// vc_gemm_w8.hip.  KPW / 2 pairs per tile and wave, all requested up front (half the registers of the image's fragments), the side
// bytes on their way with n_active, each fragment rebuilt right before its MFMAs.  grid.z = 1.
//
// The kernel supplies, in scope: KPW, RT, EPI (template or constexpr ints) and wa (const W8Args).
  using WT = bf16_t;
  constexpr bool WALL = true;
  static_assert(KPW == 2 || KPW == 4 || KPW == 8, "pairs per wave and tile: 1, 2 or 4");
  const GemmArgs& a = wa.g;
#define VC_WDS_EARLY                                                                                                                   \
  W8wSide<KPW> sb[2];                                                                                                                  \
  _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                                                        \
    sb[t].load(wa.side, (long)min(nt0 + t, a.n_tiles - 1) * a.KT + (ks * 8 + wv) * KPW);
#define VC_WDS_WDECL                                                                                                                   \
  const uint4* pp[2];                                                                                                                  \
  _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                                                      \
    const int ntc = min(nt0 + t, a.n_tiles - 1);                                                                                       \
    pp[t] = wa.planes + ((long)ntc * (a.KT >> 1) + (ktb >> 1)) * VC_W8W_PAIR_U4 + lane;                                                \
  }                                                                                                                                    \
  const int hi8 = lane & 8;                                                                                                            \
  uint4 pw[2][KPW / 2];
#define VC_WDS_WALL_LOADS                                                                                                              \
  _Pragma("unroll") for (int j = 0; j < KPW / 2; ++j)                                                                                  \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                                                      \
      pw[t][j] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(pp[t] + (size_t)j * VC_W8W_PAIR_U4))); \
  /* the pins: the side words are on their way with n_active, not behind the `active == 0` exit */                                    \
  _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                                                        \
    _Pragma("unroll") for (int i = 0; i < W8wSide<KPW>::NSW; ++i) asm volatile("" : "+s"(sb[t].w[i]));
#define VC_WDS_STEP_LOADS(c_)
#define VC_WDS_FRAG(t_, c_, h_) w8w_frag<h_>(pw[t_][c_], sb[t_].template scale<c_>(hi8))
#include "vc_gemm_wds_body.h"
