// vc_gemm_fr1.h - the one-row paired GEMM on packed weights: the host path shared by the packed formats (vc_packed, vc_common.h).
// (The kernels' shared body is vc_gemm_fr1_body.h.)
#pragma once
#include "vc_gemm_dev.h"

// What a packed kernel takes: the image kernel's arguments and the packed matrix in place of a.Wp.  (Each format derives its own type from
// it, so that its kernels keep their names.)
struct Fr1PackedArgs {
  GemmArgs g;
  const uint4* planes;      // groups in image order (group_u4 units each)
  const uint32_t* side;     // one byte per fragment, four per word = one word per group
};

// Packs `n_frags` fragments (a multiple of the group) of a bf16 image and checks the planes against it; counts = two device words, zeroed here.
typedef void (*vc_fr1_pack_kernel)(const uint4*, uint4*, unsigned char*, unsigned int*);
typedef void (*vc_fr1_check_kernel)(const uint4*, const uint4*, const unsigned char*, unsigned int*);
static inline hipError_t vc_fr1_launch_pack(int kind, vc_fr1_pack_kernel pack_k, vc_fr1_check_kernel check_k, const uint4* img, long n_frags,
                                            uint4* planes, unsigned char* side, unsigned int* counts, hipStream_t s) {
  const int gf = vc_packed(kind).group_frags;
  if (n_frags <= 0 || n_frags % gf != 0 || n_frags / gf > 0x7fffffffL) return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(counts, 0, 2 * sizeof(unsigned int), s);
  if (err != hipSuccess) return err;
  const unsigned int groups = (unsigned int)(n_frags / gf);
  hipLaunchKernelGGL(pack_k, dim3(groups), dim3(64), 0, s, img, planes, side, counts);
  hipLaunchKernelGGL(check_k, dim3(groups), dim3(64), 0, s, img, (const uint4*)planes, (const unsigned char*)side, counts);
  return hipGetLastError();
}

// vc_launch_gemm_fr1 on the packed form of a.Wp's image (`planes`, `side` from the kind's packer over the whole image).
// Kind: Args (the kernels' argument type), KIND (VC_PK_*), kernel<NG, NW, PRO, EPI>() (NG = groups per wave).
template <class Kind>
static hipError_t vc_fr1_launch_packed(const GemmArgs& a0, const uint4* planes, const uint32_t* side, int pro, int epi, hipStream_t s) {
  const bool qkv = pro == PRO_LN && epi == EPI_QKV;
  if (!qkv && !(pro == PRO_PLAIN && epi == EPI_RES)) return hipErrorInvalidValue;
  const int nw = qkv ? 4 : VC_FR_WAVES;
  const int ng = vc_gemm_packed_fr1_ng(Kind::KIND, a0.N, a0.K, VC_DTYPE_BF16, nw);
  if (!ng || a0.n_rows != 1 || !planes || !side) return hipErrorInvalidValue;
  typename Kind::Args wa;
  wa.g = a0;
  wa.g.n_tiles = a0.N / VC_TH_RES;
  wa.g.KT = a0.K / 32;
  wa.planes = planes;
  wa.side = side;
  void (*kern)(const typename Kind::Args) = nullptr;
#define VC_FR1_PACKED_CASE(G_) case G_:                                                                                                 \
    kern = qkv ? Kind::template kernel<G_, 4, PRO_LN, EPI_QKV>() : Kind::template kernel<G_, VC_FR_WAVES, PRO_PLAIN, EPI_RES>(); break;
  switch (ng) {
    VC_FR1_PACKED_CASE(1) VC_FR1_PACKED_CASE(2) VC_FR1_PACKED_CASE(4)
    default: return hipErrorInvalidValue;
  }
#undef VC_FR1_PACKED_CASE
  const size_t lds = (size_t)a0.K * sizeof(bf16_t) + (size_t)nw * 4 * sizeof(f32x4) + (size_t)nw * 3 * sizeof(float);
  ++vc_launch_counts[VC_LC_ROW_GEMM_FR1];      // the form the image kernel counts in
  ++vc_launch_counts[vc_packed(Kind::KIND).lc];
  hipLaunchKernelGGL(kern, dim3(wa.g.n_tiles), dim3(64 * nw), lds, s, wa);
  return hipGetLastError();
}
