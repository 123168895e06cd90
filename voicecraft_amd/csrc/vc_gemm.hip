// vc_gemm.hip — weight packing and the "rows GEMM": out[r][n] = sum_k W[n][k] * X[r][k] for up to
// 16 rows (token positions) per pass, streaming W once from HBM.
//
// Replaces every F.linear on the reference decode path (models/modules/activation.py:86,:637,
// models/modules/transformer.py:386-388, models/voicecraft.py:181-185,:1085) together with the
// F.layer_norm in front of it (transformer.py:73-75) and the residual adds (transformer.py:328-329).
//
// Layout: W is stored in HBM already in MFMA A-fragment order,
//   Wp[n_tile][k_tile][lane] = 16 bytes = W[16*n_tile + (lane&15)][KW*k_tile + EPL*(lane>>4) + 0..EPL)
// so one wave-wide 16-byte load is a contiguous 1 KiB burst that feeds one MFMA with no LDS round
// trip; the 16 rows of X are the B operand, staged once per block in LDS.  At batch 1 the kernel is a
// pure HBM stream (1 FLOP/byte); the MFMA is only the cheapest way to consume 1 KiB per instruction
// and makes rows 2..16 (batched decode, prefill groups, the 3-row span switch of editing) free.
//
// LayerNorm fold.  Every LayerNorm on the path feeds a linear layer (transformer.py:328-329, voicecraft.py
// :1084-1086), and LN(x) = (x - mean) * rstd * gamma + beta is affine in x up to two per-row scalars:
//   W LN(x) + c = rstd * ( (W . gamma) x  -  mean * rowsum(W . gamma) )  +  (W beta + c)
// so the engine stores W' = W . gamma (column-scaled at load time, pack_k), wg = rowsum(W') over the
// ROUNDED elements and cb = W beta + c (fold_vecs_k).  A decode GEMM then multiplies the CENTRED, un-scaled row
// xc = x - mean(x) (one block barrier for the mean; centring BEFORE the rounding to bf16 keeps the mantissa for the
// signal when the residual stream carries a large common offset - tests/test_gpu_model.py, offset case) and applies
// rstd and the small residual mean of the rounded row in its epilogue, from two wave sums computed in the shadow of
// the weight stream.  Multi-row passes normalise once per row in ln_rows_k (x_hat = (x - mean) * rstd, no affine)
// and use the same W' / cb through the plain prologue.
//
// Block = 4 waves sharing one 16-row output tile; the waves split the block's K range 4 ways and
// reduce through LDS.  Cross-block split-K (EPI_PART) leaves fp32 partial slabs that the NEXT
// kernel's LayerNorm prologue sums (launch-boundary reduce: no atomics, deterministic) - the form of ONE-row steps.
// Steps of 2..16 rows keep whole residual rows instead (finished-row form, round 4): rows_gemm_fr_k / rows_gemm_fr2_k produce
// them, the PRO_LNW prologue of rows_gemm_k folds their LayerNorm one wave per row.
#include <algorithm>
#include "vc_common.h"

// ------------------------------------------------------------------ packing
// th = output channels per tile: 16 (every lane of the A fragment), 12 (VC_TH_QKV: lanes with
// (lane & 15) >= 12 carry no weight and nothing is stored for them - a tile is 4 x 12 fragments) or 8 (VC_TH_RES: the second
// image of the out-projection / FFN-down matrices that the finished-row producers stream, d/8 whole-K tiles).
template <typename WT>
__global__ void pack_k(const float* __restrict__ src, const float* __restrict__ colscale, WT* __restrict__ dst,
                       int N, int K, int KT, long total, int th) {
  constexpr int EPL = WTr<WT>::EPL, KW = WTr<WT>::KW;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (tile, fragment slot)
  if (idx >= total) return;
  const int spt = 4 * th;                                   // slots per (n_tile, k_tile)
  const int slot = (int)(idx % spt);
  const long tile = idx / spt;
  const int kt = (int)(tile % KT);
  const int nt = (int)(tile / KT);
  const int n = nt * th + (slot % th);
  const int k = kt * KW + EPL * (slot / th);
  WT* d = dst + idx * EPL;
#pragma unroll
  for (int j = 0; j < EPL; ++j) {
    float v = (n < N) ? src[(long)n * K + k + j] : 0.0f;
    if (colscale) v *= colscale[k + j];
    WTr<WT>::st(d + j, v);
  }
}

hipError_t vc_launch_pack(const float* src, const float* colscale, void* dst, int N, int K, int dtype, int th,
                          hipStream_t s) {
  const int n_tiles = (N + th - 1) / th;
  if (dtype == VC_DTYPE_BF16) {
    const int KT = K / 32;
    long total = (long)n_tiles * KT * 4 * th;
    hipLaunchKernelGGL(pack_k<bf16_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, colscale,
                       (bf16_t*)dst, N, K, KT, total, th);
  } else {
    const int KT = K / 16;
    long total = (long)n_tiles * KT * 4 * th;
    hipLaunchKernelGGL(pack_k<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, colscale,
                       (float*)dst, N, K, KT, total, th);
  }
  return hipGetLastError();
}

// wg[n] = sum_k WT(W[n][k] * gamma[k]) (the rounded elements the MFMA will see), cb[n] = bias[n] + sum_k W[n][k] * beta[k].
// One wave per output channel.
template <typename WT>
__global__ __launch_bounds__(256) void fold_vecs_k(const float* __restrict__ W, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ bias,
                                                   float* __restrict__ wg, float* __restrict__ cb, int N, int K) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  float sg = 0.f, sb = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float w = W[(long)n * K + k];
    WT r;
    WTr<WT>::st(&r, w * gamma[k]);
    sg += WTr<WT>::ld(&r);
    sb += w * beta[k];
  }
  sg = wave_sum(sg);
  sb = wave_sum(sb);
  if (lane == 0) { wg[n] = sg; cb[n] = bias[n] + sb; }
}
hipError_t vc_launch_fold_vecs(const float* W, const float* gamma, const float* beta, const float* bias, float* wg,
                               float* cb, int N, int K, int dtype, hipStream_t s) {
  if (dtype == VC_DTYPE_BF16)
    hipLaunchKernelGGL(fold_vecs_k<bf16_t>, dim3((N + 3) / 4), dim3(256), 0, s, W, gamma, beta, bias, wg, cb, N, K);
  else
    hipLaunchKernelGGL(fold_vecs_k<float>, dim3((N + 3) / 4), dim3(256), 0, s, W, gamma, beta, bias, wg, cb, N, K);
  return hipGetLastError();
}

template <typename WT>
__global__ void cast_k(const float* __restrict__ src, WT* __restrict__ dst, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) WTr<WT>::st(dst + i, src[i]);
}
hipError_t vc_launch_cast(const float* src, void* dst, long n, int dtype, hipStream_t s) {
  unsigned g = (unsigned)((n + 255) / 256);
  if (dtype == VC_DTYPE_BF16)
    hipLaunchKernelGGL(cast_k<bf16_t>, dim3(g), dim3(256), 0, s, src, (bf16_t*)dst, n);
  else
    hipLaunchKernelGGL(cast_k<float>, dim3(g), dim3(256), 0, s, src, (float*)dst, n);
  return hipGetLastError();
}

// ------------------------------------------------------------------ rows GEMM

#include "vc_gemm_dev.h"
#include "vc_w13.h"
#include "vc_w8.h"

// Decode-step kernel.  The dependency chain of a launch is what the ~80 launches of a step pay for, so
// the kernel is written around it: (1) everything any later stage needs from HBM - epilogue operands,
// the first row's prologue operands, the "any sequence still active" word - is requested first, in the
// order it will be consumed (a wave's loads return in order); (2) the weight burst follows immediately
// behind from a wave-uniform base (SGPR addressing: no per-load VALU address arithmetic, no register
// reuse that would make the compiler wait mid-burst); (3) a scheduling barrier keeps the prologue
// arithmetic from being hoisted into the burst; (4) only then is anything waited for.
// NTW = 2 (PRO_LNW only): TWO weight tiles per workgroup, 8 waves - waves 0..3 stream tile 2x, waves 4..7 tile 2x + 1 - sharing ONE
// staged copy of the rows.  The finished-row LayerNorm prologue reads 8 rows x 8 KB of fp32 h per workgroup out of L2: with
// one tile per workgroup that is 33.5 MB per launch, as much as the weight stream itself (measured: QKV 6.9 -> 9.1 us, FFN-up
// 7.0 -> 9.5 us against the plain prologue); two tiles halve it, and each of the 8 waves folds exactly one row.
// NT: the weight stream uses non-temporal loads (decode: every byte is read exactly once per launch).  A TEMPLATE parameter, not
// the runtime flag it used to be: with both load arms in one kernel the compiler merged them and silently dropped the hint -
// through round 3 the compiled QKV, out-projection and heads-2 forms had no non-temporal load at all, the FFN forms 15 of 16.
// R2 (NTW = 2 only): every wave folds TWO rows (w and w + 8) - passes of 9..16 finished rows.
// NP (PRO_LN only): split-K slabs the prologue requests per row - 4 (any n_parts <= VC_MAX_KSPLIT, the round-1..4 form), 2 (behind
// the out-projection's two slabs) or 0 (the row in h_in is FINISHED: no slabs, no pending bias - layer 0, and behind a producer
// that wrote whole rows).  Every workgroup of a consumer launch used to pull h + 4 slabs = 40 KB out of L2 whatever n_parts said
// (unconditional loads, unused slabs discarded by a select): 512 workgroups x 40 KB = 20 MB through the CUs' vector memory
// pipes per launch, queued IN FRONT of the 25-33 MB weight burst (round 5: in-kernel stamps, profiles/r04b_kernel_stamps_*).
template <typename WT, int KTW, int PRO, int EPI, int NTW = 1, bool NT = true, bool R2 = false, int NP = VC_MAX_KSPLIT>
__global__ __launch_bounds__(256 * NTW) void rows_gemm_k(const GemmArgs a) {
  // The text is vc_gemm_rows_body.h (shared with rows_gemm_lnq_w8_k and rows_gemm_qkvq_w8_k, vc_gemm_w8.hip); the weight source of this kernel: the image, KTW
  // 16-byte fragments per lane from a wave-uniform base, refilled per chunk.
#define VC_ROWS_EARLY
#define VC_ROWS_WDECL                                                                            \
  const uint4* wbase = a.Wp + (long)grp * a.w_group_stride + ((long)nt * a.KT + kt0 + wave * KTW) * SPT;   /* wave-uniform */ \
  uint4 wf[KTW];
#define VC_ISSUE_WEIGHTS(c_)                                                                     \
  {                                                                                              \
    const uint4* wb_ = wbase + (long)(c_) * (4 * KTW * SPT);                                      \
    if constexpr (NT) {                                                                          \
      _Pragma("unroll") for (int i = 0; i < KTW; ++i)                                            \
        wf[i] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wb_ + i * SPT + wslot))); \
    } else {                                                                                     \
      _Pragma("unroll") for (int i = 0; i < KTW; ++i) wf[i] = wb_[i * SPT + wslot];              \
    }                                                                                            \
  }
#define VC_ROWS_BURST VC_ISSUE_WEIGHTS(0);
#define VC_ROWS_FRAG(i_)
#define VC_ROWS_W(i_) wf[i_]
#define VC_ROWS_REFILL(c_) if (c_ + 1 < a.nchunk) VC_ISSUE_WEIGHTS(c_ + 1);   /* refill the same registers; co-resident blocks cover the latency */
#include "vc_gemm_rows_body.h"
#undef VC_ISSUE_WEIGHTS
}

// ------------------------------------------------------------------ finished-row producers: decode passes of 2..8 rows (9..16: also rows_gemm_fr2_k below)
// A several-row decode step (config 5's per-GPU share: 8 utterances) spent 18 % of its kernel time in two 8-workgroup
// LayerNorm launches per layer: the out-projection and the FFN down-projection leave split-K slabs, the sum of h + bias +
// 4 slabs per row is too much to redo in every consumer workgroup (320 KB each), so a launch of its own did it once.  Here
// those two producers finish their rows instead: K is NOT split across workgroups - a workgroup owns 8 output channels
// (VC_TH_RES: d/8 = 256 workgroups at d = 2048) over the whole K, its 8 waves stream K/8 each in ONE burst (the FFN
// down-projection at d = 2048: 32 fragments of 512 B per wave, 128 KB per workgroup, everything requested at once), X of
// all rows is staged in LDS (8 rows x 8192 x 2 B = 128 KB), and the epilogue adds the residual and the bias and writes the
// row once.  The consumers then fold the LayerNorm of one FINISHED row per wave (PRO_LNW): no slabs, no LayerNorm launch.
// PRO_PLAIN: X = activations (FFN down); PRO_ATT: X = merge of the attention's split partials of ALL heads (out-projection;
// NS = partials per item the loads are unrolled for, rows x NS <= 16 so that one batch of loads covers every item).
// Bounded by rows x K x sizeof(WT) <= 128 KB of LDS: 8 rows in bf16, 4 in the exact fp32 mode.
template <typename WT, int KTW, int PRO, int NS, bool P16 = false>
__global__ __launch_bounds__(64 * VC_FR_WAVES) void rows_gemm_fr_k(const GemmArgs a) {
  constexpr int GROUP = 1;
  constexpr bool CHUNKS = true;
#define VC_FR_EARLY
#define VC_FR_WDECL                                                                                                                      \
  const uint4* wbase = a.Wp + ((long)nt * a.KT + wave * KTW) * SPT;      /* wave-uniform */                                               \
  uint4 wf[KTW];
#define VC_FR_WEIGHTS(c_)                                                                        \
  {                                                                                              \
    const uint4* wb_ = wbase + (long)(c_) * (NW * KTW * SPT);                                     \
    _Pragma("unroll") for (int i = 0; i < KTW; ++i)                                              \
      wf[i] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wb_ + i * SPT + wslot))); \
  }
#define VC_FR_FRAG(J, w) const uint4 w = wf[g];      /* (fragment rows 8..15 repeat slot 7) */
#include "vc_gemm_fr_body.h"
}

// The FFN down-projection of 9..16 finished rows: X (rows x 4d elements) no longer fits the LDS of one workgroup, so K goes
// through it in TWO halves - the same LDS buffer twice - while the wave's weight fragments of BOTH halves are requested at the
// very top (2 x KTW fragments in registers: the stream never waits for the staging).  The second half's X rows are requested
// as soon as the first half has been parked (they return behind the weights: a wave's loads come back in order) and parked
// once every wave has finished reading the first half.  Same sums in the same order as rows_gemm_fr_k.
template <typename WT, int KTW>
__global__ __launch_bounds__(64 * VC_FR_WAVES) void rows_gemm_fr2_k(const GemmArgs a) {
  constexpr int GROUP = 1;
#define VC_FR2_EARLY
#define VC_FR2_WDECL                                                                                                                     \
  const uint4* wbase = a.Wp + ((long)nt * a.KT + wave * KTW) * SPT;      /* wave-uniform; the second half is NW * KTW k-tiles further */  \
  uint4 wfa[KTW], wfb[KTW];
#define VC_FR2_BURST                                                                                                                     \
  _Pragma("unroll") for (int i = 0; i < KTW; ++i)                                                                                        \
    wfa[i] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wbase + i * SPT + wslot)));             \
  _Pragma("unroll") for (int i = 0; i < KTW; ++i)                                                                                        \
    wfb[i] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wbase + (long)(NW * KTW + i) * SPT + wslot)));
#define VC_FR2_FRAG(h_, J, w) const uint4 w = (h_) ? wfb[g] : wfa[g];
#include "vc_gemm_fr2_body.h"
}
template <typename WT, int KTW>
static hipError_t launch_fr2(const GemmArgs& a, size_t lds, hipStream_t s) {
  auto kern = rows_gemm_fr2_k<WT, KTW>;
  static size_t granted[16] = {0};     // per instantiation and device
  int dev = 0;
  if (hipError_t ge = hipGetDevice(&dev); ge != hipSuccess) return ge;
  if (lds > 64 * 1024 && dev >= 0 && dev < 16 && lds > granted[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    granted[dev] = lds;
  }
  ++vc_launch_counts[VC_LC_ROWS_GEMM_FR];
  hipLaunchKernelGGL(kern, dim3(a.n_tiles), dim3(64 * VC_FR_WAVES), lds, s, a);
  return hipGetLastError();
}

template <typename WT, int KTW, int PRO, int NS, bool P16 = false>
static hipError_t launch_fr_n(const GemmArgs& a, size_t lds, hipStream_t s) {
  auto kern = rows_gemm_fr_k<WT, KTW, PRO, NS, P16>;
  if (lds > 64 * 1024) {
    static size_t granted[16] = {0};   // per instantiation and device
    int dev = 0;
    if (hipError_t ge = hipGetDevice(&dev); ge != hipSuccess) return ge;
    if (dev >= 0 && dev < 16 && lds > granted[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      granted[dev] = lds;
    }
  }
  ++vc_launch_counts[VC_LC_ROWS_GEMM_FR];
  hipLaunchKernelGGL(kern, dim3(a.n_tiles), dim3(64 * VC_FR_WAVES), lds, s, a);
  return hipGetLastError();
}
template <typename WT, int KTW>
static hipError_t launch_fr_ktw(const GemmArgs& a, int pro, size_t lds, hipStream_t s) {
  if (pro == PRO_PLAIN) return launch_fr_n<WT, KTW, PRO_PLAIN, 1>(a, lds, s);
  if constexpr (KTW <= 16) {           // the out-projection: K = d <= 2048
    if (pro == PRO_ATT) {
      if constexpr (sizeof(WT) == 2) {     // bf16 mode: the attention launch in front may have left bf16 partials (GemmArgs.att_p16)
        if (a.att_p16) {
          if (a.nsplit > 4) return launch_fr_n<WT, KTW, PRO_ATT, 8, true>(a, lds, s);
          if (a.nsplit > 2) return launch_fr_n<WT, KTW, PRO_ATT, 4, true>(a, lds, s);
          return launch_fr_n<WT, KTW, PRO_ATT, 2, true>(a, lds, s);
        }
      }
      if (a.nsplit > 4) return launch_fr_n<WT, KTW, PRO_ATT, 8>(a, lds, s);
      if (a.nsplit > 2) return launch_fr_n<WT, KTW, PRO_ATT, 4>(a, lds, s);
      return launch_fr_n<WT, KTW, PRO_ATT, 2>(a, lds, s);
    }
  }
  return hipErrorInvalidValue;
}
size_t vc_gemm_fr_lds_bytes(int rows, int K, int dtype) {
  const size_t esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  return (size_t)rows * ((size_t)K * esz + 16) + (size_t)VC_FR_WAVES * 64 * sizeof(f32x4);
}
// A finished-row producer pass: out-projection (PRO_ATT) or FFN down-projection (PRO_PLAIN) of 2..VC_FR_MAX_ROWS rows; a.Wp
// is the 8-channel-tile image of the matrix, a.h_in the residual rows, a.bias the layer's bias, a.h_out the finished rows.
// Which form a finished-row producer pass takes - 0: none (the launcher refuses it), 1: X in LDS in one piece (rows_gemm_fr_k),
// 2: K through LDS in two halves (rows_gemm_fr2_k, plain prologue only).  The ONE statement of the constraints: the launcher
// below and the engine's pass planning (vc_engine.hip fr_max_rows, checked for every model width by tests/test_plan_cpu.py
// through vc_debug_plan) both go through it.
int vc_gemm_fr_form(int rows, int N, int K, int dtype, int pro, int nsplit) {
  const int KW = dtype == VC_DTYPE_BF16 ? 32 : 16, esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  if (rows < 1 || rows > VC_ROWS || N % VC_TH_RES != 0 || K % KW != 0) return 0;
  const int KT = K / KW;
  const long upr = (long)K * esz / 16, cap = 16L * 64 * VC_FR_WAVES;        // 16-byte units of X per row; units a workgroup stages per piece
  const size_t lds_max = 160 * 1024;
  if (pro == PRO_ATT) {        // the out-projection merging split partials: K = d <= 2048 (a wave's share <= 16 fragments), one batch of loads
    const int ns = nsplit > 4 ? 8 : nsplit > 2 ? 4 : 2;
    if (nsplit < 1 || nsplit > 8 || rows * ns > 16 || (long)rows * (K / 4) > 16L / ns * 64 * VC_FR_WAVES) return 0;
    if (KT % VC_FR_WAVES != 0 || KT / VC_FR_WAVES > 16) return 0;
    return vc_gemm_fr_lds_bytes(rows, K, dtype) <= lds_max ? 1 : 0;
  }
  if (pro != PRO_PLAIN) return 0;
  if (KT % VC_FR_WAVES == 0 && rows * upr <= cap && vc_gemm_fr_lds_bytes(rows, K, dtype) <= lds_max) return 1;
  const int k2 = KT / (2 * VC_FR_WAVES);
  if (KT % (2 * VC_FR_WAVES) == 0 && (k2 == 2 || k2 == 4 || k2 == 8 || k2 == 16) && rows * (upr / 2) <= cap &&
      vc_gemm_fr_lds_bytes(rows, K / 2, dtype) <= lds_max)
    return 2;
  return 0;
}

hipError_t vc_launch_gemm_fr(const GemmArgs& a0, int dtype, int pro, hipStream_t s) {
  const int form = vc_gemm_fr_form(a0.n_rows, a0.N, a0.K, dtype, pro, a0.nsplit);
  if (form == 0) return hipErrorInvalidValue;
  GemmArgs a = a0;
  const int KW = dtype == VC_DTYPE_BF16 ? 32 : 16;
  a.n_tiles = a.N / VC_TH_RES;
  a.KT = a.K / KW;
  a.r_lds = a.n_rows;
  int ktw = 32;
  while (ktw > 1 && a.KT % (VC_FR_WAVES * ktw) != 0) ktw >>= 1;
  if (a.KT % (VC_FR_WAVES * ktw) != 0 || a.N % VC_TH_RES != 0 || a.n_rows < 1 || a.n_rows > VC_ROWS) return hipErrorInvalidValue;
  a.nchunk = a.KT / (VC_FR_WAVES * ktw);
  const int esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  const int upr = a.K * esz / 16, q4 = a.K / 4;
  a.x_upr_shift = -1; a.att_q4_shift = -1;
  for (int sft = 0; sft < 20; ++sft) {
    if ((1 << sft) == upr) a.x_upr_shift = sft;
    if ((1 << sft) == q4) a.att_q4_shift = sft;
  }
  if (form == 2) {
    // X does not fit the LDS of a workgroup in one piece: K in two halves (rows_gemm_fr2_k), one burst of weights per half
    const int ktw2 = a.KT / (2 * VC_FR_WAVES);
    if (a.KT % (2 * VC_FR_WAVES) != 0 || (long)a.n_rows * (upr / 2) > 16L * 64 * VC_FR_WAVES || a.n_rows > VC_ROWS) return hipErrorInvalidValue;
    a.nchunk = 2;
    a.x_upr_shift = -1;
    for (int sft = 0; sft < 20; ++sft) if ((1 << sft) == upr / 2) a.x_upr_shift = sft;
    const size_t lds2 = vc_gemm_fr_lds_bytes(a.n_rows, a.K / 2, dtype);
#define VC_FR2_CASE(K_) case K_: return (dtype == VC_DTYPE_BF16) ? launch_fr2<bf16_t, K_>(a, lds2, s) : launch_fr2<float, K_>(a, lds2, s);
    switch (ktw2) {
      VC_FR2_CASE(2) VC_FR2_CASE(4) VC_FR2_CASE(8) VC_FR2_CASE(16)
      default: return hipErrorInvalidValue;
    }
#undef VC_FR2_CASE
  }
  if (pro == PRO_ATT && (a.nsplit < 1 || a.n_rows * (a.nsplit > 4 ? 8 : a.nsplit > 2 ? 4 : 2) > 16 || (long)a.n_rows * q4 > 16L / (a.nsplit > 4 ? 8 : a.nsplit > 2 ? 4 : 2) * 64 * VC_FR_WAVES))
    return hipErrorInvalidValue;
  const size_t lds = vc_gemm_fr_lds_bytes(a.n_rows, a.K, dtype);
#define VC_FR_CASE(K_) case K_: return (dtype == VC_DTYPE_BF16) ? launch_fr_ktw<bf16_t, K_>(a, pro, lds, s) : launch_fr_ktw<float, K_>(a, pro, lds, s);
  switch (ktw) {
    VC_FR_CASE(1) VC_FR_CASE(2) VC_FR_CASE(4) VC_FR_CASE(8) VC_FR_CASE(16) VC_FR_CASE(32)
    default: return hipErrorInvalidValue;
  }
#undef VC_FR_CASE
}

// ------------------------------------------------------------------ finished-row producer of ONE-row decode steps (round 5)
// The shared body (vc_gemm_fr1_body.h: the tile and fragment-pair arithmetic, the forms) on the 8-channel-tile image of a bf16 or fp32
// matrix: pair p of wave w = fragment pair (NPW w + p), one contiguous KB per wave instruction.
// EXACT: the matrix has exactly NW * NPW fragment pairs per tile (every real model width): no clamped addresses, no zeroed fragments.
template <typename WT, int NPW, bool EXACT, int NW, int PRO, int EPI>
__global__ __launch_bounds__(64 * NW) void row_gemm_fr1_k(const GemmArgs a) {
  constexpr int GROUP = 1;
#define VC_FR1_EARLY
#define VC_FR1_BURST                                                                                                                     \
  const uint4* wbase = a.Wp + ((long)nt * a.KT + 2 * NPW * wave) * SPT;    /* wave-uniform: a wave streams NPW consecutive KB */           \
  uint4 wf[NPW];                                                                                                                         \
  _Pragma("unroll") for (int p = 0; p < NPW; ++p) {                                                                                      \
    const int gp = EXACT ? p : min(NPW * wave + p, npairs - 1) - NPW * wave;                                                             \
    wf[p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wbase + (long)gp * (2 * SPT) + wunit))); \
  }                                                                                                                                      \
  __builtin_amdgcn_sched_barrier(0);
#define VC_FR1_FRAG(F, w)                                                              \
  uint4 w = wf[g];                                                                     \
  if constexpr (!EXACT) { if (gpr >= npairs) w = make_uint4(0u, 0u, 0u, 0u); }
#include "vc_gemm_fr1_body.h"
}
template <typename WT, int NPW, int NW, int PRO, int EPI>
static hipError_t launch_fr1_n(const GemmArgs& a, hipStream_t s) {
  auto kern = (a.KT == 2 * NW * NPW) ? row_gemm_fr1_k<WT, NPW, true, NW, PRO, EPI> : row_gemm_fr1_k<WT, NPW, false, NW, PRO, EPI>;
  const size_t lds = (size_t)a.K * sizeof(WT) + (size_t)NW * 4 * sizeof(f32x4) + (size_t)NW * 3 * sizeof(float);
  ++vc_launch_counts[VC_LC_ROW_GEMM_FR1];
  hipLaunchKernelGGL(kern, dim3(a.n_tiles), dim3(64 * NW), lds, s, a);
  return hipGetLastError();
}
// 1 when the one-row paired kernel can take an [N x K] matrix in this dtype with `nw` waves per workgroup (the engine's planning and
// the launcher agree on it)
int vc_gemm_fr1_ok(int N, int K, int dtype, int nw) {
  const int KW = dtype == VC_DTYPE_BF16 ? 32 : 16, esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  if (N % VC_TH_RES != 0 || K % (2 * KW) != 0 || (nw != 4 && nw != 8)) return 0;
  const int npairs = K / KW / 2, npw = (npairs + nw - 1) / nw;
  int cap = 1;
  while (cap < npw) cap <<= 1;
  if (cap > (nw == 4 ? 16 : 32) || (long)K * esz > 64L * 1024) return 0;      // a wave's fragments fit its registers; the row <= 4 staging registers per thread
  return 1;
}
const vc_packed_kind& vc_packed(int kind) {
  static const vc_packed_kind kinds[VC_PK_N] = {
    {VC_W13_GROUP_FRAGS, VC_W13_GROUP_U4, VC_LC_W13, vc_launch_w13_pack, vc_launch_gemm_fr1_w13, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
    {VC_W8_GROUP_FRAGS, VC_W8_GROUP_U4, VC_LC_W8, vc_launch_w8_pack, vc_launch_gemm_fr1_w8, vc_launch_gemm_frp_w8, vc_launch_gemm_qp_w8,
     vc_gemm_frp_w8_ng, vc_gemm_qp_w8_ng, vc_launch_gemm_wd_w8, vc_gemm_wd_w8_ok, vc_launch_gemm_fr_w8, vc_gemm_fr_w8_ng,
     vc_launch_gemm_lnq_w8, vc_gemm_lnq_w8_ok, vc_launch_gemm_qkvq_w8, vc_gemm_qkvq_w8_ok},
  };
  return kinds[kind];
}
// Groups per wave of a packed form for an [N x K] matrix on the one-row paired kernel with `nw` waves, 0 = no form: bf16, the kernel's
// own form (vc_gemm_fr1_ok) with EXACTLY nw x NG groups of fragment pairs per tile.  The engine's packing and the launchers agree on it.
int vc_gemm_packed_fr1_ng(int kind, int N, int K, int dtype, int nw) {
  if (kind < 0 || kind >= VC_PK_N || dtype != VC_DTYPE_BF16 || !vc_gemm_fr1_ok(N, K, dtype, nw)) return 0;
  const int npairs = K / 64, per = nw * vc_packed(kind).group_frags;
  if (npairs % per != 0) return 0;
  const int ng = npairs / per;
  return (ng == 1 || ng == 2 || ng == 4) ? ng : 0;
}
// ONE row.  pro / epi = PRO_PLAIN / EPI_RES: h_out[n] = h_in[n] + bias[n] + sum_k W[n][k] x[k] (a.x_in = the row, WT [K]; 8 waves);
// PRO_LN / EPI_QKV: the QKV projection of the finished row a.h_in (LayerNorm fold; 4 waves).  a.Wp = the 8-channel-tile image.
hipError_t vc_launch_gemm_fr1(const GemmArgs& a0, int dtype, int pro, int epi, hipStream_t s) {
  const bool qkv = pro == PRO_LN && epi == EPI_QKV;
  if (!qkv && !(pro == PRO_PLAIN && epi == EPI_RES)) return hipErrorInvalidValue;
  const int nw = qkv ? 4 : VC_FR_WAVES;        // (the QKV form with eight waves measured +1.9 % per step, profiles/r05*: four stay)
  if (!vc_gemm_fr1_ok(a0.N, a0.K, dtype, nw) || a0.n_rows != 1) return hipErrorInvalidValue;
  GemmArgs a = a0;
  const int KW = dtype == VC_DTYPE_BF16 ? 32 : 16;
  a.n_tiles = a.N / VC_TH_RES;
  a.KT = a.K / KW;
  const int npairs = a.KT / 2, npw = (npairs + nw - 1) / nw;
  int cap = 1;
  while (cap < npw) cap <<= 1;
#define VC_FR1_CASE(P_) case P_:                                                                                        \
    if (qkv) return (dtype == VC_DTYPE_BF16) ? launch_fr1_n<bf16_t, P_, 4, PRO_LN, EPI_QKV>(a, s) : launch_fr1_n<float, P_, 4, PRO_LN, EPI_QKV>(a, s);   \
    return (dtype == VC_DTYPE_BF16) ? launch_fr1_n<bf16_t, P_, VC_FR_WAVES, PRO_PLAIN, EPI_RES>(a, s) : launch_fr1_n<float, P_, VC_FR_WAVES, PRO_PLAIN, EPI_RES>(a, s);
  switch (cap) {
    VC_FR1_CASE(1) VC_FR1_CASE(2) VC_FR1_CASE(4) VC_FR1_CASE(8) VC_FR1_CASE(16)
    case 32:
      if (qkv) return hipErrorInvalidValue;      // (K <= 2048 there: at most 16 pairs per wave of four)
      return (dtype == VC_DTYPE_BF16) ? launch_fr1_n<bf16_t, 32, VC_FR_WAVES, PRO_PLAIN, EPI_RES>(a, s) : launch_fr1_n<float, 32, VC_FR_WAVES, PRO_PLAIN, EPI_RES>(a, s);
    default: return hipErrorInvalidValue;
  }
#undef VC_FR1_CASE
}

// ------------------------------------------------------------------ finished-row producer of 2..8-row steps, paired (round 5)
// The same two-k-tiles-per-fragment trick for up to EIGHT rows: the B operand has 16 columns, so row r takes columns 2r (x over
// k-tile 2p) and 2r + 1 (x over k-tile 2p + 1); D[c][2r] + D[c + 8][2r + 1] is channel c of row r.  rows_gemm_fr_k (above) issues one
// 512-byte fragment per wave instruction for the same 8-channel tiles; here every instruction is a full KB - half the vector-memory
// instructions of the FFN down-projection of config 5's per-GPU share (8 rows).  X rows sit in LDS at r K + 16 (r & 3) + 128 (r >> 2)
// bytes, so that the sixteen 16-byte reads of a lane group (8 rows x 2 k-tile parities) fall into sixteen different bank quads.
// RMAX = rows the staging is unrolled for (4 or 8); K x sizeof(WT) / 16 is a power of two (host contract).
template <typename WT, int NPW, int RMAX>
__global__ __launch_bounds__(64 * VC_FR_WAVES) void rows_gemm_frp_k(const GemmArgs a) {
  constexpr int GROUP = 1;
#define VC_FRP_EARLY
#define VC_FRP_BURST                                                                                                                     \
  const uint4* wbase = a.Wp + ((long)nt * a.KT + 2 * NPW * wave) * SPT;                                                                  \
  uint4 wf[NPW];                                                                                                                         \
  _Pragma("unroll") for (int p = 0; p < NPW; ++p)                                                                                        \
    wf[p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wbase + (long)p * (2 * SPT) + wunit)));  \
  __builtin_amdgcn_sched_barrier(0);
#define VC_FRP_FRAG(F, w) const uint4 w = wf[g];
#include "vc_gemm_frp_body.h"
}
template <typename WT, int NPW, int RMAX>
static hipError_t launch_frp_n(const GemmArgs& a, hipStream_t s) {
  auto kern = rows_gemm_frp_k<WT, NPW, RMAX>;
  const size_t lds = (size_t)RMAX * a.K * sizeof(WT) + 256 + (size_t)VC_FR_WAVES * RMAX * 4 * sizeof(f32x4);
  if (lds > 64 * 1024) {
    static size_t granted[16] = {0};   // per instantiation and device
    int dev = 0;
    if (hipError_t ge = hipGetDevice(&dev); ge != hipSuccess) return ge;
    if (dev >= 0 && dev < 16 && lds > granted[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      granted[dev] = lds;
    }
  }
  ++vc_launch_counts[VC_LC_ROWS_GEMM_FRP];
  hipLaunchKernelGGL(kern, dim3(a.n_tiles), dim3(64 * VC_FR_WAVES), lds, s, a);
  return hipGetLastError();
}
// 1 when the paired producer can take `rows` rows of an [N x K] matrix: whole fragment pairs per wave, a power-of-two unit count per
// row, X within the LDS of one workgroup
int vc_gemm_frp_ok(int rows, int N, int K, int dtype) {
  const int KW = dtype == VC_DTYPE_BF16 ? 32 : 16, esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  if (rows < 2 || rows > 8 || N % VC_TH_RES != 0 || K % (2 * KW * VC_FR_WAVES) != 0) return 0;
  const int npw = K / (2 * KW * VC_FR_WAVES), upr = K * esz / 16, rmax = rows <= 4 ? 4 : 8;
  if ((npw & (npw - 1)) != 0 || npw > 32 || (upr & (upr - 1)) != 0) return 0;
  if (rmax * ((npw * 8 + 63) / 64) > 16) return 0;                                    // staging registers per thread
  return (size_t)rmax * K * esz + 256 + (size_t)VC_FR_WAVES * rmax * 64 <= 160 * 1024 ? 1 : 0;
}
hipError_t vc_launch_gemm_frp(const GemmArgs& a0, int dtype, hipStream_t s) {
  if (!vc_gemm_frp_ok(a0.n_rows, a0.N, a0.K, dtype)) return hipErrorInvalidValue;
  GemmArgs a = a0;
  const int KW = dtype == VC_DTYPE_BF16 ? 32 : 16, esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  a.n_tiles = a.N / VC_TH_RES;
  a.KT = a.K / KW;
  const int npw = a.KT / (2 * VC_FR_WAVES), upr = a.K * esz / 16;
  a.x_upr_shift = 0;
  while ((1 << a.x_upr_shift) < upr) ++a.x_upr_shift;
  const bool r4 = a.n_rows <= 4;
#define VC_FRP_CASE(P_) case P_:                                                                                         \
    if (r4) return (dtype == VC_DTYPE_BF16) ? launch_frp_n<bf16_t, P_, 4>(a, s) : launch_frp_n<float, P_, 4>(a, s);       \
    return (dtype == VC_DTYPE_BF16) ? launch_frp_n<bf16_t, P_, 8>(a, s) : launch_frp_n<float, P_, 8>(a, s);
  switch (npw) {
    VC_FRP_CASE(1) VC_FRP_CASE(2) VC_FRP_CASE(4) VC_FRP_CASE(8) VC_FRP_CASE(16)
    case 32: if (r4) return (dtype == VC_DTYPE_BF16) ? launch_frp_n<bf16_t, 32, 4>(a, s) : launch_frp_n<float, 32, 4>(a, s);
             return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
  }
#undef VC_FRP_CASE
}

// ------------------------------------------------------------------ QKV projection of 2..8 finished rows, paired (round 6)
// The consumer the round-5 verdict asked for (item 3: "full-lane QKV tiles at 2..16 rows").  rows_gemm_k runs the QKV projection on the one-row
// kernels' 12-channel tiles: a quarter of every weight request's lanes is idle, the launch pays the vector-memory instructions of a 33.6 MB
// stream for 25.2 MB.  Here the 8-channel image of the one-row
// paired form (Wqkv8, option "qkv_p8") is read with two k-tiles per MFMA fragment exactly as rows_gemm_frp_k reads W2 - every lane's 16 bytes are
// weights -, a workgroup owns THREE consecutive tiles (24 channels: d / 8 workgroups, one per CU at d = 2048, the rows staged once for all three)
// and its 8 waves stream K / 8 of each tile in one burst.  The rows are the producers' centred copy q = WT(h - c) (PRO_LNQ, rows_gemm_k above):
// wave r copies row r to LDS as it is - whole 1 KB requests, no conversion - and sums its values and squares on the way; the epilogue applies
// rstd (acc - mean(q) rowsum(W')) + cb and the QKV scatter (q to its buffer, K / V into the caches).  B operand: row r takes columns 2r
// (k-tile 2p) and 2r + 1 (k-tile 2p + 1); D[c][2r] + D[c + 8][2r + 1] is channel c of row r, the other elements are cross terms nobody reads.
// NPW = fragment pairs per wave and tile = K sizeof(WT) / 1024 = the row's 16-byte units per lane; RMAX = 4 or 8 rows.
template <typename WT, int NPW, int RMAX>
__global__ __launch_bounds__(64 * VC_FR_WAVES) void rows_gemm_qp_k(const GemmArgs a) {
  constexpr int GROUP = 1;
#define VC_QP_EARLY
  /* the wave's share of the three tiles in one burst: pair p of wave w = fragment pair (NPW w + p) of each tile */
#define VC_QP_BURST                                                                                                                      \
  const uint4* wbase = a.Wp + ((long)blockIdx.x * NTQ * a.KT + 2 * NPW * wave) * SPT;                                                    \
  uint4 wf[NTQ][NPW];                                                                                                                    \
  _Pragma("unroll") for (int t = 0; t < NTQ; ++t)                                                                                        \
    _Pragma("unroll") for (int p = 0; p < NPW; ++p)                                                                                      \
      wf[t][p] = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wbase + ((long)t * a.KT + 2 * p) * SPT + wunit))); \
  __builtin_amdgcn_sched_barrier(0);
#define VC_QP_FRAG(t, F, w) const uint4 w = wf[t][g];
#include "vc_gemm_qp_body.h"
}
template <typename WT, int NPW, int RMAX>
static hipError_t launch_qp_n(const GemmArgs& a, hipStream_t s) {
  auto kern = rows_gemm_qp_k<WT, NPW, RMAX>;
  const size_t lds = (size_t)RMAX * a.K * sizeof(WT) + 256 + (size_t)VC_FR_WAVES * RMAX * 3 * 4 * sizeof(f32x4) + (size_t)RMAX * 2 * sizeof(float);
  if (lds > 64 * 1024) {
    static size_t granted[16] = {0};   // per instantiation and device
    int dev = 0;
    if (hipError_t ge = hipGetDevice(&dev); ge != hipSuccess) return ge;
    if (dev >= 0 && dev < 16 && lds > granted[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      granted[dev] = lds;
    }
  }
  ++vc_launch_counts[VC_LC_ROWS_GEMM_QP];
  hipLaunchKernelGGL(kern, dim3(a.n_tiles / 3), dim3(64 * VC_FR_WAVES), lds, s, a);
  return hipGetLastError();
}
// 1 when the paired QKV consumer can take `rows` rows of the centred copy through an [N x K] matrix: three 8-channel tiles per workgroup, a row of
// whole 1 KB wave requests (1, 2, 4 or 8 of them), everything within the LDS of one workgroup
int vc_gemm_qp_ok(int rows, int N, int K, int dtype) {
  const int esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  if (rows < 2 || rows > 8 || N % (3 * VC_TH_RES) != 0 || (K * esz) % 1024 != 0) return 0;
  const int npw = K * esz / 1024, rmax = rows <= 4 ? 4 : 8;
  if ((npw & (npw - 1)) != 0 || npw > 8) return 0;
  return (size_t)rmax * K * esz + 256 + (size_t)VC_FR_WAVES * rmax * 3 * 64 + (size_t)rmax * 8 <= 160 * 1024 ? 1 : 0;
}
// X = a.x_in (the producers' centred copy, WT [rows][x_ld]), a.row_mu its constants, a.Wp the 8-channel-tile image of the folded QKV matrix
hipError_t vc_launch_gemm_qp(const GemmArgs& a0, int dtype, hipStream_t s) {
  if (!vc_gemm_qp_ok(a0.n_rows, a0.N, a0.K, dtype) || a0.x_in == nullptr || a0.row_mu == nullptr) return hipErrorInvalidValue;
  GemmArgs a = a0;
  const int KW = dtype == VC_DTYPE_BF16 ? 32 : 16, esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  a.n_tiles = a.N / VC_TH_RES;
  a.KT = a.K / KW;
  const int npw = a.K * esz / 1024;
  const bool r4 = a.n_rows <= 4;
#define VC_QP_CASE(P_) case P_:                                                                                         \
    if (r4) return (dtype == VC_DTYPE_BF16) ? launch_qp_n<bf16_t, P_, 4>(a, s) : launch_qp_n<float, P_, 4>(a, s);       \
    return (dtype == VC_DTYPE_BF16) ? launch_qp_n<bf16_t, P_, 8>(a, s) : launch_qp_n<float, P_, 8>(a, s);
  switch (npw) {
    VC_QP_CASE(1) VC_QP_CASE(2) VC_QP_CASE(4) VC_QP_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef VC_QP_CASE
}

// ------------------------------------------------------------------ wide decode passes: 17..64 rows
// (round 1's prefill kernel, kept for decode passes that carry more than one 16-row tile - 17..64 sequences: such a
// pass is still a weight stream, and here the weights are read from HBM exactly once at the decode kernel's rate.)
// Same weight fragments, but a workgroup holds NTW weight tiles (NTW x 4 waves) in registers and walks
// the pass's rows in tiles of 16, so W is streamed once per 128 rows instead of once per 16, and every
// 16-row X tile staged in LDS feeds NTW output tiles (the X traffic out of L2 - 64 KB per row tile per
// workgroup at d = 2048 - is what bounds this kernel, not HBM).  The next row tile is requested
// while the current one is in the MFMAs.  LayerNorm is hoisted into ln_rows_k (one block per row).
// (the weights are read from HBM exactly once per pass: non-temporal loads, compile-time - VC_MT_NT=0 builds the comparison twin)
#ifndef VC_MT_NT
#define VC_MT_NT 1
#endif
#if VC_MT_NT
#define VC_MT_LOADW(p_) __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p_)))
#else
#define VC_MT_LOADW(p_) (*(p_))
#endif
template <typename WT, int KTW, int PRO, int EPI, int NTW>
__global__ __launch_bounds__(256 * NTW) void rows_gemm_mt_k(const GemmArgs a) {
  using T = WTr<WT>;
  constexpr int NT = 256 * NTW;          // threads
  constexpr int XP = 16 / NTW;           // X units (16 B) a thread carries for the next row tile (64 KB per workgroup)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (*a.n_active == 0) return;          // a replayed decode step after the last sequence retired
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wv >> 2, wave = wv & 3;  // weight tile of this workgroup, K quarter
  const int nt_raw = blockIdx.x * NTW + g;
  const bool tile_ok = nt_raw < a.n_tiles;
  const int nt = tile_ok ? nt_raw : a.n_tiles - 1;
  const int ks = blockIdx.y, grp = blockIdx.z;
  const int n_rows = a.n_rows;
  const int kt_blk = a.nchunk * 4 * KTW;
  const int kt0 = ks * kt_blk;
  const int kblk = kt_blk * T::KW;
  const int k0 = kt0 * T::KW;
  const int xs = kblk * (int)sizeof(WT) + 16;
  char* xl = smem;
  f32x4* red = reinterpret_cast<f32x4*>(smem + (size_t)VC_ROWS * xs) + g * 256;
  constexpr int TH = (EPI == EPI_QKV) ? VC_TH_QKV : 16;    // see rows_gemm_k
  constexpr int SPT = 4 * TH;
  const int m = lane & 15;
  const int kg = lane >> 4;
  const bool wvalid = m < TH, nvalid = 4 * kg < TH;
  const uint4* wp = a.Wp + (long)grp * a.w_group_stride + ((long)nt * a.KT) * SPT + (kg * TH + min(m, TH - 1));
  uint4 wf[KTW];
  {
    const int kt = kt0 + wave * KTW;
#pragma unroll
    for (int i = 0; i < KTW; ++i) {
      wf[i] = VC_MT_LOADW(wp + (long)(kt + i) * SPT);
      if (TH < 16 && !wvalid) wf[i] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  const int n = nt * TH + 4 * kg;
  const int upr = kblk * (int)sizeof(WT) / 16;       // 16-byte units per X row slice
  const char* xsrc = reinterpret_cast<const char*>(a.x_in) + ((long)grp * a.x_group_stride + k0) * (long)sizeof(WT);
  const long rstride = (long)a.x_ld * (long)sizeof(WT);
  const int sh = a.x_upr_shift;
  uint4 xq0, xq1, xq2, xq3, xq4, xq5, xq6, xq7;   // explicit scalars: an indexed array is demoted to scratch
  // (the 1024-thread form runs at the 128-register cap: the reciprocal of the general row split below - a loop invariant the
  // compiler keeps in a VECTOR register although it is uniform - would be spilled across the row-tile loop; there the divisor
  // is made opaque at each use, so the few instructions are redone per tile instead)
  auto upr_div = [&]() { int u = upr; if constexpr (NTW >= 4) asm volatile("" : "+s"(u)); return u; };

  // X tile of rows [row0, row0 + nr): global -> registers (first XP * NT units) ...
#define VC_XQ_LOAD(j, dst)                                                                       \
  if constexpr ((j) < XP) {                                                                      \
    const int i_ = min((j) * NT + tid, total - 1);                                               \
    const int r_ = (sh >= 0) ? (i_ >> sh) : (i_ / upr_div());                                    \
    const int u_ = i_ - r_ * upr;                                                                \
    dst = *reinterpret_cast<const uint4*>(xsrc + (long)(row0 + r_) * rstride + (long)u_ * 16);   \
  }
#define VC_XQ_STORE(j, val)                                                                      \
  if constexpr ((j) < XP) {                                                                      \
    const int i_ = (j) * NT + tid;                                                               \
    if (i_ < total) {                                                                            \
      const int r_ = (sh >= 0) ? (i_ >> sh) : (i_ / upr_div());                                  \
      const int u_ = i_ - r_ * upr;                                                              \
      *reinterpret_cast<uint4*>(xl + (size_t)r_ * xs + (size_t)u_ * 16) = val;                   \
    }                                                                                            \
  }
  auto x_fetch = [&](int row0, int nr) {
    if constexpr (PRO == PRO_PLAIN) {
      const int total = nr * upr;
      VC_XQ_LOAD(0, xq0) VC_XQ_LOAD(1, xq1) VC_XQ_LOAD(2, xq2) VC_XQ_LOAD(3, xq3)
      VC_XQ_LOAD(4, xq4) VC_XQ_LOAD(5, xq5) VC_XQ_LOAD(6, xq6) VC_XQ_LOAD(7, xq7)
    }
  };
  // ... -> LDS (plus whatever did not fit into the XP slots, copied directly)
  auto x_park = [&](int row0, int nr) {
    if constexpr (PRO == PRO_PLAIN) {
      const int total = nr * upr;
      VC_XQ_STORE(0, xq0) VC_XQ_STORE(1, xq1) VC_XQ_STORE(2, xq2) VC_XQ_STORE(3, xq3)
      VC_XQ_STORE(4, xq4) VC_XQ_STORE(5, xq5) VC_XQ_STORE(6, xq6) VC_XQ_STORE(7, xq7)
      for (int i = XP * NT + tid; i < total; i += NT) {
        const int r = (sh >= 0) ? (i >> sh) : (i / upr_div());
        const int u = i - r * upr;
        *reinterpret_cast<uint4*>(xl + (size_t)r * xs + (size_t)u * 16) =
            *reinterpret_cast<const uint4*>(xsrc + (long)(row0 + r) * rstride + (long)u * 16);
      }
    } else {   // PRO_ATT (short passes whose attention was split): merge the partials in place
      const int q4 = kblk >> 2;
      for (int idx = tid; idx < nr * q4; idx += NT) {
        const int r = idx / q4, c = k0 + (idx - r * q4) * 4;
        const int h = c >> a.hd_shift, e = c & (a.hd - 1);
        const float2* ml = reinterpret_cast<const float2*>(a.att_ml) + (long)((row0 + r) * a.H + h) * a.nsplit;
        const float* op = a.att_o + ((long)((row0 + r) * a.H + h) * a.nsplit) * a.hd + e;
        float M = -INFINITY;
        for (int sp = 0; sp < a.nsplit; ++sp) M = fmaxf(M, ml[sp].x);
        float L = 0.f;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        for (int sp = 0; sp < a.nsplit; ++sp) {
          const float2 v = ml[sp];
          const float w = (v.x == -INFINITY) ? 0.f : expf(v.x - M);
          const float4 os = *reinterpret_cast<const float4*>(op + (long)sp * a.hd);
          L += w * v.y;
          o[0] += w * os.x; o[1] += w * os.y; o[2] += w * os.z; o[3] += w * os.w;
        }
        const float inv = (L > 0.f) ? 1.0f / L : 0.f;
        o[0] *= inv; o[1] *= inv; o[2] *= inv; o[3] *= inv;
        store4(reinterpret_cast<WT*>(xl + (size_t)r * xs) + (c - k0), o);
      }
    }
  };

  x_fetch(0, min(VC_ROWS, n_rows));
  x_park(0, min(VC_ROWS, n_rows));
  for (int row0 = 0; row0 < n_rows; row0 += VC_ROWS) {
    const int nr = min(VC_ROWS, n_rows - row0);
    const int row1 = row0 + VC_ROWS;
    const int nr1 = min(VC_ROWS, n_rows - row1);
    __syncthreads();                       // X(row0) is in LDS
    // the epilogue's operands (bias, the rows' cache slots) are requested HERE, ahead of the next X tile: asked for next
    // to the stores they are a dependent L2 round trip per 16-row tile on the critical path of every workgroup
    float4 eb = make_float4(0.f, 0.f, 0.f, 0.f);
    int epos = -1, eseq = 0;
    // (the 1024-thread form runs at the 128-register cap: there the six operand registers would spill across the MFMA loop,
    // so it asks for them after the loop, under the K-reduce barrier)
    if constexpr (NTW < 4) { if (wave == 0) epi_preload<WT, EPI>(a, row0 + min(m, nr - 1), n, grp, eb, epos, eseq); }
    if (nr1 > 0) x_fetch(row1, nr1);       // next tile on its way while this one is in the MFMAs
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int mrow = (m < nr) ? m : 0;
    const char* xrow = xl + (size_t)mrow * xs + (size_t)(lane >> 4) * 16;
    for (int c = 0; c < a.nchunk; ++c) {
      if (a.nchunk > 1) {       // several chunks: the registers only ever hold one of them
        const int kt = kt0 + (c * 4 + wave) * KTW;
#pragma unroll
        for (int i = 0; i < KTW; ++i) {
          wf[i] = VC_MT_LOADW(wp + (long)(kt + i) * SPT);
          if (TH < 16 && !wvalid) wf[i] = make_uint4(0u, 0u, 0u, 0u);
        }
      }
      const int ktl = (c * 4 + wave) * KTW;
#pragma unroll
      for (int i = 0; i < KTW; ++i) {
        const uint4 xf = *reinterpret_cast<const uint4*>(xrow + (size_t)(ktl + i) * 64);
        acc = mfma_frag(wf[i], xf, acc, (WT*)nullptr);
      }
    }
    // (... and the channel index is made opaque per tile: otherwise the epilogue's loop-invariant address arithmetic - head
    // and element of the lane's channels, 64-bit products - is hoisted out of the row-tile loop and spilled across it)
    int n_e = n;
    if constexpr (NTW >= 4) {
      asm volatile("" : "+v"(n_e));
      if (wave == 0) epi_preload<WT, EPI>(a, row0 + min(m, nr - 1), n_e, grp, eb, epos, eseq);
    }
    red[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0 && m < nr && nvalid && tile_ok) {
      const f32x4 a1 = red[64 + lane], a2 = red[128 + lane], a3 = red[192 + lane];
      acc = (acc + a1) + (a2 + a3);
      gemm_epilogue<WT, EPI>(a, acc, row0 + m, n_e, ks, grp, (int)gridDim.z, eb, epos, eseq);
    }
    __syncthreads();            // x and red are rewritten for the next tile
    if (nr1 > 0) x_park(row1, nr1);
  }
#undef VC_XQ_LOAD
#undef VC_XQ_STORE
}

// h_new = h + prev_bias + sum of split-K slabs ; x_hat = (h_new - mean) * rstd as WT (the affine part of the
// LayerNorm lives in the folded weights, see the top of this file).  One block per row.
template <typename WT>
__global__ __launch_bounds__(256) void ln_rows_k(const GemmArgs a) {
  __shared__ float s_sum[4], s_sq[4];
  const int active = *a.n_active;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = a.d;
  const int nq = d >> 2;
  const bool on0 = tid < nq, on1 = tid + 256 < nq;
  const int c0 = on0 ? tid * 4 : 0, c1 = on1 ? (tid + 256) * 4 : 0;
  // every operand is requested before anything is waited for (one round trip): the row, the bias and
  // all VC_MAX_KSPLIT slabs (unused ones are read and discarded by a select)
  const float* hp = a.h_in + (long)r * d;
  float4 x0 = *reinterpret_cast<const float4*>(hp + c0), x1 = *reinterpret_cast<const float4*>(hp + c1);
  const float4 pb0 = *reinterpret_cast<const float4*>(a.prev_bias + c0), pb1 = *reinterpret_cast<const float4*>(a.prev_bias + c1);
  float4 p0[VC_MAX_KSPLIT], p1[VC_MAX_KSPLIT];
#pragma unroll
  for (int s = 0; s < VC_MAX_KSPLIT; ++s) {
    const float* pp = a.parts + ((long)(s * a.rows_cap + r)) * d;
    p0[s] = *reinterpret_cast<const float4*>(pp + c0);
    p1[s] = *reinterpret_cast<const float4*>(pp + c1);
  }
  __builtin_amdgcn_sched_barrier(0);
  if (active == 0) return;
  if (a.has_prev_bias) {
    x0.x += pb0.x; x0.y += pb0.y; x0.z += pb0.z; x0.w += pb0.w;
    x1.x += pb1.x; x1.y += pb1.y; x1.z += pb1.z; x1.w += pb1.w;
  }
#pragma unroll
  for (int s = 0; s < VC_MAX_KSPLIT; ++s) {
    const bool u = s < a.n_parts;
    x0.x += u ? p0[s].x : 0.f; x0.y += u ? p0[s].y : 0.f; x0.z += u ? p0[s].z : 0.f; x0.w += u ? p0[s].w : 0.f;
    x1.x += u ? p1[s].x : 0.f; x1.y += u ? p1[s].y : 0.f; x1.z += u ? p1[s].z : 0.f; x1.w += u ? p1[s].w : 0.f;
  }
  const float t0 = on0 ? ((x0.x + x0.y) + (x0.z + x0.w)) : 0.f, t1 = on1 ? ((x1.x + x1.y) + (x1.z + x1.w)) : 0.f;
  const float ws = wave_sum(t0 + t1);
  if (lane == 0) s_sum[wave] = ws;
  __syncthreads();
  const float mean = ((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3])) / (float)d;
  const float dx = x0.x - mean, dy = x0.y - mean, dz = x0.z - mean, dw = x0.w - mean;
  const float ex = x1.x - mean, ey = x1.y - mean, ez = x1.z - mean, ew = x1.w - mean;
  const float q0 = on0 ? ((dx * dx + dy * dy) + (dz * dz + dw * dw)) : 0.f, q1 = on1 ? ((ex * ex + ey * ey) + (ez * ez + ew * ew)) : 0.f;
  const float wq = wave_sum(q0 + q1);
  if (lane == 0) s_sq[wave] = wq;
  __syncthreads();
  const float rstd = 1.0f / sqrtf(((s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3])) / (float)d + 1e-5f);
  WT* xo = reinterpret_cast<WT*>(a.x_out) + (long)r * d;
  if (on0) {
    if (a.h_out) *reinterpret_cast<float4*>(a.h_out + (long)r * d + c0) = x0;
    f32x4 y = {dx * rstd, dy * rstd, dz * rstd, dw * rstd};
    store4(xo + c0, y);
  }
  if (on1) {
    if (a.h_out) *reinterpret_cast<float4*>(a.h_out + (long)r * d + c1) = x1;
    f32x4 y = {ex * rstd, ey * rstd, ez * rstd, ew * rstd};
    store4(xo + c1, y);
  }
}
hipError_t vc_launch_ln_rows(const GemmArgs& a, int dtype, hipStream_t s) {
  ++vc_launch_counts[VC_LC_LN_ROWS];
  // (round 3's prefetch role of this launch - option ln_pf - left the tree in round 5: it served the slab form of 3..16-row steps, which
  // the finished-row form replaced as the default in round 4, and at 17..64 rows it measured a loss, profiles/r03j_lpf32_ab.log)
  if (dtype == VC_DTYPE_BF16) hipLaunchKernelGGL(ln_rows_k<bf16_t>, dim3(a.n_rows), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(ln_rows_k<float>, dim3(a.n_rows), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ dispatch
size_t vc_gemm_lds_bytes(const GemmArgs& a, int dtype, int ksplit) {
  const int esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
  const size_t xs = (size_t)(a.K / ksplit) * esz + 16;
  return (size_t)a.r_lds * xs + 4 * 64 * sizeof(f32x4) + VC_ROWS * 4 * 3 * sizeof(float);   // X rows, K-reduce area, LN statistics + row means
}

template <typename WT, int KTW, int PRO, int EPI, int NTW, bool NT, bool R2 = false, int NP = VC_MAX_KSPLIT>
static hipError_t launch_dec_nt(const GemmArgs& a, int dtype, int ksplit, int groups, hipStream_t s) {
  auto kern = rows_gemm_k<WT, KTW, PRO, EPI, NTW, NT, R2, NP>;
  const size_t lds = vc_gemm_lds_bytes(a, dtype, ksplit) + (size_t)(NTW - 1) * 4 * 64 * sizeof(f32x4);
  if (lds > 64 * 1024) {
    static size_t granted[16] = {0};   // per instantiation and device
    int dev = 0;
    if (hipError_t ge = hipGetDevice(&dev); ge != hipSuccess) return ge;
    if (dev >= 0 && dev < 16 && lds > granted[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      granted[dev] = lds;
    }
  }
  GemmArgs b = a;
  {
    const int esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
    const int upr = (a.K / ksplit) * esz / 16;
    const int q4 = (a.K / ksplit) / 4;
    b.x_upr_shift = -1;
    b.att_q4_shift = -1;
    for (int sft = 0; sft < 20; ++sft) {
      if ((1 << sft) == upr) b.x_upr_shift = sft;
      if ((1 << sft) == q4) b.att_q4_shift = sft;
    }
  }
  ++vc_launch_counts[VC_LC_ROWS_GEMM];
  hipLaunchKernelGGL(kern, dim3(a.n_tiles / NTW, ksplit, groups), dim3(256 * NTW), lds, s, b);
  return hipGetLastError();
}

template <typename WT, int KTW, int PRO, int EPI, int NTW = 1>
static hipError_t launch_dec(const GemmArgs& a, int dtype, int ksplit, int groups, hipStream_t s) {
  if constexpr (PRO == PRO_LN && NTW == 1) {
    // slabs the LayerNorm prologue requests per row: as many as the pass really has (round 5, -1.7..-2.8 % per one-row step; the
    // trimmed forms exist with the non-temporal weight stream only - the comparison arm nt = 0 keeps the four-slab form)
    if (a.nt) {
      if (a.n_parts == 0 && !a.has_prev_bias) return launch_dec_nt<WT, KTW, PRO, EPI, NTW, true, false, 0>(a, dtype, ksplit, groups, s);
      if (a.n_parts <= 2) return launch_dec_nt<WT, KTW, PRO, EPI, NTW, true, false, 2>(a, dtype, ksplit, groups, s);
    }
  }
  if (a.nt) return launch_dec_nt<WT, KTW, PRO, EPI, NTW, true>(a, dtype, ksplit, groups, s);
  return launch_dec_nt<WT, KTW, PRO, EPI, NTW, false>(a, dtype, ksplit, groups, s);
}

template <typename WT, int KTW, int PRO, int EPI, int NTW>
static hipError_t launch_mt_n(const GemmArgs& a, int dtype, int ksplit, int groups, hipStream_t s) {
  auto kern = rows_gemm_mt_k<WT, KTW, PRO, EPI, NTW>;
  GemmArgs b = a;
  b.r_lds = VC_ROWS;
  {
    const int esz = dtype == VC_DTYPE_BF16 ? 2 : 4;
    const int upr = (a.K / ksplit) * esz / 16;
    b.x_upr_shift = -1;
    for (int sft = 0; sft < 20; ++sft)
      if ((1 << sft) == upr) b.x_upr_shift = sft;
  }
  const size_t lds = vc_gemm_lds_bytes(b, dtype, ksplit) + (size_t)(NTW - 1) * 4 * 64 * sizeof(f32x4);
  if (lds > 64 * 1024) {
    static size_t granted[16] = {0};   // per instantiation and device
    int dev = 0;
    if (hipError_t ge = hipGetDevice(&dev); ge != hipSuccess) return ge;
    if (dev >= 0 && dev < 16 && lds > granted[dev]) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      granted[dev] = lds;
    }
  }
  ++vc_launch_counts[NTW == 4 ? VC_LC_MT4 : VC_LC_MT2];
  hipLaunchKernelGGL(kern, dim3((a.n_tiles + NTW - 1) / NTW, ksplit, groups), dim3(256 * NTW), lds, s, b);
  return hipGetLastError();
}

template <typename WT, int KTW, int PRO, int EPI>
static hipError_t launch_mt(const GemmArgs& a, int dtype, int ksplit, int groups, hipStream_t s) {
  if constexpr (PRO == PRO_LN) {
    return hipErrorInvalidValue;       // multi-tile passes take their LayerNorm from ln_rows_k
  } else {
    // two weight tiles per workgroup: twice the workgroups of the four-tile form of rounds 2-4 - every CU busy (-2.6 % / -3.0 % per
    // step at 32 / 64 rows, profiles/r05t_mt_tiles_ab.log; the four-tile form left the tree in round 6)
    return launch_mt_n<WT, KTW, PRO, EPI, 2>(a, dtype, ksplit, groups, s);
  }
}

template <typename WT, int KTW, int PRO, int EPI>
static hipError_t launch_one(const GemmArgs& a, int dtype, int ksplit, int groups, hipStream_t s) {
  if (a.mt == 2) return launch_mt<WT, KTW, PRO, EPI>(a, dtype, ksplit, groups, s);     // wide decode pass (17..64 rows)
  return launch_dec<WT, KTW, PRO, EPI>(a, dtype, ksplit, groups, s);
}

template <typename WT, int KTW>
static hipError_t launch_ktw(const GemmArgs& a, int dtype, int pro, int epi, int ksplit, int groups,
                             hipStream_t s) {
  if (pro == PRO_LN && epi == EPI_QKV) return launch_one<WT, KTW, PRO_LN, EPI_QKV>(a, dtype, ksplit, groups, s);
  if (pro == PRO_LN && epi == EPI_RELU) return launch_one<WT, KTW, PRO_LN, EPI_RELU>(a, dtype, ksplit, groups, s);
  if (pro == PRO_LN && epi == EPI_GELU) return launch_one<WT, KTW, PRO_LN, EPI_GELU>(a, dtype, ksplit, groups, s);
  if (pro == PRO_LNQ) {      // finished-row consumers on the producers' centred copy (round 6): the same three shapes as PRO_LNW below
    if (a.mt == 4 && a.n_tiles % 2 == 0 && groups == 1) {
      if (epi == EPI_QKV) return a.nt ? launch_dec_nt<WT, KTW, PRO_LNQ, EPI_QKV, 2, true, true>(a, dtype, ksplit, groups, s)
                                      : launch_dec_nt<WT, KTW, PRO_LNQ, EPI_QKV, 2, false, true>(a, dtype, ksplit, groups, s);
      if (epi == EPI_RELU) return a.nt ? launch_dec_nt<WT, KTW, PRO_LNQ, EPI_RELU, 2, true, true>(a, dtype, ksplit, groups, s)
                                       : launch_dec_nt<WT, KTW, PRO_LNQ, EPI_RELU, 2, false, true>(a, dtype, ksplit, groups, s);
    }
    if (a.n_rows > VC_FR_MAX_ROWS) return hipErrorInvalidValue;
    if (a.mt == 3 && a.n_tiles % 2 == 0 && groups == 1) {
      if (epi == EPI_QKV) return launch_dec<WT, KTW, PRO_LNQ, EPI_QKV, 2>(a, dtype, ksplit, groups, s);
      if (epi == EPI_RELU) return launch_dec<WT, KTW, PRO_LNQ, EPI_RELU, 2>(a, dtype, ksplit, groups, s);
    }
    if (epi == EPI_QKV) return launch_dec<WT, KTW, PRO_LNQ, EPI_QKV>(a, dtype, ksplit, groups, s);
    if (epi == EPI_RELU) return launch_dec<WT, KTW, PRO_LNQ, EPI_RELU>(a, dtype, ksplit, groups, s);
    if (epi == EPI_GELU) return launch_dec<WT, KTW, PRO_LNQ, EPI_GELU>(a, dtype, ksplit, groups, s);
    return hipErrorInvalidValue;
  }
  if (pro == PRO_LNW && a.mt == 4 && a.n_tiles % 2 == 0 && groups == 1) {     // ... and two rows per wave (9..16 finished rows)
    if (epi == EPI_QKV) return a.nt ? launch_dec_nt<WT, KTW, PRO_LNW, EPI_QKV, 2, true, true>(a, dtype, ksplit, groups, s)
                                    : launch_dec_nt<WT, KTW, PRO_LNW, EPI_QKV, 2, false, true>(a, dtype, ksplit, groups, s);
    if (epi == EPI_RELU) return a.nt ? launch_dec_nt<WT, KTW, PRO_LNW, EPI_RELU, 2, true, true>(a, dtype, ksplit, groups, s)
                                     : launch_dec_nt<WT, KTW, PRO_LNW, EPI_RELU, 2, false, true>(a, dtype, ksplit, groups, s);
  }
  if (pro == PRO_LNW && a.n_rows > VC_FR_MAX_ROWS) return hipErrorInvalidValue;   // (9..16 rows exist only in the two-rows-per-wave form above)
  if (pro == PRO_LNW && a.mt == 3 && a.n_tiles % 2 == 0 && groups == 1) {     // two tiles per workgroup (finished-row consumers, GemmArgs.mt)
    if (epi == EPI_QKV) return launch_dec<WT, KTW, PRO_LNW, EPI_QKV, 2>(a, dtype, ksplit, groups, s);
    if (epi == EPI_RELU) return launch_dec<WT, KTW, PRO_LNW, EPI_RELU, 2>(a, dtype, ksplit, groups, s);
  }
  if (pro == PRO_LNW && epi == EPI_QKV) return launch_dec<WT, KTW, PRO_LNW, EPI_QKV>(a, dtype, ksplit, groups, s);
  if (pro == PRO_LNW && epi == EPI_RELU) return launch_dec<WT, KTW, PRO_LNW, EPI_RELU>(a, dtype, ksplit, groups, s);
  if (pro == PRO_LNW && epi == EPI_GELU) return launch_dec<WT, KTW, PRO_LNW, EPI_GELU>(a, dtype, ksplit, groups, s);
  if (pro == PRO_ATT && epi == EPI_PART) return launch_one<WT, KTW, PRO_ATT, EPI_PART>(a, dtype, ksplit, groups, s);
  if (pro == PRO_PLAIN && epi == EPI_PART) return launch_one<WT, KTW, PRO_PLAIN, EPI_PART>(a, dtype, ksplit, groups, s);
  if (pro == PRO_PLAIN && epi == EPI_LOGITS) return launch_one<WT, KTW, PRO_PLAIN, EPI_LOGITS>(a, dtype, ksplit, groups, s);
  if (pro == PRO_PLAIN && epi == EPI_QKV) return launch_one<WT, KTW, PRO_PLAIN, EPI_QKV>(a, dtype, ksplit, groups, s);
  if (pro == PRO_PLAIN && epi == EPI_QKV16) {      // the 16-channel image: wide decode passes only here (prefill: vc_gemm_pf.hip)
    if (a.mt == 2) return launch_mt<WT, KTW, PRO_PLAIN, EPI_QKV16>(a, dtype, ksplit, groups, s);
    return hipErrorInvalidValue;
  }
  if (pro == PRO_PLAIN && epi == EPI_RELU) return launch_one<WT, KTW, PRO_PLAIN, EPI_RELU>(a, dtype, ksplit, groups, s);
  if (pro == PRO_PLAIN && epi == EPI_GELU) return launch_one<WT, KTW, PRO_PLAIN, EPI_GELU>(a, dtype, ksplit, groups, s);
  return hipErrorInvalidValue;
}

template <typename WT>
static hipError_t launch_wt(const GemmArgs& a, int dtype, int pro, int epi, int ksplit, int groups,
                            hipStream_t s) {
  // the caller fixed a.nchunk; recover KTW from KT = ksplit * nchunk * 4 * KTW
  const int ktw = a.KT / (ksplit * a.nchunk * 4);
  switch (ktw) {
    case 2: return launch_ktw<WT, 2>(a, dtype, pro, epi, ksplit, groups, s);
    case 4: return launch_ktw<WT, 4>(a, dtype, pro, epi, ksplit, groups, s);
    case 8: return launch_ktw<WT, 8>(a, dtype, pro, epi, ksplit, groups, s);
    case 16: return launch_ktw<WT, 16>(a, dtype, pro, epi, ksplit, groups, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t vc_launch_gemm(const GemmArgs& a, int dtype, int pro, int epi, int ksplit, int groups,
                          hipStream_t s) {
  if (a.mt == 1) {     // prefill pass: block GEMM
    if (groups != 1) return hipErrorInvalidValue;
    return vc_launch_gemm_blk(a, dtype, pro, epi, ksplit, s);      // vc_gemm_pf.hip
  }
  if (dtype == VC_DTYPE_BF16) return launch_wt<bf16_t>(a, dtype, pro, epi, ksplit, groups, s);
  return launch_wt<float>(a, dtype, pro, epi, ksplit, groups, s);
}
