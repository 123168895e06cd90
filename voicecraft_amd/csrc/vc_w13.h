// vc_w13.h - "w13": bf16 weights stored bit-exactly in 13 bits per value.  Shared by the device packer and its check
// (vc_gemm_w13.hip), the one-row kernels that stream the planes, and the host round-trip program (tools/w13_check.cpp):
// plain C++, no HIP type in any signature.
//
// Unit: the 512-value MFMA fragment one wave instruction loads (64 lanes x 8 bf16 = 64 lanes x four dwords).  Per value
//   hi7 = bits 14..8 (the upper seven exponent bits), lo = bits 7..0, sign = bit 15.
// Per fragment ONE side byte `base` (1..127); per value a 4-bit code:
//   code 0      : hi7 = 0 (zeros, -0.0, the denormal range; lo is stored like any other)
//   code 1..15  : hi7 = base + code - 1  (a window of 15 steps = 30 binades)
// A GROUP is four consecutive fragments.  A lane's share of a group (32 values, 64 bytes as bf16) is stored as
//   lo[8]   one dword per half fragment (fragment f, half g -> lo[2 f + g]): the low bytes of values 4 g .. 4 g + 3
//   nib[4]  one dword per fragment: byte j = code of value j (low nibble) | code of value 4 + j (high nibble)
//   sign    value j' = 0..3 of (fragment f, half g) at bit 8 j' + 7 - (2 f + g): (sign << (2 f + g)) & 0x80808080 puts the
//           four signs of a half on top of its four high bytes, and the eight shifts 0..7 partition the 32 bits
// = 52 bytes.  A wave's share of a group in memory: lo[0..3] of its 64 lanes (1 KB), lo[4..7] (1 KB), nib (1 KB), sign
// (256 bytes) = VC_W13_GROUP_BYTES, every piece one contiguous request of the wave.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_W13_FN __host__ __device__ __forceinline__
#else
#define VC_W13_FN static inline
#endif

#define VC_W13_CODES 15                 // hi7 steps a fragment's non-zero values may span
#define VC_W13_GROUP_FRAGS 4
#define VC_W13_GROUP_BYTES 3328         // 64 lanes x 52 bytes
#define VC_W13_GROUP_U4 208             // ... in 16-byte units: lo A at 0, lo B at 64, nib at 128, sign (dwords) at 192

struct vc_w13_lane { uint32_t lo[8]; uint32_t nib[4]; uint32_t sign; };

// v_perm_b32: byte i of the result = byte (sel >> 8 i) & 7 of {hi : lo} (lo = bytes 0..3); only selectors 0..7 are used here
VC_W13_FN uint32_t vc_w13_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(hi, lo, sel);
#else
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) r |= (uint32_t)((v >> (8 * ((sel >> (8 * i)) & 7))) & 0xff) << (8 * i);
  return r;
#endif
}

// The smallest and largest non-zero hi7 among a lane's eight values of one fragment (128 / 0 when it has none).
VC_W13_FN void vc_w13_minmax(const uint32_t w[4], int* mn, int* mx) {
  int lo = 128, hi = 0;
  for (int q = 0; q < 4; ++q)
    for (int h = 0; h < 2; ++h) {
      const int v = (int)((w[q] >> (16 * h + 8)) & 0x7f);
      if (v != 0) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    }
  *mn = lo; *mx = hi;
}
// The fragment's side byte from the minimum / maximum over all its lanes; *ok = 0 when the span does not fit the codes.
VC_W13_FN int vc_w13_base(int mn, int mx, int* ok) {
  if (mx == 0) { *ok = 1; return 1; }     // nothing but code 0
  *ok = (mx - mn) < VC_W13_CODES ? 1 : 0;
  return mn;
}

// Encodes a lane's share of a group: w[f] = its four dwords of fragment f (value j = half-word j), base[f] from vc_w13_base.
// Returns a mask of the fragments that hold a value outside their window (such a value is stored as code 15: the check finds it).
VC_W13_FN int vc_w13_encode(const uint32_t w[4][4], const int base[4], vc_w13_lane* out) {
  int bad = 0;
  uint32_t sign = 0;
  for (int f = 0; f < 4; ++f) {
    uint32_t nib = 0;
    for (int g = 0; g < 2; ++g) {
      uint32_t lo = 0;
      for (int j = 0; j < 4; ++j) {
        const uint32_t v = (w[f][2 * g + (j >> 1)] >> (16 * (j & 1))) & 0xffffu;
        const int hi7 = (int)((v >> 8) & 0x7f);
        int code = 0;
        if (hi7 != 0) {
          code = hi7 - base[f] + 1;
          if (code < 1 || code > VC_W13_CODES) { bad |= 1 << f; code = VC_W13_CODES; }
        }
        lo |= (v & 0xffu) << (8 * j);
        nib |= (uint32_t)code << (8 * j + 4 * g);
        sign |= (v >> 15) << (8 * j + 7 - (2 * f + g));
      }
      out->lo[2 * f + g] = lo;
    }
    out->nib[f] = nib;
  }
  out->sign = sign;
  return bad;
}

// The side byte as the decoder takes it: base - 1 in both 16-bit halves (wave-uniform: scalar arithmetic in the kernels).
VC_W13_FN uint32_t vc_w13_bm1(uint32_t base) { return (base - 1u) * 0x00010001u; }

// One half fragment (values 4 g .. 4 g + 3 of fragment f) back to its two bf16 dwords: nine integer operations.
//   lo = the half's low bytes, nib = the fragment's code dword, sign = the group's sign dword, fg = 2 f + g.
VC_W13_FN void vc_w13_decode_half(uint32_t lo, uint32_t nib, uint32_t sign, int fg, uint32_t bm1, uint32_t* d0, uint32_t* d1) {
  const uint32_t c = ((fg & 1) ? nib >> 4 : nib) & 0x0f0f0f0fu;
  const uint32_t nz = ((c + 0x7f7f7f7fu) >> 7) & 0x01010101u;            // 1 per non-zero code (a code is at most 15: no carry leaves a byte)
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short vc_w13_u16x2 __attribute__((ext_vector_type(2)));
  const uint32_t h = __builtin_bit_cast(uint32_t, (vc_w13_u16x2)(__builtin_bit_cast(vc_w13_u16x2, nz) * __builtin_bit_cast(vc_w13_u16x2, bm1) +
                                                                 __builtin_bit_cast(vc_w13_u16x2, c)));      // v_pk_mad_u16
#else
  const uint32_t h = nz * (bm1 & 0xffu) + c;                             // base - 1 + code <= 127 in every byte
#endif
  const uint32_t hs = ((sign << fg) & 0x80808080u) | h;
  *d0 = vc_w13_perm(hs, lo, 0x05010400u);
  *d1 = vc_w13_perm(hs, lo, 0x07030602u);
}

VC_W13_FN void vc_w13_decode_frag(const vc_w13_lane* in, int f, int base, uint32_t w[4]) {
  const uint32_t bm1 = vc_w13_bm1((uint32_t)base);
  vc_w13_decode_half(in->lo[2 * f], in->nib[f], in->sign, 2 * f, bm1, &w[0], &w[1]);
  vc_w13_decode_half(in->lo[2 * f + 1], in->nib[f], in->sign, 2 * f + 1, bm1, &w[2], &w[3]);
}
