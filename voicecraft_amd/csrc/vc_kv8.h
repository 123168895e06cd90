// vc_kv8.h - "kv8": cached K / V rows once more as one OCP E4M3 (e4m3fn) byte per value plus one shift byte per cached row of one
// head.  Shared by the device packer (vc_attn.hip kv8_pack_k), the host statement of the grid (vc_kv8_quantize_host, include/vc_engine.h)
// and the stand-alone check (tools/kv8_check.cpp): plain C++, no HIP type in any signature.  Unlike "w8" (vc_w8.h), which stores
// values that already lie on its grid, this ROUNDS: 3 mantissa bits are what is left of a cached value.
//
// Unit: the hd values of one head at one cached position.  value ~ q . 2^s, q an E4M3 number (never the NaN code S.1111.111):
//   code byte   S.EEEE.MMM: E = 0: M . 2^-9;  E > 0: (8 + M) . 2^(E - 10)        (bias 7; 448 = 0x7e is the largest)
//   shift byte  s, int8 in VC_W8_SHIFT_MIN .. VC_W8_SHIFT_MAX: every code times 2^s is a normal bf16 number or +-0
// The shift is the rule of voicecraft_amd/quant.py block_shifts with the row as the block: s = floor(log2 amax) - 8 puts the row's
// largest value into E4M3's top binade (256 .. 448), clamped to the range; one more where amax . 2^-s > 464 (past the midpoint between
// 448 and the NaN code 480: at the next shift 480 and 512 exist as 240 and 256); a row of zeros takes 0.  A value is scaled by 2^-s,
// clamped to +-448 and rounded to the nearest code, ties to the even code.  Everything below is integer arithmetic on the bf16 bits, so
// the host and the device agree by construction.
//
// "kv8c" (vc_request_kv8c, centred K): K rows lose a fixed vector before they meet the grid.  The contract, stated once:
//   The centre.  For every layer, cache slot and head there is a bf16 vector c[hd]: the mean of the slot's bf16 K rows at positions
//     0 .. n0-1, accumulated in fp32 and rounded to bf16 (nearest even), n0 = the number of rows of that sequence in the prefill pass
//     that wrote its position 0.  It is recomputed whenever a slot is prefilled from position 0 (a new call, a session admission) and
//     never updated by decode passes or by later prefill passes of the same sequence.
//   Call kinds.  Best-of-N: the copy that gives the siblings the source slot's rows gives them its centre.  A call with a shared text
//     prefix: every sequence of the call takes SEQUENCE 0's centre (positions below the prefix are read from slot 0's cache, and a row
//     must meet one c for all its 8-bit positions); slot 0's centre exists before any row of the call is packed.
//   K codes and shifts: the grid above applied to bf16_rne(float(k) - float(c)) (vc_kv8c_sub; the subtraction in fp32).  V codes and
//     shifts are the plain ones.
//   Scores.  A position read from the E4M3 cache scores (q . k8) . 2^s + q . c, q pre-scaled as for the other term: q . (k - c) + q . c
//     is the true score, so every score of a row is a true score and softmax, the split partials and their merge are as before.
//     The pass's own positions lo..pos come from the bf16 cache, uncentred.
#pragma once
#include <stdint.h>
#include "vc_w8.h"

// The largest magnitude (bits 14..0) among the eight bf16 values of four dwords: bf16 magnitudes order like their bit patterns.
VC_W8_FN uint32_t vc_kv8_amax8(const uint32_t w[4]) {
  uint32_t a = 0;
  for (int q = 0; q < 4; ++q) {
    const uint32_t lo = w[q] & 0x7fffu, hi = (w[q] >> 16) & 0x7fffu;
    a = lo > a ? lo : a;
    a = hi > a ? hi : a;
  }
  return a;
}

// The row's shift from its largest magnitude (bf16 bits 14..0).
VC_W8_FN int vc_kv8_shift(uint32_t amax) {
  if (amax == 0) return 0;
  const int field = (int)(amax >> 7);
  if (field == 0) return VC_W8_SHIFT_MIN;                     // a row of bf16 denormals
  const int sig = (int)(0x80u | (amax & 0x7fu));              // amax = sig . 2^(field - 134)
  int s = field - 127 - VC_W8_TOP;
  if (s < VC_W8_SHIFT_MIN) s = VC_W8_SHIFT_MIN;               // (amax . 2^-s < 256 then: no step)
  else if (sig > 232) s += 1;                                 // amax . 2^-s = 2 sig > 464
  return s > VC_W8_SHIFT_MAX ? VC_W8_SHIFT_MAX : s;
}

// n >> sh rounded to nearest, ties to even (sh >= 1).
VC_W8_FN uint32_t vc_kv8_rne(uint32_t n, int sh) {
  const uint32_t k = n >> sh, rem = n & ((1u << sh) - 1u), half = 1u << (sh - 1);
  return k + ((rem > half || (rem == half && (k & 1u))) ? 1u : 0u);
}

// One bf16 value (16 bits) as the code byte nearest to value / 2^shift.
VC_W8_FN uint32_t vc_kv8_encode_value(uint32_t v, int shift) {
  const uint32_t sign = (v >> 8) & 0x80u;
  int field = (int)((v >> 7) & 0xffu);
  uint32_t sig = v & 0x7fu;
  if (field == 0) {                                           // +-0, or a bf16 denormal: normalised by hand
    if (sig == 0) return sign;
    field = 1;
    while (sig < 0x80u) { sig <<= 1; --field; }
  } else {
    if (field == 255) return sign | 0x7eu;                    // (no cached value is infinite; the clamp, for a defined result)
    sig |= 0x80u;
  }
  const int qe = field - 127 - shift;                         // binade of q = sig . 2^(qe - 7)
  if (qe > VC_W8_TOP) return sign | 0x7eu;
  if (qe >= -6) {                                             // a normal code: three mantissa bits, quantum 2^(qe - 3)
    const uint32_t k = vc_kv8_rne(sig, 4);                    // 8 .. 16
    const uint32_t c = ((uint32_t)(qe + 7) << 3) + (k - 8u);  // (k = 16 carries into the exponent field)
    return sign | (c > 0x7eu ? 0x7eu : c);                    // beyond 448: clamped, the NaN code is never stored
  }
  const int sh = -2 - qe;                                     // denormal codes: q = (sig >> sh) . 2^-9, sh >= 5
  if (sh > 8) return sign;                                    // below half the smallest code
  return sign | vc_kv8_rne(sig, sh);                          // 0 .. 8 (8 = the first normal code, 0x08)
}

// Eight values (four dwords of bf16 pairs) -> eight code bytes (two dwords).
VC_W8_FN void vc_kv8_encode8(const uint32_t w[4], int shift, uint32_t d[2]) {
  d[0] = d[1] = 0u;
  for (int j = 0; j < 8; ++j) {
    const uint32_t v = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    d[j >> 2] |= vc_kv8_encode_value(v, shift) << (8 * (j & 3));
  }
}

// A code byte at a shift -> the bf16 value it stands for (exact: at most four significant bits, a normal number or +-0).
VC_W8_FN uint32_t vc_kv8_decode_value(uint32_t c, int shift) {
  const uint32_t sign = (c & 0x80u) << 8;
  const int E = (int)((c >> 3) & 15u);
  uint32_t k = c & 7u;
  int e2;                                                     // magnitude = k . 2^e2
  if (E == 0) { if (k == 0) return sign; e2 = -9 + shift; }
  else { k |= 8u; e2 = E - 10 + shift; }
  int top = 3;
  while (!(k >> top)) --top;                                  // k = 1.xxx . 2^top
  const uint32_t field = (uint32_t)(e2 + top + 127);
  const uint32_t m7 = (k << (7 - top)) & 0x7fu;
  return sign | (field << 7) | m7;
}

// "kv8c": bf16_rne(float(k) - float(c)) on bf16 bit patterns (finite values; the fp32 difference of two bf16 numbers, rounded to
// nearest even bf16 - an overflow gives the infinity the encode clamps).
VC_W8_FN uint32_t vc_kv8c_sub(uint32_t k, uint32_t c) {
  const uint32_t ku = k << 16, cu = c << 16;
  float kf, cf;
  memcpy(&kf, &ku, 4);
  memcpy(&cf, &cu, 4);
  const float d = kf - cf;
  uint32_t u;
  memcpy(&u, &d, 4);
  return ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16) & 0xffffu;
}
// Eight values (four dwords of bf16 pairs) minus eight centre values, in place.
VC_W8_FN void vc_kv8c_sub8(uint32_t w[4], const uint32_t c[4]) {
  for (int q = 0; q < 4; ++q)
    w[q] = vc_kv8c_sub(w[q] & 0xffffu, c[q] & 0xffffu) | (vc_kv8c_sub(w[q] >> 16, c[q] >> 16) << 16);
}

// One row of hd bf16 values: its shift and its hd code bytes.
VC_W8_FN int vc_kv8_quantize_row(const uint16_t* row, int hd, uint8_t* codes) {
  uint32_t amax = 0;
  for (int j = 0; j < hd; ++j) { const uint32_t a = row[j] & 0x7fffu; amax = a > amax ? a : amax; }
  const int s = vc_kv8_shift(amax);
  for (int j = 0; j < hd; ++j) codes[j] = (uint8_t)vc_kv8_encode_value(row[j], s);
  return s;
}
// "kv8c": one K row of hd bf16 values against its head's centre.
VC_W8_FN int vc_kv8c_quantize_row(const uint16_t* row, const uint16_t* centre, int hd, uint8_t* codes) {
  uint32_t amax = 0;
  for (int j = 0; j < hd; ++j) { const uint32_t a = vc_kv8c_sub(row[j], centre[j]) & 0x7fffu; amax = a > amax ? a : amax; }
  const int s = vc_kv8_shift(amax);
  for (int j = 0; j < hd; ++j) codes[j] = (uint8_t)vc_kv8_encode_value(vc_kv8c_sub(row[j], centre[j]), s);
  return s;
}
