// vc_w8.h - "w8": bf16 weights that lie on a block-scaled 8-bit grid, stored as one OCP E4M3 (e4m3fn) byte per value plus one shift
// byte per fragment.  Shared by the device packers and their checks (vc_gemm_w8.hip), the kernels that stream the planes, and the
// host round-trip programs (tools/w8_check.cpp, tools/w8_wide_check.cpp): plain C++, no HIP type in any signature.  The second half
// of the file is the same grid for the 16-channel images of wide steps, stored by PAIRS ("w8w"), the third section the pairs of the
// 12-channel QKV image ("w8q": tools/w8_qkv_check.cpp).
//
// Unit: the 512-value MFMA fragment one wave instruction loads (64 lanes x 8 bf16 = 64 lanes x four dwords; in matrix terms an aligned
// block of 8 output channels x 64 inputs of the 8-channel-tile images, vc_gemm.hip pack_k).  A fragment is ON THE GRID when one integer
// shift s exists with every value = q . 2^s, q an E4M3 number (normal, denormal or +-0, never the NaN code S.1111.111) and the product
// a normal bf16 number or +-0.  The storage is lossless for such a fragment and refuses every other one:
//   code byte per value   S.EEEE.MMM: E = 0: M . 2^-9;  E > 0: (8 + M) . 2^(E - 10)        (bias 7; 448 = 0x7e is the largest)
//   side byte per fragment  b = s + 127: (b << 23) IS the fp32 scale 2^s the conversion instruction takes
// The shift follows from the fragment's extreme exponents: s = emax - 8 puts the largest value into E4M3's top binade, so the grid
// reaches 17 binades below it - and it is the SMALLEST shift that can hold the fragment, hence right whenever any shift is.  One
// exception: a value 1.111b . 2^emax would be the NaN code there; such a fragment takes s = emax - 7 (240 . 2^s, the smallest shift
// that avoids the code).  s stays inside VC_W8_SHIFT_MIN .. VC_W8_SHIFT_MAX, the shifts at which EVERY code gives a normal bf16
// number (2^-9 . 2^s >= 2^-126, 448 . 2^s < 2^128): a fragment of tiny values takes VC_W8_SHIFT_MIN and smaller codes; a fragment that
// holds a bf16 denormal (smallest non-zero exponent field 0) would need a shift below the range: refused.  A fragment of zeros takes 0.
// A GROUP is four consecutive fragments.  A lane's share of a group (32 values) is 32 bytes: piece A = its 16 bytes of fragments 0, 1
// (dwords: f0 values 0..3, f0 values 4..7, f1 ..), piece B = fragments 2, 3.  A wave's share in memory: piece A of its 64 lanes (1 KB),
// piece B (1 KB) = VC_W8_GROUP_BYTES, every piece one contiguous 16-byte-per-lane request of the wave; + one side WORD per group.
// gfx950 rebuilds two bf16 values from two code bytes and the scale in one instruction (v_cvt_scalef32_pk_bf16_fp8): four per fragment.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VC_W8_FN __host__ __device__ __forceinline__
#else
#define VC_W8_FN static inline
#endif

#define VC_W8_GROUP_FRAGS 4
#define VC_W8_GROUP_BYTES 2048          // 64 lanes x 32 bytes
#define VC_W8_GROUP_U4 128              // ... in 16-byte units: piece A at 0, piece B at 64
#define VC_W8_SHIFT_MIN (-117)          // 2^-9 (the smallest denormal code) . 2^s is the smallest normal bf16 number
#define VC_W8_SHIFT_MAX 119             // 448 . 2^s < 2^128
#define VC_W8_TOP 8                     // E4M3's top binade: 256 .. 448

struct vc_w8_lane { uint32_t a[4]; uint32_t b[4]; };      // pieces A and B of one lane

// The smallest and largest non-zero exponent FIELD (bits 14..7) among a lane's eight values of one fragment (256 / -1 when all are +-0).
VC_W8_FN void vc_w8_minmax(const uint32_t w[4], int* mn, int* mx) {
  int lo = 256, hi = -1;
  for (int q = 0; q < 4; ++q)
    for (int h = 0; h < 2; ++h) {
      const uint32_t v = (w[q] >> (16 * h)) & 0x7fffu;
      if (v != 0) { const int e = (int)(v >> 7); lo = e < lo ? e : lo; hi = e > hi ? e : hi; }
    }
  *mn = lo; *mx = hi;
}
// 1 when one of the lane's values in the fragment's top binade (exponent field mx) has the mantissa 1.111b: the NaN code at emax - 8.
VC_W8_FN int vc_w8_top111(const uint32_t w[4], int mx) {
  int t = 0;
  for (int q = 0; q < 4; ++q)
    for (int h = 0; h < 2; ++h) {
      const uint32_t v = (w[q] >> (16 * h)) & 0x7fffu;
      t |= ((int)(v >> 7) == mx && ((v >> 4) & 7u) == 7u) ? 1 : 0;
    }
  return t;
}
// The fragment's shift from the extreme exponent fields over all its lanes and the OR of vc_w8_top111; *ok = 0 when no shift of the
// allowed range can hold it (a denormal, an infinity / NaN exponent, 1.111b in the very last binade).
VC_W8_FN int vc_w8_shift(int mn, int mx, int top111, int* ok) {
  if (mx < 0) { *ok = 1; return 0; }                 // nothing but +-0
  int s = mx - 127 - VC_W8_TOP + (top111 ? 1 : 0);
  *ok = (mn >= 1 && mx <= 254 && s <= VC_W8_SHIFT_MAX) ? 1 : 0;
  s = s < VC_W8_SHIFT_MIN ? VC_W8_SHIFT_MIN : s;
  return s > VC_W8_SHIFT_MAX ? VC_W8_SHIFT_MAX : s;
}
VC_W8_FN uint32_t vc_w8_side(int shift) { return (uint32_t)(shift + 127); }
VC_W8_FN uint32_t vc_w8_scale_bits(uint32_t side) { return (side & 0xffu) << 23; }

// One bf16 value (16 bits) as the code byte of q = value / 2^shift; *bad |= 1 when the value is not on the grid at this shift
// (the byte stored then decodes to something else: the check finds it too).
VC_W8_FN uint32_t vc_w8_encode_value(uint32_t v, int shift, int* bad) {
  const uint32_t sign = (v >> 8) & 0x80u;
  const int field = (int)((v >> 7) & 0xffu);
  const uint32_t m7 = v & 0x7fu;
  if ((v & 0x7fffu) == 0) return sign;
  if (field == 0 || field == 255) { *bad |= 1; return sign; }
  const int qe = field - 127 - shift;                // q's binade
  if (qe > VC_W8_TOP) { *bad |= 1; return sign | 0x7eu; }
  if (qe >= -6) {                                    // a normal code: three mantissa bits
    if (m7 & 0xfu) *bad |= 1;
    const uint32_t c = ((uint32_t)(qe + 7) << 3) | (m7 >> 4);
    if (c == 0x7fu) { *bad |= 1; return sign | 0x7eu; }      // the NaN code is never stored
    return sign | c;
  }
  const int sh = -2 - qe;                            // a denormal code: (1.m7) . 2^qe = k . 2^-9, k = (0x80 | m7) >> sh
  if (sh > 7) { *bad |= 1; return sign; }
  const uint32_t sig = 0x80u | m7;
  if (sig & ((1u << sh) - 1u)) *bad |= 1;
  return sign | (sig >> sh);
}

// Encodes a lane's share of a group: w[f] = its four dwords of fragment f (value j = half-word j), shift[f] from vc_w8_shift.
// Returns a mask of the fragments that hold a value off their grid.
VC_W8_FN int vc_w8_encode(const uint32_t w[4][4], const int shift[4], vc_w8_lane* out) {
  int bad = 0;
  for (int f = 0; f < 4; ++f) {
    int b = 0;
    uint32_t d[2] = {0u, 0u};
    for (int j = 0; j < 8; ++j) {
      const uint32_t v = (w[f][j >> 1] >> (16 * (j & 1))) & 0xffffu;
      d[j >> 2] |= vc_w8_encode_value(v, shift[f], &b) << (8 * (j & 3));
    }
    uint32_t* piece = f < 2 ? out->a : out->b;
    piece[2 * (f & 1)] = d[0];
    piece[2 * (f & 1) + 1] = d[1];
    bad |= b << f;
  }
  return bad;
}

// The host mirror of the conversion's INTENDED result: two code bytes (the low or the high half of `src`) times the fp32 scale,
// rounded to nearest even to two bf16 values.  Exact for a power-of-two scale whose products are normal bf16 numbers.
VC_W8_FN uint32_t vc_w8_cvt_mirror(uint32_t src, int hi, uint32_t scale_bits) {
  float scale;
  memcpy(&scale, &scale_bits, 4);
  uint32_t out = 0;
  for (int i = 0; i < 2; ++i) {
    const uint32_t c = (src >> (16 * hi + 8 * i)) & 0xffu;
    const int E = (int)((c >> 3) & 15u), M = (int)(c & 7u);
    float q = E == 0 ? (float)M * (1.0f / 512.0f) : (float)(8 + M) * (E >= 10 ? (float)(1 << (E - 10)) : 1.0f / (float)(1 << (10 - E)));
    if ((c & 0x7fu) == 0x7fu) q = 0.0f;              // never stored; the mirror gives +-0 where the instruction gives a NaN
    const float r = (c & 0x80u ? -q : q) * scale;
    uint32_t u;
    memcpy(&u, &r, 4);
    u += 0x7fffu + ((u >> 16) & 1u);                 // to nearest even
    out |= (u >> 16) << (16 * i);
  }
  return out;
}
// Two code bytes -> two bf16 values: the instruction on the device, its mirror on the host.
VC_W8_FN uint32_t vc_w8_cvt(uint32_t src, int hi, uint32_t scale_bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __bf16 vc_w8_bf2 __attribute__((ext_vector_type(2)));
  const float scale = __builtin_bit_cast(float, scale_bits);
  return hi ? __builtin_bit_cast(uint32_t, (vc_w8_bf2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(src, scale, true))
            : __builtin_bit_cast(uint32_t, (vc_w8_bf2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(src, scale, false));
#else
  return vc_w8_cvt_mirror(src, hi, scale_bits);
#endif
}

// One fragment (its two code dwords d0 = values 0..3, d1 = values 4..7) back to its four bf16 dwords: four conversions.
VC_W8_FN void vc_w8_decode_dwords(uint32_t d0, uint32_t d1, uint32_t scale_bits, uint32_t w[4]) {
  w[0] = vc_w8_cvt(d0, 0, scale_bits);
  w[1] = vc_w8_cvt(d0, 1, scale_bits);
  w[2] = vc_w8_cvt(d1, 0, scale_bits);
  w[3] = vc_w8_cvt(d1, 1, scale_bits);
}
VC_W8_FN void vc_w8_decode_frag(const vc_w8_lane* in, int f, uint32_t side, uint32_t w[4]) {
  const uint32_t* piece = f < 2 ? in->a : in->b;
  vc_w8_decode_dwords(piece[2 * (f & 1)], piece[2 * (f & 1) + 1], vc_w8_scale_bits(side), w);
}

// ------------------------------------------------------------------ "w8w": the 16-channel images of wide steps (17..64 rows), by PAIRS
// The wide kernel (vc_gemm_wd.hip rows_gemm_wds_k) reads images of 16-channel tiles: lane l of fragment (tile nt, k-tile kt) holds
// channel 16 nt + (l & 15), inputs 32 kt + 8 (l >> 4) .. + 7.  A PAIR is k-tiles 2j, 2j + 1 of one tile: 16 channels x 64 inputs = 1024
// values, 2 KB of the image (two consecutive fragments).  Its lanes with (l & 8) == 0 hold channels 0..7 x 64 inputs, the others
// channels 8..15 x 64 inputs: two aligned 8 x 64 blocks, i.e. two fragments of the grid above in another lane order.  Each HALF is held
// to the rule above (vc_w8_shift, vc_w8_encode_value, the NaN-code exception) with a shift of its own.  Storage of a pair:
//   1 KB of codes: 16 bytes per lane = its eight codes of k-tile 2j (two dwords), then its eight of k-tile 2j + 1 - one contiguous,
//     16-byte-per-lane request of the wave;
//   2 side bytes: shift + 127 of channels 0..7, then of channels 8..15.
// Pairs follow the image's order (tile major, then k), so a wave's KPW / 2 pairs of a tile are contiguous and so are their side bytes.
#define VC_W8W_PAIR_BYTES 1024
#define VC_W8W_PAIR_U4 64

VC_W8_FN int vc_w8w_half(int lane) { return (lane >> 3) & 1; }

// Encodes a lane's share of a pair: w[h] = its four dwords of k-tile 2j + h, `shift` = its half's.  Returns 1 when a value is off the grid.
VC_W8_FN int vc_w8w_encode_lane(const uint32_t w[2][4], int shift, uint32_t out[4]) {
  int bad = 0;
  for (int h = 0; h < 2; ++h) {
    uint32_t d[2] = {0u, 0u};
    for (int j = 0; j < 8; ++j) {
      const uint32_t v = (w[h][j >> 1] >> (16 * (j & 1))) & 0xffffu;
      d[j >> 2] |= vc_w8_encode_value(v, shift, &bad) << (8 * (j & 3));
    }
    out[2 * h] = d[0];
    out[2 * h + 1] = d[1];
  }
  return bad;
}
// A lane's 16 code bytes and its half's side byte back to its four dwords of each of the two k-tiles: eight conversions.
VC_W8_FN void vc_w8w_decode_lane(const uint32_t in[4], uint32_t side, uint32_t w[2][4]) {
  vc_w8_decode_dwords(in[0], in[1], vc_w8_scale_bits(side), w[0]);
  vc_w8_decode_dwords(in[2], in[3], vc_w8_scale_bits(side), w[1]);
}

// One whole pair in plain C++ (the host export vc_w8w_pack_host and tools/w8_wide_check.cpp; the device packer runs the same per-lane
// text with wave reductions in place of the loops over the lanes).  img = the pair's 2 x 64 x 4 dwords in image order, codes = 64 x 4
// dwords, side = 2 bytes.  Returns a mask of the halves refused (no shift of the range, or a value off the grid at the shift).
VC_W8_FN int vc_w8w_encode_pair(const uint32_t* img, uint32_t* codes, uint8_t side[2]) {
  int mn[2] = {256, 256}, mx[2] = {-1, -1}, top[2] = {0, 0}, shift[2], refused = 0;
  for (int l = 0; l < 64; ++l)
    for (int h = 0; h < 2; ++h) {
      int a, b;
      vc_w8_minmax(img + (h * 64 + l) * 4, &a, &b);
      const int half = vc_w8w_half(l);
      mn[half] = a < mn[half] ? a : mn[half];
      mx[half] = b > mx[half] ? b : mx[half];
    }
  for (int l = 0; l < 64; ++l)
    for (int h = 0; h < 2; ++h) top[vc_w8w_half(l)] |= vc_w8_top111(img + (h * 64 + l) * 4, mx[vc_w8w_half(l)]);
  for (int half = 0; half < 2; ++half) {
    int ok;
    shift[half] = vc_w8_shift(mn[half], mx[half], top[half], &ok);
    refused |= ok ? 0 : 1 << half;
    side[half] = (uint8_t)vc_w8_side(shift[half]);
  }
  for (int l = 0; l < 64; ++l) {
    uint32_t w[2][4];
    for (int h = 0; h < 2; ++h)
      for (int q = 0; q < 4; ++q) w[h][q] = img[(h * 64 + l) * 4 + q];
    if (vc_w8w_encode_lane(w, shift[vc_w8w_half(l)], codes + l * 4)) refused |= 1 << vc_w8w_half(l);
  }
  return refused;
}
VC_W8_FN void vc_w8w_decode_pair(const uint32_t* codes, const uint8_t side[2], uint32_t* img) {
  for (int l = 0; l < 64; ++l) {
    uint32_t w[2][4];
    vc_w8w_decode_lane(codes + l * 4, side[vc_w8w_half(l)], w);
    for (int h = 0; h < 2; ++h)
      for (int q = 0; q < 4; ++q) img[(h * 64 + l) * 4 + q] = w[h][q];
  }
}

// ------------------------------------------------------------------ "w8q": the 12-channel image of the QKV projection, by PAIRS
// rows_gemm_k's QKV form reads Wqkv in 12-channel tiles (vc_gemm.hip pack_k with th = 12): a (tile nt, k-tile kt) is 48 slots of 16
// bytes, slot s = kg * 12 + m = channel 12 nt + m, inputs 32 kt + 8 kg .. + 7 - natural channel order, the values of the 8- and 16-channel
// images.  A PAIR is k-tiles 2j, 2j + 1 of one tile: 12 channels x 64 inputs = 768 values, 1536 B of the image (two consecutive
// fragments of 768 B).  A 12-channel tile straddles the quantiser's 8-channel blocks, so a pair has two PARTS, split at the block
// boundary: an even tile's channels are 8 (a whole block) + 4 (the first four of the next block), an odd tile's 4 (the last four of
// that block) + 8 (a whole block).  Each part is held to the rule at the top of the file (vc_w8_shift, vc_w8_encode_value, the NaN-code
// exception) with the smallest shift that holds ITS values.  A subset of a block that is on the grid is on the grid at its own shift:
// that shift is never larger than the block's, normal codes keep their three mantissa bits and denormal codes stay multiples of the
// smaller step - so every pair of a quantised checkpoint packs.  Storage of a pair:
//   768 B of codes: 16 bytes per slot = its eight codes of k-tile 2j (two dwords), then its eight of k-tile 2j + 1 (the lane layout
//     w8w_frag decodes): one contiguous 16-byte-per-lane request of the wave's 48 lanes that carry a weight;
//   2 side bytes: shift + 127 of part 0, then of part 1.
// Pairs follow the image's order (tile major, then k), so a wave's KTW / 2 pairs of a tile are contiguous and so are their KTW side
// bytes (whole aligned words for KTW >= 4).  Lossless, or the pair is refused.
#define VC_W8Q_SLOTS 48
#define VC_W8Q_PAIR_BYTES 768
#define VC_W8Q_PAIR_U4 48

// the part of channel m (0..11) of a tile of parity `odd`
VC_W8_FN int vc_w8q_part(int m, int odd) { return odd ? (m >= 4 ? 1 : 0) : (m >= 8 ? 1 : 0); }

// One whole pair in plain C++ (the host export vc_w8q_pack_host and tools/w8_qkv_check.cpp; the device packer runs the same per-lane text
// with wave reductions over a part's lanes in place of the loops).  img = the pair's 2 x 48 x 4 dwords in image order, codes = 48 x 4
// dwords, side = 2 bytes, odd = the tile's parity.  Returns a mask of the parts refused.
VC_W8_FN int vc_w8q_encode_pair(const uint32_t* img, int odd, uint32_t* codes, uint8_t side[2]) {
  int mn[2] = {256, 256}, mx[2] = {-1, -1}, top[2] = {0, 0}, shift[2], refused = 0;
  for (int s = 0; s < VC_W8Q_SLOTS; ++s)
    for (int h = 0; h < 2; ++h) {
      int a, b;
      vc_w8_minmax(img + (h * VC_W8Q_SLOTS + s) * 4, &a, &b);
      const int part = vc_w8q_part(s % 12, odd);
      mn[part] = a < mn[part] ? a : mn[part];
      mx[part] = b > mx[part] ? b : mx[part];
    }
  for (int s = 0; s < VC_W8Q_SLOTS; ++s)
    for (int h = 0; h < 2; ++h) {
      const int part = vc_w8q_part(s % 12, odd);
      top[part] |= vc_w8_top111(img + (h * VC_W8Q_SLOTS + s) * 4, mx[part]);
    }
  for (int part = 0; part < 2; ++part) {
    int ok;
    shift[part] = vc_w8_shift(mn[part], mx[part], top[part], &ok);
    refused |= ok ? 0 : 1 << part;
    side[part] = (uint8_t)vc_w8_side(shift[part]);
  }
  for (int s = 0; s < VC_W8Q_SLOTS; ++s) {
    uint32_t w[2][4];
    for (int h = 0; h < 2; ++h)
      for (int q = 0; q < 4; ++q) w[h][q] = img[(h * VC_W8Q_SLOTS + s) * 4 + q];
    const int part = vc_w8q_part(s % 12, odd);
    if (vc_w8w_encode_lane(w, shift[part], codes + s * 4)) refused |= 1 << part;
  }
  return refused;
}
VC_W8_FN void vc_w8q_decode_pair(const uint32_t* codes, const uint8_t side[2], int odd, uint32_t* img) {
  for (int s = 0; s < VC_W8Q_SLOTS; ++s) {
    uint32_t w[2][4];
    vc_w8w_decode_lane(codes + s * 4, side[vc_w8q_part(s % 12, odd)], w);
    for (int h = 0; h < 2; ++h)
      for (int q = 0; q < 4; ++q) img[(h * VC_W8Q_SLOTS + s) * 4 + q] = w[h][q];
  }
}
