// Host round trip of the PAIR planes of the 16-channel images (voicecraft_amd/csrc/vc_w8.h, "w8w"): build with the host compiler and
// -fsanitize=address,undefined and run once:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/w8_wide_check.cpp -o w8_wide_check && ./w8_wide_check
// Prints "ok <pairs> <refused>" and exits 0, or says what broke.  The decode is the header's host mirror of
// v_cvt_scalef32_pk_bf16_fp8; the device check (w8w_check_k) runs the instruction itself.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../voicecraft_amd/csrc/vc_w8.h"

// bf16 bits of q(code) . 2^s, computed apart from the header: the value as a double, then its (exact) bf16 pattern
static uint16_t value_bits(int code, int s) {
  const int E = (code >> 3) & 15, M = code & 7;
  const double q = E == 0 ? std::ldexp((double)M, -9) : std::ldexp((double)(8 + M), E - 10);
  const float v = (float)std::ldexp(code & 0x80 ? -q : q, s);
  uint32_t u;
  std::memcpy(&u, &v, 4);
  if (u & 0xffffu) { std::printf("code %02x at shift %d is not a bf16 number\n", code, s); std::exit(1); }
  return (uint16_t)(u >> 16);
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// A pair in image order: img[h][lane][j] = value j of the lane in k-tile 2j + h.  The lane's half: (lane >> 3) & 1.
struct Pair { uint16_t v[2][64][8]; };

// Encodes the pair, checks the stored bytes (never the NaN code; exactly 1 KB + 2 bytes written) and, for halves that were not refused,
// that the decode gives the image back bit for bit.  Returns the refusal mask in *mask and the two shifts.
static int round_trip(const Pair& p, int* mask, int shifts[2]) {
  std::vector<uint32_t> img(512), codes(256 + 2, 0xa5a5a5a5u), back(512);      // heap buffers: the sanitizer sees every byte past them
  std::memcpy(img.data(), p.v, 2048);
  uint8_t side[2] = {0xa5, 0xa5};
  *mask = vc_w8w_encode_pair(img.data(), codes.data(), side);
  if (codes[256] != 0xa5a5a5a5u || codes[257] != 0xa5a5a5a5u) { std::printf("the encode wrote past its 1 KB\n"); return 1; }
  for (int h = 0; h < 2; ++h) {
    shifts[h] = (int)side[h] - 127;
    if (shifts[h] < VC_W8_SHIFT_MIN || shifts[h] > VC_W8_SHIFT_MAX) { std::printf("shift %d out of range\n", shifts[h]); return 1; }
  }
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(codes.data());
  for (int i = 0; i < VC_W8W_PAIR_BYTES; ++i)
    if ((bytes[i] & 0x7f) == 0x7f) { std::printf("the NaN code was stored (byte %d)\n", i); return 1; }
  vc_w8w_decode_pair(codes.data(), side, back.data());
  for (int h = 0; h < 2; ++h)
    for (int l = 0; l < 64; ++l) {
      const int half = vc_w8w_half(l);
      if (half != ((l & 8) ? 1 : 0)) { std::printf("lane %d: half %d\n", l, half); return 1; }
      if (std::memcmp(&back[(h * 64 + l) * 4], &img[(h * 64 + l) * 4], 16) != 0 && !((*mask >> half) & 1)) {
        std::printf("k-tile %d lane %d decoded to other bits (shift %d) and its half was not refused\n", h, l, shifts[half]);
        return 1;
      }
      // the layout as stated: the lane's 16 bytes are its eight codes of k-tile 2j, then its eight of k-tile 2j + 1
      if (!((*mask >> half) & 1))
        for (int j = 0; j < 8; ++j)
          if (value_bits(bytes[l * 16 + h * 8 + j], shifts[half]) != p.v[h][l][j] && (p.v[h][l][j] & 0x7fff) != 0) {
            std::printf("byte %d of lane %d is not value %d of k-tile %d\n", h * 8 + j, l, j, h);
            return 1;
          }
    }
  return 0;
}

// every value of half `half` = a random code <= top at shift s; one lane holds `top` itself
static void fill_half(Pair& p, int half, int top, int s) {
  for (int h = 0; h < 2; ++h)
    for (int l = 0; l < 64; ++l)
      if (vc_w8w_half(l) == half)
        for (int j = 0; j < 8; ++j) p.v[h][l][j] = value_bits((int)(rnd() % (uint32_t)(top + 1)) | ((rnd() & 1) << 7), s);
  p.v[1][half * 8 + 16 * 2 + 3][5] = value_bits(top, s);
}

// every value of half `half` = a normal code 1.0 .. 416 at shift s (three mantissa bits: on the grid at s + 1 too); one lane holds 448
static void fill_normal(Pair& p, int half, int s) {
  for (int h = 0; h < 2; ++h)
    for (int l = 0; l < 64; ++l)
      if (vc_w8w_half(l) == half)
        for (int j = 0; j < 8; ++j) p.v[h][l][j] = value_bits(0x40 + (int)(rnd() % 0x3e), s);
  p.v[1][half * 8 + 16 * 2 + 3][5] = value_bits(0x7e, s);
}

int main() {
  static_assert(VC_W8W_PAIR_BYTES == 64 * 16 && VC_W8W_PAIR_U4 * 16 == VC_W8W_PAIR_BYTES, "pair layout");
  long pairs = 0, refused = 0;
  int mask, sh[2];
  Pair p;
  // (1) a pseudo-random on-grid image: both halves at shifts of their own, every top code; the packer must find exactly the shifts
  for (int it = 0; it < 4000; ++it) {
    int s[2], top[2];
    for (int half = 0; half < 2; ++half) {
      s[half] = VC_W8_SHIFT_MIN + (int)(rnd() % (uint32_t)(VC_W8_SHIFT_MAX - VC_W8_SHIFT_MIN + 1));
      top[half] = 0x78 + (int)(rnd() % 7u);          // a code of the top binade: 256 .. 448
      fill_half(p, half, top[half], s[half]);
    }
    if (round_trip(p, &mask, sh)) return 1;
    if (mask || sh[0] != s[0] || sh[1] != s[1]) { std::printf("random pair %d: mask %d, shifts %d %d for %d %d\n", it, mask, sh[0], sh[1], s[0], s[1]); return 1; }
    ++pairs;
  }
  // (2) all 254 non-NaN codes in each half, halves 2^6 apart; zeros; +-0 mixes
  for (int half = 0; half < 2; ++half) {
    int i = 0;
    for (int h = 0; h < 2; ++h)
      for (int l = 0; l < 64; ++l)
        if (vc_w8w_half(l) == half)
          for (int j = 0; j < 8; ++j, ++i) {
            int c = i < 256 ? i : (int)(rnd() & 0xff);
            if ((c & 0x7f) == 0x7f) c ^= 1;
            p.v[h][l][j] = value_bits(c, half ? -4 : -10);
          }
  }
  if (round_trip(p, &mask, sh)) return 1;
  if (mask || sh[0] != -10 || sh[1] != -4) { std::printf("all codes: mask %d shifts %d %d\n", mask, sh[0], sh[1]); return 1; }
  ++pairs;
  std::memset(&p, 0, sizeof p);
  if (round_trip(p, &mask, sh) || mask || sh[0] != 0 || sh[1] != 0) { std::printf("zeros: mask %d shifts %d %d\n", mask, sh[0], sh[1]); return 1; }
  ++pairs;
  for (int l = 0; l < 64; ++l) p.v[l & 1][l][l & 7] = 0x8000;
  if (round_trip(p, &mask, sh) || mask || sh[0] != 0 || sh[1] != 0) { std::printf("signed zeros: mask %d\n", mask); return 1; }
  ++pairs;
  // (3) off-grid cases, one cause each, in one half: exactly that half is refused, the other is packed
  struct Case { const char* what; int half; uint16_t bits; int s; } cases[] = {
      {"a fifth significant bit", 1, 0x3c88, -12},                                     // (1 + 2^-4 + 2^-7 ..): channel 8..15
      {"eight significant bits", 1, 0x3c81, -14},                                      // (1 + 2^-7) . 2^-6
      {"a bf16 denormal", 0, 0x0040, VC_W8_SHIFT_MIN},
      {"an infinity", 0, 0x7f80, 20},
      {"a NaN", 1, 0x7fc1, 20},
      {"a value below the grid's reach", 0, value_bits(0x08, -12 - 18), -12},          // 17 binades below the top one is the last
  };
  for (const Case& c : cases) {
    fill_normal(p, 0, -12);
    fill_normal(p, 1, -12);
    fill_normal(p, c.half, c.s);
    p.v[0][c.half * 8 + 16 + 3][2] = c.bits;          // channel 3 or 11
    if (round_trip(p, &mask, sh)) return 1;
    if (mask != 1 << c.half) { std::printf("%s in half %d: refusal mask %d\n", c.what, c.half, mask); return 1; }
    ++pairs; ++refused;
  }
  //   1.111b . 2^emax alone moves its half one shift up (240 . 2^(s + 1)); next to the smallest denormal code it is refused
  fill_normal(p, 0, -12);
  fill_half(p, 1, 0x70, -12);
  p.v[1][2][0] = (uint16_t)(value_bits(0x7e, -12) + 0x10);
  if (round_trip(p, &mask, sh)) return 1;
  if (mask || sh[0] != -11 || sh[1] != -12 + (0x70 >> 3) - 15) { std::printf("1.111b: mask %d shifts %d %d\n", mask, sh[0], sh[1]); return 1; }
  ++pairs;
  for (int h = 0; h < 2; ++h)
    for (int l = 0; l < 64; ++l)
      if (vc_w8w_half(l) == 0)
        for (int j = 0; j < 8; ++j) p.v[h][l][j] = value_bits(0x40, -12);
  p.v[1][2][0] = (uint16_t)(value_bits(0x7e, -12) + 0x10);
  p.v[0][35][6] = value_bits(0x01, -12);
  if (round_trip(p, &mask, sh)) return 1;
  if (mask != 1) { std::printf("1.111b next to 2^-9: mask %d\n", mask); return 1; }
  ++pairs; ++refused;
  // (4) arbitrary bf16 patterns: refused, or they come back exactly (round_trip)
  for (int it = 0; it < 500; ++it) {
    for (int h = 0; h < 2; ++h)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) p.v[h][l][j] = (uint16_t)(vc_w8w_half(l) ? rnd() : 0x3c00 + (rnd() & 0x3ff));
    if (round_trip(p, &mask, sh)) return 1;
    if (mask != 3) { std::printf("arbitrary bf16 pair %d: mask %d, expected 3\n", it, mask); return 1; }
    ++pairs; ++refused;
  }
  std::printf("ok %ld %ld\n", pairs, refused);
  return 0;
}
