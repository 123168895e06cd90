// Host round trip of the pairs of the 12-channel QKV image (voicecraft_amd/csrc/vc_w8.h, "w8q"): build with the host compiler and
// -fsanitize=address,undefined and run once (tests/test_w8_qkv_rows_cpu.py does):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/w8_qkv_check.cpp -o w8_qkv_check && ./w8_qkv_check
// Prints "ok <pairs> <refused>" and exits 0, or says what broke.  The decode is the header's host mirror of
// v_cvt_scalef32_pk_bf16_fp8; the device check (w8q_check_k) runs the instruction itself.
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

// A pair in image order: v[h][slot][j] = value j of the slot in k-tile 2j + h; slot = kg * 12 + m, m the channel of the tile.
struct Pair { uint16_t v[2][48][8]; };

// The part of a slot as the format states it, apart from the header: an even tile splits at channel 8, an odd one at channel 4.
static int part_of(int slot, int odd) { const int m = slot % 12; return odd ? (m >= 4) : (m >= 8); }

// Encodes the pair, checks the stored bytes (never the NaN code; exactly 768 B + 2 bytes written) and, for parts that were not refused,
// that the decode gives the image back bit for bit.  Returns the refusal mask in *mask and the two shifts.
static int round_trip(const Pair& p, int odd, int* mask, int shifts[2]) {
  std::vector<uint32_t> img(384), codes(192 + 2, 0xa5a5a5a5u), back(384);      // heap buffers: the sanitizer sees every byte past them
  std::memcpy(img.data(), p.v, 1536);
  std::vector<uint8_t> side(2, 0xa5);
  *mask = vc_w8q_encode_pair(img.data(), odd, codes.data(), side.data());
  if (codes[192] != 0xa5a5a5a5u || codes[193] != 0xa5a5a5a5u) { std::printf("the encode wrote past its 768 B\n"); return 1; }
  for (int h = 0; h < 2; ++h) {
    shifts[h] = (int)side[h] - 127;
    if (shifts[h] < VC_W8_SHIFT_MIN || shifts[h] > VC_W8_SHIFT_MAX) { std::printf("shift %d out of range\n", shifts[h]); return 1; }
  }
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(codes.data());
  for (int i = 0; i < VC_W8Q_PAIR_BYTES; ++i)
    if ((bytes[i] & 0x7f) == 0x7f) { std::printf("the NaN code was stored (byte %d)\n", i); return 1; }
  vc_w8q_decode_pair(codes.data(), side.data(), odd, back.data());
  for (int h = 0; h < 2; ++h)
    for (int s = 0; s < 48; ++s) {
      const int part = vc_w8q_part(s % 12, odd);
      if (part != part_of(s, odd)) { std::printf("slot %d of an %s tile: part %d\n", s, odd ? "odd" : "even", part); return 1; }
      if (std::memcmp(&back[(h * 48 + s) * 4], &img[(h * 48 + s) * 4], 16) != 0 && !((*mask >> part) & 1)) {
        std::printf("k-tile %d slot %d decoded to other bits (shift %d) and its part was not refused\n", h, s, shifts[part]);
        return 1;
      }
      // the layout as stated: the slot's 16 bytes are its eight codes of k-tile 2j, then its eight of k-tile 2j + 1
      if (!((*mask >> part) & 1))
        for (int j = 0; j < 8; ++j)
          if (value_bits(bytes[s * 16 + h * 8 + j], shifts[part]) != p.v[h][s][j] && (p.v[h][s][j] & 0x7fff) != 0) {
            std::printf("byte %d of slot %d is not value %d of k-tile %d\n", h * 8 + j, s, j, h);
            return 1;
          }
    }
  return 0;
}

// the first slot of a part in row group kg = 2
static int a_slot(int part, int odd) { return 2 * 12 + (part ? (odd ? 4 : 8) : 0) + 1; }

// every value of part `part` = a random code <= top at shift s; one slot holds `top` itself
static void fill_part(Pair& p, int odd, int part, int top, int s) {
  for (int h = 0; h < 2; ++h)
    for (int sl = 0; sl < 48; ++sl)
      if (part_of(sl, odd) == part)
        for (int j = 0; j < 8; ++j) p.v[h][sl][j] = value_bits((int)(rnd() % (uint32_t)(top + 1)) | ((rnd() & 1) << 7), s);
  p.v[1][a_slot(part, odd)][5] = value_bits(top, s);
}

// every value of part `part` = a normal code 1.0 .. 416 at shift s (three mantissa bits); one slot holds 448
static void fill_normal(Pair& p, int odd, int part, int s) {
  for (int h = 0; h < 2; ++h)
    for (int sl = 0; sl < 48; ++sl)
      if (part_of(sl, odd) == part)
        for (int j = 0; j < 8; ++j) p.v[h][sl][j] = value_bits(0x40 + (int)(rnd() % 0x3e), s);
  p.v[1][a_slot(part, odd)][5] = value_bits(0x7e, s);
}

int main() {
  static_assert(VC_W8Q_PAIR_BYTES == VC_W8Q_SLOTS * 16 && VC_W8Q_PAIR_U4 * 16 == VC_W8Q_PAIR_BYTES, "pair layout");
  long pairs = 0, refused = 0;
  int mask, sh[2];
  Pair p;
  for (int odd = 0; odd < 2; ++odd) {
    // (1) a pseudo-random on-grid image: both parts at shifts of their own, every top code; the packer must find exactly the shifts
    for (int it = 0; it < 2000; ++it) {
      int s[2], top[2];
      for (int part = 0; part < 2; ++part) {
        s[part] = VC_W8_SHIFT_MIN + (int)(rnd() % (uint32_t)(VC_W8_SHIFT_MAX - VC_W8_SHIFT_MIN + 1));
        top[part] = 0x78 + (int)(rnd() % 7u);          // a code of the top binade: 256 .. 448
        fill_part(p, odd, part, top[part], s[part]);
      }
      if (round_trip(p, odd, &mask, sh)) return 1;
      if (mask || sh[0] != s[0] || sh[1] != s[1]) {
        std::printf("random pair %d (odd %d): mask %d, shifts %d %d for %d %d\n", it, odd, mask, sh[0], sh[1], s[0], s[1]);
        return 1;
      }
      ++pairs;
    }
    // (2) the parts 2^6 apart with the same codes; zeros; +-0 mixes
    fill_normal(p, odd, 0, -10);
    for (int h = 0; h < 2; ++h)
      for (int sl = 0; sl < 48; ++sl)
        if (part_of(sl, odd) == 1)
          for (int j = 0; j < 8; ++j) p.v[h][sl][j] = value_bits(0x7e, -4);
    if (round_trip(p, odd, &mask, sh)) return 1;
    if (mask || sh[0] != -10 || sh[1] != -4) { std::printf("parts apart: mask %d shifts %d %d\n", mask, sh[0], sh[1]); return 1; }
    ++pairs;
    std::memset(&p, 0, sizeof p);
    if (round_trip(p, odd, &mask, sh) || mask || sh[0] != 0 || sh[1] != 0) { std::printf("zeros: mask %d shifts %d %d\n", mask, sh[0], sh[1]); return 1; }
    ++pairs;
    for (int sl = 0; sl < 48; ++sl) p.v[sl & 1][sl][sl & 7] = 0x8000;
    if (round_trip(p, odd, &mask, sh) || mask || sh[0] != 0 || sh[1] != 0) { std::printf("signed zeros: mask %d\n", mask); return 1; }
    ++pairs;
    // (3) off-grid cases, one cause each, in one part: exactly that part is refused, the other is packed
    struct Case { const char* what; int part; uint16_t bits; int s; } cases[] = {
        {"a fifth significant bit", 1, 0x3c88, -12},
        {"eight significant bits", 1, 0x3c81, -14},                                      // (1 + 2^-7) . 2^-6
        {"eight significant bits", 0, 0x3c81, -14},
        {"a bf16 denormal", 0, 0x0040, VC_W8_SHIFT_MIN},
        {"an infinity", 0, 0x7f80, 20},
        {"a NaN", 1, 0x7fc1, 20},
        {"a value below the grid's reach", 0, value_bits(0x08, -12 - 18), -12},          // 17 binades below the top one is the last
    };
    for (const Case& c : cases) {
      fill_normal(p, odd, 0, -12);
      fill_normal(p, odd, 1, -12);
      fill_normal(p, odd, c.part, c.s);
      p.v[0][a_slot(c.part, odd) - 12][2] = c.bits;
      if (round_trip(p, odd, &mask, sh)) return 1;
      if (mask != 1 << c.part) { std::printf("%s in part %d (odd %d): refusal mask %d\n", c.what, c.part, odd, mask); return 1; }
      ++pairs; ++refused;
    }
    //   1.111b . 2^emax alone moves its part one shift up (240 . 2^(s + 1))
    fill_normal(p, odd, 0, -12);
    fill_normal(p, odd, 1, -12);
    p.v[1][a_slot(0, odd)][0] = (uint16_t)(value_bits(0x7e, -12) + 0x10);
    if (round_trip(p, odd, &mask, sh)) return 1;
    if (mask || sh[0] != -11 || sh[1] != -12) { std::printf("1.111b: mask %d shifts %d %d\n", mask, sh[0], sh[1]); return 1; }
    ++pairs;
    // (4) arbitrary bf16 patterns: refused, or they come back exactly (round_trip)
    for (int it = 0; it < 300; ++it) {
      for (int h = 0; h < 2; ++h)
        for (int sl = 0; sl < 48; ++sl)
          for (int j = 0; j < 8; ++j) p.v[h][sl][j] = (uint16_t)(part_of(sl, odd) ? rnd() : 0x3c00 + (rnd() & 0x3ff));
      if (round_trip(p, odd, &mask, sh)) return 1;
      if (mask != 3) { std::printf("arbitrary bf16 pair %d: mask %d, expected 3\n", it, mask); return 1; }
      ++pairs; ++refused;
    }
  }
  std::printf("ok %ld %ld\n", pairs, refused);
  return 0;
}
