// Host round trip of the block-scaled E4M3 weight bytes (voicecraft_amd/csrc/vc_w8.h): build with the host compiler and
// -fsanitize=address,undefined, run by tests/test_w8_cpu.py.  Prints "ok <fragments> <refused>" and exits 0, or says what broke.
// The decode is the header's host mirror of v_cvt_scalef32_pk_bf16_fp8; the device check (w8_check_k) runs the instruction itself.
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

// A group of four 512-value fragments: vals[f][lane][j].  Packs it the way the device packer does (shift per fragment from the
// extremes over its 64 lanes), returns the refusal mask, and checks that every accepted fragment decodes bit for bit.
static int round_trip(const uint16_t vals[4][64][8], int* refused_mask, int shifts[4]) {
  uint32_t w[64][4][4];
  int ok[4];
  for (int f = 0; f < 4; ++f) {
    int mn = 256, mx = -1, top = 0;
    for (int l = 0; l < 64; ++l) {
      for (int q = 0; q < 4; ++q) w[l][f][q] = (uint32_t)vals[f][l][2 * q] | ((uint32_t)vals[f][l][2 * q + 1] << 16);
      int a, b;
      vc_w8_minmax(w[l][f], &a, &b);
      mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    for (int l = 0; l < 64; ++l) top |= vc_w8_top111(w[l][f], mx);
    shifts[f] = vc_w8_shift(mn, mx, top, &ok[f]);
    if (shifts[f] < VC_W8_SHIFT_MIN || shifts[f] > VC_W8_SHIFT_MAX) { std::printf("shift %d out of range\n", shifts[f]); return 1; }
  }
  *refused_mask = 0;
  for (int f = 0; f < 4; ++f) *refused_mask |= ok[f] ? 0 : 1 << f;
  std::vector<vc_w8_lane> L(64);
  for (int l = 0; l < 64; ++l) {
    std::memset(&L[l], 0xa5, sizeof L[l]);
    *refused_mask |= vc_w8_encode(w[l], shifts, &L[l]);
  }
  for (int l = 0; l < 64; ++l)
    for (int f = 0; f < 4; ++f) {
      const uint32_t* piece = f < 2 ? L[l].a : L[l].b;
      for (int j = 0; j < 8; ++j)
        if (((piece[2 * (f & 1) + (j >> 2)] >> (8 * (j & 3))) & 0x7fu) == 0x7fu) { std::printf("the NaN code was stored (fragment %d lane %d)\n", f, l); return 1; }
      uint32_t d[4];
      vc_w8_decode_frag(&L[l], f, vc_w8_side(shifts[f]), d);
      const bool same = std::memcmp(d, w[l][f], sizeof d) == 0;
      if (!same && !((*refused_mask >> f) & 1)) {
        std::printf("fragment %d lane %d: %08x %08x %08x %08x decoded as %08x %08x %08x %08x (shift %d) and was not refused\n", f, l, w[l][f][0],
                    w[l][f][1], w[l][f][2], w[l][f][3], d[0], d[1], d[2], d[3], shifts[f]);
        return 1;
      }
    }
  return 0;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main() {
  static_assert(sizeof(vc_w8_lane) == 32, "32 bytes per lane and group");
  static_assert(VC_W8_GROUP_BYTES == 64 * 32 && VC_W8_GROUP_U4 * 16 == VC_W8_GROUP_BYTES, "group layout");
  std::vector<uint16_t> buf(4 * 64 * 8);
  auto vals = reinterpret_cast<uint16_t(*)[64][8]>(buf.data());
  long frags = 0, refused = 0;
  int mask, sh[4];
  // (1) all 254 non-NaN codes (+-0 among them) in one fragment, at both ends of the allowed shifts, next to them, and in between:
  //     the fragment holds 448 . 2^s, so the packer must find exactly s, and every value must come back
  const int ends[8] = {VC_W8_SHIFT_MIN, VC_W8_SHIFT_MIN + 1, -9, 0, 1, VC_W8_SHIFT_MAX - 1, VC_W8_SHIFT_MAX, -60};
  for (int g = 0; g < 2; ++g) {
    for (int f = 0; f < 4; ++f) {
      const int s = ends[4 * g + f];
      int i = 0;
      for (int c = 0; c < 256; ++c)
        if ((c & 0x7f) != 0x7f) { vals[f][i >> 3][i & 7] = value_bits(c, s); ++i; }
      for (; i < 512; ++i) { const int c = (int)(rnd() & 0xff); vals[f][i >> 3][i & 7] = value_bits((c & 0x7f) == 0x7f ? c ^ 1 : c, s); }
    }
    if (round_trip(vals, &mask, sh)) return 1;
    if (mask) { std::printf("all codes: refused (mask %d)\n", mask); return 1; }
    for (int f = 0; f < 4; ++f) if (sh[f] != ends[4 * g + f]) { std::printf("all codes at shift %d: packed at %d\n", ends[4 * g + f], sh[f]); return 1; }
    frags += 4;
  }
  // (2) the shift follows the largest value: fragments whose top code is c hold q <= c, at every top code; zeros only; +-0 mixes
  for (int top = 1; top < 0x7f; top += 4) {
    for (int f = 0; f < 4; ++f)
      for (int i = 0; i < 512; ++i) {
        const int c = i == 7 ? top + f : (int)(rnd() % (uint32_t)(top + f + 1));
        vals[f][i >> 3][i & 7] = value_bits((c > 0x7e ? 0x7e : c) | ((rnd() & 1) << 7), top - 80);
      }
    if (round_trip(vals, &mask, sh) || mask) { std::printf("top code %d: mask %d\n", top, mask); return 1; }
    frags += 4;
  }
  for (int f = 0; f < 4; ++f)
    for (int i = 0; i < 512; ++i) vals[f][i >> 3][i & 7] = f == 0 ? 0 : f == 1 ? (uint16_t)((i & 1) << 15) : f == 2 ? (uint16_t)((i % 3 == 0) << 15) : 0x8000;
  if (round_trip(vals, &mask, sh) || mask) { std::printf("zero fragments: mask %d\n", mask); return 1; }
  frags += 4;
  // (3) refusals, one cause per fragment, ordinary codes around it
  auto fill = [&](int f, int s) {
    for (int i = 0; i < 512; ++i) vals[f][i >> 3][i & 7] = value_bits(0x40 + (int)(rnd() % 0x3e), s);   // 1.0 .. 416 . 2^s; 448 below
    vals[f][5][5] = value_bits(0x7e, s);
  };
  //   f0: a value with a fifth significant bit; f1: 1.111b . 2^emax (the NaN code at emax - 8) next to a denormal code 2^-9 . 2^s that
  //   the next shift cannot hold; f2: a bf16 denormal; f3: an infinity
  fill(0, -12); vals[0][17][3] = 0x3c88;
  fill(1, -12); vals[1][9][1] = (uint16_t)(value_bits(0x7e, -12) + 0x10); vals[1][40][6] = value_bits(0x01, -12);
  fill(2, VC_W8_SHIFT_MIN); vals[2][0][0] = 0x0040;
  fill(3, 20); vals[3][63][7] = 0x7f80;
  if (round_trip(vals, &mask, sh)) return 1;
  if (mask != 15) { std::printf("off-grid fragments: refusal mask %d, expected 15\n", mask); return 1; }
  frags += 4; refused += 4;
  //   the same fragments without their cause are packed; 1.111b . 2^emax ALONE moves the fragment one shift up (240 . 2^(s + 1))
  fill(0, -12);
  fill(1, -12); vals[1][9][1] = (uint16_t)(value_bits(0x7e, -12) + 0x10);
  fill(2, VC_W8_SHIFT_MIN);
  fill(3, 20);
  if (round_trip(vals, &mask, sh)) return 1;
  if (mask != 0 || sh[0] != -12 || sh[1] != -11 || sh[2] != VC_W8_SHIFT_MIN || sh[3] != 20) {
    std::printf("on-grid twins: mask %d, shifts %d %d %d %d\n", mask, sh[0], sh[1], sh[2], sh[3]);
    return 1;
  }
  frags += 4;
  //   tiny values: below 2^-109 the shift stays at its minimum and the codes get smaller
  for (int f = 0; f < 4; ++f) {
    for (int i = 0; i < 512; ++i) vals[f][i >> 3][i & 7] = value_bits((int)(rnd() % (uint32_t)(0x30 - 8 * f)) | ((rnd() & 1) << 7), VC_W8_SHIFT_MIN);
  }
  if (round_trip(vals, &mask, sh) || mask) { std::printf("tiny fragments: mask %d\n", mask); return 1; }
  for (int f = 0; f < 4; ++f) if (sh[f] != VC_W8_SHIFT_MIN) { std::printf("tiny fragment %d: shift %d\n", f, sh[f]); return 1; }
  frags += 4;
  // (4) random fragments on the grid at random shifts; and arbitrary bf16 patterns, which are refused or come back exactly (round_trip)
  for (int it = 0; it < 2000; ++it) {
    for (int f = 0; f < 4; ++f) {
      const int s = VC_W8_SHIFT_MIN + (int)(rnd() % (uint32_t)(VC_W8_SHIFT_MAX - VC_W8_SHIFT_MIN + 1));
      const int span = 1 + (int)(rnd() % 0x7eu);
      for (int i = 0; i < 512; ++i) vals[f][i >> 3][i & 7] = value_bits((int)(rnd() % (uint32_t)(span + 1)) | ((rnd() & 1) << 7), s);
    }
    if (round_trip(vals, &mask, sh) || mask) { std::printf("random group %d: mask %d\n", it, mask); return 1; }
    frags += 4;
  }
  for (int it = 0; it < 500; ++it) {
    for (int f = 0; f < 4; ++f)
      for (int i = 0; i < 512; ++i) vals[f][i >> 3][i & 7] = (uint16_t)(f < 2 ? rnd() : 0x3c00 + (rnd() & 0x3ff));
    if (round_trip(vals, &mask, sh)) return 1;
    if (mask != 15) { std::printf("arbitrary bf16 group %d: mask %d, expected 15\n", it, mask); return 1; }
    frags += 4; refused += 4;
  }
  std::printf("ok %ld %ld\n", frags, refused);
  return 0;
}
