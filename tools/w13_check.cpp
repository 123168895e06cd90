// Host round trip of the 13-bit weight planes (voicecraft_amd/csrc/vc_w13.h): build with the host compiler and
// -fsanitize=address,undefined, run by tests/test_w13_cpu.py.  Prints "ok <fragments> <refused>" and exits 0, or says what broke.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../voicecraft_amd/csrc/vc_w13.h"

// A group of four 512-value fragments: vals[f][lane][j].  Returns the refusal mask the way the device packer finds it (per fragment,
// from the minimum / maximum over its 64 lanes), and checks that every accepted fragment decodes bit for bit.
static int round_trip(const uint16_t vals[4][64][8], int* refused_mask) {
  uint32_t w[64][4][4];
  int base[4], ok[4];
  for (int f = 0; f < 4; ++f) {
    int mn = 128, mx = 0;
    for (int l = 0; l < 64; ++l) {
      for (int q = 0; q < 4; ++q) w[l][f][q] = (uint32_t)vals[f][l][2 * q] | ((uint32_t)vals[f][l][2 * q + 1] << 16);
      int a, b;
      vc_w13_minmax(w[l][f], &a, &b);
      mn = a < mn ? a : mn; mx = b > mx ? b : mx;
    }
    base[f] = vc_w13_base(mn, mx, &ok[f]);
    if (base[f] < 1 || base[f] > 127) { std::printf("base %d out of range\n", base[f]); return 1; }
  }
  *refused_mask = 0;
  int bad_any = 0;
  for (int f = 0; f < 4; ++f) *refused_mask |= ok[f] ? 0 : 1 << f;
  for (int l = 0; l < 64; ++l) {
    vc_w13_lane L;
    std::memset(&L, 0xa5, sizeof L);
    const int bad = vc_w13_encode(w[l], base, &L);
    bad_any |= bad;
    if (bad & ~*refused_mask) { std::printf("lane %d: a value outside the window of an ACCEPTED fragment (mask %d)\n", l, bad); return 1; }
    for (int f = 0; f < 4; ++f) {
      if (!ok[f]) continue;
      uint32_t d[4];
      vc_w13_decode_frag(&L, f, base[f], d);
      if (std::memcmp(d, w[l][f], sizeof d) != 0) {
        std::printf("fragment %d lane %d: %08x %08x %08x %08x decoded as %08x %08x %08x %08x (base %d)\n", f, l, w[l][f][0], w[l][f][1],
                    w[l][f][2], w[l][f][3], d[0], d[1], d[2], d[3], base[f]);
        return 1;
      }
    }
  }
  if (bad_any != *refused_mask) { std::printf("refusal by span (%d) and by encoding (%d) disagree\n", *refused_mask, bad_any); return 1; }
  return 0;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main() {
  static_assert(sizeof(vc_w13_lane) == 52, "52 bytes per lane and group");
  static_assert(VC_W13_GROUP_BYTES == 64 * 52 && VC_W13_GROUP_U4 * 16 == VC_W13_GROUP_BYTES, "group layout");
  std::vector<uint16_t> buf(4 * 64 * 8);
  auto vals = reinterpret_cast<uint16_t(*)[64][8]>(buf.data());
  long frags = 0, refused = 0;
  int mask;
  // (1) every bf16 bit pattern: hi7 = h fills one fragment with all 512 (sign, lo) combinations; four values of h per group.  On top,
  //     the same patterns with the fragment's window spread to both ends (h .. h + 14), zeros and denormals mixed in.
  for (int pass = 0; pass < 2; ++pass)
    for (int h0 = 0; h0 < 128; h0 += 4) {
      for (int f = 0; f < 4; ++f)
        for (int i = 0; i < 512; ++i) {
          int h = h0 + f;
          if (pass == 1) {
            const int r = i % 17;                      // 0..14: the window's steps, 15: hi7 = 0 (zero / denormal), 16: the top end again
            h = r == 15 ? 0 : h + (r == 16 ? 14 : r);
            if (h > 127) h = h0 + f;
          }
          vals[f][i >> 3][i & 7] = (uint16_t)(((i >> 8) << 15) | (h << 8) | (i & 0xff));
        }
      if (round_trip(vals, &mask)) return 1;
      if (mask) { std::printf("pass %d, hi7 %d..: refused (mask %d)\n", pass, h0, mask); return 1; }
      frags += 4;
    }
  // (2) fragments of zeros only, of +-0 mixes, of denormals only
  for (int f = 0; f < 4; ++f)
    for (int i = 0; i < 512; ++i)
      vals[f][i >> 3][i & 7] = f == 0 ? 0 : f == 1 ? (uint16_t)((i & 1) << 15) : f == 2 ? (uint16_t)(((i & 1) << 15) | (i & 0xff)) : (uint16_t)((i % 3 == 0) << 15);
  if (round_trip(vals, &mask) || mask) { std::printf("zero fragments: mask %d\n", mask); return 1; }
  frags += 4;
  // (3) the window's limits: a span of exactly 15 steps (30 binades) is packed wherever it sits; one step more is refused, never mis-encoded
  for (int lo = 1; lo <= 127; ++lo)
    for (int span = 14; span <= 16 && lo + span <= 127; ++span) {
      for (int f = 0; f < 4; ++f)
        for (int i = 0; i < 512; ++i) {
          const uint32_t r = rnd();
          int h = lo + (int)(r % (uint32_t)(span + 1));
          if (i == 5 * f) h = lo;
          if (i == 300 + f) h = lo + span;
          if (i % 29 == 7) h = 0;
          vals[f][i >> 3][i & 7] = (uint16_t)((((r >> 9) & 1) << 15) | (h << 8) | ((r >> 10) & 0xff));
        }
      if (round_trip(vals, &mask)) return 1;
      const int want = span >= VC_W13_CODES ? 15 : 0;
      if (mask != want) { std::printf("hi7 %d..%d: refusal mask %d, expected %d\n", lo, lo + span, mask, want); return 1; }
      frags += 4; refused += span >= VC_W13_CODES ? 4 : 0;
    }
  // (4) one stray tiny value next to ordinary weights refuses its fragment alone
  for (int f = 0; f < 4; ++f)
    for (int i = 0; i < 512; ++i) vals[f][i >> 3][i & 7] = (uint16_t)(0x3c00 + (rnd() & 0x3ff));      // around 0.01 .. 0.03
  vals[2][17][3] = 0x2b8d;                                                                              // ~1e-12
  if (round_trip(vals, &mask)) return 1;
  if (mask != 4) { std::printf("stray value: refusal mask %d, expected 4\n", mask); return 1; }
  frags += 4; refused += 1;
  // (5) random groups, random windows
  for (int it = 0; it < 2000; ++it) {
    for (int f = 0; f < 4; ++f) {
      const int lo = 1 + (int)(rnd() % 113u), span = (int)(rnd() % 15u);
      for (int i = 0; i < 512; ++i) {
        const uint32_t r = rnd();
        const int h = (r & 31) == 0 ? 0 : lo + (int)((r >> 5) % (uint32_t)(span + 1));
        vals[f][i >> 3][i & 7] = (uint16_t)((((r >> 12) & 1) << 15) | (h << 8) | ((r >> 13) & 0xff));
      }
    }
    if (round_trip(vals, &mask) || mask) { std::printf("random group %d: mask %d\n", it, mask); return 1; }
    frags += 4;
  }
  std::printf("ok %ld %ld\n", frags, refused);
  return 0;
}
