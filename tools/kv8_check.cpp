// Host check of the K/V cache's 8-bit grid (voicecraft_amd/csrc/vc_kv8.h): build with the host compiler and
// -fsanitize=address,undefined, run by tests/test_kv8_cpu.py.  Prints "ok <rows> <values>" (with "centred": "ok <rows> <values> centred
// <centred rows>") and exits 0, or says what broke.
// The reference here shares nothing with the header: the 127 E4M3 magnitudes by enumeration, the nearest one by search over doubles.
// With the argument "centred" the rows also go through vc_kv8c_quantize_row against centres of several sizes: the centred row is
// restated in doubles (the exact difference, rounded to fp32 by the cast and to bf16 by nearbyint on the scaled mantissa).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../voicecraft_amd/csrc/vc_kv8.h"

static double mags[127];

static double bf16_value(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return (double)f;
}

// nearest non-NaN code of |x| (x already divided by 2^s), ties to the even code; beyond 448: 0x7e
static int nearest_code(double x) {
  if (x >= 448.0) return 0x7e;
  int best = 0;
  for (int c = 1; c < 127; ++c) {
    const double d = std::fabs(mags[c] - x), db = std::fabs(mags[best] - x);
    if (d < db || (d == db && !(c & 1))) best = c;
  }
  return best;
}

static long n_rows = 0, n_vals = 0, n_centred = 0;

static int check_row(const std::vector<uint16_t>& row) {
  const int hd = (int)row.size();
  std::vector<uint8_t> codes(hd);
  const int s = vc_kv8_quantize_row(row.data(), hd, codes.data());
  double amax = 0;
  for (int j = 0; j < hd; ++j) amax = std::fmax(amax, std::fabs(bf16_value(row[j])));
  int want = 0;
  if (amax > 0) {
    int e;
    std::frexp(amax, &e);
    want = e - 1 - 8;
    if (want < VC_W8_SHIFT_MIN) want = VC_W8_SHIFT_MIN;
    if (want > VC_W8_SHIFT_MAX) want = VC_W8_SHIFT_MAX;
    if (std::ldexp(amax, -want) > 464.0) ++want;
    if (want > VC_W8_SHIFT_MAX) want = VC_W8_SHIFT_MAX;
  }
  if (s != want) { std::printf("shift %d, want %d (amax %g)\n", s, want, amax); return 1; }
  for (int j = 0; j < hd; ++j) {
    const double v = bf16_value(row[j]);
    const int c = nearest_code(std::ldexp(std::fabs(v), -s)) | (row[j] & 0x8000 ? 0x80 : 0);
    if (codes[j] != c) { std::printf("value %04x at shift %d: code %02x, want %02x\n", row[j], s, codes[j], c); return 1; }
    if ((codes[j] & 0x7f) == 0x7f) { std::printf("the NaN code was stored\n"); return 1; }
    // decode: the exact bf16 pattern of q . 2^s, and encode(decode) = the code (idempotence)
    const uint32_t back = vc_kv8_decode_value(codes[j], s);
    const double q = std::ldexp(mags[codes[j] & 0x7f], s);
    if (bf16_value((uint16_t)back) != (codes[j] & 0x80 ? -q : q) || (back >> 16)) { std::printf("decode of %02x at %d: %04x\n", codes[j], s, back); return 1; }
    if (vc_kv8_encode_value(back, s) != codes[j]) { std::printf("encode(decode(%02x)) at %d differs\n", codes[j], s); return 1; }
    ++n_vals;
  }
  ++n_rows;
  return 0;
}

// bf16_rne(float(k) - float(c)), restated: the difference of two bf16 numbers is exact in a double
static uint16_t centred_value(uint16_t k, uint16_t c) {
  const float d = (float)(bf16_value(k) - bf16_value(c));      // the cast rounds to nearest even: what the fp32 subtraction gives
  if (d == 0.0f) { uint32_t u; std::memcpy(&u, &d, 4); return (uint16_t)(u >> 16); }
  int e;
  const double m = std::frexp((double)d, &e);                  // |m| in [0.5, 1)
  double r;
  if (e < -125) r = std::ldexp(std::nearbyint(std::ldexp((double)d, 133)), -133);      // a bf16 denormal: steps of 2^-133
  else r = std::ldexp(std::nearbyint(std::ldexp(m, 8)), e - 8);
  const float f = (float)r;
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if (u & 0xffffu) { std::printf("centred value not a bf16 number\n"); std::exit(1); }
  return (uint16_t)(u >> 16);
}

static int check_centred(const std::vector<uint16_t>& row, const std::vector<uint16_t>& centre) {
  const int hd = (int)row.size();
  std::vector<uint16_t> moved(hd);
  for (int j = 0; j < hd; ++j) {
    moved[j] = centred_value(row[j], centre[j]);
    if ((moved[j] & 0x7f80) == 0x7f80) return 0;               // an overflow of the difference: no cached row does that
  }
  std::vector<uint8_t> a(hd), b(hd);
  const int sa = vc_kv8c_quantize_row(row.data(), centre.data(), hd, a.data());
  const int sb = vc_kv8_quantize_row(moved.data(), hd, b.data());
  if (sa != sb || a != b) { std::printf("centred row: shift %d / %d or codes differ from the restated row's\n", sa, sb); return 1; }
  ++n_centred;
  return check_row(moved);
}

int main(int argc, char** argv) {
  const bool centred = argc > 1 && !std::strcmp(argv[1], "centred");
  for (int c = 0; c < 127; ++c) {
    const int E = c >> 3, M = c & 7;
    mags[c] = E == 0 ? std::ldexp((double)M, -9) : std::ldexp((double)(8 + M), E - 10);
  }
  uint32_t rng = 12345u;
  auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
  for (int hd : {32, 64, 128}) {
    // every bf16 pattern of 40 binades around a maximum at each mantissa of the top binade (both sides of 464), once per row
    for (int top_m = 0; top_m < 128; ++top_m)
      for (int base = 90; base <= 160; base += 35) {
        std::vector<uint16_t> row(hd, 0);
        row[0] = (uint16_t)((base << 7) | top_m);
        for (int j = 1; j < hd; ++j) {
          const int field = base - (int)(next() % 20);
          row[j] = (uint16_t)(((next() & 1) << 15) | (field << 7) | (next() & 0x7f));
          if ((row[j] & 0x7fff) > row[0]) row[j] = row[0];
        }
        row[hd - 1] = 0x8000;      // -0
        if (check_row(row)) return 1;
        if (centred)               // centres of nothing, of the rows' own size, of 32 times it, and one equal to the row
          for (int kind = 0; kind < 4; ++kind) {
            std::vector<uint16_t> c(hd, 0);
            for (int j = 0; j < hd && kind; ++j)
              c[j] = kind == 3 ? row[j] : (uint16_t)(((next() & 1) << 15) | ((base - 2 + (kind == 2 ? 5 : 0) - (int)(next() % 3)) << 7) | (next() & 0x7f));
            if (check_centred(row, c)) return 1;
          }
      }
    // rows of zeros, of bf16 denormals, of the smallest and the largest normal numbers, and ties at every binade
    if (check_row(std::vector<uint16_t>(hd, 0))) return 1;
    { std::vector<uint16_t> r(hd, 0); for (int j = 0; j < hd; ++j) r[j] = (uint16_t)(next() & 0x7f); if (check_row(r)) return 1; }
    { std::vector<uint16_t> r(hd, 0x0080); r[1] = 0x00ff; r[2] = 0x8001; if (check_row(r)) return 1; }
    { std::vector<uint16_t> r(hd, 0x7f00); r[1] = 0x7f7f; r[2] = 0xff7f; r[3] = 0x7000; if (check_row(r)) return 1; }
    for (int e = 100; e < 150; ++e) {
      std::vector<uint16_t> r(hd, 0);
      r[0] = (uint16_t)((e << 7) | 0x60);                       // 448 . 2^s
      for (int j = 1; j < hd; ++j) r[j] = (uint16_t)(((e - j % 18) << 7) | ((j * 8 + 8) & 0x78) | ((j & 32) ? 0x8000 : 0));   // odd sixteenths: ties
      if (check_row(r)) return 1;
    }
  }
  if (centred) std::printf("ok %ld %ld centred %ld\n", n_rows, n_vals, n_centred);
  else std::printf("ok %ld %ld\n", n_rows, n_vals);
  return 0;
}
