// The byte arithmetic of the curriculum starts (tiler_slider_amd/csrc/ts_bytes.h) on the host, against byte loops: ge_bytes over
// every pair of byte values, nibble_of over all sixteen nibbles, and the classification of a piece, its deepest distance, byte_of
// and the j-th set bit over random pieces whose bytes crowd the edges (0 .. 5, 248 .. 255), bands wide and narrow, whole and cut
// pieces.  Prints "ok" and exits 0, or says what failed.  tests/test_starts_cpu.py compiles it with the toolchain's clang++.
#include <cstdio>
#include "../../tiler_slider_amd/csrc/ts_bytes.h"
using namespace ts;
#include <cstdlib>
int main() {
  unsigned long checks = 0;
  for (uint32_t c = 0; c < 256; ++c)
    for (uint32_t x = 0; x < 256; ++x) {
      const uint32_t w = x | ((x ^ 0x5a) << 8) | (((x * 7) & 0xff) << 16) | ((255 - x) << 24);
      const uint32_t h = ge_bytes(w, c);
      for (int b = 0; b < 4; ++b) {
        const uint32_t v = (w >> (8 * b)) & 0xff;
        if ((((h >> (8 * b + 7)) & 1) != 0) != (v >= c)) { printf("ge_bytes %u %u\n", v, c); return 1; }
        ++checks;
      }
      if (h & ~kHigh) return 2;
    }
  for (uint32_t n = 0; n < 16; ++n) {
    uint32_t h = 0;
    for (int b = 0; b < 4; ++b) h |= ((n >> b) & 1u) << (8 * b + 7);
    if (nibble_of(h) != n) { printf("nibble_of %u\n", n); return 3; }
  }
  srand(5);
  for (int it = 0; it < 2000000; ++it) {
    Piece p;
    for (int i = 0; i < 4; ++i) {
      p.w[i] = 0;
      for (int b = 0; b < 4; ++b) {
        uint32_t v = rand() & 0xff;
        if (rand() % 3 == 0) v = 248 + rand() % 8;
        if (rand() % 4 == 0) v = rand() % 6;
        p.w[i] |= v << (8 * b);
      }
    }
    uint32_t lo = rand() % 253, hi = rand() % 253;
    if (it % 3 == 0) lo = rand() % 6, hi = lo + rand() % 4;
    if (lo > hi) { uint32_t t = lo; lo = hi; hi = t; }
    const uint32_t rb = it % 5 == 0 ? (uint32_t)(rand() & 0xffff) : 0xffffu;
    classify(p, lo, hi, rb);
    uint32_t band = 0, dist = 0, deep = 0;
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t v = byte_of(p, k);
      if (v != ((p.w[k / 4] >> (8 * (k % 4))) & 0xff)) return 4;
      if (!((rb >> k) & 1)) continue;
      if (v >= lo && v <= hi) band |= 1u << k;
      if (v <= 252) { dist |= 1u << k; if (v + 1 > deep) deep = v + 1; }
    }
    if (band != p.in_band || dist != p.is_dist) { printf("classify %x %x %x %x\n", band, p.in_band, dist, p.is_dist); return 5; }
    if (deepest_plus_one(p) != deep) { printf("deepest %u %u\n", deepest_plus_one(p), deep); return 6; }
    uint32_t seen = 0;
    for (uint32_t k = 0; k < 16; ++k)
      if ((band >> k) & 1) { if (nth_set_bit(band, seen) != k) return 7; ++seen; }
  }
  printf("ok %lu\n", checks);
  return 0;
}
