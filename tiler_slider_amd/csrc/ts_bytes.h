// ts_bytes.h — the byte arithmetic of the curriculum starts (ts_starts.hip): sixteen table bytes, four words, classified four
// bytes at a time (SWAR), without a GPU in sight.  TS_HD like ts_core.h and for the same reason: tests/native/starts_bytes_check.cpp
// runs these exact functions on the host over every byte value and every band edge.  No product code path executes them on the
// host.  Needs clang (the packed 16-bit maximum is a vector builtin): hipcc for the kernels, the toolchain's clang++ for the check.
#pragma once
#include "ts_core.h"

namespace ts {

constexpr uint32_t kPieceBytes = 16;
constexpr uint32_t kMaxDistance = 252;  // TS_TABLE_MAX_DEPTH: a larger byte is no distance

constexpr uint32_t kHigh = 0x80808080u, kLow7 = 0x7f7f7f7fu;

// bit 7 of every byte of x that is >= c (c = 0 .. 255, the same for the four bytes).  The low seven bits are compared by a
// subtraction that cannot borrow across bytes - (x & 0x7f | 0x80) - (c & 0x7f) keeps bit 7 <=> x & 0x7f >= c & 0x7f -, the high
// bits decide the rest: c < 128: x >= 128 or the low bits say so; c >= 128: x >= 128 and the low bits say so.
TS_HD uint32_t ge_bytes(uint32_t x, uint32_t c) {
  const uint32_t d = ((x & kLow7) | kHigh) - ((c & 0x7fu) * 0x01010101u);
  return (c & 0x80u ? x & d : x | d) & kHigh;
}
// the four bits 7, 15, 23, 31 of h as bits 0 .. 3: the products 2^(8 b + 7 k) are all distinct, and b + k = 3 lands on 21 + b
TS_HD uint32_t nibble_of(uint32_t h) { return (((h >> 7) * 0x00204081u) >> 21) & 0xfu; }

// What a lane keeps of one piece: the sixteen bytes, bit k of `in_band` <=> byte k lies in the row and in the band, bit k of
// `is_dist` <=> byte k lies in the row and is a distance (<= 252).
struct Piece {
  uint32_t w[4];
  uint32_t in_band, is_dist;
};
// lo <= hi <= 252 (an empty band never gets here); row_bits: the bytes of the piece that belong to the row
TS_HD void classify(Piece &p, uint32_t lo, uint32_t hi, uint32_t row_bits) {
  uint32_t band = 0, dist = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    band |= nibble_of(ge_bytes(p.w[i], lo) & ~ge_bytes(p.w[i], hi + 1u)) << (4 * i);
    dist |= nibble_of(~ge_bytes(p.w[i], kMaxDistance + 1u) & kHigh) << (4 * i);
  }
  p.in_band = band & row_bits, p.is_dist = dist & row_bits;
}
// k = 0 .. 15.  All four words are read and the choice is made on values: a word picked by address would turn the piece
// into an indexed array, which the compiler then keeps in LDS.
TS_HD uint32_t byte_of(const Piece &p, uint32_t k) {
  const uint64_t low = p.w[0] | (uint64_t)p.w[1] << 32, high = p.w[2] | (uint64_t)p.w[3] << 32;
  return (uint32_t)((k < 8u ? low : high) >> (8u * (k & 7u))) & 0xffu;
}
// the larger of the two 16-bit halves, half by half (v_pk_max_u16)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
TS_HD uint32_t max_halves(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// 1 + the largest distance of the piece, 0 where it holds none.  Bit b of a nibble becomes bit 0 of byte b (the products
// 2^(b + 7 k) are all distinct, k = b lands on 8 b); a distance is at most 252, so adding 1 to its byte carries nowhere.
TS_HD uint32_t deepest_plus_one(const Piece &p) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t ones = (((p.is_dist >> (4 * i)) & 0xfu) * 0x00204081u) & 0x01010101u;
    const uint32_t y = (p.w[i] & (ones * 0xffu)) + ones;
    m = max_halves(max_halves(m, y & 0x00ff00ffu), (y >> 8) & 0x00ff00ffu);
  }
  return (m & 0xffffu) > (m >> 16) ? (m & 0xffffu) : (m >> 16);
}
// the position of the (k + 1)-th set bit of m; the caller guarantees popc(m) > k
TS_HD uint32_t nth_set_bit(uint32_t m, uint32_t k) {
  for (; k; --k) m &= m - 1u;
  return (uint32_t)lsb(m);
}

}  // namespace ts
