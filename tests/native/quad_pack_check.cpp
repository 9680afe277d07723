// The descriptor of the in-place step's quad store (tiler_slider_amd/csrc/ts_quad.h) on the host.
//  1. One slot, exhaustively: every cell 0 .. 63, every value 0 .. 2, present and absent, in each of the four positions of a
//     word, beside every filler of the other three positions (nothing, the largest legal slot, a mixed one): what comes out is
//     what went in, an absent slot is zero whatever its cell and value, and no position disturbs another.
//  2. The kernel's words, exhaustively for S <= 4 and over edge cells for S = 5 .. 8: for every board size, tile count 1 and 2,
//     every cell a tile enters and leaves, both values of an entered cell (tile index + 1, or 1 in single colour) and every
//     presence of the 2 T slots, the word is packed as step_update_body packs it and unpacked as its four passes unpack it.
//     A word of zero <=> nothing present.
//  3. The four passes of a quad: four such words, one per lane; pass j hands lane k slot k of lane j's word.  The stores that
//     come out are, as a multiset of (board, cell, value), those of the per-lane loop.
// Prints "ok" and exits 0, or says what failed.  tests/test_update_quad_cpu.py compiles it with the toolchain's clang++.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <tuple>
#include "../../tiler_slider_amd/csrc/ts_quad.h"
using namespace ts;

struct Store {
  bool present;
  uint32_t cell, value;
};

static uint32_t pack(const Store *s, int n) {  // as step_update_body: slot 2 t enters, slot 2 t + 1 leaves
  uint32_t word = 0;
  for (int k = 0; k < n; ++k) word |= quad_word(quad_slot(s[k].present, s[k].cell, s[k].value), (uint32_t)k);
  return word;
}

static int check_word(uint32_t word, const Store *s, int n) {
  bool any = false;
  for (uint32_t k = 0; k < kQuadSlots; ++k) {
    const uint32_t slot = quad_slot_of(word, k);
    const bool want = (int)k < n && s[k].present;
    any |= want;
    if (quad_present(slot) != want) return 1;
    if (want && (quad_cell(slot) != s[k].cell || quad_value(slot) != s[k].value)) return 2;
    if (!want && slot != 0) return 3;
  }
  if ((word == 0) == any) return 4;
  return 0;
}

int main() {
  unsigned long checks = 0;
  static_assert(kQuadSlots == 4 && kQuadMaxCell == 63 && kQuadMaxValue == 2, "the layout the comments describe");
  // 1. one slot beside fillers
  const uint32_t fillers[3] = {0u, quad_slot(true, kQuadMaxCell, kQuadMaxValue), quad_slot(true, 21, 1)};
  if (fillers[1] != 0xffu) { printf("the largest slot is %#x\n", fillers[1]); return 1; }
  for (uint32_t k = 0; k < 4; ++k)
    for (uint32_t f = 0; f < 3; ++f)
      for (uint32_t cell = 0; cell <= kQuadMaxCell; ++cell)
        for (uint32_t value = 0; value <= kQuadMaxValue; ++value)
          for (int present = 0; present < 2; ++present) {
            const uint32_t slot = quad_slot(present != 0, cell, value);
            if (slot > 0xffu || (!present && slot != 0)) { printf("slot %u %u %d = %#x\n", cell, value, present, slot); return 1; }
            uint32_t word = 0;
            for (uint32_t i = 0; i < 4; ++i) word |= quad_word(i == k ? slot : fillers[f], i);
            for (uint32_t i = 0; i < 4; ++i) {
              const uint32_t got = quad_slot_of(word, i);
              if (got != (i == k ? slot : fillers[f])) { printf("position %u beside filler %u: %#x\n", i, f, got); return 1; }
            }
            const uint32_t got = quad_slot_of(word, k);
            if (quad_present(got) != (present != 0)) { printf("presence %u %u %d\n", cell, value, present); return 1; }
            if (present && (quad_cell(got) != cell || quad_value(got) != value)) { printf("content %u %u\n", cell, value); return 1; }
            ++checks;
          }
  // 2. the kernel's words
  for (int S = 1; S <= 8; ++S) {
    const uint32_t C = (uint32_t)(S * S);
    std::vector<uint32_t> cells;
    if (S <= 4) {
      for (uint32_t c = 0; c < C; ++c) cells.push_back(c);
    } else {
      for (uint32_t c : {0u, 1u, (uint32_t)S - 1u, (uint32_t)S, C / 2, C - (uint32_t)S, C - 2u, C - 1u}) cells.push_back(c);
    }
    for (int T = 1; T <= 2 && (uint32_t)T <= C; ++T)
      for (uint32_t mask = 0; mask < (1u << (2 * T)); ++mask)
        for (uint32_t values = 0; values < (1u << T); ++values)
          for (uint32_t e0 : cells)
            for (uint32_t l0 : cells)
              for (uint32_t e1 : (T == 2 ? cells : std::vector<uint32_t>{0u}))
                for (uint32_t l1 : (T == 2 ? cells : std::vector<uint32_t>{0u})) {
                  const Store s[4] = {{(mask & 1u) != 0, e0, 1u + (values & 1u)}, {(mask & 2u) != 0, l0, 0u},
                                      {(mask & 4u) != 0, e1, 1u + ((values >> 1) & 1u)}, {(mask & 8u) != 0, l1, 0u}};
                  const uint32_t word = pack(s, 2 * T);
                  if (const int rc = check_word(word, s, 2 * T)) {
                    printf("S %d T %d mask %#x values %#x cells %u %u %u %u: word %#x, check %d\n", S, T, mask, values, e0, l0, e1, l1, word, rc);
                    return 2;
                  }
                  ++checks;
                }
  }
  // 3. the four passes of a quad against the per-lane loop
  srand(7);
  for (int it = 0; it < 200000; ++it) {
    const int S = 1 + rand() % 8, T = 1 + rand() % 2;
    const uint32_t C = (uint32_t)(S * S);
    Store s[4][4];
    uint32_t word[4];
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> per_lane, quad;
    for (uint32_t lane = 0; lane < 4; ++lane) {
      const bool live = rand() % 8 != 0;  // a lane past the batch carries a word of zero
      for (int k = 0; k < 4; ++k) {
        s[lane][k] = {live && k < 2 * T && rand() % 2 != 0, (uint32_t)rand() % C, k % 2 ? 0u : 1u + (uint32_t)rand() % 2u};
        if (s[lane][k].present) per_lane.emplace_back(lane, s[lane][k].cell, s[lane][k].value);
      }
      word[lane] = pack(s[lane], 2 * T);
      if (!live && word[lane] != 0) { printf("a lane past the batch packs %#x\n", word[lane]); return 3; }
    }
    for (uint32_t j = 0; j < 4; ++j)      // pass j: every lane reads lane j's word ...
      for (uint32_t k = 0; k < 4; ++k) {  // ... and lane k takes slot k
        const uint32_t slot = quad_slot_of(word[j], k);
        if (quad_present(slot)) quad.emplace_back(j, quad_cell(slot), quad_value(slot));
      }
    std::sort(per_lane.begin(), per_lane.end());
    std::sort(quad.begin(), quad.end());
    if (per_lane != quad) { printf("quad %d: %zu stores per lane, %zu by passes\n", it, per_lane.size(), quad.size()); return 3; }
    ++checks;
  }
  printf("ok %lu checks\n", checks);
  return 0;
}
