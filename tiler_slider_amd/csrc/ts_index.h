// ts_index.h — the index space shared by the solver, the distance tables and the table policy of the rollouts.
//
// A board of T tiles on S x S cells is the state  idx = sum_t cell_t * C^t  (C = S * S): one index per placement of the tiles
// IN ORDER.  What belongs to that space and to nothing else is written here once: the obstacle load, the win test on an index,
// a placement to and from its index, how the threads of a block are dealt over boards, and the expert rule over a board's table
// entry and those of its four successors.  ts_search.hip, ts_table.hip and ts_rollout.hip compile these into their own kernels
// (TS_HD, always inlined: nothing here becomes a symbol).
#pragma once
#include "ts_core.h"

namespace ts {

constexpr int kWave = 64;
constexpr int kBlockThreads = 256;  // the block form of a search or a table build, and a lookup block: four waves
constexpr int kMaxTiles = 5;        // C^T <= 65536 with T <= C: 9^5 = 59,049 is the longest tuple (3x3)

template <int S>
using mask_of = typename Bitboard<S>::mask_t;

// C^t as a constant, for loops that are fully unrolled
template <int C>
constexpr uint32_t pow_c(int t) {
  uint32_t m = 1;
  for (int i = 0; i < t; ++i) m *= (uint32_t)C;
  return m;
}

TS_HD uint32_t clamp_cell(uint32_t cell, uint32_t C) { return min(cell, C - 1u); }  // as the step kernels clamp

// the obstacle bitboard of board n (word-major: word w of board n at blk[w * N + n])
template <int S>
TS_HD mask_of<S> load_obstacles(const uint32_t *blk, int64_t N, int64_t n) {
  using M = mask_of<S>;
  M m = (M)blk[n];
  if constexpr (Bitboard<S>::wide) m |= (M)blk[N + n] << 32;
  return m;
}

// Win test (state.py:172-186) on a placement's index and occupancy.  Multi-colour: tile i on target i for every i and
// T == Tt <=> the state IS the targets' index; single colour: the set of tile cells equals the set of target cells.
template <int S>
struct WinTest {
  mask_of<S> tgm = 0;     // the set of target cells
  uint32_t tgt_idx = 0;   // the targets of the first T tiles as an index
  bool mc = false, mc_can_win = false;
  TS_HD bool operator()(uint32_t idx, mask_of<S> occ) const { return mc ? (mc_can_win && idx == tgt_idx) : occ == tgm; }
};
template <int S>
TS_HD WinTest<S> load_win_test(const uint8_t *tgt, int64_t N, int64_t n, int T, int Tt, bool mc) {
  using M = mask_of<S>;
  constexpr uint32_t C = Bitboard<S>::C;
  WinTest<S> w;
  uint32_t mul = 1;
  for (int j = 0; j < Tt; ++j) {
    const uint32_t tj = clamp_cell(tgt[(int64_t)j * N + n], C);
    w.tgm |= M(1) << tj;
    if (j < T) {
      w.tgt_idx += tj * mul;
      mul *= C;
    }
  }
  w.mc = mc, w.mc_can_win = T == Tt;
  return w;
}

// the index of the cells of board n as they lie in memory (clamped: the index stays inside C^T), with the cells and their occupancy
template <int S>
TS_HD uint32_t encode_cells(const uint8_t *pos, int64_t N, int64_t n, int T, uint32_t (&p)[kMaxTiles], mask_of<S> &occ) {
  constexpr uint32_t C = Bitboard<S>::C;
  uint32_t idx = 0, mul = 1;
  occ = 0;
#pragma unroll
  for (int t = 0; t < kMaxTiles; ++t) {
    p[t] = 0;
    if (t < T) {
      p[t] = clamp_cell(pos[(int64_t)t * N + n], C);
      idx += p[t] * mul;
      mul *= C;
      occ |= mask_of<S>(1) << p[t];
    }
  }
  return idx;
}

// the cells and the occupancy of index s; false where s is no placement (two tiles on a cell, or a tile on an obstacle)
template <int S>
TS_HD bool decode_cells(uint32_t s, int T, mask_of<S> blk, uint32_t (&p)[kMaxTiles], mask_of<S> &occ) {
  using M = mask_of<S>;
  constexpr uint32_t C = Bitboard<S>::C;
  bool valid = true;
  occ = 0;
#pragma unroll
  for (int t = 0; t < kMaxTiles; ++t) {
    p[t] = 0;
    if (t < T) {
      p[t] = s % C;
      s /= C;
      const M bit = M(1) << p[t];
      valid = valid && !((occ | blk) & bit);
      occ |= bit;
    }
  }
  return valid;
}

// The index of the board one slide on, sum_t slide_cell(p_t) * C^t, is NOT a function here: as one (by reference, by value, per
// direction or all four at once) it cost the wave-form kernels a wave per SIMD (profiles/shared_core_codegen.md), so the loop
// stays written out in the five places that need it.

// How the threads of a block are dealt over boards.  Block form: the whole block works board blockIdx.x.  Wave form: a block
// is ONE wave, cut into 64 >> lanes_log2 groups of 1 << lanes_log2 lanes, a board per group.
struct Group {
  uint32_t G, g, grp;  // threads per board, this thread among them, the group among the block's
  int64_t n, nl;       // the board, and the board to read: idle groups read the last board (N >= 1) and write nothing
  bool live;
};
template <bool BLOCK>
TS_HD Group group_of(uint32_t thread, uint32_t block, uint32_t lanes_log2, int64_t N) {
  Group r;
  r.G = BLOCK ? (uint32_t)kBlockThreads : (1u << lanes_log2);
  r.g = thread & (r.G - 1u);
  r.grp = BLOCK ? 0u : thread >> lanes_log2;
  r.n = BLOCK ? (int64_t)block : (int64_t)block * (int64_t)(kWave >> lanes_log2) + r.grp;
  r.live = r.n < N;
  r.nl = r.live ? r.n : N - 1;
  return r;
}

// The expert rule.  d0: the table entry of a board, a distance >= 1; d[dir]: the entries of its four successors.  Bit dir is
// set where Move dir starts a shortest solution; the expert plays the lowest such move, 255 where there is none.
TS_HD uint32_t best_moves(uint32_t d0, const uint32_t (&d)[4]) {
  uint32_t best = 0;
#pragma unroll
  for (int dir = 0; dir < 4; ++dir) best |= (d[dir] == d0 - 1u ? 1u : 0u) << dir;
  return best;
}
TS_HD uint32_t lowest_move(uint32_t best) { return best ? (uint32_t)lsb(best) : 255u; }

}  // namespace ts
