// ts_table.hip — distance-to-win tables: solve each level once, look up every step (include/tiler_slider_table.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_table.so): the step library and the search library
// are pinned symbol by symbol and kernel by kernel, and nothing here touches either.
//
// The table of a board has one byte per index  idx = sum_t cell_t * C^t  (C = S * S) of the solver's index space: at most
// 65,536 bytes, kept in GLOBAL memory and written exactly once per entry.  What the build keeps in LDS is three bitmaps over
// that space (96 B at 4x4 / 2 tiles, 24 KiB at the cap - never near the 64 KiB a block gets without asking, so no launch
// here needs the large-LDS attribute):
//     closed   entries that are final: invalid, won, or resolved in an earlier round
//     prev     R(d - 1): the placements resolved last round
//     cur      R(d): the placements resolved this round (merged into closed and moved to prev between rounds)
// plus two control words (alternating "R(d) is not empty" flags).
//
// Slides cannot be undone, so there is no search from the goal.  Round d visits EVERY open placement - not a frontier -,
// slides it in the four directions (ts::slide_cell<S>, the arithmetic of the step kernels) and resolves it to d when some
// successor is in R(d - 1): all placements nearer than d are closed by then, so an open placement with a successor at d - 1
// is at exactly d.  Invalid placements are closed before round 0 and are nobody's successor.
//
// Two launch forms of the same body (table_body), as in ts_search.hip:
//   k_table_wave<S>   blocks of ONE wave (no s_barrier); a board is worked by G = 1 .. 64 lanes, 64 / G boards per wave
//   k_table_block<S>  one board per block of four waves
// and the lookup, k_table_lookup<S>: one board per lane, no LDS, five byte reads.
//
// The index space, the win test and the expert rule are the solver's and the rollouts' too (ts_index.h), and so is the host side
// of a launch (ts_launch.h); the measured policy of THIS library stays here.
#include "../../include/tiler_slider_table.h"
#include "ts_launch.h"

namespace {

using ts::kBlockThreads, ts::kMaxTiles, ts::kWave;  // kBlockThreads: k_table_block and k_table_lookup
// LDS of a board (ts::kMaxBlockLds bounds a block's): the largest request is one board of 65,536 states, 3 * 8 KiB + 8 B, so the
// default limit of a block is kept on purpose (bitmaps, not bytes, in LDS).
constexpr int kBitmaps = 3, kCtlWords = 2;
static_assert(TS_TABLE_FORM_NONE == ts::kFormNone && TS_TABLE_FORM_WAVE == ts::kFormWave && TS_TABLE_FORM_BLOCK == ts::kFormBlock);

namespace policy {
// Measured, MI355X, us per launch of ts_table_build on random levels, wave form (64 lanes per board) / block form
// (profiles/table_timing.log, tools/table_timing.py):
//     256 states (4x4 / 2 tiles, 1M boards)    2534 /  3266        4096 (4x4 / 3, 128k)    6641 /  5972
//     625        (5x5 / 2, 256k)               1562 /  1735        4096 (8x8 / 2, 128k)    7110 /  6390
//    1296        (6x6 / 2, 128k)               2594 /  2494        6561 (3x3 / 4, 128k)   13270 / 11772
//    2401        (7x7 / 2, 128k)               4671 /  4364       15625 (5x5 / 3, 256k)   44968 / 37156
//   46656        (6x6 / 3, 16k)               25058 / 10784       65536 (4x4 / 4, 8k)     45065 / 14940
// A round visits every open placement, so both forms do the same work; the wave form saves the barriers while a board is a few
// placements per lane, the block form ends a deep board four times sooner and keeps more boards resident once the bitmaps
// are kilobytes.  The forms cross between 625 and 1296 states: index spaces up to kWaveMaxStates take the wave form
// (ts_table_tuning(TS_TABLE_TUNE_WAVE_MAX_STATES)).
constexpr int64_t kWaveMaxStates = 1024;
// One wave per board fills the GPU only from tens of thousands of boards on, and tables are mostly built for a few hundred
// distinct levels.  Same log, wave / block, us:  256 states: 1024 boards 39.2 / 18.7, 4096 45.9 / 26.3, 16384 76.1 / 64.2,
// 32768 119.5 / 116.4, 65536 194.9 / 219.1;  625 states: 1024 103.1 / 43.0, 16384 220.1 / 154.1, 32768 308.5 / 254.1, 65536
// 472.8 / 458.3, 262144 1562 / 1735;  the 46 screenshot levels of 4x4 / 2 tiles 39.1 / 16.6.  Batches of fewer boards than
// this take the block form if the index space has a placement for each of its 256 threads
// (ts_table_tuning(TS_TABLE_TUNE_BLOCK_BELOW_BOARDS)); the 256-state tie at 32768 boards sets the value.
constexpr int64_t kBlockBelowBoards = 32768;
// Placements per lane and round of the wave form (ts_table_tuning(TS_TABLE_TUNE_STATES_PER_LANE)): lanes per board =
// pow2ceil(ceil(states / kStatesPerLane)), at most 64.  Same log, 4x4 / 2 tiles at 1M boards: 64 lanes per board 2534 us,
// 32 lanes 3190, 8 lanes 4685 - boards of one wave wait for its deepest one - so every board gets as many lanes as it has placements.
constexpr int64_t kStatesPerLane = 1;
}  // namespace policy

std::atomic<int64_t> g_wave_max_states{policy::kWaveMaxStates};
std::atomic<int64_t> g_states_per_lane{policy::kStatesPerLane};
std::atomic<int64_t> g_block_below_boards{policy::kBlockBelowBoards};

struct BArgs {
  const uint8_t *tgt;  // cell_t = uint8 (S <= 8)
  const uint32_t *blk;
  uint8_t *table;
  int64_t N;
  int32_t T, Tt, mc, max_depth;
  uint32_t states;
  uint32_t words;        // uint32 words per bitmap
  uint32_t board_words;  // LDS words per board: kBitmaps * words + kCtlWords
  uint32_t lanes_log2;   // k_table_wave: log2 of the lanes per board
};

template <int S, bool BLOCK>
__device__ __forceinline__ void table_body(const BArgs &a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr uint32_t C = BB::C;
  extern __shared__ uint32_t lds[];

  const auto [G, g, grp, n, nl, live] = ts::group_of<BLOCK>(threadIdx.x, blockIdx.x, a.lanes_log2, a.N);
  const int64_t N = a.N;
  const int T = a.T, Tt = a.Tt;
  const uint32_t W = a.words, states = a.states;

  uint32_t *base = lds + grp * a.board_words;
  uint32_t *closed = base, *prev = base + W, *cur = base + 2 * W, *ctl = base + kBitmaps * W;
  for (uint32_t i = g; i < a.board_words; i += G) base[i] = 0;

  // the level (cell ids clamped as the step kernels clamp them) and the solver's win test
  M blk = ts::load_obstacles<S>(a.blk, N, nl);
  const ts::WinTest<S> is_won = ts::load_win_test<S>(a.tgt, N, nl, T, Tt, a.mc != 0);
  uint8_t *row = a.table + nl * (int64_t)states;  // written only where `live`

  __syncthreads();
  // round 0: invalid placements and won ones; the bits of one word come from several lanes (ds_or)
  if (live) {
    for (uint32_t s = g; s < states; s += G) {
      uint32_t p[kMaxTiles];
      M occ;
      const bool valid = ts::decode_cells<S>(s, T, blk, p, occ);
      const bool won = valid && is_won(s, occ);
      const uint32_t w = s >> 5, bit = 1u << (s & 31);
      if (!valid || won) {
        atomicOr(&closed[w], bit);
        row[s] = valid ? (uint8_t)0 : (uint8_t)TS_TABLE_INVALID;
      }
      if (won) {
        atomicOr(&prev[w], bit);
        ctl[0] = 1u;
      }
    }
  }
  __syncthreads();

  // ctl[d & 1]: R(d) is not empty
  bool alive = live;
  uint32_t fill = TS_TABLE_NONE;
  int32_t d = 0;
  for (;;) {
    if (alive) {
      if (ctl[d & 1] == 0u) {
        alive = false;  // R(d) is empty: whatever is open stays out of reach
      } else if (d >= a.max_depth) {
        fill = TS_TABLE_DEEP;
        alive = false;
      }
    }
    if constexpr (BLOCK) {
      if (!alive) break;  // uniform: one board per block
    } else {
      if (__builtin_amdgcn_ballot_w64(alive) == 0) break;
    }
    ++d;
    if (alive) {
      for (uint32_t s = g; s < states; s += G) {
        const uint32_t w = s >> 5, bit = 1u << (s & 31);
        if (closed[w] & bit) continue;
        uint32_t p[kMaxTiles];
        M occ;
        ts::decode_cells<S>(s, T, blk, p, occ);  // a placement: every invalid one is closed
        bool hit = false;
#pragma unroll
        for (int dir = 0; dir < 4; ++dir) {
          uint32_t idx = 0, mul = 1;  // the successor index, in place (ts_index.h says why)
#pragma unroll
          for (int t = 0; t < kMaxTiles; ++t) {
            if (t < T) {
              idx += (uint32_t)ts::slide_cell<S>((int)p[t], occ, blk, dir) * mul;
              mul *= C;
            }
          }
          hit = hit || ((prev[idx >> 5] >> (idx & 31)) & 1u);  // idx == s (nothing slid) is open, so not in prev
        }
        if (hit) {
          atomicOr(&cur[w], bit);
          ctl[d & 1] = 1u;
          row[s] = (uint8_t)d;
        }
      }
    }
    __syncthreads();
    if (alive) {
      for (uint32_t w = g; w < W; w += G) {
        const uint32_t c = cur[w];
        if (c) closed[w] |= c;
        prev[w] = c;
        cur[w] = 0;
      }
      if (g == 0) ctl[(d + 1) & 1] = 0u;
    }
    __syncthreads();
  }
  if (live) {
    for (uint32_t s = g; s < states; s += G)
      if (!((closed[s >> 5] >> (s & 31)) & 1u)) row[s] = (uint8_t)fill;
  }
}

template <int S>
__global__ __launch_bounds__(kWave) void k_table_wave(const BArgs a) {
  table_body<S, false>(a);
}
template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_table_block(const BArgs a) {
  table_body<S, true>(a);
}

struct LArgs {
  const uint8_t *pos;
  const uint32_t *blk;
  const uint8_t *table;
  const int32_t *rows;  // may be NULL
  int16_t *moves;       // each output may be NULL
  uint8_t *best, *action;
  int64_t N, n_rows;
  int32_t T;
  uint32_t states;
};

template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_table_lookup(const LArgs a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr uint32_t C = BB::C;
  const int64_t n = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (n >= a.N) return;
  const int64_t N = a.N;
  const int T = a.T;
  const int64_t r = a.rows ? (int64_t)a.rows[n] : n;
  int32_t moves = TS_SOLVE_NONE;
  uint32_t best = 0;
  if (r >= 0 && r < a.n_rows) {
    const uint8_t *row = a.table + r * (int64_t)a.states;
    M blk = ts::load_obstacles<S>(a.blk, N, n);
    uint32_t p[kMaxTiles];
    M occ;
    const uint32_t d0 = row[ts::encode_cells<S>(a.pos, N, n, T, p, occ)];  // both indices read here stay inside the row
    if (d0 <= (uint32_t)TS_TABLE_MAX_DEPTH) {
      moves = (int32_t)d0;
      if (d0 >= 1u && (a.best || a.action)) {
        uint32_t d[4];
#pragma unroll
        for (int dir = 0; dir < 4; ++dir) {
          uint32_t idx = 0, mul = 1;  // the successor index, in place (ts_index.h says why)
#pragma unroll
          for (int t = 0; t < kMaxTiles; ++t) {
            if (t < T) {
              idx += (uint32_t)ts::slide_cell<S>((int)p[t], occ, blk, dir) * mul;  // a cell < C whatever the board: inside the row
              mul *= C;
            }
          }
          d[dir] = row[idx];
        }
        best = ts::best_moves(d0, d);
      }
    } else if (d0 == (uint32_t)TS_TABLE_DEEP) {
      moves = TS_SOLVE_DEPTH;
    }
  }
  if (a.moves) a.moves[n] = (int16_t)moves;
  if (a.best) a.best[n] = (uint8_t)best;
  if (a.action) a.action[n] = (uint8_t)ts::lowest_move(best);
}

using BuildKernel = void (*)(const BArgs);
using LookupKernel = void (*)(const LArgs);

BuildKernel wave_kernel(int S) {
  return ts::by_size<BuildKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> BuildKernel { return k_table_wave<s>; });
}
// the block form is compiled where an index space of at least kBlockThreads placements exists: every size but 1x1
BuildKernel block_kernel(int S) {
  return ts::by_size<BuildKernel, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> BuildKernel { return k_table_block<s>; });
}
LookupKernel lookup_kernel(int S) {
  return ts::by_size<LookupKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> LookupKernel { return k_table_lookup<s>; });
}

struct BuildPlan {
  ts::FormPlan<BuildKernel> f;
  BArgs a{};
  ts_table_desc desc{};
};

// Everything ts_table_build decides before it launches; touches no device (ts_describe_table_build reports it).
int32_t plan_build(const ts_dims *d, BuildPlan &p) {
  // a block per board for large index spaces, and for batches too small to fill the GPU with one wave per board - where the
  // block has a placement for every thread
  const auto choose = [&](int64_t states, uint32_t) -> ts::FormChoice<BuildKernel> {
    const bool large = states > g_wave_max_states.load(std::memory_order_relaxed);
    const bool few = states >= kBlockThreads && d->n_boards < g_block_below_boards.load(std::memory_order_relaxed);
    const int64_t spl = std::max<int64_t>(g_states_per_lane.load(std::memory_order_relaxed), 1);
    return {large || few ? block_kernel(d->size) : nullptr, wave_kernel(d->size), (states + spl - 1) / spl};
  };
  if (const int32_t rc = ts::plan_forms(d, kBitmaps, kCtlWords, "k_table", choose, p.f); rc != TS_OK) return rc;
  BArgs &a = p.a;
  a.N = d->n_boards, a.T = d->n_tiles, a.Tt = d->n_targets, a.mc = d->multi_color;
  a.states = (uint32_t)p.f.states, a.words = p.f.words, a.board_words = p.f.board_words, a.lanes_log2 = p.f.lanes_log2;
  ts::describe_forms(p.f, p.desc);
  p.desc.lds_bytes_max = (int32_t)ts::kMaxBlockLds;
  p.desc.table_bytes = d->n_boards * p.f.states;
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_table_abi_version(void) { return TS_TABLE_ABI_VERSION; }
int32_t ts_table_last_hip_error(void) { return ts::t_last_hip_error; }

int64_t ts_table_states(const ts_dims *dims) { return ts::checked_states(dims); }

int32_t ts_describe_table_build(const ts_dims *dims, ts_table_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  BuildPlan p;
  const int32_t rc = plan_build(dims, p);
  if (rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_table_build(const ts_dims *dims, const ts_state *st, int32_t max_depth, uint8_t *table, void *stream) {
  if (!dims) return TS_ERR_NULL;
  BuildPlan p;
  if (const int32_t rc = plan_build(dims, p); rc != TS_OK) return rc;
  if (max_depth < 0 || max_depth > TS_TABLE_MAX_DEPTH) return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !table || !st->blk || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  p.a.tgt = static_cast<const uint8_t *>(st->tgt), p.a.blk = st->blk;
  p.a.table = table, p.a.max_depth = max_depth;
  hipLaunchKernelGGL(p.f.kernel, dim3(p.f.blocks), dim3(p.f.threads), p.f.lds, static_cast<hipStream_t>(stream), p.a);
  return ts::finish_launch();
}

int32_t ts_table_lookup(const ts_dims *dims, const ts_state *st, const uint8_t *table, int64_t n_rows, const int32_t *rows,
                        int16_t *moves, uint8_t *best, uint8_t *action, void *stream) {
  if (!dims) return TS_ERR_NULL;
  const int64_t states = ts::checked_states(dims);
  if (states < 0) return (int32_t)states;
  if (states == 0) return TS_ERR_LIMIT;
  if (n_rows < 0) return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !st->blk || (dims->n_tiles > 0 && !st->pos) || (n_rows > 0 && !table) || (!moves && !best && !action)) return TS_ERR_NULL;
  const int64_t blocks = (dims->n_boards + kBlockThreads - 1) / kBlockThreads;
  LookupKernel k = lookup_kernel(dims->size);
  if (!k || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  LArgs a{};
  a.pos = static_cast<const uint8_t *>(st->pos), a.blk = st->blk, a.table = table, a.rows = rows;
  a.moves = moves, a.best = best, a.action = action;
  a.N = dims->n_boards, a.n_rows = n_rows, a.T = dims->n_tiles, a.states = (uint32_t)states;
  hipLaunchKernelGGL(k, dim3((uint32_t)blocks), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int64_t ts_table_tuning(int32_t key, int64_t value) {
  std::atomic<int64_t> *knob = key == TS_TABLE_TUNE_WAVE_MAX_STATES      ? &g_wave_max_states
                               : key == TS_TABLE_TUNE_STATES_PER_LANE    ? &g_states_per_lane
                               : key == TS_TABLE_TUNE_BLOCK_BELOW_BOARDS ? &g_block_below_boards
                                                                         : nullptr;
  return ts::tune(knob, value);
}

}  // extern "C"
