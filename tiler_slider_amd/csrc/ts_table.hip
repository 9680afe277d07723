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
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>

#include "../../include/tiler_slider_table.h"
#include "ts_core.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlockThreads = 256;  // k_table_block and k_table_lookup: four waves
constexpr int kMaxTiles = 5;        // C^T <= 65536 with T <= C: 9^5 = 59,049 is the longest tuple (3x3)
constexpr int kBitmaps = 3, kCtlWords = 2;
// Dynamic LDS a block may ask for.  The largest request here is one board of 65,536 states: 3 * 8 KiB + 8 B, so the
// default limit of a block is kept on purpose (bitmaps, not bytes, in LDS) and hipFuncSetAttribute is never needed.
constexpr size_t kMaxBlockLds = 64 * 1024;

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

thread_local int32_t t_last_hip_error = 0;
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

  const uint32_t G = BLOCK ? (uint32_t)kBlockThreads : (1u << a.lanes_log2);  // threads per board
  const uint32_t g = threadIdx.x & (G - 1u);
  const uint32_t grp = BLOCK ? 0u : threadIdx.x >> a.lanes_log2;
  const int64_t n = BLOCK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (int64_t)(kWave >> a.lanes_log2) + grp;
  const bool live = n < a.N;
  const int64_t nl = live ? n : a.N - 1;  // idle groups read the last board (N >= 1) and write nothing
  const int64_t N = a.N;
  const int T = a.T, Tt = a.Tt;
  const uint32_t W = a.words, states = a.states;

  uint32_t *base = lds + grp * a.board_words;
  uint32_t *closed = base, *prev = base + W, *cur = base + 2 * W, *ctl = base + kBitmaps * W;
  for (uint32_t i = g; i < a.board_words; i += G) base[i] = 0;

  // the level (cell ids clamped as the step kernels clamp them)
  M blk = (M)a.blk[nl];
  if constexpr (BB::wide) blk |= (M)a.blk[N + nl] << 32;
  // win test (state.py:172-186), the two comparisons of the solver: multi-colour: the state IS the targets' index (and
  // T == Tt); single colour: the set of tile cells equals the set of target cells
  M tgm = 0;
  uint32_t tgt_idx = 0;
  {
    uint32_t mul = 1;
    for (int j = 0; j < Tt; ++j) {
      const uint32_t tj = min((uint32_t)a.tgt[(int64_t)j * N + nl], C - 1u);
      tgm |= M(1) << tj;
      if (j < T) {
        tgt_idx += tj * mul;
        mul *= C;
      }
    }
  }
  const bool mc = a.mc != 0, mc_can_win = T == Tt;
  uint8_t *row = a.table + nl * (int64_t)states;  // written only where `live`

  auto decode = [&](uint32_t s, uint32_t (&p)[kMaxTiles], M &occ, bool &valid) {
    uint32_t r = s;
    occ = 0;
    valid = true;
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t) {
      p[t] = 0;
      if (t < T) {
        p[t] = r % C;
        r /= C;
        const M bit = M(1) << p[t];
        valid = valid && !((occ | blk) & bit);
        occ |= bit;
      }
    }
  };

  __syncthreads();
  // round 0: invalid placements and won ones; the bits of one word come from several lanes (ds_or)
  if (live) {
    for (uint32_t s = g; s < states; s += G) {
      uint32_t p[kMaxTiles];
      M occ;
      bool valid;
      decode(s, p, occ, valid);
      const bool won = valid && (mc ? (mc_can_win && s == tgt_idx) : occ == tgm);
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
        bool valid;
        decode(s, p, occ, valid);  // valid: every invalid placement is closed
        bool hit = false;
#pragma unroll
        for (int dir = 0; dir < 4; ++dir) {
          uint32_t idx = 0, mul = 1;
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
    M blk = (M)a.blk[n];
    if constexpr (BB::wide) blk |= (M)a.blk[N + n] << 32;
    uint32_t p[kMaxTiles], idx0 = 0;
    M occ = 0;
    {
      uint32_t mul = 1;
#pragma unroll
      for (int t = 0; t < kMaxTiles; ++t) {
        p[t] = 0;
        if (t < T) {
          p[t] = min((uint32_t)a.pos[(int64_t)t * N + n], C - 1u);  // idx0 <= C^T - 1: inside the row
          idx0 += p[t] * mul;
          mul *= C;
          occ |= M(1) << p[t];
        }
      }
    }
    const uint32_t d0 = row[idx0];
    if (d0 <= (uint32_t)TS_TABLE_MAX_DEPTH) {
      moves = (int32_t)d0;
      if (d0 >= 1u && (a.best || a.action)) {
#pragma unroll
        for (int dir = 0; dir < 4; ++dir) {
          uint32_t idx = 0, mul = 1;
#pragma unroll
          for (int t = 0; t < kMaxTiles; ++t) {
            if (t < T) {
              idx += (uint32_t)ts::slide_cell<S>((int)p[t], occ, blk, dir) * mul;  // a cell < C whatever the board: inside the row
              mul *= C;
            }
          }
          best |= ((uint32_t)row[idx] == d0 - 1u ? 1u : 0u) << dir;
        }
      }
    } else if (d0 == (uint32_t)TS_TABLE_DEEP) {
      moves = TS_SOLVE_DEPTH;
    }
  }
  if (a.moves) a.moves[n] = (int16_t)moves;
  if (a.best) a.best[n] = (uint8_t)best;
  if (a.action) a.action[n] = best ? (uint8_t)ts::lsb(best) : (uint8_t)255;
}

using BuildKernel = void (*)(const BArgs);
using LookupKernel = void (*)(const LArgs);

template <class K, int... Vs, class F>
K by_size(int v, F f) {
  K k = nullptr;
  (void)((v == Vs && (k = f(std::integral_constant<int, Vs>{}), true)) || ...);
  return k;
}
BuildKernel wave_kernel(int S) {
  return by_size<BuildKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> BuildKernel { return k_table_wave<s>; });
}
// the block form is compiled where an index space of at least kBlockThreads placements exists: every size but 1x1
BuildKernel block_kernel(int S) {
  return by_size<BuildKernel, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> BuildKernel { return k_table_block<s>; });
}
LookupKernel lookup_kernel(int S) {
  return by_size<LookupKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> LookupKernel { return k_table_lookup<s>; });
}

int32_t check_dims(const ts_dims *d) {
  if (!d) return TS_ERR_NULL;
  if (d->n_boards < 0 || d->size < 1 || d->n_tiles < 0 || d->n_targets < 0 || (d->multi_color != 0 && d->multi_color != 1)) return TS_ERR_DIMS;
  if (d->size > TS_MAX_SIZE || d->n_tiles > TS_MAX_TILES || d->n_targets > TS_MAX_TILES) return TS_ERR_LIMIT;
  if (d->n_tiles > d->size * d->size) return TS_ERR_DIMS;
  return TS_OK;
}

int64_t table_states(const ts_dims *d) {
  if (const int32_t rc = check_dims(d); rc != TS_OK) return rc;
  if (d->size > TS_SOLVE_MAX_SIZE) return 0;
  const int64_t C = (int64_t)d->size * d->size;
  int64_t states = 1;
  for (int t = 0; t < d->n_tiles; ++t) {
    states *= C;
    if (states > TS_SOLVE_MAX_STATES) return 0;
  }
  return states;
}

struct BuildPlan {
  BuildKernel kernel = nullptr;
  BArgs a{};
  uint32_t blocks = 0, threads = 0;
  size_t lds = 0;
  ts_table_desc desc{};
};

// Everything ts_table_build decides before it launches; touches no device (ts_describe_table_build reports it).
int32_t plan_build(const ts_dims *d, BuildPlan &p) {
  const int64_t states = table_states(d);
  if (states < 0) return (int32_t)states;
  if (states == 0) return TS_ERR_LIMIT;
  const int S = d->size;
  BArgs &a = p.a;
  a.N = d->n_boards, a.T = d->n_tiles, a.Tt = d->n_targets, a.mc = d->multi_color;
  a.states = (uint32_t)states;
  a.words = (uint32_t)((states + 31) / 32);
  a.board_words = kBitmaps * a.words + kCtlWords;
  p.desc.states = states;
  p.desc.bitmap_words = (int32_t)a.words;
  p.desc.lds_bytes_board = (int32_t)(a.board_words * 4u);
  p.desc.lds_bytes_max = (int32_t)kMaxBlockLds;
  p.desc.table_bytes = d->n_boards * states;
  if (d->n_boards == 0) return TS_OK;  // TS_TABLE_FORM_NONE
  // a block per board for large index spaces, and for batches too small to fill the GPU with one wave per board - where the
  // block has a placement for every thread
  const bool large = states > g_wave_max_states.load(std::memory_order_relaxed);
  const bool few = states >= kBlockThreads && d->n_boards < g_block_below_boards.load(std::memory_order_relaxed);
  BuildKernel blockk = large || few ? block_kernel(S) : nullptr;
  int64_t blocks;
  if (blockk) {
    p.kernel = blockk;
    p.threads = kBlockThreads;
    p.desc.form = TS_TABLE_FORM_BLOCK, p.desc.lanes_per_board = kBlockThreads, p.desc.boards_per_block = 1;
    blocks = d->n_boards;
    snprintf(p.desc.name, sizeof p.desc.name, "k_table_block<%d>", S);
  } else {
    p.kernel = wave_kernel(S);
    int64_t spl = g_states_per_lane.load(std::memory_order_relaxed);
    if (spl < 1) spl = 1;
    const int64_t want = (states + spl - 1) / spl;
    while ((1 << a.lanes_log2) < kWave && (1 << a.lanes_log2) < want) ++a.lanes_log2;
    const int lanes = 1 << a.lanes_log2, bpb = kWave / lanes;
    p.threads = kWave;
    p.desc.form = TS_TABLE_FORM_WAVE, p.desc.lanes_per_board = lanes, p.desc.boards_per_block = bpb;
    blocks = (d->n_boards + bpb - 1) / bpb;
    snprintf(p.desc.name, sizeof p.desc.name, "k_table_wave<%d>", S);
  }
  p.lds = (size_t)p.desc.boards_per_block * a.board_words * 4u;
  if (!p.kernel || p.lds > kMaxBlockLds || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  p.desc.threads_per_block = (int32_t)p.threads;
  p.desc.lds_bytes_block = (int32_t)p.lds;
  p.desc.blocks = blocks;
  return TS_OK;
}

int32_t finish_launch() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    t_last_hip_error = (int32_t)e;
    return TS_ERR_HIP;
  }
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_table_abi_version(void) { return TS_TABLE_ABI_VERSION; }
int32_t ts_table_last_hip_error(void) { return t_last_hip_error; }

int64_t ts_table_states(const ts_dims *dims) { return table_states(dims); }

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
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), p.a);
  return finish_launch();
}

int32_t ts_table_lookup(const ts_dims *dims, const ts_state *st, const uint8_t *table, int64_t n_rows, const int32_t *rows,
                        int16_t *moves, uint8_t *best, uint8_t *action, void *stream) {
  if (!dims) return TS_ERR_NULL;
  const int64_t states = table_states(dims);
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
  return finish_launch();
}

int64_t ts_table_tuning(int32_t key, int64_t value) {
  std::atomic<int64_t> *knob = key == TS_TABLE_TUNE_WAVE_MAX_STATES      ? &g_wave_max_states
                               : key == TS_TABLE_TUNE_STATES_PER_LANE    ? &g_states_per_lane
                               : key == TS_TABLE_TUNE_BLOCK_BELOW_BOARDS ? &g_block_below_boards
                                                                         : nullptr;
  if (!knob) return -1;
  return value >= 0 ? knob->exchange(value, std::memory_order_relaxed) : knob->load(std::memory_order_relaxed);
}

}  // extern "C"
