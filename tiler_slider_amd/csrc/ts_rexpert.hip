// ts_rexpert.hip — the reach-table experts: K steps of the epsilon-greedy expert of a reachable distance table in one launch, and
// that table's answer on every board a logged rollout visited (include/tiler_slider_rexpert.h, which defines both).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_rexpert.so): ts_rtable.hip, ts_rollout.hip and
// ts_targets.hip are not touched and no existing code object is rebuilt.  It shares ts_core.h (the slide arithmetic) and
// ts_launch.h (dims check, error tail) with the other libraries and RESTATES the probe from the table format that
// tiler_slider_rtable.h fixes: a slot is 0 or  bit 63 | entry << 48 | key,  linear probing from
// home(key) = (uint32)((key * 0x9e3779b97f4a7c15) >> 32) >> (32 - log2(slots)).
//
// k_rexpert_rollout<S> has the shape of k_rollout<S, TABLE>: ONE BOARD PER LANE, the level and the dynamic state in registers
// for all K steps, no LDS, no scratch, no barrier, a wave-uniform step loop, the same strict-mode early exit with its tail that
// still writes the logs.  Keys are ts_rtable's ordered 48-bit keys, built by 64-bit multiply-add; the multi-colour win test is
// on the key, the single-colour one on the occupancy mask.
//
// Latency.  What a step costs is its dependent memory round trips (ts_rollout.hip's header).  The board is slid in all four
// directions - one of them is the step about to be played -, the five keys are formed, and the five HOME-SLOT loads are issued
// together and unconditionally (a won successor's is issued too and its result dropped: the address lies inside the row).
// Tables are at most half full, so most probes end there: a hit, or an empty slot.  Only then the probes that did neither walk
// on, all that are still open together, one more slot each per round.  A probe reads at most `slots` slots, each index masked
// into the row: a row of arbitrary bytes ends, and nothing outside it is read.
//
// k_rexpert_labels<S>: ONE SAMPLE PER LANE, block (x, k) the boards 256 x .. of step k - the header says why.  The same lookup.
#include "ts_launch.h"  // the HIP runtime first: ts_core.h's TS_HD needs it

#include "ts_core.h"

#include "../../include/tiler_slider_rexpert.h"

namespace {

using ts::kWave;
constexpr int kThreads = 256;  // four waves per block; waves never interact
constexpr int kMaxTargets = TS_ROLLOUT_MAX_TILES;

constexpr uint64_t kOcc = 1ull << 63, kKeyMask = (1ull << 48) - 1;
constexpr int kEntryShift = 48;
constexpr uint32_t kNoEntry = 0x100u;  // a probe's answer where the row does not hold the key (an entry is a byte)

__device__ __forceinline__ uint32_t home_of(uint64_t key, uint32_t slots_log2) {
  return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 32) >> (32u - slots_log2);
}

// C^t as a 64-bit constant, for loops that are fully unrolled (t <= 7, C <= 64: below 2^42)
template <int C>
constexpr uint64_t pow64(int t) {
  uint64_t m = 1;
  for (int i = 0; i < t; ++i) m *= (uint64_t)C;
  return m;
}

// tiles a lane keeps: 8, fewer where the board has fewer cells
template <int S>
constexpr int max_tiles() {
  return S * S < TS_ROLLOUT_MAX_TILES ? S * S : TS_ROLLOUT_MAX_TILES;
}

// What the lookup needs of a level beside the obstacles: the win test of ts_rtable (multi-colour: the state IS the targets' key
// and T == Tt; single colour: the sets of cells).
template <int S>
struct WinTest {
  using M = typename ts::Bitboard<S>::mask_t;
  M tgm = 0;
  uint64_t tgt_key = 0;
  bool mc = false, mc_can_win = false;
  __device__ __forceinline__ bool operator()(uint64_t key, M occ) const { return mc ? (mc_can_win && key == tgt_key) : occ == tgm; }
};

// the table as a kernel sees it
struct Table {
  const uint64_t *table;
  const int32_t *count;
  const int32_t *rows;  // may be NULL
  int64_t n_rows;
  uint32_t slots, slots_log2;
};

// a board's row: ts_rtable_lookup's first and third rule
enum : uint32_t { kRowOutside = 0, kRowFull = 1, kRowUsable = 2 };
struct Row {
  const uint64_t *at = nullptr;
  uint32_t kind = kRowOutside;
};
__device__ __forceinline__ Row row_of(const Table &tb, int64_t n) {
  Row row;
  const int64_t r = tb.rows ? (int64_t)tb.rows[n] : n;
  if (r >= 0 && r < tb.n_rows) {  // outside: nothing of table or count is read
    row.kind = tb.count[r] == TS_REACH_FULL ? kRowFull : kRowUsable;
    row.at = tb.table + (uint64_t)r * tb.slots;
  }
  return row;
}

// One board's five probes.  in: key[0] the board's key, key[1 + dir] its successors'; skip bit i: probe i is not wanted (a won
// placement is not stored).  out: ent[i] the entry of key[i], kNoEntry where the row does not hold it or the probe was skipped.
// The five home-slot loads go out together, skipped ones included; then every probe that met neither its key nor an empty slot
// walks on, the open ones together.  Each probe reads at most `slots` slots, every index masked: all inside the row.
__device__ __forceinline__ void probe5(const uint64_t *row, uint32_t slots, uint32_t slots_log2, const uint64_t (&key)[5], uint32_t skip,
                                       uint32_t (&ent)[5]) {
  const uint32_t mask = slots - 1u;
  uint32_t slot[5], open = 0;
  uint64_t e[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) slot[i] = home_of(key[i], slots_log2) & mask;
#pragma unroll
  for (int i = 0; i < 5; ++i) e[i] = row[slot[i]];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const bool hit = (e[i] & kOcc) && (e[i] & kKeyMask) == key[i];
    ent[i] = hit ? (uint32_t)(e[i] >> kEntryShift) & 0xffu : kNoEntry;
    open |= (!hit && e[i] != 0 && !((skip >> i) & 1u)) ? 1u << i : 0u;
  }
  for (uint32_t probe = 1; open != 0 && probe < slots; ++probe) {  // per lane: rare in a table at most half full
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      if ((open >> i) & 1u) {
        slot[i] = (slot[i] + 1u) & mask;
        e[i] = row[slot[i]];
      }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      if ((open >> i) & 1u) {
        const bool hit = (e[i] & kOcc) && (e[i] & kKeyMask) == key[i];
        if (hit) ent[i] = (uint32_t)(e[i] >> kEntryShift) & 0xffu;
        if (hit || e[i] == 0) open &= ~(1u << i);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i)
    if ((skip >> i) & 1u) ent[i] = kNoEntry;
}

// ts_rtable_lookup's (moves, best) of a board inside the table (its row is not kRowOutside) from what probe5 found; won[0]: the
// board is won, won[1 + dir]: its successor is.
__device__ __forceinline__ void answer_of(uint32_t row_kind, const bool (&won)[5], const uint32_t (&ent)[5], int32_t &moves, uint32_t &best) {
  best = 0;
  if (won[0]) {
    moves = 0;
  } else if (row_kind == kRowFull) {
    moves = TS_REACH_FULL;
  } else if (ent[0] == kNoEntry) {
    moves = TS_RTABLE_ABSENT;
  } else if (ent[0] >= 1u && ent[0] <= (uint32_t)TS_TABLE_MAX_DEPTH) {
    moves = (int32_t)ent[0];
#pragma unroll
    for (int dir = 0; dir < 4; ++dir) {
      // a won successor is 0 from the win; an entry 0 is never stored and is no distance
      const uint32_t d = won[1 + dir] ? 0u : (ent[1 + dir] == kNoEntry || ent[1 + dir] == 0u) ? (uint32_t)TS_TABLE_NONE : ent[1 + dir];
      best |= (d == ent[0] - 1u ? 1u : 0u) << dir;
    }
  } else {
    moves = ent[0] == (uint32_t)TS_TABLE_DEEP ? TS_SOLVE_DEPTH : TS_SOLVE_NONE;
  }
}

// The board with the clamped cells pc slid in all four directions: the successors' cells, keys and win tests beside its own,
// then the lookup.  Returns (moves, best); `successors` false: only the board's own entry is wanted (moves alone).  A
// successor's cells are packed a byte each (cell t in bits 8 t .. 8 t + 7): four times eight registers would cost a wave a SIMD.
template <int S, int MT>
struct Looked {
  uint64_t q4[4];
  uint64_t key[5];
  bool won[5];
  int32_t moves;
  uint32_t best;
};
template <int S, int MT>
__device__ __forceinline__ void look(const uint32_t (&pc)[MT], int T, typename ts::Bitboard<S>::mask_t blk, const WinTest<S> &win, const Row &row,
                                     uint32_t slots, uint32_t slots_log2, bool successors, Looked<S, MT> &o) {
  using M = typename ts::Bitboard<S>::mask_t;
  constexpr int C = S * S;
  M occ = 0;
  o.key[0] = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t)
    if (t < T) occ |= M(1) << pc[t], o.key[0] += (uint64_t)pc[t] * pow64<C>(t);
  o.won[0] = win(o.key[0], occ);
#pragma unroll
  for (int dir = 0; dir < 4; ++dir) {
    M occ2 = 0;
    o.key[1 + dir] = 0, o.q4[dir] = 0;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      if (t < T) {
        const uint32_t q = (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir);  // a cell < C whatever the board
        o.key[1 + dir] += (uint64_t)q * pow64<C>(t);
        o.q4[dir] |= (uint64_t)q << (8 * t);
        occ2 |= M(1) << q;
      }
    }
    o.won[1 + dir] = win(o.key[1 + dir], occ2);
  }
  uint32_t ent[5] = {kNoEntry, kNoEntry, kNoEntry, kNoEntry, kNoEntry};
  if (row.kind == kRowUsable && !o.won[0]) {
    uint32_t skip = successors ? 0u : 0x1eu;
#pragma unroll
    for (int dir = 0; dir < 4; ++dir) skip |= o.won[1 + dir] ? 2u << dir : 0u;
    probe5(row.at, slots, slots_log2, o.key, skip, ent);
  }
  o.moves = TS_SOLVE_NONE, o.best = 0;  // a row outside the table
  if (row.kind != kRowOutside) answer_of(row.kind, o.won, ent, o.moves, o.best);
}

struct RArgs {
  uint8_t *pos;  // cell_t = uint8 (S <= 8)
  const uint8_t *init, *tgt;
  const uint32_t *blk;
  int32_t *step_count;
  uint8_t *done;
  Table tb;
  int32_t *wins, *finished, *first_win, *win_moves, *reward_sum;  // each output may be NULL
  uint8_t *flags, *act_log, *flags_log, *pos_log;
  int64_t N, step_index, board_offset;
  uint64_t seed, threshold;
  int32_t T, Tt, mc, max_steps, steps, autoreset, write_state;
};

template <int S>
__global__ __launch_bounds__(kThreads) void k_rexpert_rollout(const RArgs a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr int C = BB::C;
  constexpr int MT = max_tiles<S>();
  constexpr M kFull = C == 64 ? ~M(0) : (M(1) << (C & 63)) - 1;

  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  // lanes past the batch play a copy of the LAST board and write nothing
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  const int T = a.T, Tt = a.Tt, K = a.steps;
  const bool mc = a.mc != 0, autoreset = a.autoreset != 0;

  // ---- the board, once: every load before the first one is consumed (rows past the tile or target count read the last row)
  M blk = ts::load_obstacles<S>(a.blk, N, nl);
  blk &= kFull;
  uint32_t p0[MT], in0[MT], tg[kMaxTargets];
#pragma unroll
  for (int t = 0; t < MT; ++t) p0[t] = 0, in0[t] = 0;
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) tg[j] = 0;
  if (T > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) p0[t] = a.pos[(int64_t)min(t, T - 1) * N + nl];
    if (autoreset) {
#pragma unroll
      for (int t = 0; t < MT; ++t) in0[t] = a.init[(int64_t)min(t, T - 1) * N + nl];
    }
  }
  if (Tt > 0) {
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j) tg[j] = a.tgt[(int64_t)min(j, Tt - 1) * N + nl];
  }
  int32_t sc = a.step_count[nl];
  uint32_t done = a.done[nl];
  const Row row = row_of(a.tb, nl);
  WinTest<S> win;
  win.mc = mc, win.mc_can_win = T == Tt;
  // What lives through the step loop is packed a byte a cell (cell t in bits 8 t .. 8 t + 7): p, the cells as they lie in memory
  // (an id >= C stays until a step moves the board), `in`, the initial cells, clamped, and the clamped targets.  Eight registers
  // each would cost the kernels of the larger boards a wave a SIMD.
  uint64_t p = 0, in = 0, tgp = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    p |= (uint64_t)p0[t] << (8 * t);
    in |= (uint64_t)min(in0[t], (uint32_t)(C - 1)) << (8 * t);
  }
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) {
    tg[j] = min(tg[j], (uint32_t)(C - 1));
    tgp |= (uint64_t)tg[j] << (8 * j);
    if (j < Tt) {
      win.tgm |= M(1) << tg[j];
      if (j < MT && j < T) win.tgt_key += (uint64_t)tg[j] * pow64<C>(j);
    }
  }
  auto cell_of = [](uint64_t packed, int t) -> uint32_t { return (uint32_t)(packed >> (8 * t)) & 0xffu; };
  const uint64_t draw = (uint64_t)(a.board_offset + nl) * ts::kDrawMul;

  // build-defined Manhattan reward of the cells c[] (include/tiler_slider.h: ts_reward)
  auto manhattan = [](uint32_t x, uint32_t y) -> int {
    return abs((int)(x / S) - (int)(y / S)) + abs((int)(x % S) - (int)(y % S));
  };
  auto reward_of = [&](uint64_t cells) -> int32_t {
    uint32_t c[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) c[t] = min(cell_of(cells, t), (uint32_t)(C - 1));
    int sum = 0;
    if (mc) {
      const int m = T < Tt ? T : Tt;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < m) sum += manhattan(c[t], cell_of(tgp, t));
    } else if (Tt > 0) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (t < T) {
          int best = 1 << 30;
#pragma unroll
          for (int j = 0; j < kMaxTargets; ++j)
            if (j < Tt) best = min(best, manhattan(c[t], cell_of(tgp, j)));
          sum += best;
        }
      }
    }
    return -sum;
  };
  // the 64-bit draw of (step, board): its top two bits are ts_fill_actions' action
  auto draw_of = [&](int k) -> uint64_t {
    const uint64_t key = ts::mix64(a.seed ^ ((uint64_t)(a.step_index + k) * ts::kBoardMul));  // uniform: a scalar per step
    return ts::mix64(key + draw);
  };
  auto choose = [&](uint32_t e, uint64_t r) -> uint32_t {
    const bool explore = (r & 0xffffffffull) < a.threshold;
    return (explore || e == 255u) ? (uint32_t)(r >> 62) : e;
  };
  const bool want_reward = a.reward_sum != nullptr;  // uniform
  const bool want_logs = a.act_log || a.flags_log || a.pos_log;
  auto write_logs = [&](int k, uint32_t act, uint32_t flags) {
    if (!live) return;
    if (a.act_log) a.act_log[(int64_t)k * N + n] = (uint8_t)act;
    if (a.flags_log) a.flags_log[(int64_t)k * N + n] = (uint8_t)flags;
    if (a.pos_log) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < T) a.pos_log[((int64_t)k * T + t) * N + n] = (uint8_t)cell_of(p, t);
    }
  };

  int32_t wins = 0, finished = 0, first_win = 0, win_moves = 0, reward_sum = 0;
  uint32_t flags = 0;

  int k = 0;
  for (; k < K; ++k) {
    // strict mode: once every board of the wave is done nothing moves any more - the rest is written by the tail below
    if (!autoreset && __builtin_amdgcn_ballot_w64(done == 0u) == 0) break;

    uint32_t pc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) pc[t] = min(cell_of(p, t), (uint32_t)(C - 1));  // clamp: malformed ids stay in-board

    // all four successors: the table's keys, and the step itself
    Looked<S, MT> o;
    look<S, MT>(pc, T, blk, win, row, a.tb.slots, a.tb.slots_log2, true, o);
    const uint32_t act = choose(ts::lowest_move(o.best), draw_of(k));  // 0 .. 3: the draw plays where the expert has no move
    const uint32_t dir = act & 3u;
    const uint64_t q = dir == 0u ? o.q4[0] : dir == 1u ? o.q4[1] : dir == 2u ? o.q4[2] : o.q4[3];
    const uint64_t qkey = dir == 0u ? o.key[1] : dir == 1u ? o.key[2] : dir == 2u ? o.key[3] : o.key[4];
    const bool won = dir == 0u ? o.won[1] : dir == 1u ? o.won[2] : dir == 2u ? o.won[3] : o.won[4];  // state.py:172-186
    const bool same = qkey == o.key[0];  // cells below C: the key is the placement

    // ---- ts_step (environment.py:100-143): done on entry, slide (the action is a move) ----
    if (done) {  // environment.py:113-114
      flags = autoreset ? TS_FLAG_AUTORESET : TS_FLAG_STEPPED_DONE;
      if (autoreset) {
        p = in;
        sc = 0;
        done = 0;
      }
    } else {
      flags = (won ? (TS_FLAG_IS_WON | TS_FLAG_SUCCESS) : 0u) | (same ? TS_FLAG_INVALID_MOVE : 0u);
      sc += 1;
      done = won ? 1u : 0u;
      if (sc >= a.max_steps) {
        done = 1u;
        flags |= TS_FLAG_TIMEOUT;
      }
      p = q;
    }

    // ---- the reductions ----
    const bool success = (flags & TS_FLAG_SUCCESS) != 0;
    wins += success ? 1 : 0;
    finished += (flags & (TS_FLAG_SUCCESS | TS_FLAG_TIMEOUT)) ? 1 : 0;
    first_win = (success && first_win == 0) ? k + 1 : first_win;
    win_moves += success ? sc : 0;
    if (want_reward) reward_sum += reward_of(p);
    if (want_logs) write_logs(k, act, flags);
  }

  // ---- strict mode, every board of the wave done: what the loop would still write, without sliding ----
  if (k < K) {
    flags = TS_FLAG_STEPPED_DONE;
    if (want_reward) reward_sum += (K - k) * reward_of(p);
    if (a.act_log) {
      // the board stands still, and so does its expert move
      uint32_t pc[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) pc[t] = min(cell_of(p, t), (uint32_t)(C - 1));
      Looked<S, MT> o;
      look<S, MT>(pc, T, blk, win, row, a.tb.slots, a.tb.slots_log2, true, o);
      const uint32_t e = ts::lowest_move(o.best);
      for (; k < K; ++k) write_logs(k, choose(e, draw_of(k)), flags);
    } else if (want_logs) {
      for (; k < K; ++k) write_logs(k, 0u, flags);
    }
  }

  if (!live) return;
  if (a.write_state) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < T) a.pos[(int64_t)t * N + n] = (uint8_t)cell_of(p, t);
    a.step_count[n] = sc;
    a.done[n] = (uint8_t)done;
  }
  if (a.wins) a.wins[n] = wins;
  if (a.finished) a.finished[n] = finished;
  if (a.first_win) a.first_win[n] = first_win;
  if (a.win_moves) a.win_moves[n] = win_moves;
  if (a.reward_sum) a.reward_sum[n] = reward_sum;
  if (a.flags) a.flags[n] = (uint8_t)flags;
}

struct LArgs {
  const uint8_t *first, *pos_log, *tgt;
  const uint32_t *blk;
  Table tb;
  int16_t *moves;  // each output may be NULL
  uint8_t *best, *action;
  int64_t N;
  int32_t T, Tt, mc, steps;
};

template <int S>
__global__ __launch_bounds__(kThreads) void k_rexpert_labels(const LArgs a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr int C = BB::C;
  constexpr int MT = max_tiles<S>();
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  const int k = (int)blockIdx.y;  // below a.steps: the grid is the steps high
  const int T = a.T, Tt = a.Tt;

  // the sample's cells, the level and the row: every load before the first one is consumed
  const uint8_t *src = k == 0 ? a.first : a.pos_log + (int64_t)(k - 1) * T * N;
  uint32_t pc[MT], tg[kMaxTargets];
#pragma unroll
  for (int t = 0; t < MT; ++t) pc[t] = 0;
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) tg[j] = 0;
  if (T > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) pc[t] = src[(int64_t)min(t, T - 1) * N + n];
  }
  if (Tt > 0) {
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j) tg[j] = a.tgt[(int64_t)min(j, Tt - 1) * N + n];
  }
  const M blk = ts::load_obstacles<S>(a.blk, N, n);
  const Row row = row_of(a.tb, n);
  WinTest<S> win;
  win.mc = a.mc != 0, win.mc_can_win = T == Tt;
#pragma unroll
  for (int t = 0; t < MT; ++t) pc[t] = min(pc[t], (uint32_t)(C - 1));
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) {
    tg[j] = min(tg[j], (uint32_t)(C - 1));
    if (j < Tt) {
      win.tgm |= M(1) << tg[j];
      if (j < MT && j < T) win.tgt_key += (uint64_t)tg[j] * pow64<C>(j);
    }
  }
  Looked<S, MT> o;
  look<S, MT>(pc, T, blk, win, row, a.tb.slots, a.tb.slots_log2, a.best || a.action, o);
  const int64_t i = (int64_t)k * N + n;
  if (a.moves) a.moves[i] = (int16_t)o.moves;
  if (a.best) a.best[i] = (uint8_t)o.best;
  if (a.action) a.action[i] = (uint8_t)ts::lowest_move(o.best);
}

using RolloutKernel = void (*)(const RArgs);
using LabelsKernel = void (*)(const LArgs);

RolloutKernel rollout_kernel(int S) {
  return ts::by_size<RolloutKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> RolloutKernel { return k_rexpert_rollout<s>; });
}
LabelsKernel labels_kernel(int S) {
  return ts::by_size<LabelsKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> LabelsKernel { return k_rexpert_labels<s>; });
}

// valid dims: ts_rollout_supported(dims, TS_ROLLOUT_RANDOM)'s rule and ts_rtable_supported's
bool shape_supported(const ts_dims *d) {
  return d->size <= TS_ROLLOUT_MAX_SIZE && d->size <= TS_REACH_MAX_SIZE && d->n_tiles <= TS_ROLLOUT_MAX_TILES && d->n_tiles <= TS_REACH_MAX_TILES &&
         d->n_targets <= TS_ROLLOUT_MAX_TILES;
}
// ts_rtable_lookup's rule for its table arguments
bool table_args_ok(int64_t n_rows, int64_t slots) { return n_rows >= 0 && slots >= 2 && slots <= (1ll << 31) && !(slots & (slots - 1)); }

Table table_of(const uint64_t *table, int64_t slots, const int32_t *count, int64_t n_rows, const int32_t *rows) {
  Table tb{};
  tb.table = table, tb.count = count, tb.rows = rows, tb.n_rows = n_rows, tb.slots = (uint32_t)slots;
  while ((1ll << tb.slots_log2) < slots) ++tb.slots_log2;
  return tb;
}

struct Plan {
  uint32_t bx = 0, by = 0;  // 0: nothing is launched
  ts_rexpert_desc desc{};
};
void plan_grid(int64_t bx, int64_t by, Plan &p) {
  p.bx = (uint32_t)bx, p.by = (uint32_t)by;
  p.desc.blocks = bx * by;
  p.desc.waves = p.desc.blocks * (kThreads / kWave);
}

// Every check of ts_rexpert_rollout that needs no pointer of st / out, and the launch it would make; touches no device.
int32_t plan_rollout(const ts_dims *d, const ts_rexpert_cfg *cfg, uint32_t out_mask, Plan &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (!cfg) return TS_ERR_NULL;
  if (!shape_supported(d)) return TS_ERR_LIMIT;
  if ((cfg->mode & ~TS_MODE_AUTORESET) || cfg->steps < 0 || cfg->steps > TS_ROLLOUT_MAX_STEPS || cfg->explore_threshold > (1ull << 32) ||
      !table_args_ok(cfg->n_rows, cfg->slots))
    return TS_ERR_ARG;
  p.desc.threads_per_block = kThreads;
  p.desc.lds_bytes = 0;
  p.desc.samples = (int64_t)cfg->steps * d->n_boards;
  if (d->n_boards == 0 || cfg->steps == 0) return TS_OK;  // nothing is launched
  const int64_t per_step = ((out_mask & TS_ROLLOUT_OUT_ACT_LOG) ? 1 : 0) + ((out_mask & TS_ROLLOUT_OUT_FLAGS_LOG) ? 1 : 0) +
                           ((out_mask & TS_ROLLOUT_OUT_POS_LOG) ? d->n_tiles : 0);
  p.desc.bytes = per_step * p.desc.samples;
  const int64_t blocks = (d->n_boards + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  plan_grid(blocks, 1, p);
  snprintf(p.desc.name, sizeof p.desc.name, "k_rexpert_rollout<%d>", d->size);
  return TS_OK;
}

constexpr uint32_t kLabelsOut = TS_LABELS_OUT_MOVES | TS_LABELS_OUT_BEST | TS_LABELS_OUT_ACTION;

// the same for ts_rexpert_labels, after dims, in / out and the table arguments
int32_t plan_labels(const ts_dims *d, int32_t steps, uint32_t what, Plan &p) {
  if (!shape_supported(d)) return TS_ERR_LIMIT;
  if (steps < 1 || steps > TS_ROLLOUT_MAX_STEPS) return TS_ERR_ARG;
  if ((what & ~kLabelsOut) || !(what & kLabelsOut)) return TS_ERR_ARG;
  p.desc.threads_per_block = kThreads;
  p.desc.lds_bytes = 0;
  p.desc.samples = (int64_t)steps * d->n_boards;
  if (d->n_boards == 0) return TS_OK;  // nothing is launched
  const int64_t blocks = (d->n_boards + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  plan_grid(blocks, steps, p);  // steps <= 65535, the height a grid may have
  p.desc.bytes = p.desc.samples * (((what & TS_LABELS_OUT_MOVES) ? 2 : 0) + ((what & TS_LABELS_OUT_BEST) ? 1 : 0) + ((what & TS_LABELS_OUT_ACTION) ? 1 : 0));
  snprintf(p.desc.name, sizeof p.desc.name, "k_rexpert_labels<%d>", d->size);
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_rexpert_abi_version(void) { return TS_REXPERT_ABI_VERSION; }
int32_t ts_rexpert_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_rexpert_supported(const ts_dims *dims) {
  const int32_t rc = ts::check_dims(dims);
  if (rc == TS_ERR_LIMIT) return 0;
  if (rc != TS_OK) return rc;
  return shape_supported(dims) ? 1 : 0;
}

int32_t ts_describe_rexpert_rollout(const ts_dims *dims, const ts_rexpert_cfg *cfg, uint32_t out_mask, ts_rexpert_desc *desc) {
  if (!dims || !cfg || !desc) return TS_ERR_NULL;
  Plan p;
  if (const int32_t rc = plan_rollout(dims, cfg, out_mask, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_describe_rexpert_labels(const ts_dims *dims, int32_t steps, uint32_t what, ts_rexpert_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  Plan p;
  if (const int32_t rc = plan_labels(dims, steps, what, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_rexpert_rollout(const ts_dims *dims, const ts_state *st, const ts_rexpert_cfg *cfg, const ts_rollout_out *out, void *stream) {
  const uint32_t mask = !out ? 0u
                             : (out->wins ? TS_ROLLOUT_OUT_WINS : 0u) | (out->finished ? TS_ROLLOUT_OUT_FINISHED : 0u) |
                                   (out->first_win ? TS_ROLLOUT_OUT_FIRST_WIN : 0u) | (out->win_moves ? TS_ROLLOUT_OUT_WIN_MOVES : 0u) |
                                   (out->reward_sum ? TS_ROLLOUT_OUT_REWARD_SUM : 0u) | (out->flags ? TS_ROLLOUT_OUT_FLAGS : 0u) |
                                   (out->act_log ? TS_ROLLOUT_OUT_ACT_LOG : 0u) | (out->flags_log ? TS_ROLLOUT_OUT_FLAGS_LOG : 0u) |
                                   (out->pos_log ? TS_ROLLOUT_OUT_POS_LOG : 0u);
  Plan p;
  if (const int32_t rc = plan_rollout(dims, cfg, mask, p); rc != TS_OK) return rc;
  if (!p.bx) return TS_OK;  // an empty batch or no step: nothing to launch, no pointer is looked at
  const bool autoreset = (cfg->mode & TS_MODE_AUTORESET) != 0;
  if (!st || !out || !st->blk || !st->step_count || !st->done || (dims->n_tiles > 0 && !st->pos) ||
      (dims->n_tiles > 0 && autoreset && !st->init) || (dims->n_targets > 0 && !st->tgt) ||
      (cfg->n_rows > 0 && (!cfg->table || !cfg->count)) || (mask == 0u && !cfg->write_state))
    return TS_ERR_NULL;
  RolloutKernel k = rollout_kernel(dims->size);
  if (!k) return TS_ERR_LIMIT;
  RArgs a{};
  a.pos = static_cast<uint8_t *>(st->pos), a.init = static_cast<const uint8_t *>(st->init), a.tgt = static_cast<const uint8_t *>(st->tgt);
  a.blk = st->blk, a.step_count = st->step_count, a.done = st->done;
  a.tb = table_of(cfg->table, cfg->slots, cfg->count, cfg->n_rows, cfg->rows);
  a.wins = out->wins, a.finished = out->finished, a.first_win = out->first_win, a.win_moves = out->win_moves, a.reward_sum = out->reward_sum;
  a.flags = out->flags, a.act_log = out->act_log, a.flags_log = out->flags_log, a.pos_log = static_cast<uint8_t *>(out->pos_log);
  a.N = dims->n_boards, a.step_index = cfg->step_index, a.board_offset = cfg->board_offset;
  a.seed = cfg->seed, a.threshold = cfg->explore_threshold;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.max_steps = dims->max_steps, a.steps = cfg->steps;
  a.autoreset = autoreset ? 1 : 0, a.write_state = cfg->write_state ? 1 : 0;
  hipLaunchKernelGGL(k, dim3(p.bx), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_rexpert_labels(const ts_dims *dims, const ts_state *st, const ts_rexpert_labels_in *in, const ts_labels_out *out, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!in || !out) return TS_ERR_NULL;
  if (!shape_supported(dims)) return TS_ERR_LIMIT;
  if (in->steps < 1 || in->steps > TS_ROLLOUT_MAX_STEPS || !table_args_ok(in->n_rows, in->slots)) return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  const bool tiles = dims->n_tiles > 0;
  if (!st || !st->blk || (dims->n_targets > 0 && !st->tgt) || (tiles && !in->first) || (tiles && in->steps > 1 && !in->pos_log) ||
      (in->n_rows > 0 && (!in->table || !in->count)) || (!out->moves && !out->best && !out->action))
    return TS_ERR_NULL;
  const uint32_t what = (out->moves ? TS_LABELS_OUT_MOVES : 0u) | (out->best ? TS_LABELS_OUT_BEST : 0u) | (out->action ? TS_LABELS_OUT_ACTION : 0u);
  Plan p;
  if (const int32_t rc = plan_labels(dims, in->steps, what, p); rc != TS_OK) return rc;
  LabelsKernel k = labels_kernel(dims->size);
  if (!k) return TS_ERR_LIMIT;
  LArgs a{};
  a.first = static_cast<const uint8_t *>(in->first), a.pos_log = static_cast<const uint8_t *>(in->pos_log);
  a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  a.tb = table_of(in->table, in->slots, in->count, in->n_rows, in->rows);
  a.moves = out->moves, a.best = out->best, a.action = out->action;
  a.N = dims->n_boards, a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.steps = in->steps;
  hipLaunchKernelGGL(k, dim3(p.bx, p.by), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
