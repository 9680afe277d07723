// ts_mixed.hip — mixed rollouts: K steps in which a network and a table expert share the play, the table's answers logged, one
// launch (include/tiler_slider_mixed.h, which defines it).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_mixed.so): every earlier code object is pinned kernel
// by kernel, and nothing here touches any of them.  ts_mlp.h is included unchanged.
//
// k_mixed_rollout<S, SELECT, KIND>: ONE BOARD PER LANE, as k_policy_rollout (ts_policy.hip).  The step body below - clamp, slide,
// win test, done / auto-reset, reductions, logs, the strict-mode early exit and its tail - is one more COPY of k_policy_rollout's,
// not a shared header: ts_policy.hip says what lifting it did to the kernels that were there.  The network - stage_weights,
// static_preact, logits_of - and the block plan are ts_mlp.h's.
//
// What is new is the lookup on every board visited, RESTATED from the two table formats as ts_rexpert.hip restates the probe:
//   TS_MIXED_DENSE  ts_table_lookup's five byte reads of the board's row: entry idx = sum_t cell_t * C^t of the board and of its
//                   four successors (tiler_slider_table.h; the expert rule is ts_index.h's best_moves / lowest_move);
//   TS_MIXED_REACH  ts_rtable_lookup's five probes: a slot is 0 or  bit 63 | entry << 48 | key,  linear probing from
//                   home(key) = (uint32)((key * 0x9e3779b97f4a7c15) >> 32) >> (32 - log2(slots)) (tiler_slider_rtable.h).
// Latency: the five addresses are formed and the five loads - bytes, or home slots - are issued BEFORE the network is evaluated,
// unconditionally for every lane whose row lies inside the table, and consumed after it: the scattered reads hide behind the H
// LDS reads and multiply-adds of logits_of.  A reach probe that met neither its key nor an empty slot then walks on as in
// ts_rexpert.hip, at most `slots` reads in all, every index masked into the row.
//
// THE TABLE IS READ or not by a UNIFORM BRANCH on a kernel argument (a.table_read), not by a template parameter: 32 kernels, not
// 64, and with table_read == 0 the kernel executes no instruction that forms a table address.  Where it is read, EVERY lane looks
// its board up, whether or not its answer is needed (a lane whose draw explores, or does not teach, with no table log asked for):
// the wave waits for its slowest lane anyway, and the logs usually want every answer.  The step itself slides the board in the
// direction played, as the copy it is; the lookup's four successors are not reused for it.
#include "../../include/tiler_slider_mixed.h"
#include "ts_mlp.h"

namespace {

struct MArgs {
  static constexpr bool kValue = false;  // no value head
  uint8_t *pos;  // cell_t = uint8 (S <= 8)
  const uint8_t *init, *tgt;
  const uint32_t *blk;
  int32_t *step_count;
  uint8_t *done;
  const float *w1, *b1, *w2, *b2;
  int32_t *wins, *finished, *first_win, *win_moves, *reward_sum;  // each output may be NULL
  uint8_t *flags, *act_log, *flags_log, *pos_log;
  float *logits_log;
  uint8_t *expert_log, *best_log, *who_log;
  int16_t *moves_log;
  const uint8_t *dense;     // DENSE: uint8 [n_rows][states]
  const uint64_t *rtable;   // REACH: uint64 [n_rows][rslots]
  const int32_t *count;     // REACH: int32 [n_rows]
  const int32_t *rows;      // may be NULL
  int64_t N, step_index, board_offset, n_rows;
  uint64_t seed, threshold, beta;
  uint32_t states, rslots, rslots_log2;
  int32_t table_read;  // uniform: 0 = no byte of the table is read
  int32_t T, Tt, mc, max_steps, steps, autoreset, write_state;
  int32_t H, slots, staged, wt_floats;  // slots: T' * S*S; wt_floats: LDS floats of the staged tile-plane weights
};

// e of the definition; <= 3 whatever z holds (ts_policy.hip's select_action)
template <int SELECT>
__device__ __forceinline__ uint32_t select_action(const float (&z)[4], uint64_t r) {
  const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
  if constexpr (SELECT == TS_POLICY_GREEDY) {
    return z[0] == m ? 0u : z[1] == m ? 1u : z[2] == m ? 2u : 3u;
  } else {
    const float c0 = __expf(z[0] - m), c1 = c0 + __expf(z[1] - m), c2 = c1 + __expf(z[2] - m), c3 = c2 + __expf(z[3] - m);
    const float u = (float)(uint32_t)((r >> 32) & 0xffffffu) * 0x1p-24f;
    const float x = u * c3;
    return x < c0 ? 0u : x < c1 ? 1u : x < c2 ? 2u : 3u;
  }
}

template <int S>
struct Board {
  using M = typename ts::Bitboard<S>::mask_t;
  static constexpr int MT = max_tiles<S>();
  M blk, tgm;
  uint32_t p[MT], in[MT], tg[kMaxTargets];
};

// the board of lane nl: obstacles, targets, cells as they lie in memory, and (auto-reset) the clamped initial cells
template <int S>
__device__ __forceinline__ void load_board(const MArgs &a, int64_t nl, bool want_init, Board<S> &b) {
  using M = typename Board<S>::M;
  constexpr int C = S * S, MT = Board<S>::MT;
  constexpr M kFull = C == 64 ? ~M(0) : (M(1) << (C & 63)) - 1;
  const int64_t N = a.N;
  b.blk = ts::load_obstacles<S>(a.blk, N, nl) & kFull;
#pragma unroll
  for (int t = 0; t < MT; ++t) b.p[t] = 0, b.in[t] = 0;
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) b.tg[j] = 0;
  // loads go out unconditionally, all before the first one is consumed: rows past the count read the last row, results unused
  if (a.T > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) b.p[t] = a.pos[(int64_t)min(t, a.T - 1) * N + nl];
    if (want_init) {
#pragma unroll
      for (int t = 0; t < MT; ++t) b.in[t] = a.init[(int64_t)min(t, a.T - 1) * N + nl];
    }
  }
  if (a.Tt > 0) {
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j) b.tg[j] = a.tgt[(int64_t)min(j, a.Tt - 1) * N + nl];
  }
  b.tgm = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) b.in[t] = min(b.in[t], (uint32_t)(C - 1));
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) {
    b.tg[j] = min(b.tg[j], (uint32_t)(C - 1));
    if (j < a.Tt) b.tgm |= M(1) << b.tg[j];
  }
}

// ---- the lookups, restated from tiler_slider_table.h and tiler_slider_rtable.h ----

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

// (m, bits, x) of the definition
struct Answer {
  int32_t moves = TS_SOLVE_NONE;
  uint32_t best = 0;
  __device__ __forceinline__ uint32_t action() const { return ts::lowest_move(best); }
};

// One lookup in flight: begin() forms the five addresses and issues the five loads, end() consumes them.  A row index outside
// the table leaves `row` null: nothing is read, and end() gives ts_table_lookup's TS_SOLVE_NONE, 0, 255.
template <int S, int KIND>
struct Lookup;

template <int S>
struct Lookup<S, TS_MIXED_DENSE> {
  using M = typename ts::Bitboard<S>::mask_t;
  static constexpr int C = S * S, MT = max_tiles<S>();
  const uint8_t *row = nullptr;
  uint32_t d0 = 0, d[4] = {0, 0, 0, 0};

  __device__ __forceinline__ void init(const MArgs &a, int64_t nl, M, const uint32_t (&)[kMaxTargets]) {
    const int64_t r = a.rows ? (int64_t)a.rows[nl] : nl;
    if (r >= 0 && r < a.n_rows) row = a.dense + r * (int64_t)a.states;
  }
  // clamped cells and slid cells are < C and the dense shapes have (S*S)^T = states: every index stays inside the row
  __device__ __forceinline__ void begin(const MArgs &a, const uint32_t (&pc)[MT], M occ, M blk) {
    if (!row) return;
    const int T = a.T;
    uint32_t idx0 = 0, idx[4];
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < T) idx0 += pc[t] * (uint32_t)pow64<C>(t);
#pragma unroll
    for (int dir = 0; dir < 4; ++dir) {
      idx[dir] = 0;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < T) idx[dir] += (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir) * (uint32_t)pow64<C>(t);
    }
    d0 = row[idx0];
#pragma unroll
    for (int dir = 0; dir < 4; ++dir) d[dir] = row[idx[dir]];
  }
  __device__ __forceinline__ Answer end(const MArgs &) {
    Answer o;
    if (!row) return o;
    if (d0 <= (uint32_t)TS_TABLE_MAX_DEPTH) {
      o.moves = (int32_t)d0;
      if (d0 >= 1u) o.best = ts::best_moves(d0, d);
    } else if (d0 == (uint32_t)TS_TABLE_DEEP) {
      o.moves = TS_SOLVE_DEPTH;
    }
    return o;
  }
};

template <int S>
struct Lookup<S, TS_MIXED_REACH> {
  using M = typename ts::Bitboard<S>::mask_t;
  static constexpr int C = S * S, MT = max_tiles<S>();
  const uint64_t *row = nullptr;
  bool full = false, mc = false, mc_can_win = false;
  M tgm = 0;
  uint64_t tgt_key = 0;
  // of the lookup in flight
  uint64_t key[5], e[5];
  uint32_t slot[5];
  bool won[5], probing;

  __device__ __forceinline__ bool win(uint64_t k, M occ) const { return mc ? (mc_can_win && k == tgt_key) : occ == tgm; }

  __device__ __forceinline__ void init(const MArgs &a, int64_t nl, M tgm_, const uint32_t (&tg)[kMaxTargets]) {
    const int64_t r = a.rows ? (int64_t)a.rows[nl] : nl;
    if (r >= 0 && r < a.n_rows) {  // outside: nothing of table or count is read
      full = a.count[r] == TS_REACH_FULL;
      row = a.rtable + (uint64_t)r * a.rslots;
    }
    mc = a.mc != 0, mc_can_win = a.T == a.Tt, tgm = tgm_;
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j)
      if (j < a.Tt && j < MT && j < a.T) tgt_key += (uint64_t)tg[j] * pow64<C>(j);
  }
  // the five home-slot loads go out together, those of won placements included (the address lies inside the row; the result is dropped)
  __device__ __forceinline__ void begin(const MArgs &a, const uint32_t (&pc)[MT], M occ, M blk) {
    const int T = a.T;
    key[0] = 0;
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < T) key[0] += (uint64_t)pc[t] * pow64<C>(t);
    won[0] = win(key[0], occ);
#pragma unroll
    for (int dir = 0; dir < 4; ++dir) {
      M occ2 = 0;
      key[1 + dir] = 0;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (t < T) {
          const uint32_t q = (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir);  // a cell < C whatever the board
          key[1 + dir] += (uint64_t)q * pow64<C>(t);
          occ2 |= M(1) << q;
        }
      }
      won[1 + dir] = win(key[1 + dir], occ2);
    }
    probing = row && !full && !won[0];
    if (probing) {
      const uint32_t mask = a.rslots - 1u;
#pragma unroll
      for (int i = 0; i < 5; ++i) slot[i] = home_of(key[i], a.rslots_log2) & mask;
#pragma unroll
      for (int i = 0; i < 5; ++i) e[i] = row[slot[i]];
    }
  }
  __device__ __forceinline__ Answer end(const MArgs &a) {
    Answer o;
    if (!row) return o;
    uint32_t ent[5] = {kNoEntry, kNoEntry, kNoEntry, kNoEntry, kNoEntry};
    if (probing) {
      const uint32_t mask = a.rslots - 1u;
      uint32_t open = 0;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const bool hit = (e[i] & kOcc) && (e[i] & kKeyMask) == key[i];
        ent[i] = hit ? (uint32_t)(e[i] >> kEntryShift) & 0xffu : kNoEntry;
        open |= (!hit && e[i] != 0 && !won[i]) ? 1u << i : 0u;
      }
      for (uint32_t probe = 1; open != 0 && probe < a.rslots; ++probe) {  // per lane: rare in a table at most half full
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
      for (int i = 1; i < 5; ++i)
        if (won[i]) ent[i] = kNoEntry;  // a won placement is not stored
    }
    // ts_rtable_lookup's answers, in its order
    if (won[0]) {
      o.moves = 0;
    } else if (full) {
      o.moves = TS_REACH_FULL;
    } else if (ent[0] == kNoEntry) {
      o.moves = TS_RTABLE_ABSENT;
    } else if (ent[0] >= 1u && ent[0] <= (uint32_t)TS_TABLE_MAX_DEPTH) {
      o.moves = (int32_t)ent[0];
#pragma unroll
      for (int dir = 0; dir < 4; ++dir) {
        // a won successor is 0 from the win; an entry 0 is never stored and is no distance
        const uint32_t dd = won[1 + dir] ? 0u : (ent[1 + dir] == kNoEntry || ent[1 + dir] == 0u) ? (uint32_t)TS_TABLE_NONE : ent[1 + dir];
        o.best |= (dd == ent[0] - 1u ? 1u : 0u) << dir;
      }
    } else {
      o.moves = ent[0] == (uint32_t)TS_TABLE_DEEP ? TS_SOLVE_DEPTH : TS_SOLVE_NONE;
    }
    return o;
  }
};

template <int S, int SELECT, int KIND>
__global__ __launch_bounds__(kMaxThreads) void k_mixed_rollout(const MArgs a) {
  using M = typename Board<S>::M;
  constexpr int C = S * S, MT = Board<S>::MT;

  stage_weights(a, C);
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  // lanes past the batch play a copy of the LAST board and write nothing
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  const int T = a.T, Tt = a.Tt, K = a.steps;
  const bool mc = a.mc != 0, autoreset = a.autoreset != 0;
  const bool table_read = a.table_read != 0;  // uniform

  // ---- the board, once ----
  Board<S> b;
  load_board<S>(a, nl, autoreset, b);
  uint32_t(&p)[MT] = b.p;
  const uint32_t(&in)[MT] = b.in;
  const uint32_t(&tg)[kMaxTargets] = b.tg;
  const M blk = b.blk, tgm = b.tgm;
  int32_t sc = a.step_count[nl];
  uint32_t done = a.done[nl];
  const uint64_t draw = (uint64_t)(a.board_offset + nl) * ts::kDrawMul;
  Lookup<S, KIND> look;
  if (table_read) look.init(a, nl, tgm, tg);

  // ---- the network's constant part, once ----
  Hs hs(g_lds + head_floats<MArgs::kValue>(a.H) + a.wt_floats + threadIdx.x, (int)blockDim.x);
  static_preact<S>(a, hs, blk, tgm, tg);

  // build-defined Manhattan reward of the cells c[] (include/tiler_slider.h: ts_reward)
  auto manhattan = [](uint32_t x, uint32_t y) -> int {
    return abs((int)(x / S) - (int)(y / S)) + abs((int)(x % S) - (int)(y % S));
  };
  auto reward_of = [&](const uint32_t(&c)[MT]) -> int32_t {
    int sum = 0;
    if (mc) {
      const int m = T < Tt ? T : Tt;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < m) sum += manhattan(c[t], tg[t]);
    } else if (Tt > 0) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (t < T) {
          int best = 1 << 30;
#pragma unroll
          for (int j = 0; j < kMaxTargets; ++j)
            if (j < Tt) best = min(best, manhattan(c[t], tg[j]));
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
  // a and who of the definition from e's logits, the draw and the expert's move x
  auto choose = [&](const float(&z)[4], uint64_t r, uint32_t x, uint32_t &who) -> uint32_t {
    const uint32_t e = select_action<SELECT>(z, r);
    const bool explore = (r & 0xffffffffull) < a.threshold;
    const bool teach = (ts::mix64(r ^ TS_MIXED_SALT) & 0xffffffffull) < a.beta && x != 255u;
    who = explore ? (uint32_t)TS_MIXED_WHO_RANDOM : teach ? (uint32_t)TS_MIXED_WHO_EXPERT : (uint32_t)TS_MIXED_WHO_NETWORK;
    return explore ? (uint32_t)(r >> 62) : teach ? x : e;
  };
  const bool want_reward = a.reward_sum != nullptr;  // uniform
  const bool want_labels = a.expert_log || a.moves_log || a.best_log;
  const bool want_logs = a.act_log || a.flags_log || a.pos_log || a.logits_log || want_labels || a.who_log;
  auto write_logs = [&](int k, uint32_t act, uint32_t flags, const float(&z)[4], const Answer &o, uint32_t who) {
    if (!live) return;
    const int64_t i = (int64_t)k * N + n;
    if (a.act_log) a.act_log[i] = (uint8_t)act;
    if (a.flags_log) a.flags_log[i] = (uint8_t)flags;
    if (a.pos_log) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < T) a.pos_log[((int64_t)k * T + t) * N + n] = (uint8_t)p[t];
    }
    if (a.logits_log) reinterpret_cast<float4 *>(a.logits_log)[i] = make_float4(z[0], z[1], z[2], z[3]);
    if (a.expert_log) a.expert_log[i] = (uint8_t)o.action();
    if (a.moves_log) a.moves_log[i] = (int16_t)o.moves;
    if (a.best_log) a.best_log[i] = (uint8_t)o.best;
    if (a.who_log) a.who_log[i] = (uint8_t)who;
  };

  int32_t wins = 0, finished = 0, first_win = 0, win_moves = 0, reward_sum = 0;
  uint32_t flags = 0;

  int k = 0;
  for (; k < K; ++k) {
    // strict mode: once every board of the wave is done nothing moves any more - the rest is written by the tail below
    if (!autoreset && __builtin_amdgcn_ballot_w64(done == 0u) == 0) break;

    uint32_t pc[MT];
    M occ = 0;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      pc[t] = min(p[t], (uint32_t)(C - 1));  // clamp: malformed ids stay in-board
      if (t < T) occ |= M(1) << pc[t];
    }

    if (table_read) look.begin(a, pc, occ, blk);  // the five loads go out in front of the network
    float z[4];
    logits_of<S, MT>(a, hs, pc, z);
    Answer o;
    if (table_read) o = look.end(a);
    uint32_t who;
    const uint32_t act = choose(z, draw_of(k), o.action(), who);  // <= 3: x is 255 or a move
    const int dir = (int)(act & 3u);
    uint32_t q[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      q[t] = pc[t];
      if (t < T) q[t] = (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir);
    }

    // ---- ts_step (environment.py:100-143), the order of k_rollout: done on entry, slide ----
    bool same = true, ordered = T == Tt;
    M occ2 = 0;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      if (t < T) {
        same &= q[t] == pc[t];
        ordered &= q[t] == tg[t];
        occ2 |= M(1) << q[t];
      }
    }
    const bool won = mc ? ordered : (occ2 == tgm);  // state.py:172-186
    if (done) {                                     // environment.py:113-114
      flags = autoreset ? TS_FLAG_AUTORESET : TS_FLAG_STEPPED_DONE;
      if (autoreset) {
#pragma unroll
        for (int t = 0; t < MT; ++t) p[t] = in[t];
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
#pragma unroll
      for (int t = 0; t < MT; ++t) p[t] = q[t];
    }

    // ---- the reductions ----
    const bool success = (flags & TS_FLAG_SUCCESS) != 0;
    wins += success ? 1 : 0;
    finished += (flags & (TS_FLAG_SUCCESS | TS_FLAG_TIMEOUT)) ? 1 : 0;
    first_win = (success && first_win == 0) ? k + 1 : first_win;
    win_moves += success ? sc : 0;
    if (want_reward) {
      uint32_t c[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) c[t] = min(p[t], (uint32_t)(C - 1));
      reward_sum += reward_of(c);
    }
    if (want_logs) write_logs(k, act, flags, z, o, who);
  }

  // ---- strict mode, every board of the wave done: what the loop would still write, without sliding ----
  if (k < K) {
    flags = TS_FLAG_STEPPED_DONE;
    uint32_t c[MT];
    M occ = 0;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      c[t] = min(p[t], (uint32_t)(C - 1));
      if (t < T) occ |= M(1) << c[t];
    }
    if (want_reward) reward_sum += (K - k) * reward_of(c);
    if (want_logs) {
      // the board stands still, and so do its logits and the table's answer on it
      float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      Answer o;
      if (table_read && (a.act_log || a.who_log || want_labels)) {
        look.begin(a, c, occ, blk);
        o = look.end(a);
      }
      if (a.act_log || a.logits_log) logits_of<S, MT>(a, hs, c, z);
      const uint32_t x = o.action();
      for (; k < K; ++k) {
        uint32_t who = 0, act = 0;
        if (a.act_log || a.who_log) act = choose(z, draw_of(k), x, who);
        write_logs(k, act, flags, z, o, who);
      }
    }
  }

  if (!live) return;
  if (a.write_state) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < T) a.pos[(int64_t)t * N + n] = (uint8_t)p[t];
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

using Kernel = void (*)(const MArgs);

template <int SELECT, int KIND>
Kernel select_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_mixed_rollout<s, SELECT, KIND>; });
}
Kernel rollout_kernel(int S, int select, int kind) {
  if (kind == TS_MIXED_DENSE) return select == TS_POLICY_GREEDY ? select_kernel<TS_POLICY_GREEDY, TS_MIXED_DENSE>(S) : select_kernel<TS_POLICY_SAMPLE, TS_MIXED_DENSE>(S);
  return select == TS_POLICY_GREEDY ? select_kernel<TS_POLICY_GREEDY, TS_MIXED_REACH>(S) : select_kernel<TS_POLICY_SAMPLE, TS_MIXED_REACH>(S);
}

bool valid_select(int32_t s) { return s == TS_POLICY_GREEDY || s == TS_POLICY_SAMPLE; }
bool valid_kind(int32_t k) { return k == TS_MIXED_DENSE || k == TS_MIXED_REACH; }
// ts_rtable_lookup's rule for slots
bool slots_ok(int64_t slots) { return slots >= 2 && slots <= (1ll << 31) && !(slots & (slots - 1)); }
// ts_rtable_supported's rule
bool reach_shape(const ts_dims *d) { return d->size <= TS_REACH_MAX_SIZE && d->n_tiles <= TS_REACH_MAX_TILES; }

// TS_ERR_LIMIT / TS_ERR_ARG / TS_OK of check 3: the policy's shape first, then the kind, then the kind's own shape
int32_t check_shape(const ts_dims *d, int32_t hidden, int32_t kind) {
  if (!shape_supported(d, hidden)) return TS_ERR_LIMIT;
  if (!valid_kind(kind)) return TS_ERR_ARG;
  if (kind == TS_MIXED_DENSE ? ts::index_states(d) == 0 : !reach_shape(d)) return TS_ERR_LIMIT;
  return TS_OK;
}

constexpr uint32_t kLabelLogs = TS_MIXED_OUT_EXPERT_LOG | TS_MIXED_OUT_MOVES_LOG | TS_MIXED_OUT_BEST_LOG;

using MixedPlan = Plan<MArgs, ts_mixed_desc>;

// Every check of ts_mixed_rollout that needs no pointer of st / mlp's parameters / out, and the launch it would make
int32_t plan_rollout(const ts_dims *d, int32_t hidden, const ts_mixed_cfg *cfg, uint32_t out_mask, MixedPlan &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (!cfg) return TS_ERR_NULL;
  if (const int32_t rc = check_shape(d, hidden, cfg->kind); rc != TS_OK) return rc;
  if ((cfg->mode & ~TS_MODE_AUTORESET) || !valid_select(cfg->select) || cfg->steps < 0 || cfg->steps > TS_ROLLOUT_MAX_STEPS ||
      cfg->explore_threshold > (1ull << 32) || cfg->beta_threshold > (1ull << 32) || cfg->n_rows < 0 ||
      (cfg->kind == TS_MIXED_REACH && !slots_ok(cfg->slots)))
    return TS_ERR_ARG;
  plan_forward_block(d, hidden, p);
  p.desc.threads_per_block = (int32_t)p.threads;
  p.desc.lds_bytes = (int32_t)p.lds;
  p.desc.weights_in_lds = p.staged;
  p.desc.table_read = (cfg->beta_threshold != 0 || (out_mask & kLabelLogs)) ? 1 : 0;
  if (d->n_boards == 0 || cfg->steps == 0) return TS_OK;  // nothing is launched
  const int64_t per_step = ((out_mask & TS_ROLLOUT_OUT_ACT_LOG) ? 1 : 0) + ((out_mask & TS_ROLLOUT_OUT_FLAGS_LOG) ? 1 : 0) +
                           ((out_mask & TS_ROLLOUT_OUT_POS_LOG) ? d->n_tiles : 0) + ((out_mask & TS_POLICY_OUT_LOGITS_LOG) ? 16 : 0) +
                           ((out_mask & TS_MIXED_OUT_EXPERT_LOG) ? 1 : 0) + ((out_mask & TS_MIXED_OUT_MOVES_LOG) ? 2 : 0) +
                           ((out_mask & TS_MIXED_OUT_BEST_LOG) ? 1 : 0) + ((out_mask & TS_MIXED_OUT_WHO_LOG) ? 1 : 0);
  p.desc.logged_bytes = per_step * cfg->steps * d->n_boards;
  p.kernel = rollout_kernel(d->size, cfg->select, cfg->kind);
  const int64_t blocks = (d->n_boards + p.threads - 1) / p.threads;
  if (!p.kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  p.desc.blocks = blocks;
  snprintf(p.desc.name, sizeof p.desc.name, "k_mixed_rollout<%d, %d, %d>", d->size, cfg->select, cfg->kind);
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_mixed_abi_version(void) { return TS_MIXED_ABI_VERSION; }
int32_t ts_mixed_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_mixed_supported(const ts_dims *dims, int32_t hidden, int32_t kind) {
  const int32_t rc = ts::check_dims(dims);
  if (rc == TS_ERR_LIMIT) return 0;
  if (rc != TS_OK) return rc;
  const int32_t shape = check_shape(dims, hidden, kind);
  return shape == TS_OK ? 1 : shape == TS_ERR_LIMIT ? 0 : shape;
}

int32_t ts_describe_mixed_rollout(const ts_dims *dims, int32_t hidden, const ts_mixed_cfg *cfg, uint32_t out_mask, ts_mixed_desc *desc) {
  if (!dims || !cfg || !desc) return TS_ERR_NULL;
  MixedPlan p;
  const int32_t rc = plan_rollout(dims, hidden, cfg, out_mask, p);
  if (rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_mixed_rollout(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const ts_mixed_cfg *cfg, const ts_mixed_out *out,
                         void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!cfg || !mlp) return TS_ERR_NULL;
  const uint32_t mask = !out ? 0u
                             : (out->wins ? TS_ROLLOUT_OUT_WINS : 0u) | (out->finished ? TS_ROLLOUT_OUT_FINISHED : 0u) |
                                   (out->first_win ? TS_ROLLOUT_OUT_FIRST_WIN : 0u) | (out->win_moves ? TS_ROLLOUT_OUT_WIN_MOVES : 0u) |
                                   (out->reward_sum ? TS_ROLLOUT_OUT_REWARD_SUM : 0u) | (out->flags ? TS_ROLLOUT_OUT_FLAGS : 0u) |
                                   (out->act_log ? TS_ROLLOUT_OUT_ACT_LOG : 0u) | (out->flags_log ? TS_ROLLOUT_OUT_FLAGS_LOG : 0u) |
                                   (out->pos_log ? TS_ROLLOUT_OUT_POS_LOG : 0u) | (out->logits_log ? TS_POLICY_OUT_LOGITS_LOG : 0u) |
                                   (out->expert_log ? TS_MIXED_OUT_EXPERT_LOG : 0u) | (out->moves_log ? TS_MIXED_OUT_MOVES_LOG : 0u) |
                                   (out->best_log ? TS_MIXED_OUT_BEST_LOG : 0u) | (out->who_log ? TS_MIXED_OUT_WHO_LOG : 0u);
  MixedPlan p;
  if (const int32_t rc = plan_rollout(dims, mlp->hidden, cfg, mask, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch or no step: nothing to launch, no pointer is looked at
  const bool autoreset = (cfg->mode & TS_MODE_AUTORESET) != 0;
  const bool table_read = p.desc.table_read != 0;
  const bool table_missing = table_read && cfg->n_rows > 0 && (cfg->kind == TS_MIXED_DENSE ? !cfg->dense : (!cfg->table || !cfg->count));
  if (!st || !out || !mlp_complete(mlp) || !st->blk || !st->step_count || !st->done || (dims->n_tiles > 0 && !st->pos) ||
      (dims->n_tiles > 0 && autoreset && !st->init) || (dims->n_targets > 0 && !st->tgt) || (mask == 0u && !cfg->write_state) || table_missing)
    return TS_ERR_NULL;
  if (((uintptr_t)out->logits_log & 15u) || ((uintptr_t)out->moves_log & 1u)) return TS_ERR_ARG;
  MArgs a{};
  a.pos = static_cast<uint8_t *>(st->pos), a.init = static_cast<const uint8_t *>(st->init), a.tgt = static_cast<const uint8_t *>(st->tgt);
  a.blk = st->blk, a.step_count = st->step_count, a.done = st->done;
  a.w1 = mlp->w1, a.b1 = mlp->b1, a.w2 = mlp->w2, a.b2 = mlp->b2;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.max_steps = dims->max_steps;
  a.H = mlp->hidden, a.slots = p.slots, a.staged = p.staged, a.wt_floats = p.wt_floats;
  a.wins = out->wins, a.finished = out->finished, a.first_win = out->first_win, a.win_moves = out->win_moves, a.reward_sum = out->reward_sum;
  a.flags = out->flags, a.act_log = out->act_log, a.flags_log = out->flags_log, a.pos_log = static_cast<uint8_t *>(out->pos_log);
  a.logits_log = out->logits_log;
  a.expert_log = out->expert_log, a.moves_log = out->moves_log, a.best_log = out->best_log, a.who_log = out->who_log;
  a.step_index = cfg->step_index, a.board_offset = cfg->board_offset;
  a.seed = cfg->seed, a.threshold = cfg->explore_threshold, a.beta = cfg->beta_threshold;
  a.steps = cfg->steps, a.autoreset = autoreset ? 1 : 0, a.write_state = cfg->write_state ? 1 : 0;
  a.table_read = table_read ? 1 : 0;
  a.rows = cfg->rows, a.n_rows = cfg->n_rows;
  if (cfg->kind == TS_MIXED_DENSE) {
    a.dense = cfg->dense, a.states = (uint32_t)ts::index_states(dims);
  } else {
    a.rtable = cfg->table, a.count = cfg->count, a.rslots = (uint32_t)cfg->slots;
    while ((1ll << a.rslots_log2) < cfg->slots) ++a.rslots_log2;
  }
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
