// ts_rollout.hip — fused on-device rollouts: K steps, policy included, one launch (include/tiler_slider_rollout.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_rollout.so): the step, search and table libraries
// are pinned symbol by symbol and kernel by kernel, and nothing here touches any of them.
//
// k_rollout<S, POLICY>: ONE BOARD PER LANE.  The lane loads its board once - the level (obstacle bitboard, target cells, and
// in auto-reset mode the initial cells) and the dynamic state (tile cells, step counter, done latch) -, plays `steps` steps
// with all of it in registers, and stores the dynamic state once.  No LDS, no scratch, no barrier: tiles live in a register
// array walked by fully unrolled loops predicated on t < T (T is uniform, so the predicates are scalar branches).
//
// The transition is ts::slide_cell<S> and the win test the bitboard comparison of ts_core.h - the arithmetic of the step
// kernels -, the action stream is ts::mix64 with the constants of ts_fill_actions, and the expert move is the rule of
// k_table_lookup (ts_index.h: best_moves, lowest_move) over the same five bytes of the board's row.  What the kernel must compute is fixed by the loop over
// ts_fill_actions / ts_table_lookup / ts_step in the header; tests hold it to that loop byte for byte.
//
// Latency: the step loop is wave-uniform, key_k is a scalar per step.  The GIVEN action byte of step
// k + 1 is loaded while step k slides.  The TABLE policy slides the board in all four directions - one of them is the step it is
// about to play - and issues the five table reads of a step together, unconditionally, so that a step costs ONE memory round
// trip where k_table_lookup's own order (the successors only once the board's entry is known) would cost two; the first table
// read of step k + 1 depends on the cells step k produced, and that round trip per step is the floor of the policy.
#include "../../include/tiler_slider_rollout.h"
#include "ts_launch.h"

namespace {

using ts::kWave;
constexpr int kThreads = 256;  // four waves per block; waves never interact
constexpr int kMaxTargets = TS_ROLLOUT_MAX_TILES;

struct RArgs {
  uint8_t *pos;  // cell_t = uint8 (S <= 8)
  const uint8_t *init, *tgt;
  const uint32_t *blk;
  int32_t *step_count;
  uint8_t *done;
  const uint8_t *actions, *table;
  const int32_t *rows;  // may be NULL
  int32_t *wins, *finished, *first_win, *win_moves, *reward_sum;  // each output may be NULL
  uint8_t *flags, *act_log, *flags_log, *pos_log;
  int64_t N, n_rows, step_index, board_offset;
  uint64_t seed, threshold;
  int32_t T, Tt, mc, max_steps, steps, autoreset, write_state;
  uint32_t states;
};

// tiles a lane keeps: 8, fewer where the board has fewer cells or the table's index space fewer tiles (C^T <= 65536, T <= C:
// 9^5 is the longest tuple)
template <int S, int POLICY>
constexpr int max_tiles() {
  constexpr int C = S * S;
  constexpr int cap = POLICY == TS_ROLLOUT_TABLE ? ts::kMaxTiles : TS_ROLLOUT_MAX_TILES;
  return C < cap ? C : cap;
}

template <int S, int POLICY>
__global__ __launch_bounds__(kThreads) void k_rollout(const RArgs a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr int C = BB::C;
  constexpr int MT = max_tiles<S, POLICY>();
  constexpr M kFull = C == 64 ? ~M(0) : (M(1) << (C & 63)) - 1;

  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  // lanes past the batch play a copy of the LAST board and write nothing
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  const int T = a.T, Tt = a.Tt, K = a.steps;
  const bool mc = a.mc != 0, autoreset = a.autoreset != 0;

  // ---- the board, once ----
  M blk = ts::load_obstacles<S>(a.blk, N, nl);
  blk &= kFull;
  // Loads go out UNCONDITIONALLY, all before the first one is consumed: rows past the tile (target) count read the last row,
  // results unused.  (With a predicate per row the compiler waited for every single load: 2 T + Tt dependent round trips.)
  uint32_t p[MT], in[MT], tg[kMaxTargets];  // p: the cells as they lie in memory (an id >= C stays until a step moves the board)
#pragma unroll
  for (int t = 0; t < MT; ++t) p[t] = 0, in[t] = 0;
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) tg[j] = 0;
  if (T > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t) p[t] = a.pos[(int64_t)min(t, T - 1) * N + nl];
    if (autoreset) {
#pragma unroll
      for (int t = 0; t < MT; ++t) in[t] = a.init[(int64_t)min(t, T - 1) * N + nl];
    }
  }
  if (Tt > 0) {
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j) tg[j] = a.tgt[(int64_t)min(j, Tt - 1) * N + nl];
  }
  int32_t sc = a.step_count[nl];
  uint32_t done = a.done[nl];
  M tgm = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) in[t] = min(in[t], (uint32_t)(C - 1));
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) {
    tg[j] = min(tg[j], (uint32_t)(C - 1));
    if (j < Tt) tgm |= M(1) << tg[j];
  }

  // TABLE: the board's row (ts_table_lookup's contract: a row outside the table gives no expert move and is never read)
  const uint8_t *row = nullptr;
  if constexpr (POLICY == TS_ROLLOUT_TABLE) {
    const int64_t r = a.rows ? (int64_t)a.rows[nl] : nl;
    if (r >= 0 && r < a.n_rows) row = a.table + r * (int64_t)a.states;
  }
  const uint64_t draw = (uint64_t)(a.board_offset + nl) * ts::kDrawMul;

  // build-defined Manhattan reward of the cells c[] (include/tiler_slider.h: ts_reward)
  auto manhattan = [](uint32_t x, uint32_t y) -> int {
    return abs((int)(x / S) - (int)(y / S)) + abs((int)(x % S) - (int)(y % S));
  };
  auto reward_of = [&](const uint32_t (&c)[MT]) -> int32_t {
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
  // k_table_lookup's answer from the board's own entry d0 and the entries d[] of its four successors
  auto expert_of = [](uint32_t d0, const uint32_t (&d)[4]) -> uint32_t {
    return ts::lowest_move(d0 >= 1u && d0 <= (uint32_t)TS_TABLE_MAX_DEPTH ? ts::best_moves(d0, d) : 0u);
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
        if (t < T) a.pos_log[((int64_t)k * T + t) * N + n] = (uint8_t)p[t];
    }
  };

  int32_t wins = 0, finished = 0, first_win = 0, win_moves = 0, reward_sum = 0;
  uint32_t flags = 0;
  [[maybe_unused]] uint32_t given = 0;  // GIVEN: the action byte of the step about to be played, loaded one step ahead
  if constexpr (POLICY == TS_ROLLOUT_GIVEN) given = a.actions[nl];

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

    uint32_t act;
    uint32_t q[MT];
    if constexpr (POLICY == TS_ROLLOUT_TABLE) {
      // all four successors: the table's indices, and the step itself
      uint32_t q4[4][MT], idx[4], idx0 = 0;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < T) idx0 += pc[t] * ts::pow_c<C>(t);
#pragma unroll
      for (int dir = 0; dir < 4; ++dir) {
        idx[dir] = 0;  // the successor index, in place (ts_index.h says why)
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          q4[dir][t] = pc[t];
          if (t < T) {
            q4[dir][t] = (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir);  // a cell < C whatever the board: inside the row
            idx[dir] += q4[dir][t] * ts::pow_c<C>(t);
          }
        }
      }
      uint32_t d0 = TS_TABLE_NONE, d[4] = {0, 0, 0, 0};
      if (row) {  // five reads in flight at once
        d0 = row[idx0];
#pragma unroll
        for (int dir = 0; dir < 4; ++dir) d[dir] = row[idx[dir]];
      }
      act = choose(expert_of(d0, d), draw_of(k));
      const uint32_t dir = act & 3u;
#pragma unroll
      for (int t = 0; t < MT; ++t) q[t] = dir == 0u ? q4[0][t] : dir == 1u ? q4[1][t] : dir == 2u ? q4[2][t] : q4[3][t];
    } else {
      if constexpr (POLICY == TS_ROLLOUT_GIVEN) {
        act = given;
        if (k + 1 < K) given = a.actions[(int64_t)(k + 1) * N + nl];  // in flight while this step slides
      } else {
        act = (uint32_t)(draw_of(k) >> 62);
      }
      const int dir = (int)(act & 3u);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        q[t] = pc[t];
        if (t < T) q[t] = (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir);
      }
    }

    // ---- ts_step (environment.py:100-143), the order of k_small: done on entry, bad action, slide ----
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
    } else if (act > 3u) {  // environment.py:116-117
      flags = TS_FLAG_BAD_ACTION;
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
    if (want_logs) write_logs(k, act, flags);
  }

  // ---- strict mode, every board of the wave done: what the loop would still write, without sliding ----
  if (k < K) {
    flags = TS_FLAG_STEPPED_DONE;
    if (want_reward) {
      uint32_t c[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) c[t] = min(p[t], (uint32_t)(C - 1));
      reward_sum += (K - k) * reward_of(c);
    }
    if (a.act_log) {
      uint32_t e = 255u;  // the board stands still, and so does its expert move
      if constexpr (POLICY == TS_ROLLOUT_TABLE) {
        if (row) {
          uint32_t pc[MT], idx0 = 0, d[4];
          M occ = 0;
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            pc[t] = min(p[t], (uint32_t)(C - 1));
            if (t < T) occ |= M(1) << pc[t], idx0 += pc[t] * ts::pow_c<C>(t);
          }
#pragma unroll
          for (int dir = 0; dir < 4; ++dir) {
            uint32_t idx = 0;
#pragma unroll
            for (int t = 0; t < MT; ++t)
              if (t < T) idx += (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir) * ts::pow_c<C>(t);
            d[dir] = row[idx];
          }
          e = expert_of(row[idx0], d);
        }
      }
      for (; k < K; ++k) {
        uint32_t act;
        if constexpr (POLICY == TS_ROLLOUT_GIVEN) act = a.actions[(int64_t)k * N + nl];
        else if constexpr (POLICY == TS_ROLLOUT_RANDOM) act = (uint32_t)(draw_of(k) >> 62);
        else act = choose(e, draw_of(k));
        write_logs(k, act, flags);
      }
    } else if (want_logs) {
      for (; k < K; ++k) write_logs(k, 0u, flags);
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

using Kernel = void (*)(const RArgs);

template <int P>
Kernel policy_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_rollout<s, P>; });
}
Kernel kernel_of(int S, int policy) {
  switch (policy) {
    case TS_ROLLOUT_GIVEN: return policy_kernel<TS_ROLLOUT_GIVEN>(S);
    case TS_ROLLOUT_RANDOM: return policy_kernel<TS_ROLLOUT_RANDOM>(S);
    case TS_ROLLOUT_TABLE: return policy_kernel<TS_ROLLOUT_TABLE>(S);
  }
  return nullptr;
}

bool valid_policy(int32_t p) { return p == TS_ROLLOUT_GIVEN || p == TS_ROLLOUT_RANDOM || p == TS_ROLLOUT_TABLE; }

// valid dims: does a board fit a lane's registers (and, for TABLE, the tables)?  An unknown policy has no table rule.
bool shape_supported(const ts_dims *d, int32_t policy) {
  if (d->size > TS_ROLLOUT_MAX_SIZE || d->n_tiles > TS_ROLLOUT_MAX_TILES || d->n_targets > TS_ROLLOUT_MAX_TILES) return false;
  return policy != TS_ROLLOUT_TABLE || ts::index_states(d) > 0;  // ts_table_states' rule
}

struct Plan {
  Kernel kernel = nullptr;
  uint32_t blocks = 0;
  ts_rollout_desc desc{};
};

// Every check of ts_rollout that needs no pointer of st / out, and the launch it would make; touches no device.
int32_t plan_rollout(const ts_dims *d, const ts_rollout_cfg *cfg, uint32_t out_mask, Plan &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (!cfg) return TS_ERR_NULL;
  if (!shape_supported(d, cfg->policy)) return TS_ERR_LIMIT;
  if ((cfg->mode & ~TS_MODE_AUTORESET) || !valid_policy(cfg->policy) || cfg->steps < 0 || cfg->steps > TS_ROLLOUT_MAX_STEPS ||
      cfg->explore_threshold > (1ull << 32) || cfg->n_rows < 0)
    return TS_ERR_ARG;
  p.desc.threads_per_block = kThreads;
  p.desc.lds_bytes = 0;
  if (d->n_boards == 0 || cfg->steps == 0) return TS_OK;  // nothing is launched
  const int64_t per_step = ((out_mask & TS_ROLLOUT_OUT_ACT_LOG) ? 1 : 0) + ((out_mask & TS_ROLLOUT_OUT_FLAGS_LOG) ? 1 : 0) +
                           ((out_mask & TS_ROLLOUT_OUT_POS_LOG) ? d->n_tiles : 0);
  p.desc.logged_bytes = per_step * cfg->steps * d->n_boards;
  const int64_t blocks = (d->n_boards + kThreads - 1) / kThreads;
  p.kernel = kernel_of(d->size, cfg->policy);
  if (!p.kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  p.desc.blocks = blocks;
  snprintf(p.desc.name, sizeof p.desc.name, "k_rollout<%d, %d>", d->size, cfg->policy);
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_rollout_abi_version(void) { return TS_ROLLOUT_ABI_VERSION; }
int32_t ts_rollout_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_rollout_supported(const ts_dims *dims, int32_t policy) {
  const int32_t rc = ts::check_dims(dims);
  if (rc == TS_ERR_LIMIT) return 0;
  if (rc != TS_OK) return rc;
  if (!valid_policy(policy)) return TS_ERR_ARG;
  return shape_supported(dims, policy) ? 1 : 0;
}

int32_t ts_describe_rollout(const ts_dims *dims, const ts_rollout_cfg *cfg, uint32_t out_mask, ts_rollout_desc *desc) {
  if (!dims || !cfg || !desc) return TS_ERR_NULL;
  Plan p;
  const int32_t rc = plan_rollout(dims, cfg, out_mask, p);
  if (rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_rollout(const ts_dims *dims, const ts_state *st, const ts_rollout_cfg *cfg, const ts_rollout_out *out, void *stream) {
  const uint32_t mask = !out ? 0u
                             : (out->wins ? TS_ROLLOUT_OUT_WINS : 0u) | (out->finished ? TS_ROLLOUT_OUT_FINISHED : 0u) |
                                   (out->first_win ? TS_ROLLOUT_OUT_FIRST_WIN : 0u) | (out->win_moves ? TS_ROLLOUT_OUT_WIN_MOVES : 0u) |
                                   (out->reward_sum ? TS_ROLLOUT_OUT_REWARD_SUM : 0u) | (out->flags ? TS_ROLLOUT_OUT_FLAGS : 0u) |
                                   (out->act_log ? TS_ROLLOUT_OUT_ACT_LOG : 0u) | (out->flags_log ? TS_ROLLOUT_OUT_FLAGS_LOG : 0u) |
                                   (out->pos_log ? TS_ROLLOUT_OUT_POS_LOG : 0u);
  Plan p;
  if (const int32_t rc = plan_rollout(dims, cfg, mask, p); rc != TS_OK) return rc;
  if (!p.kernel) return TS_OK;  // an empty batch or no step: nothing to launch, no pointer is looked at
  const bool autoreset = (cfg->mode & TS_MODE_AUTORESET) != 0;
  if (!st || !out || !st->blk || !st->step_count || !st->done || (dims->n_tiles > 0 && !st->pos) ||
      (dims->n_tiles > 0 && autoreset && !st->init) || (dims->n_targets > 0 && !st->tgt) ||
      (cfg->policy == TS_ROLLOUT_GIVEN && !cfg->actions) || (cfg->policy == TS_ROLLOUT_TABLE && cfg->n_rows > 0 && !cfg->table) ||
      (mask == 0u && !cfg->write_state))
    return TS_ERR_NULL;
  RArgs a{};
  a.pos = static_cast<uint8_t *>(st->pos), a.init = static_cast<const uint8_t *>(st->init), a.tgt = static_cast<const uint8_t *>(st->tgt);
  a.blk = st->blk, a.step_count = st->step_count, a.done = st->done;
  a.actions = cfg->actions, a.table = cfg->table, a.rows = cfg->rows;
  a.wins = out->wins, a.finished = out->finished, a.first_win = out->first_win, a.win_moves = out->win_moves, a.reward_sum = out->reward_sum;
  a.flags = out->flags, a.act_log = out->act_log, a.flags_log = out->flags_log, a.pos_log = static_cast<uint8_t *>(out->pos_log);
  a.N = dims->n_boards, a.n_rows = cfg->n_rows, a.step_index = cfg->step_index, a.board_offset = cfg->board_offset;
  a.seed = cfg->seed, a.threshold = cfg->explore_threshold;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.max_steps = dims->max_steps, a.steps = cfg->steps;
  a.autoreset = autoreset ? 1 : 0, a.write_state = cfg->write_state ? 1 : 0;
  a.states = cfg->policy == TS_ROLLOUT_TABLE ? (uint32_t)ts::index_states(dims) : 0u;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
