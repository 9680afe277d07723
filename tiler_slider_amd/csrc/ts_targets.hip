// ts_targets.hip — trajectory targets: rewards, advantages, returns and expert labels of a logged trajectory
// (include/tiler_slider_targets.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_targets.so): the other six libraries are pinned symbol
// by symbol and kernel by kernel, and nothing here touches any of them.  The Manhattan reward - manhattan, reward_of - is a COPY
// of the lambdas of ts_rollout.hip, not a header both include: moving device code between files changes the pinned kernels
// (DESIGN.md section 14).  tests/test_gpu_targets.py holds this copy to the rollout's own reward_sum exactly.  The expert rule
// is ts_index.h's (best_moves, lowest_move), the one k_table_lookup and k_rollout compile.
//
// k_traj_returns<S>: ONE BOARD PER LANE, the log walked BACKWARDS in chunks of kChunk steps.  No address depends on loaded
// data, so a chunk's loads - a flag byte, T cell bytes and a value per step - are all issued before the first is consumed and
// held in registers; then the chunk's kChunk steps of the recursion run and store.  m(pos_log[k]) is m(c[k + 1]): every row of
// cells is read and reduced once, and carried to the step below it, as is V_(k + 1).  Across lanes every read and write is
// contiguous (a byte or a dword per lane).  No LDS, no barrier, no atomics: results are reproducible bit for bit.
//
// k_traj_labels<S>: ONE BOARD PER LANE, forwards in chunks of kChunk steps: the cells of a chunk are loaded together, then the
// five table indices of each of its steps are computed (the board slid in all four directions, as k_rollout's table policy
// does) and the 5 * kChunk byte reads go out together, unconditionally; ts_table_lookup's own order - the successors only once
// the board's entry is known - would cost two dependent round trips per step.  Lanes whose row lies outside the table write
// ts_table_lookup's answer for them and leave before the loop: no read of theirs is ever issued.
#include "../../include/tiler_slider_targets.h"
#include "ts_launch.h"

#include <cmath>

namespace {

using ts::kWave;
constexpr int kThreads = 256;  // four waves per block; waves never interact
constexpr int kChunk = 4;      // steps of a board whose loads are in flight together
constexpr int kMaxTargets = TS_ROLLOUT_MAX_TILES;

struct RArgs {
  const uint8_t *first, *pos_log, *flags_log, *tgt;  // cell_t = uint8 (S <= 8)
  const float *values, *last_value;
  float *reward, *adv, *ret;
  uint8_t *mask;
  int64_t N;
  int32_t T, Tt, mc, steps, vstride;
  int32_t cells, progress;  // uniform: m() is needed at all; m(c[k]) is needed beside m(pos_log[k])
  float gamma, lam, w_step, w_win, w_timeout, w_invalid, w_dist, w_progress;
};

template <int S>
constexpr int returns_tiles() {
  return S * S < TS_ROLLOUT_MAX_TILES ? S * S : TS_ROLLOUT_MAX_TILES;
}

// The whole kernel for one answer of two uniform questions - are the cells read (CELLS), are there values (VALUES) - so that the
// loads of a chunk are one straight run of code: with the questions asked per step inside the loop, every step's loads sat in
// a block of their own and were waited for there.
template <int S, bool CELLS, bool VALUES>
__device__ __forceinline__ void returns_body(const RArgs &a) {
  constexpr int C = S * S, MT = returns_tiles<S>();
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  // lanes past the batch walk a copy of the LAST board and write nothing
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  const int T = a.T, Tt = a.Tt, K = a.steps;
  const bool mc = a.mc != 0, progress = a.progress != 0;
  constexpr bool cells = CELLS;

  uint32_t tg[kMaxTargets];
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) tg[j] = 0;
  if (cells && Tt > 0) {
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j) tg[j] = a.tgt[(int64_t)min(j, Tt - 1) * N + nl];
  }
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) tg[j] = min(tg[j], (uint32_t)(C - 1));

  // ---- copied from ts_rollout.hip: the build-defined Manhattan reward of the cells c[] (include/tiler_slider.h: ts_reward) ----
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
  // ---- end of the copy ----

  // a row of cells as it lies in memory: rows past the tile count read the last row, results unused
  auto load_row = [&](const uint8_t *src, uint32_t (&c)[MT]) {
#pragma unroll
    for (int t = 0; t < MT; ++t) c[t] = src[(int64_t)min(t, T - 1) * N + nl];
  };
  auto m_of = [&](uint32_t (&c)[MT]) -> int32_t {
#pragma unroll
    for (int t = 0; t < MT; ++t) c[t] = min(c[t], (uint32_t)(C - 1));
    return reward_of(c);
  };
  // c[k]: `first`, or the row below in the log (without w_progress m(c[0]) is not used: any row that can be read)
  auto row_before = [&](int k) -> const uint8_t * {
    return k > 0 ? a.pos_log + (int64_t)(k - 1) * T * N : (progress ? a.first : a.pos_log);
  };

  const float gamma = a.gamma, gl = a.gamma * a.lam;
  int32_t m_carry = 0;  // m(pos_log[k]) of the step about to be walked
  if (cells) {
    uint32_t c[MT];
    load_row(a.pos_log + (int64_t)(K - 1) * T * N, c);
    m_carry = m_of(c);
  }
  float v_carry = a.last_value ? a.last_value[nl] : 0.0f;  // V_(k + 1)
  float adv_carry = 0.0f;                                   // A+

  for (int k0 = K - 1; k0 >= 0; k0 -= kChunk) {
    // ---- the chunk's loads, all before the first use: steps k0, k0 - 1, ...; steps below 0 read step 0 again, results unused
    uint32_t f[kChunk], c[kChunk][MT];
    float v[kChunk];
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
      const int k = max(k0 - kk, 0);
      const int64_t i = (int64_t)k * N + nl;
      f[kk] = a.flags_log[i];
      v[kk] = 0.0f;
      if constexpr (VALUES) v[kk] = a.values[i * a.vstride];
      if constexpr (CELLS) {
        load_row(row_before(k), c[kk]);
      } else {
#pragma unroll
        for (int t = 0; t < MT; ++t) c[kk][t] = 0;
      }
    }
    // ---- the recursion
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
      const int k = k0 - kk;
      if (k < 0) break;  // uniform
      const int32_t m_after = m_carry;
      const int32_t m_before = cells ? m_of(c[kk]) : 0;
      const float v_plus = v_carry;
      m_carry = m_before, v_carry = v[kk];
      const uint32_t fl = f[kk];
      const bool is_void = (fl & (TS_FLAG_STEPPED_DONE | TS_FLAG_AUTORESET | TS_FLAG_BAD_ACTION)) != 0;
      const bool end = (fl & (TS_FLAG_SUCCESS | TS_FLAG_TIMEOUT)) != 0;
      float r = a.w_step;
      r += (fl & TS_FLAG_SUCCESS) ? a.w_win : 0.0f;
      r += (fl & TS_FLAG_TIMEOUT) ? a.w_timeout : 0.0f;
      r += (fl & TS_FLAG_INVALID_MOVE) ? a.w_invalid : 0.0f;
      if (cells) {
        r = fmaf(a.w_dist, (float)m_after, r);
        if (progress) r = fmaf(a.w_progress, (float)(m_after - m_before), r);
      }
      const float delta = fmaf(gamma, end ? 0.0f : v_plus, r) - v[kk];
      const float adv = end ? delta : fmaf(gl, adv_carry, delta);
      if (!is_void) adv_carry = adv;
      if (live) {
        const int64_t i = (int64_t)k * N + n;
        if (a.reward) a.reward[i] = is_void ? 0.0f : r;
        if (a.adv) a.adv[i] = is_void ? 0.0f : adv;
        if (a.ret) a.ret[i] = is_void ? 0.0f : adv + v[kk];
        if (a.mask) a.mask[i] = is_void ? (uint8_t)0 : (uint8_t)1;
      }
    }
  }
}

template <int S>
__global__ __launch_bounds__(kThreads) void k_traj_returns(const RArgs a) {
  const bool cells = a.cells != 0 && a.T > 0;
  if (cells) {
    if (a.values) returns_body<S, true, true>(a);
    else returns_body<S, true, false>(a);
  } else {
    if (a.values) returns_body<S, false, true>(a);
    else returns_body<S, false, false>(a);
  }
}

struct LArgs {
  const uint8_t *first, *pos_log, *table;
  const uint32_t *blk;
  const int32_t *rows;  // may be NULL
  int16_t *moves;       // each output may be NULL
  uint8_t *best, *action;
  int64_t N, n_rows;
  int32_t T, steps;
  uint32_t states;
};

template <int S>
constexpr int labels_tiles() {
  return S * S < ts::kMaxTiles ? S * S : ts::kMaxTiles;
}

template <int S>
__global__ __launch_bounds__(kThreads) void k_traj_labels(const LArgs a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr int C = BB::C, MT = labels_tiles<S>();
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  const int T = a.T, K = a.steps;
  const bool successors = a.best || a.action;  // uniform: ts_table_lookup reads them for these outputs only

  const M blk = ts::load_obstacles<S>(a.blk, N, nl);  // as k_table_lookup loads it
  // ts_table_lookup's contract: a row outside the table gives -1, 0, 255 and is never read
  const uint8_t *row = nullptr;
  {
    const int64_t r = a.rows ? (int64_t)a.rows[nl] : nl;
    if (r >= 0 && r < a.n_rows) row = a.table + r * (int64_t)a.states;
  }
  if (!row) {  // these lanes leave here, so that below every lane's reads are unconditional
    if (live) {
      for (int k = 0; k < K; ++k) {
        const int64_t i = (int64_t)k * N + n;
        if (a.moves) a.moves[i] = (int16_t)TS_SOLVE_NONE;
        if (a.best) a.best[i] = 0;
        if (a.action) a.action[i] = 255;
      }
    }
    return;
  }

  for (int k0 = 0; k0 < K; k0 += kChunk) {
    // ---- the chunk's cells, all loads before the first use; steps past K read step K - 1 again, results unused
    uint32_t pc[kChunk][MT];
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
#pragma unroll
      for (int t = 0; t < MT; ++t) pc[kk][t] = 0;
    }
    if (T > 0) {
#pragma unroll
      for (int kk = 0; kk < kChunk; ++kk) {
        const int k = min(k0 + kk, K - 1);
        const uint8_t *src = k == 0 ? a.first : a.pos_log + (int64_t)(k - 1) * T * N;
#pragma unroll
        for (int t = 0; t < MT; ++t) pc[kk][t] = src[(int64_t)min(t, T - 1) * N + nl];
      }
    }
    // ---- five indices per step (clamped cells and slid cells are < C: every index stays inside the row), 5 * kChunk reads
    uint32_t d0[kChunk], d[kChunk][4], idx0[kChunk], idx[kChunk][4];
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
      idx0[kk] = 0;
      M occ = 0;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        pc[kk][t] = ts::clamp_cell(pc[kk][t], (uint32_t)C);
        if (t < T) occ |= M(1) << pc[kk][t], idx0[kk] += pc[kk][t] * ts::pow_c<C>(t);
      }
#pragma unroll
      for (int dir = 0; dir < 4; ++dir) {
        idx[kk][dir] = 0;
#pragma unroll
        for (int t = 0; t < MT; ++t)  // the successor index, in place (ts_index.h says why)
          if (t < T) idx[kk][dir] += (uint32_t)ts::slide_cell<S>((int)pc[kk][t], occ, blk, dir) * ts::pow_c<C>(t);
      }
    }
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
      d0[kk] = row[idx0[kk]];
#pragma unroll
      for (int dir = 0; dir < 4; ++dir) d[kk][dir] = 0;
    }
    if (successors) {
#pragma unroll
      for (int kk = 0; kk < kChunk; ++kk) {
#pragma unroll
        for (int dir = 0; dir < 4; ++dir) d[kk][dir] = row[idx[kk][dir]];
      }
    }
    // ---- k_table_lookup's answers
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
      const int k = k0 + kk;
      if (k >= K) break;  // uniform
      int32_t moves = TS_SOLVE_NONE;
      uint32_t best = 0;
      if (d0[kk] <= (uint32_t)TS_TABLE_MAX_DEPTH) {
        moves = (int32_t)d0[kk];
        if (d0[kk] >= 1u) best = ts::best_moves(d0[kk], d[kk]);
      } else if (d0[kk] == (uint32_t)TS_TABLE_DEEP) {
        moves = TS_SOLVE_DEPTH;
      }
      if (live) {
        const int64_t i = (int64_t)k * N + n;
        if (a.moves) a.moves[i] = (int16_t)moves;
        if (a.best) a.best[i] = (uint8_t)best;
        if (a.action) a.action[i] = (uint8_t)ts::lowest_move(best);
      }
    }
  }
}

using ReturnsKernel = void (*)(const RArgs);
using LabelsKernel = void (*)(const LArgs);

ReturnsKernel returns_kernel(int S) {
  return ts::by_size<ReturnsKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> ReturnsKernel { return k_traj_returns<s>; });
}
LabelsKernel labels_kernel(int S) {
  return ts::by_size<LabelsKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> LabelsKernel { return k_traj_labels<s>; });
}

// valid dims: ts_rollout_supported(dims, TS_ROLLOUT_RANDOM)'s rule, and ts_table_states(dims) > 0
bool returns_supported(const ts_dims *d) {
  return d->size <= TS_ROLLOUT_MAX_SIZE && d->n_tiles <= TS_ROLLOUT_MAX_TILES && d->n_targets <= TS_ROLLOUT_MAX_TILES;
}
bool labels_supported(const ts_dims *d) { return ts::index_states(d) > 0; }

bool valid_steps(int32_t steps) { return steps >= 1 && steps <= TS_ROLLOUT_MAX_STEPS; }
bool unit_interval(float x) { return x >= 0.0f && x <= 1.0f; }  // false for a NaN

constexpr uint32_t kReturnsOut = TS_RETURNS_OUT_REWARD | TS_RETURNS_OUT_ADV | TS_RETURNS_OUT_RET | TS_RETURNS_OUT_MASK;
constexpr uint32_t kReturnsIn = TS_RETURNS_IN_CELLS | TS_RETURNS_IN_FIRST | TS_RETURNS_IN_VALUES | TS_RETURNS_IN_LAST_VALUE;
constexpr uint32_t kLabelsOut = TS_LABELS_OUT_MOVES | TS_LABELS_OUT_BEST | TS_LABELS_OUT_ACTION;

struct Plan {
  uint32_t blocks = 0;  // 0: nothing is launched
  ts_targets_desc desc{};
};

// Every check that needs no pointer, after dims, and the launch a call would make
int32_t plan(const ts_dims *d, bool labels, int32_t steps, uint32_t what, Plan &p) {
  if (!(labels ? labels_supported(d) : returns_supported(d))) return TS_ERR_LIMIT;
  if (!valid_steps(steps)) return TS_ERR_ARG;
  const uint32_t outs = labels ? kLabelsOut : kReturnsOut, all = labels ? kLabelsOut : (kReturnsOut | kReturnsIn);
  if ((what & ~all) || !(what & outs)) return TS_ERR_ARG;
  p.desc.threads_per_block = kThreads;
  p.desc.lds_bytes = 0;
  p.desc.chunk_steps = kChunk;
  const int64_t N = d->n_boards, K = steps, T = d->n_tiles;
  p.desc.samples = K * N;
  if (N == 0) return TS_OK;  // nothing is launched
  const int64_t blocks = (N + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  p.desc.blocks = blocks;
  const auto bit = [&](uint32_t b) -> int64_t { return (what & b) ? 1 : 0; };
  if (labels) {
    const int64_t words = d->size * d->size > 32 ? 2 : 1;
    p.desc.bytes_read = K * T * N + K * N * (1 + 4 * (bit(TS_LABELS_OUT_BEST) | bit(TS_LABELS_OUT_ACTION))) + 4 * words * N;
    p.desc.bytes_written = K * N * (2 * bit(TS_LABELS_OUT_MOVES) + bit(TS_LABELS_OUT_BEST) + bit(TS_LABELS_OUT_ACTION));
  } else {
    const int64_t cells = bit(TS_RETURNS_IN_CELLS) | bit(TS_RETURNS_IN_FIRST);
    p.desc.bytes_read = K * N + cells * ((K + bit(TS_RETURNS_IN_FIRST)) * T * N + (int64_t)d->n_targets * N) +
                        4 * K * N * bit(TS_RETURNS_IN_VALUES) + 4 * N * bit(TS_RETURNS_IN_LAST_VALUE);
    p.desc.bytes_written =
        K * N * (4 * (bit(TS_RETURNS_OUT_REWARD) + bit(TS_RETURNS_OUT_ADV) + bit(TS_RETURNS_OUT_RET)) + bit(TS_RETURNS_OUT_MASK));
  }
  snprintf(p.desc.name, sizeof p.desc.name, labels ? "k_traj_labels<%d>" : "k_traj_returns<%d>", d->size);
  return TS_OK;
}

int32_t describe(const ts_dims *dims, bool labels, int32_t steps, uint32_t what, ts_targets_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  Plan p;
  if (const int32_t rc = plan(dims, labels, steps, what, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

bool misaligned(const void *p) { return ((uintptr_t)p & 3u) != 0; }

}  // namespace

extern "C" {

int32_t ts_targets_abi_version(void) { return TS_TARGETS_ABI_VERSION; }
int32_t ts_targets_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_targets_supported(const ts_dims *dims, int32_t which) {
  const int32_t rc = ts::check_dims(dims);
  if (rc == TS_ERR_LIMIT) return 0;
  if (rc != TS_OK) return rc;
  if (which != TS_TARGETS_RETURNS && which != TS_TARGETS_LABELS) return TS_ERR_ARG;
  return (which == TS_TARGETS_LABELS ? labels_supported(dims) : returns_supported(dims)) ? 1 : 0;
}

int32_t ts_describe_traj_returns(const ts_dims *dims, int32_t steps, uint32_t what, ts_targets_desc *desc) {
  return describe(dims, false, steps, what, desc);
}
int32_t ts_describe_traj_labels(const ts_dims *dims, int32_t steps, uint32_t what, ts_targets_desc *desc) {
  return describe(dims, true, steps, what, desc);
}

int32_t ts_traj_returns(const ts_dims *dims, const ts_state *st, const ts_returns_in *in, const ts_returns_out *out, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!in || !out) return TS_ERR_NULL;
  if (!returns_supported(dims)) return TS_ERR_LIMIT;
  if (!valid_steps(in->steps) || !unit_interval(in->gamma) || !unit_interval(in->lam) || (in->value_stride != 1 && in->value_stride != 4))
    return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  const bool progress = in->w_progress != 0.0f, cells = progress || in->w_dist != 0.0f;
  const bool tiles = dims->n_tiles > 0;
  if (!in->flags_log || (cells && tiles && !in->pos_log) || (progress && tiles && !in->first) ||
      (cells && tiles && dims->n_targets > 0 && (!st || !st->tgt)) || (!out->reward && !out->adv && !out->ret && !out->mask))
    return TS_ERR_NULL;
  if (misaligned(in->values) || misaligned(in->last_value) || misaligned(out->reward) || misaligned(out->adv) || misaligned(out->ret))
    return TS_ERR_ARG;
  const uint32_t what = (out->reward ? TS_RETURNS_OUT_REWARD : 0u) | (out->adv ? TS_RETURNS_OUT_ADV : 0u) |
                        (out->ret ? TS_RETURNS_OUT_RET : 0u) | (out->mask ? TS_RETURNS_OUT_MASK : 0u);
  Plan p;
  if (const int32_t rc = plan(dims, false, in->steps, what, p); rc != TS_OK) return rc;
  ReturnsKernel k = returns_kernel(dims->size);
  if (!k) return TS_ERR_LIMIT;
  RArgs a{};
  a.first = static_cast<const uint8_t *>(in->first), a.pos_log = static_cast<const uint8_t *>(in->pos_log), a.flags_log = in->flags_log;
  a.tgt = cells && st ? static_cast<const uint8_t *>(st->tgt) : nullptr;
  a.values = in->values, a.last_value = in->last_value;
  a.reward = out->reward, a.adv = out->adv, a.ret = out->ret, a.mask = out->mask;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.steps = in->steps, a.vstride = in->value_stride;
  a.cells = cells ? 1 : 0, a.progress = progress ? 1 : 0;
  a.gamma = in->gamma, a.lam = in->lam;
  a.w_step = in->w_step, a.w_win = in->w_win, a.w_timeout = in->w_timeout, a.w_invalid = in->w_invalid;
  a.w_dist = in->w_dist, a.w_progress = in->w_progress;
  hipLaunchKernelGGL(k, dim3(p.blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_traj_labels(const ts_dims *dims, const ts_state *st, const ts_labels_in *in, const ts_labels_out *out, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!in || !out) return TS_ERR_NULL;
  if (!labels_supported(dims)) return TS_ERR_LIMIT;
  if (!valid_steps(in->steps) || in->n_rows < 0) return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  const bool tiles = dims->n_tiles > 0;
  if (!st || !st->blk || (tiles && !in->first) || (tiles && in->steps > 1 && !in->pos_log) || (in->n_rows > 0 && !in->table) ||
      (!out->moves && !out->best && !out->action))
    return TS_ERR_NULL;
  const uint32_t what = (out->moves ? TS_LABELS_OUT_MOVES : 0u) | (out->best ? TS_LABELS_OUT_BEST : 0u) | (out->action ? TS_LABELS_OUT_ACTION : 0u);
  Plan p;
  if (const int32_t rc = plan(dims, true, in->steps, what, p); rc != TS_OK) return rc;
  LabelsKernel k = labels_kernel(dims->size);
  if (!k) return TS_ERR_LIMIT;
  LArgs a{};
  a.first = static_cast<const uint8_t *>(in->first), a.pos_log = static_cast<const uint8_t *>(in->pos_log);
  a.table = in->table, a.blk = st->blk, a.rows = in->rows;
  a.moves = out->moves, a.best = out->best, a.action = out->action;
  a.N = dims->n_boards, a.n_rows = in->n_rows, a.T = dims->n_tiles, a.steps = in->steps;
  a.states = (uint32_t)ts::index_states(dims);
  hipLaunchKernelGGL(k, dim3(p.blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
