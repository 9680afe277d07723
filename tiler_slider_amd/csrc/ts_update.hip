// ts_update.hip — the in-place step: ts_step with the observation updated where it changes (include/tiler_slider_update.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_update.so): the step library is pinned symbol by
// symbol and kernel by kernel, and nothing here touches it.
//
// k_step_update<S, TMAX, U8>: ONE BOARD PER LANE, no LDS, no scratch, no barrier.  The lane loads its board - the level
// (obstacle bitboard, target cells, in auto-reset mode the initial cells), the dynamic state (tile cells, step counter, done
// latch), the action byte and the cells the observation displays (`shown`) - with every load issued before the first is
// consumed (rows past the tile / target count read the last row, results unused: a predicate per row costs a memory round
// trip per row, ts_rollout.hip), plays one step with the arithmetic of ts_core.h in the order of k_small, and stores the state
// as ts_step does.  Tiles live in a register array of TMAX (2 or 8) walked by fully unrolled loops predicated on t < T (T is
// uniform, so the predicates are scalar branches).
//
// The observation is never written as a whole: for every cell a tile leaves or enters, the channel-1 value under the old
// cells (`shown`) and under the new ones is evaluated, and the new value is stored where they differ - one scattered 4-byte
// (float32) or 1-byte (uint8) store per changed cell.  Most boards store nothing or two cells.
#include "../../include/tiler_slider_update.h"
#include "ts_launch.h"

namespace {

using ts::kWave;
constexpr int kThreads = 256;  // four waves per block; waves never interact
constexpr int64_t kInfinityCacheBytes = 256ll << 20;

struct UArgs {
  uint8_t *pos, *shown;  // cell_t = uint8 (S <= 8)
  const uint8_t *init, *tgt;
  const uint32_t *blk;
  int32_t *step_count;
  uint8_t *done;
  const uint8_t *actions;
  uint8_t *flags;
  int32_t *reward;  // may be NULL
  float *obs;       // one of obs / obs_u8, by the kernel's U8
  uint8_t *obs_u8;
  int64_t N;
  int32_t T, Tt, mc, max_steps, autoreset;
};

// The scattered observation stores.  Plain stores leave the touched lines dirty in the XCD's L2 until the end of the kernel;
// -DTS_UPDATE_STORE_SC1 builds the agent-scope flavour (written through the L2) for the A/B of profiles/update_timing.md.
__device__ __forceinline__ void put(float *dst, uint32_t v) {
#if defined(TS_UPDATE_STORE_SC1)
  asm volatile("global_store_dword %0, %1, off sc1" ::"v"(dst), "v"((float)v) : "memory");
#else
  *dst = (float)v;
#endif
}
__device__ __forceinline__ void put(uint8_t *dst, uint32_t v) {
#if defined(TS_UPDATE_STORE_SC1)
  asm volatile("global_store_byte %0, %1, off sc1" ::"v"(dst), "v"(v) : "memory");
#else
  *dst = (uint8_t)v;
#endif
}

template <int S, int TMAX, bool U8>
__global__ __launch_bounds__(kThreads) void k_step_update(const UArgs a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr int C = BB::C;
  constexpr int MT = C < TMAX ? C : TMAX;  // tiles a lane keeps (T <= C)
  constexpr M kFull = C == 64 ? ~M(0) : (M(1) << (C & 63)) - 1;

  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  // lanes past the batch play a copy of the LAST board and write nothing
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  const int T = a.T, Tt = a.Tt;  // 1 <= T <= MT, Tt <= TMAX
  const bool mc = a.mc != 0, autoreset = a.autoreset != 0;

  // ---- loads: all unconditional, all issued before the first one is consumed ----
  const M blk = ts::load_obstacles<S>(a.blk, N, nl) & kFull;
  uint32_t p[MT], sh[MT], in[MT], tg[TMAX];  // p: the cells as they lie in memory (an id >= C stays until the board moves)
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    p[t] = a.pos[(int64_t)min(t, T - 1) * N + nl];
    sh[t] = a.shown[(int64_t)min(t, T - 1) * N + nl];
    in[t] = 0;
  }
  if (autoreset) {
#pragma unroll
    for (int t = 0; t < MT; ++t) in[t] = a.init[(int64_t)min(t, T - 1) * N + nl];
  }
#pragma unroll
  for (int j = 0; j < TMAX; ++j) tg[j] = 0;
  if (Tt > 0) {
#pragma unroll
    for (int j = 0; j < TMAX; ++j) tg[j] = a.tgt[(int64_t)min(j, Tt - 1) * N + nl];
  }
  int32_t sc = a.step_count[nl];
  uint32_t done = a.done[nl];
  const uint32_t act = a.actions[nl];

  // ---- the step (environment.py:100-143), the order of k_small: done on entry, bad action, slide ----
  M tgm = 0, occ = 0;
  uint32_t pc[MT];
#pragma unroll
  for (int j = 0; j < TMAX; ++j) {
    tg[j] = min(tg[j], (uint32_t)(C - 1));
    if (j < Tt) tgm |= M(1) << tg[j];
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    pc[t] = min(p[t], (uint32_t)(C - 1));  // clamp: malformed ids stay in-board
    if (t < T) occ |= M(1) << pc[t];
  }
  const int dir = (int)(act & 3u);
  uint32_t q[MT];
  bool same = true, ordered = T == Tt;
  M occ2 = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    q[t] = pc[t];
    if (t < T) {
      q[t] = (uint32_t)ts::slide_cell<S>((int)pc[t], occ, blk, dir);
      same &= q[t] == pc[t];
      ordered &= q[t] == tg[t];  // MT <= TMAX
      occ2 |= M(1) << q[t];
    }
  }
  const bool won = mc ? ordered : (occ2 == tgm);  // state.py:172-186
  uint32_t flags;
  bool touched = true;  // a board the step leaves untouched keeps every state byte
  uint32_t r[MT];       // the cells after the step, as they will lie in memory
  if (done) {           // environment.py:113-114
    flags = autoreset ? TS_FLAG_AUTORESET : TS_FLAG_STEPPED_DONE;
    touched = autoreset;
#pragma unroll
    for (int t = 0; t < MT; ++t) r[t] = autoreset ? min(in[t], (uint32_t)(C - 1)) : p[t];
    if (autoreset) sc = 0, done = 0;
  } else if (act > 3u) {  // environment.py:116-117
    flags = TS_FLAG_BAD_ACTION;
    touched = false;
#pragma unroll
    for (int t = 0; t < MT; ++t) r[t] = p[t];
  } else {
    flags = (won ? (TS_FLAG_IS_WON | TS_FLAG_SUCCESS) : 0u) | (same ? TS_FLAG_INVALID_MOVE : 0u);
    sc += 1;
    done = won ? 1u : 0u;
    if (sc >= a.max_steps) {
      done = 1u;
      flags |= TS_FLAG_TIMEOUT;
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) r[t] = q[t];
  }

  // ---- the observation delta: old cells = shown, new cells = r, both clamped as the encoder clamps ----
  uint32_t o[MT], c[MT];
  M occ_new = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    o[t] = min(sh[t], (uint32_t)(C - 1));
    c[t] = min(r[t], (uint32_t)(C - 1));
    if (t < T) occ_new |= M(1) << c[t];
  }
  using obs_t = typename std::conditional<U8, uint8_t, float>::type;
  obs_t *mine;  // channel 1 of cell 0 of this board
  if constexpr (U8) mine = a.obs_u8 + (n * C * 3 + 1);
  else mine = a.obs + (n * C * 3 + 1);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t < T) {
      // the cell tile t stands on: the highest index on it wins, before and after (ascending u: the last match stays)
      uint32_t nv = 0, ov = 0;
#pragma unroll
      for (int u = 0; u < MT; ++u) {
        if (u < T) {
          nv = c[u] == c[t] ? (uint32_t)(u + 1) : nv;
          ov = o[u] == c[t] ? (uint32_t)(u + 1) : ov;
        }
      }
      if (!mc) nv = nv ? 1u : 0u, ov = ov ? 1u : 0u;
      if (live && nv != ov) put(mine + 3 * c[t], nv);
      // the cell it was drawn on, where no tile stands any more (else the line above stores that cell's value)
      if (live && !((occ_new >> o[t]) & M(1))) put(mine + 3 * o[t], 0u);
    }
  }

  // ---- build-defined Manhattan reward of the cells after the step (include/tiler_slider.h: ts_reward) ----
  if (a.reward) {  // uniform
    auto manhattan = [](uint32_t x, uint32_t y) -> int {
      return abs((int)(x / S) - (int)(y / S)) + abs((int)(x % S) - (int)(y % S));
    };
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
          for (int j = 0; j < TMAX; ++j)
            if (j < Tt) best = min(best, manhattan(c[t], tg[j]));
          sum += best;
        }
      }
    }
    if (live) a.reward[n] = -sum;
  }

  if (!live) return;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t < T) {
      if (touched) a.pos[(int64_t)t * N + n] = (uint8_t)r[t];
      if (r[t] != sh[t]) a.shown[(int64_t)t * N + n] = (uint8_t)r[t];
    }
  }
  if (touched) {
    a.step_count[n] = sc;
    a.done[n] = (uint8_t)done;
  }
  a.flags[n] = (uint8_t)flags;
}

using Kernel = void (*)(const UArgs);

template <int TMAX, bool U8>
Kernel sized_kernel(int S) {
  return ts::by_size<Kernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> Kernel { return k_step_update<s, TMAX, U8>; });
}
Kernel kernel_of(int S, int tmax, bool u8) {
  if (tmax == 2) return u8 ? sized_kernel<2, true>(S) : sized_kernel<2, false>(S);
  return u8 ? sized_kernel<8, true>(S) : sized_kernel<8, false>(S);
}

constexpr uint32_t kKnownOutputs = TS_OUT_OBS | TS_OUT_REWARD | TS_OUT_ONEHOT | TS_OUT_VALID | TS_OUT_OBS_U8 | TS_OUT_VALID4 | TS_OUT_FLAGS;

// dims have passed check_dims: the shape, then the outputs
int32_t check_supported(const ts_dims *d, uint32_t outputs) {
  if (d->size > TS_UPDATE_MAX_SIZE || d->n_tiles < 1 || d->n_tiles > TS_UPDATE_MAX_TILES || d->n_targets > TS_UPDATE_MAX_TILES) return TS_ERR_LIMIT;
  const bool f32 = (outputs & TS_OUT_OBS) != 0, u8 = (outputs & TS_OUT_OBS_U8) != 0;
  if ((outputs & ~kKnownOutputs) || (outputs & (TS_OUT_ONEHOT | TS_OUT_VALID | TS_OUT_VALID4)) || f32 == u8) return TS_ERR_ARG;
  return TS_OK;
}

struct Plan {
  Kernel kernel = nullptr;
  uint32_t blocks = 0;
  ts_launch_desc desc{};
};

// Every check of ts_step_update that needs no pointer, and the launch it would make; touches no device.
int32_t plan_update(const ts_dims *d, uint32_t outputs, Plan &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (const int32_t rc = check_supported(d, outputs); rc != TS_OK) return rc;
  const bool u8 = (outputs & TS_OUT_OBS_U8) != 0;
  const int tmax = (d->n_tiles <= 2 && d->n_targets <= 2) ? 2 : 8;
  ts_launch_desc &k = p.desc;
  k.kernel = TS_KERNEL_NONE;
  k.lanes_per_board = k.boards_per_lane = 1;
  k.boards_per_wave = kWave;
  k.tiles_per_lane = tmax;
  k.extras = (outputs & TS_OUT_REWARD) ? 1 : 0;
  k.xcd_piece = -1;
  k.waves_per_block = kThreads / kWave;
  k.output_bytes = k.resident_bytes = (int64_t)(u8 ? 3 : 12) * d->size * d->size * d->n_boards;
  k.out_of_cache = k.resident_bytes > kInfinityCacheBytes ? 1 : 0;
  if (d->n_boards == 0) return TS_OK;  // nothing is launched
  const int64_t blocks = (d->n_boards + kThreads - 1) / kThreads;
  p.kernel = kernel_of(d->size, tmax, u8);
  if (!p.kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  k.kernel = TS_KERNEL_UPDATE;
  k.blocks = blocks;
  snprintf(k.name, sizeof k.name, "k_step_update<%d, %d, %s>", d->size, tmax, u8 ? "true" : "false");
  return TS_OK;
}

uint32_t outputs_of(const ts_step_out *out) {
  return (out->obs ? TS_OUT_OBS : 0u) | (out->reward ? TS_OUT_REWARD : 0u) | (out->onehot ? TS_OUT_ONEHOT : 0u) |
         (out->valid ? TS_OUT_VALID : 0u) | (out->obs_u8 ? TS_OUT_OBS_U8 : 0u) | (out->valid4 ? TS_OUT_VALID4 : 0u) |
         (out->flags ? TS_OUT_FLAGS : 0u);
}

}  // namespace

extern "C" {

int32_t ts_update_abi_version(void) { return TS_UPDATE_ABI_VERSION; }
int32_t ts_update_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_update_supported(const ts_dims *dims, uint32_t outputs) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  return check_supported(dims, outputs);
}

int32_t ts_describe_step_update(const ts_dims *dims, uint32_t outputs, ts_launch_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  Plan p;
  if (const int32_t rc = plan_update(dims, outputs, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_step_update(const ts_dims *dims, const ts_state *st, const uint8_t *actions, uint32_t mode, const ts_step_out *out,
                       void *shown, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!out) return TS_ERR_NULL;
  Plan p;
  if (const int32_t rc = plan_update(dims, outputs_of(out), p); rc != TS_OK) return rc;
  if (mode & ~TS_MODE_AUTORESET) return TS_ERR_ARG;
  if (!p.kernel) return TS_OK;  // an empty batch: nothing to launch, no pointer is looked at
  const bool autoreset = (mode & TS_MODE_AUTORESET) != 0;
  if (!st || !st->pos || !st->blk || !st->step_count || !st->done || (autoreset && !st->init) || (dims->n_targets > 0 && !st->tgt) ||
      !actions || !out->flags || !shown)
    return TS_ERR_NULL;
  if ((((uintptr_t)out->obs) | ((uintptr_t)out->reward)) & 3u) return TS_ERR_ARG;
  UArgs a{};
  a.pos = static_cast<uint8_t *>(st->pos), a.shown = static_cast<uint8_t *>(shown);
  a.init = static_cast<const uint8_t *>(st->init), a.tgt = static_cast<const uint8_t *>(st->tgt);
  a.blk = st->blk, a.step_count = st->step_count, a.done = st->done, a.actions = actions;
  a.flags = out->flags, a.reward = out->reward, a.obs = out->obs, a.obs_u8 = out->obs_u8;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.max_steps = dims->max_steps, a.autoreset = autoreset ? 1 : 0;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
