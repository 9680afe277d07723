// ts_ptable.hip — policy tables: a network's greedy play on every placement, exactly (include/tiler_slider_ptable.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_ptable.so): the other twelve libraries are pinned symbol
// by symbol and kernel by kernel, and nothing here touches any of them.
//
// Three kernel families, S = 1 .. 8 each:
//   k_ptable_actions<S>     ONE PLACEMENT PER LANE: the placements of all levels, in the order of the output, are dealt over the
//                           lanes of the grid.  A lane decodes its index into cells (ts::decode_cells), builds the static
//                           first-layer part of its level (static_preact: per lane, as k_policy_logits builds it per board - the
//                           lanes of a level read the same w1 rows, a broadcast through L2) and evaluates the network with
//                           logits_of.  Both are ts_mlp.h's, so the float operations of a placement are those of
//                           ts_policy_logits on a board standing there, in the same order: the logits are bit-equal.  The block
//                           plan (threads, staged or gathered tile-plane weights) is plan_forward_block, the policy library's.
//   k_ptable_walk_wave<S>,  ts_table.hip's round loop with ONE successor, succ(i), in place of four: three LDS bitmaps over the
//   k_ptable_walk_block<S>  index space (closed, R(d - 1), R(d)) and two control words; round d visits every open placement and
//                           resolves it to d when its successor is in R(d - 1).  The frontier lives in LDS, so no round reads
//                           what an earlier round stored to global memory; `act` is read-only here and complete before the launch.
//   k_ptable_score<S>       the wave form of k_starts_place: a group of G = 1 .. 64 lanes per level, eight integer counters per
//                           lane, summed across the group by xor shuffles.  No LDS, no atomics, no barrier.
//
// No kernel has static LDS or scratch; the host side of a launch is ts_launch.h's.
#include "../../include/tiler_slider_ptable.h"
#include "ts_mlp.h"

namespace {

using ts::kBlockThreads, ts::kMaxTiles;
constexpr int kBitmaps = 3, kCtlWords = 2;  // the walk's LDS per level, as the table build's
constexpr int kScoreColumns = TS_PTABLE_SCORE_COLUMNS;
static_assert(TS_PTABLE_FORM_NONE == ts::kFormNone && TS_PTABLE_FORM_WAVE == ts::kFormWave && TS_PTABLE_FORM_BLOCK == ts::kFormBlock);

namespace policy {
// Which form the walk takes is the table build's rule with the table build's constants (ts_table.hip: measured there, on the
// same round loop with four successors): index spaces above kWaveMaxStates take a block per level, and so do batches of fewer
// than kBlockBelowBoards levels whose index space has a placement for each of the block's 256 threads.
constexpr int64_t kWaveMaxStates = 1024;
constexpr int64_t kBlockBelowBoards = 32768;
}  // namespace policy

// ---- 1. the actions ----

struct AArgs {
  static constexpr bool kValue = false;  // no value head
  const uint8_t *tgt;
  const uint32_t *blk;
  const float *w1, *b1, *w2, *b2;
  uint8_t *act;
  float *logits;  // may be NULL
  int64_t N, total;  // total = N * states
  int32_t T, Tt, mc;
  int32_t H, slots, staged, wt_floats;
  uint32_t states;
};

template <int S>
__global__ __launch_bounds__(kMaxThreads) void k_ptable_actions(const AArgs a) {
  using M = typename ts::Bitboard<S>::mask_t;
  constexpr int C = S * S, MT = C < kMaxTiles ? C : kMaxTiles;
  stage_weights(a, C);
  const int64_t base = (int64_t)blockIdx.x * blockDim.x;  // uniform: the one 64-bit division of the block
  const int64_t q = base + threadIdx.x;
  if (q - (int64_t)(threadIdx.x & (kWave - 1)) >= a.total) return;  // wave-uniform
  // lanes past the last placement work the last placement of the last level and write nothing
  const bool live = q < a.total;
  const uint32_t states = a.states;
  const int64_t n0 = base / (int64_t)states;
  uint32_t s = (uint32_t)(base - n0 * (int64_t)states) + threadIdx.x;  // < states + 256
  const uint32_t dn = s / states;
  s -= dn * states;
  int64_t n = n0 + dn;
  if (!live) n = a.N - 1, s = states - 1u;

  Level<S> b;
  load_level<S>(a, n, b);
  Hs hs(g_lds + head_floats<AArgs::kValue>(a.H) + a.wt_floats + threadIdx.x, (int)blockDim.x);
  static_preact<S>(a, hs, b.blk, b.tgm, b.tg);

  uint32_t p[kMaxTiles];
  M occ;
  const bool valid = ts::decode_cells<S>(s, a.T, b.blk, p, occ);  // cells < C whatever the index: every weight read stays inside
  uint32_t pc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) pc[t] = p[t];
  float z[4];
  logits_of<S, MT>(a, hs, pc, z);
  // TS_POLICY_GREEDY: the lowest action among the largest logits; <= 3 whatever z holds
  const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
  const uint32_t e = z[0] == m ? 0u : z[1] == m ? 1u : z[2] == m ? 2u : 3u;
  if (!live) return;
  a.act[q] = valid ? (uint8_t)e : (uint8_t)TS_PTABLE_NO_ACTION;
  if (a.logits) reinterpret_cast<float4 *>(a.logits)[q] = valid ? make_float4(z[0], z[1], z[2], z[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- 2. the walk ----

struct WArgs {
  const uint8_t *tgt;
  const uint32_t *blk;
  const uint8_t *act;
  uint8_t *table;
  int64_t N;
  int32_t T, Tt, mc, max_depth;
  uint32_t states;
  uint32_t words;        // uint32 words per bitmap
  uint32_t board_words;  // LDS words per level: kBitmaps * words + kCtlWords
  uint32_t lanes_log2;   // wave form: log2 of the lanes per level
};

template <int S, bool BLOCK>
__device__ __forceinline__ void walk_body(const WArgs &a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr uint32_t C = BB::C;
  uint32_t *lds = reinterpret_cast<uint32_t *>(g_lds);

  const auto [G, g, grp, n, nl, live] = ts::group_of<BLOCK>(threadIdx.x, blockIdx.x, a.lanes_log2, a.N);
  (void)n;
  const int64_t N = a.N;
  const int T = a.T, Tt = a.Tt;
  const uint32_t W = a.words, states = a.states;

  uint32_t *base = lds + grp * a.board_words;
  uint32_t *closed = base, *prev = base + W, *cur = base + 2 * W, *ctl = base + kBitmaps * W;
  for (uint32_t i = g; i < a.board_words; i += G) base[i] = 0;

  M blk = ts::load_obstacles<S>(a.blk, N, nl);
  const ts::WinTest<S> is_won = ts::load_win_test<S>(a.tgt, N, nl, T, Tt, a.mc != 0);
  uint8_t *row = a.table + nl * (int64_t)states;  // written only where `live`
  const uint8_t *act = a.act + nl * (int64_t)states;

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
      if (!alive) break;  // uniform: one level per block
    } else {
      if (__builtin_amdgcn_ballot_w64(alive) == 0) break;
    }
    ++d;
    if (alive) {
      for (uint32_t s = g; s < states; s += G) {
        const uint32_t w = s >> 5, bit = 1u << (s & 31);
        if (closed[w] & bit) continue;
        const uint32_t dir = act[s];
        if (dir > 3u) continue;  // succ(s) = s, which is open: not in R(d - 1)
        uint32_t p[kMaxTiles];
        M occ;
        ts::decode_cells<S>(s, T, blk, p, occ);  // a placement: every invalid one is closed
        uint32_t idx = 0, mul = 1;               // the successor index, in place (ts_index.h says why)
#pragma unroll
        for (int t = 0; t < kMaxTiles; ++t) {
          if (t < T) {
            idx += (uint32_t)ts::slide_cell<S>((int)p[t], occ, blk, (int)dir) * mul;
            mul *= C;
          }
        }
        if ((prev[idx >> 5] >> (idx & 31)) & 1u) {  // idx == s (nothing slid) is open, so not in prev
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
__global__ __launch_bounds__(kWave) void k_ptable_walk_wave(const WArgs a) {
  walk_body<S, false>(a);
}
template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_ptable_walk_block(const WArgs a) {
  walk_body<S, true>(a);
}

// ---- 3. the score ----

struct SArgs {
  const uint32_t *blk;
  const uint8_t *ptable, *act, *table;
  int32_t *score;
  int64_t N;
  int32_t T;
  uint32_t states, lanes_log2;
};

template <int S>
__global__ __launch_bounds__(kWave) void k_ptable_score(const SArgs a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr uint32_t C = BB::C;
  const auto [G, g, grp, n, nl, live] = ts::group_of<false>(threadIdx.x, blockIdx.x, a.lanes_log2, a.N);
  (void)grp;
  const uint32_t states = a.states;
  const int T = a.T;
  const M blk = ts::load_obstacles<S>(a.blk, a.N, nl);
  const int64_t row = nl * (int64_t)states;
  const uint8_t *pt = a.ptable + row, *ac = a.act + row, *ot = a.table + row;
  constexpr uint32_t kMax = TS_TABLE_MAX_DEPTH;

  int32_t c[kScoreColumns];
#pragma unroll
  for (int k = 0; k < kScoreColumns; ++k) c[k] = 0;
  for (uint32_t s = g; s < states; s += G) {
    uint32_t cell[kMaxTiles];
    M occ;
    if (!ts::decode_cells<S>(s, T, blk, cell, occ)) continue;
    const uint32_t p = pt[s], o = ot[s], dir = ac[s];
    const bool solvable = o >= 1u && o <= kMax, solved = p >= 1u && p <= kMax;
    bool agree = false;
    if (solvable && dir <= 3u) {
      uint32_t idx = 0, mul = 1;  // the successor index, in place (ts_index.h says why); cells < C: inside the row
#pragma unroll
      for (int t = 0; t < kMaxTiles; ++t) {
        if (t < T) {
          idx += (uint32_t)ts::slide_cell<S>((int)cell[t], occ, blk, (int)dir) * mul;
          mul *= C;
        }
      }
      agree = (uint32_t)ot[idx] == o - 1u;
    }
    c[0] += 1;
    c[1] += solvable ? 1 : 0;
    c[2] += solved ? 1 : 0;
    c[3] += (solved && p == o) ? 1 : 0;
    c[4] += agree ? 1 : 0;
    c[5] += (solved && solvable) ? (int32_t)p - (int32_t)o : 0;
    c[6] += p == (uint32_t)TS_TABLE_DEEP ? 1 : 0;
    c[7] += p == 0u ? 1 : 0;
  }
  for (uint32_t o = 1; o < G; o <<= 1) {  // the lanes of a group are a power of two, aligned in the wave: xor stays inside
#pragma unroll
    for (int k = 0; k < kScoreColumns; ++k) c[k] += __shfl_xor(c[k], (int)o);
  }
  if (live && g == 0) {
#pragma unroll
    for (int k = 0; k < kScoreColumns; ++k) a.score[n * kScoreColumns + k] = c[k];
  }
}

// ---- the host side ----

using ActionsKernel = void (*)(const AArgs);
using WalkKernel = void (*)(const WArgs);
using ScoreKernel = void (*)(const SArgs);

ActionsKernel actions_kernel(int S) {
  return ts::by_size<ActionsKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> ActionsKernel { return k_ptable_actions<s>; });
}
WalkKernel walk_wave_kernel(int S) {
  return ts::by_size<WalkKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> WalkKernel { return k_ptable_walk_wave<s>; });
}
// the block form is compiled where an index space of at least kBlockThreads placements exists: every size but 1x1
WalkKernel walk_block_kernel(int S) {
  return ts::by_size<WalkKernel, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> WalkKernel { return k_ptable_walk_block<s>; });
}
ScoreKernel score_kernel(int S) {
  return ts::by_size<ScoreKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> ScoreKernel { return k_ptable_score<s>; });
}

// dims, then the shape: TS_OK where ts_ptable_supported is 1
int32_t check_shape(const ts_dims *d, int32_t hidden) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  return shape_supported(d, hidden) && ts::index_states(d) > 0 ? TS_OK : TS_ERR_LIMIT;
}

using MlpPlan = Plan<AArgs, ts_ptable_desc>;
struct ActionsPlan {
  MlpPlan m;
  int64_t states = 0, total = 0;
};

// Everything ts_ptable_actions decides before it launches; touches no device
int32_t plan_actions(const ts_dims *d, int32_t hidden, ActionsPlan &p) {
  if (const int32_t rc = check_shape(d, hidden); rc != TS_OK) return rc;
  plan_forward_block(d, hidden, p.m);
  p.states = ts::index_states(d), p.total = d->n_boards * p.states;
  ts_ptable_desc &desc = p.m.desc;
  desc.threads_per_block = (int32_t)p.m.threads, desc.lds_bytes = (int32_t)p.m.lds, desc.weights_in_lds = p.m.staged;
  desc.states = p.states;
  if (d->n_boards == 0) return TS_OK;
  const int64_t blocks = (p.total + p.m.threads - 1) / p.m.threads;
  p.m.kernel = actions_kernel(d->size);
  if (!p.m.kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.m.blocks = (uint32_t)blocks;
  desc.form = TS_PTABLE_FORM_FLAT, desc.passes = 1, desc.blocks = blocks;
  desc.lanes_per_level = (int32_t)std::min<int64_t>(p.states, p.m.threads);
  snprintf(desc.name, sizeof desc.name, "k_ptable_actions<%d>", d->size);
  return TS_OK;
}

template <class K>
void describe_plan(const ts::FormPlan<K> &f, const char *name, ts_ptable_desc &desc) {
  desc.form = f.form, desc.lanes_per_level = f.lanes_per_board, desc.threads_per_block = (int32_t)f.threads;
  desc.lds_bytes = (int32_t)f.lds;
  desc.states = f.states, desc.blocks = f.n_blocks;
  if (f.form != ts::kFormNone) {
    desc.passes = (int32_t)((f.states + f.lanes_per_board - 1) / f.lanes_per_board);
    snprintf(desc.name, sizeof desc.name, "%s", name);
  }
}

struct WalkPlan {
  ts::FormPlan<WalkKernel> f;
  ts_ptable_desc desc{};
};
int32_t plan_walk(const ts_dims *d, WalkPlan &p) {
  if (const int32_t rc = check_shape(d, 1); rc != TS_OK) return rc;
  const auto choose = [&](int64_t states, uint32_t) -> ts::FormChoice<WalkKernel> {
    const bool large = states > policy::kWaveMaxStates;
    const bool few = states >= kBlockThreads && d->n_boards < policy::kBlockBelowBoards;
    return {large || few ? walk_block_kernel(d->size) : nullptr, walk_wave_kernel(d->size), states};
  };
  if (const int32_t rc = ts::plan_forms(d, kBitmaps, kCtlWords, "k_ptable_walk", choose, p.f); rc != TS_OK) return rc;
  describe_plan(p.f, p.f.name, p.desc);
  return TS_OK;
}

struct ScorePlan {
  ts::FormPlan<ScoreKernel> f;
  ts_ptable_desc desc{};
};
int32_t plan_score(const ts_dims *d, ScorePlan &p) {
  if (const int32_t rc = check_shape(d, 1); rc != TS_OK) return rc;
  // the wave form always; a level would like a lane for each placement
  const auto choose = [&](int64_t states, uint32_t) -> ts::FormChoice<ScoreKernel> { return {nullptr, score_kernel(d->size), states}; };
  if (const int32_t rc = ts::plan_forms(d, 0, 0, "k_ptable_score", choose, p.f); rc != TS_OK) return rc;
  char name[64];
  snprintf(name, sizeof name, "k_ptable_score<%d>", d->size);
  describe_plan(p.f, name, p.desc);
  return TS_OK;
}

// [p, p + n) and [q, q + n) share a byte
bool overlaps(const void *p, const void *q, int64_t n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return n > 0 && a < b + (uintptr_t)n && b < a + (uintptr_t)n;
}

}  // namespace

extern "C" {

int32_t ts_ptable_abi_version(void) { return TS_PTABLE_ABI_VERSION; }
int32_t ts_ptable_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_ptable_supported(const ts_dims *dims, int32_t hidden) {
  const int32_t rc = supported(dims, hidden);
  return rc == 1 ? (ts::index_states(dims) > 0 ? 1 : 0) : rc;
}

int32_t ts_describe_ptable_actions(const ts_dims *dims, int32_t hidden, ts_ptable_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  ActionsPlan p;
  if (const int32_t rc = plan_actions(dims, hidden, p); rc != TS_OK) return rc;
  *desc = p.m.desc;
  return TS_OK;
}

int32_t ts_describe_ptable_walk(const ts_dims *dims, ts_ptable_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  WalkPlan p;
  if (const int32_t rc = plan_walk(dims, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_describe_ptable_score(const ts_dims *dims, ts_ptable_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  ScorePlan p;
  if (const int32_t rc = plan_score(dims, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_ptable_actions(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, uint8_t *act, float *logits, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!mlp) return TS_ERR_NULL;
  ActionsPlan p;
  if (const int32_t rc = plan_actions(dims, mlp->hidden, p); rc != TS_OK) return rc;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !act || !mlp_complete(mlp) || !st->blk || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  if ((uintptr_t)logits & 15u) return TS_ERR_ARG;
  AArgs a{};
  a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  a.w1 = mlp->w1, a.b1 = mlp->b1, a.w2 = mlp->w2, a.b2 = mlp->b2;
  a.act = act, a.logits = logits;
  a.N = dims->n_boards, a.total = p.total;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color;
  a.H = mlp->hidden, a.slots = p.m.slots, a.staged = p.m.staged, a.wt_floats = p.m.wt_floats;
  a.states = (uint32_t)p.states;
  hipLaunchKernelGGL(p.m.kernel, dim3(p.m.blocks), dim3(p.m.threads), p.m.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_ptable_walk(const ts_dims *dims, const ts_state *st, const uint8_t *act, int32_t max_depth, uint8_t *dist, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  WalkPlan p;
  if (const int32_t rc = plan_walk(dims, p); rc != TS_OK) return rc;
  if (max_depth < 0 || max_depth > TS_TABLE_MAX_DEPTH) return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !act || !dist || !st->blk || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  if (overlaps(act, dist, dims->n_boards * p.f.states)) return TS_ERR_ARG;
  WArgs a{};
  a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk, a.act = act, a.table = dist;
  a.N = dims->n_boards, a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.max_depth = max_depth;
  a.states = (uint32_t)p.f.states, a.words = p.f.words, a.board_words = p.f.board_words, a.lanes_log2 = p.f.lanes_log2;
  hipLaunchKernelGGL(p.f.kernel, dim3(p.f.blocks), dim3(p.f.threads), p.f.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_ptable_score(const ts_dims *dims, const ts_state *st, const uint8_t *ptable, const uint8_t *act, const uint8_t *table,
                        int32_t *score, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  ScorePlan p;
  if (const int32_t rc = plan_score(dims, p); rc != TS_OK) return rc;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !ptable || !act || !table || !score || !st->blk) return TS_ERR_NULL;
  if ((uintptr_t)score & 3u) return TS_ERR_ARG;
  SArgs a{};
  a.blk = st->blk, a.ptable = ptable, a.act = act, a.table = table, a.score = score;
  a.N = dims->n_boards, a.T = dims->n_tiles, a.states = (uint32_t)p.f.states, a.lanes_log2 = p.f.lanes_log2;
  hipLaunchKernelGGL(p.f.kernel, dim3(p.f.blocks), dim3(p.f.threads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
