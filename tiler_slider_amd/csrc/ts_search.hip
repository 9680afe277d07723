// ts_search.hip — on-device breadth-first solver: optimal move counts and first moves (include/tiler_slider_search.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_search.so): the step library's code object is
// pinned kernel by kernel (tests/test_kernel_instantiations.py), and nothing here touches the step path.
//
// What is searched.  A board of T tiles on S x S cells is the state  idx = sum_t cell_t * C^t  (C = S * S): one index
// per placement of the tiles IN ORDER - tile identity matters in multi-colour mode, and single-colour boards are not
// canonicalised (two orders of the same cells are two states; both are searched, the answer is the same).  The index space
// has C^T entries, at most 65,536 here, and the whole search of a board lives in LDS as seven bitmaps over it:
//     visited            every state reached so far (written between depths only)
//     cur, nxt           the frontier being expanded and the one being built (swapped after every depth)
//     first[0 .. 3]      bit s of first[a] set <=> some SHORTEST path from the root to s starts with Move a
// plus three control words (found mask, two alternating "next frontier is not empty" flags).  Nothing but the inputs and
// the two outputs is in global memory.
//
// Level-synchronous: depth d expands every state of cur by the four moves - decode, rebuild the occupancy bitboard, T calls
// of ts::slide_cell<S> per move (the arithmetic of the step kernels, ts_core.h), encode, win test (state.py:172-186) - and
// ORs each new state into nxt (ds_or) together with the first-move bits of the state it came from; a state reached twice in
// one depth collects the first moves of both parents, which is what `best` needs: every first move of every shortest solution.
// A won successor ORs its parent's first-move bits into the found mask instead.  The depth always runs to its end.
//
// Two launch forms of the same body (solve_body):
//   k_solve_wave<S>   blocks of ONE wave, so that __syncthreads() compiles to no s_barrier at all (__launch_bounds__(64): the
//                     backend lowers it to a wave barrier and the LDS wait); a board is searched by G = 1 .. 64 lanes (a
//                     power of two: one lane per bitmap word by default), 64 / G boards per wave.  The depth loop is
//                     wave-uniform: groups whose board is finished idle until the wave's last board is.
//   k_solve_block<S>  one board per block of four waves, for index spaces of thousands of words.
// The boundary between them is policy::kWaveMaxStates below.
//
// Shared with ts_table.hip and ts_rollout.hip: the index space (ts_index.h) and the host side of a launch - the checks, the
// wave-or-block plan, the error tail, the knobs (ts_launch.h).  What was measured for THIS library stays here.
#include "ts_launch.h"

namespace {

using ts::kBlockThreads, ts::kMaxTiles, ts::kWave;
// LDS of a board (ts::kMaxBlockLds bounds a block's): the largest request is one board of 65,536 states, 7 * 8 KiB + 12 B
constexpr int kBitmaps = 7, kCtlWords = 3;
static_assert(TS_SOLVE_FORM_NONE == ts::kFormNone && TS_SOLVE_FORM_WAVE == ts::kFormWave && TS_SOLVE_FORM_BLOCK == ts::kFormBlock);

namespace policy {
// Index spaces up to this size take the wave form (ts_search_tuning(TS_SOLVE_TUNE_WAVE_MAX_STATES)).  Measured, MI355X, us per
// launch, wave form / block form (profiles/solver_timing.log):
//     256 states (4x4 / 2 tiles, 1M boards)    1188 / 10807        4096 (4x4 / 3, 128k)   2070 /  3248
//     625        (5x5 / 2, 256k)                910 /  3360        6561 (3x3 / 4, 128k)   4127 /  4968
//    1296        (6x6 / 2, 128k)               1160 /  2770       15625 (5x5 / 3, 256k)  19336 / 14256
//   46656        (6x6 / 3, 16k)                8790 /  3747       65536 (4x4 / 4, 8k)    10848 /  3793
// One wave per board wins while a bitmap is a few words per lane (205 words at 6561 states: no barriers, four times the boards in
// flight); from 15625 states (489 words) on, four waves share the scan and the expansion of frontiers of hundreds of states.  No
// shape has an index space between 6561 and 15625, so the boundary sits between them.
constexpr int64_t kWaveMaxStates = 8192;
// Bitmap words per lane of the wave form (ts_search_tuning(TS_SOLVE_TUNE_WORDS_PER_LANE)): lanes per board =
// pow2ceil(ceil(words / kWordsPerLane)), at most 64.  Same log, us per launch with 1 / 2 / 4 / 8 words per lane: 4x4 / 2 tiles
// (8 words) 1188 / 1195 / 1364 / 2139; 5x5 / 2 (20 words) 910 / 906 / 795; 6x6 / 2 (41 words) 1160 / 1217.  No value wins
// everywhere; one word per lane is the best or within 13 % of it.
constexpr int64_t kWordsPerLane = 1;
}  // namespace policy

std::atomic<int64_t> g_wave_max_states{policy::kWaveMaxStates};
std::atomic<int64_t> g_words_per_lane{policy::kWordsPerLane};

struct SArgs {
  const uint8_t *pos, *tgt;  // cell_t = uint8 (S <= 8)
  const uint32_t *blk;
  int16_t *moves;
  uint8_t *best;  // may be NULL
  int64_t N;
  int32_t T, Tt, mc, max_depth;
  uint32_t words;        // uint32 words per bitmap
  uint32_t board_words;  // LDS words per board: kBitmaps * words + kCtlWords
  uint32_t lanes_log2;   // k_solve_wave: log2 of the lanes per board
};

template <int S, bool BLOCK>
__device__ __forceinline__ void solve_body(const SArgs &a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr uint32_t C = BB::C;
  extern __shared__ uint32_t lds[];

  const auto [G, g, grp, n, nl, live] = ts::group_of<BLOCK>(threadIdx.x, blockIdx.x, a.lanes_log2, a.N);
  const int64_t N = a.N;
  const int T = a.T, Tt = a.Tt;
  const uint32_t W = a.words;

  uint32_t *base = lds + grp * a.board_words;
  uint32_t *visited = base, *cur = base + W, *nxt = base + 2 * W, *first = base + 3 * W, *ctl = base + kBitmaps * W;
  for (uint32_t i = g; i < a.board_words; i += G) base[i] = 0;

  // the level and the root (cell ids clamped as the step kernels clamp them)
  M blk = ts::load_obstacles<S>(a.blk, N, nl);
  // root encode, win test and decode stay in place here: as ts_index.h's functions they changed all 12 search kernels (ts_index.h)
  uint32_t root = 0;
  M occ_root = 0;
  {
    uint32_t mul = 1;
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t) {
      if (t < T) {
        const uint32_t p = min((uint32_t)a.pos[(int64_t)t * N + nl], C - 1u);
        root += p * mul;
        mul *= C;
        occ_root |= M(1) << p;
      }
    }
  }
  // win test (state.py:172-186): multi-colour: tile i on target i for every i and T == Tt <=> the state IS the targets'
  // index; single colour: the set of tile cells equals the set of target cells
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
  auto is_won = [&](uint32_t idx, M occ) { return mc ? (mc_can_win && idx == tgt_idx) : occ == tgm; };

  int32_t result = 0;
  uint32_t best = 0;
  bool alive = live && !is_won(root, occ_root);
  __syncthreads();
  if (alive && g == 0) {
    visited[root >> 5] = 1u << (root & 31);
    cur[root >> 5] = 1u << (root & 31);
    ctl[1] = 1u;
  }
  __syncthreads();

  // ctl[0]: first-move bits of the parents of won successors; ctl[1 + (d & 1)]: the frontier of depth d is not empty
  int32_t d = 0;
  for (;;) {
    if (alive) {
      if (ctl[1 + (d & 1)] == 0u) {
        result = TS_SOLVE_NONE;
        alive = false;
      } else if (d >= a.max_depth) {
        result = TS_SOLVE_DEPTH;
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
      for (uint32_t w = g; w < W; w += G) {
        uint32_t bits = cur[w];
        while (bits) {
          const uint32_t b = (uint32_t)ts::lsb(bits);
          bits &= bits - 1u;
          const uint32_t s = w * 32u + b;
          uint32_t p[kMaxTiles];
          M occ = 0;  // decode, in place (see the root)
          {
            uint32_t r = s;
#pragma unroll
            for (int t = 0; t < kMaxTiles; ++t) {
              p[t] = 0;
              if (t < T) {
                p[t] = r % C;
                r /= C;
                occ |= M(1) << p[t];
              }
            }
          }
          uint32_t from = 0;  // first moves of the shortest paths to s
          if (d > 1) {
#pragma unroll
            for (int m = 0; m < 4; ++m) from |= ((first[m * W + w] >> b) & 1u) << m;
          }
#pragma unroll
          for (int dir = 0; dir < 4; ++dir) {
            uint32_t idx = 0, mul = 1;  // the successor index, in place (ts_index.h says why)
            M occ2 = 0;
#pragma unroll
            for (int t = 0; t < kMaxTiles; ++t) {
              if (t < T) {
                const uint32_t q = (uint32_t)ts::slide_cell<S>((int)p[t], occ, blk, dir);
                idx += q * mul;
                mul *= C;
                occ2 |= M(1) << q;
              }
            }
            if (idx == s) continue;  // nothing slid: never on a shortest path
            const uint32_t f = d == 1 ? (1u << dir) : from;
            if (is_won(idx, occ2)) {
              atomicOr(&ctl[0], f);
            } else {
              const uint32_t w2 = idx >> 5, bit = 1u << (idx & 31);
              if (!(visited[w2] & bit)) {
                atomicOr(&nxt[w2], bit);
#pragma unroll
                for (int m = 0; m < 4; ++m)
                  if (f & (1u << m)) atomicOr(&first[m * W + w2], bit);
                ctl[1 + (d & 1)] = 1u;
              }
            }
          }
        }
      }
    }
    __syncthreads();
    if (alive) {
      const uint32_t found = ctl[0];
      if (found) {
        result = d;
        best = found;
        alive = false;
      } else {
        for (uint32_t w = g; w < W; w += G) {
          const uint32_t nx = nxt[w];
          if (nx) visited[w] |= nx;
          cur[w] = 0;  // the frontier just expanded becomes the next one to build
        }
        if (g == 0) ctl[1 + ((d + 1) & 1)] = 0u;
      }
    }
    uint32_t *tmp = cur;
    cur = nxt;
    nxt = tmp;
    __syncthreads();
  }
  if (live && g == 0) {
    a.moves[n] = (int16_t)result;
    if (a.best) a.best[n] = (uint8_t)best;
  }
}

template <int S>
__global__ __launch_bounds__(kWave) void k_solve_wave(const SArgs a) {
  solve_body<S, false>(a);
}
template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_solve_block(const SArgs a) {
  solve_body<S, true>(a);
}

using SolveKernel = void (*)(const SArgs);

SolveKernel wave_kernel(int S) {
  return ts::by_size<SolveKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> SolveKernel { return k_solve_wave<s>; });
}
// the block form is compiled where an index space above policy::kWaveMaxStates exists: 9^5, 16^4, 25^3, 36^3 (49^2 and 64^2 stay below)
SolveKernel block_kernel(int S) {
  return ts::by_size<SolveKernel, 3, 4, 5, 6>(S, [](auto s) -> SolveKernel { return k_solve_block<s>; });
}

struct SolvePlan {
  ts::FormPlan<SolveKernel> f;
  SArgs a{};
  ts_solve_desc desc{};
};

// Everything ts_solve decides before it launches; touches no device (ts_describe_solve reports it).
int32_t plan_solve(const ts_dims *d, SolvePlan &p) {
  const auto choose = [&](int64_t states, uint32_t words) -> ts::FormChoice<SolveKernel> {
    const int64_t wpl = std::max<int64_t>(g_words_per_lane.load(std::memory_order_relaxed), 1);
    return {states > g_wave_max_states.load(std::memory_order_relaxed) ? block_kernel(d->size) : nullptr, wave_kernel(d->size),
            ((int64_t)words + wpl - 1) / wpl};
  };
  if (const int32_t rc = ts::plan_forms(d, kBitmaps, kCtlWords, "k_solve", choose, p.f); rc != TS_OK) return rc;
  SArgs &a = p.a;
  a.N = d->n_boards, a.T = d->n_tiles, a.Tt = d->n_targets, a.mc = d->multi_color;
  a.words = p.f.words, a.board_words = p.f.board_words, a.lanes_log2 = p.f.lanes_log2;
  ts::describe_forms(p.f, p.desc);
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_search_abi_version(void) { return TS_SEARCH_ABI_VERSION; }
int32_t ts_search_last_hip_error(void) { return ts::t_last_hip_error; }

int64_t ts_solve_states(const ts_dims *dims) { return ts::checked_states(dims); }

int32_t ts_describe_solve(const ts_dims *dims, ts_solve_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  SolvePlan p;
  const int32_t rc = plan_solve(dims, p);
  if (rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_solve(const ts_dims *dims, const ts_state *st, int32_t max_depth, int16_t *moves, uint8_t *best, void *stream) {
  if (!dims) return TS_ERR_NULL;
  SolvePlan p;
  if (const int32_t rc = plan_solve(dims, p); rc != TS_OK) return rc;
  if (max_depth < 0 || max_depth > TS_SOLVE_MAX_DEPTH) return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !moves || !st->blk || (dims->n_tiles > 0 && !st->pos) || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  p.a.pos = static_cast<const uint8_t *>(st->pos), p.a.tgt = static_cast<const uint8_t *>(st->tgt), p.a.blk = st->blk;
  p.a.moves = moves, p.a.best = best, p.a.max_depth = max_depth;
  hipLaunchKernelGGL(p.f.kernel, dim3(p.f.blocks), dim3(p.f.threads), p.f.lds, static_cast<hipStream_t>(stream), p.a);
  return ts::finish_launch();
}

int64_t ts_search_tuning(int32_t key, int64_t value) {
  std::atomic<int64_t> *knob = key == TS_SOLVE_TUNE_WAVE_MAX_STATES ? &g_wave_max_states : key == TS_SOLVE_TUNE_WORDS_PER_LANE ? &g_words_per_lane : nullptr;
  return ts::tune(knob, value);
}

}  // extern "C"
