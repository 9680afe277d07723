// ts_rptable.hip — reach policy tables: a network's greedy play on every state of a reachable distance table, the walk of an
// action table over those states, and its integer score against the optimal table (include/tiler_slider_rptable.h, which defines
// all three).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_rptable.so): no existing code object is rebuilt.  The
// network - stage_weights, static_preact, logits_of - is ts_mlp.h's, shared with the policy, train, actor-critic and policy-table
// libraries; moves are ts_core.h's, the host side of a launch ts_launch.h's.  The slot format, the home function and the probe of
// tiler_slider_rtable.h are restated here on 64-bit keys, as ts_rtable.hip and ts_rstarts.hip restate them.
//
// Every kernel takes min(L, 1024) blocks, block b the levels b, b + gridDim.x, ..., as k_rtable_build does.
//   k_rptable_actions<S>      A row is at most half occupied and usually far less, so a lane per slot would evaluate a network
//                             on a few lanes of each wave.  The block reads the row 1,024 slots at a time: a slot that is not
//                             live gets its 255 / 0.0f rows there and then (coalesced), a live one takes a ticket - one LDS
//                             atomic per wave and pass, the lanes' offsets from the ballot - and goes into a list in LDS.
//                             Whenever the list holds a block of states they are dealt over the lanes, one each, and evaluated
//                             with logits_of; the rest of a row is evaluated at its end.  All lanes of a block work one level, so
//                             static_preact builds the same column in every lane - the float operations of a state are those of
//                             ts_policy_logits on a board standing there, in the same order.  The block plan is the policy
//                             library's with the list beside it; everything lies in the dynamic region, whose base stays
//                             16-byte aligned for the float4 reads of the second layer.
//   k_rptable_walk<S, false>  Rows of at most kLdsSlots slots.  Scan: the live slots go into a list (uint16) and their entries
//                             (uint8, by slot) start at TS_TABLE_NONE.  Then succ is resolved once per live slot, dealt densely
//                             over the lanes: one move, one probe.  Then the rounds of ts_rtable.hip over the list: a round only
//                             tests for d - 1 and only writes d, and neither NONE nor d is d - 1, so one copy of the entries is
//                             enough and what a racing lane reads does not matter.  A lane owns every 256th position of the list
//                             and packs what it has not resolved to the front of them, so a round visits the unresolved
//                             states only.  The final pass re-reads the row for the keys.
//   k_rptable_walk<S, true>   Rows above that.  There is no workspace, so the pairs live in the output row: a live slot holds
//                             bit 63 | entry << 48 | succ (32 bits) during the rounds, which run over the whole row - `slots`
//                             reads a round, up to 252 rounds: the cost of a capacity above 4,096 on a deep level.  The row is
//                             touched by four waves of one block: every access to it is a relaxed agent-scope atomic and every
//                             barrier is preceded by s_waitcnt vmcnt(0) (ts_rtable.hip's reading of the memory model).
//   k_rptable_score<S>        A lane per slot and pass, eight integer counters per lane, summed by xor shuffles in the wave and
//                             through 32 words of LDS across the four waves.  No atomics.
// The walk and the score hold no float instruction; no kernel has scratch.
#include "../../include/tiler_slider_rptable.h"
#include "ts_mlp.h"

namespace {

using ts::kBlockThreads;
constexpr int kTiles = TS_REACH_MAX_TILES;
constexpr int64_t kMaxBlocks = 1024;  // four blocks of four waves on each of 256 CUs
constexpr int kScoreColumns = TS_PTABLE_SCORE_COLUMNS;
static_assert(kScoreColumns == 8 && kMaxTilesLane == kTiles);

constexpr uint64_t kOcc = 1ull << 63, kKeyMask = (1ull << 48) - 1;
constexpr int kEntryShift = 48;
constexpr uint32_t kWon = 0xffffffffu;  // succ: the board after the move is won
constexpr uint32_t kNone = TS_TABLE_NONE, kDeep = TS_TABLE_DEEP, kMaxDepth = TS_TABLE_MAX_DEPTH;

// the actions: slots of a pass, and the list behind the hs columns: a pass on top of less than a block, and two tickets
constexpr uint32_t kPass = 1024;
constexpr uint32_t kListWords = kPass + kMaxThreads;
constexpr size_t kListBytes = (kListWords + 4u) * 4u;
static_assert(kPass % kMaxThreads == 0 && kListBytes % 16u == 0);
// the walk in LDS: an entry byte, a list word and a successor word per slot
constexpr uint32_t kLdsSlots = 8192;
constexpr uint32_t kWon16 = 0xffffu;
static_assert(kLdsSlots < kWon16);

__device__ __forceinline__ uint64_t ld64(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st64(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// what this wave stored has arrived, then the block's barrier
__device__ __forceinline__ void block_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
__device__ __forceinline__ uint32_t entry_of(uint64_t e) { return (uint32_t)(e >> kEntryShift) & 0xffu; }
__device__ __forceinline__ uint32_t home_of(uint64_t key, uint32_t slots_log2) {
  return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 32) >> (32u - slots_log2);
}
// an entry as ts_table_lookup maps it
__device__ __forceinline__ int32_t moves_of(uint32_t entry) {
  return entry >= 1u && entry <= kMaxDepth ? (int32_t)entry : entry == kDeep ? TS_SOLVE_DEPTH : TS_SOLVE_NONE;
}

// the slot of `key` in a row, `held` false where the row does not hold it: at most `slots` reads, all inside the row
__device__ __forceinline__ uint32_t probe_row(const uint64_t *row, uint32_t slots, uint32_t slots_log2, uint64_t key, bool &held) {
  const uint32_t mask = slots - 1u;
  uint32_t slot = home_of(key, slots_log2) & mask;
  held = false;
  for (uint32_t probe = 0; probe < slots; ++probe, slot = (slot + 1u) & mask) {
    const uint64_t e = row[slot];
    if (e == 0) return 0;
    if ((e & kOcc) && (e & kKeyMask) == key) {
      held = true;
      return slot;
    }
  }
  return 0;
}

// A level as every lane of a block holds it: obstacles and the win test on a 64-bit key (ts_rtable.hip's).
template <int S>
struct RLevel {
  using M = typename ts::Bitboard<S>::mask_t;
  static constexpr uint32_t C = ts::Bitboard<S>::C;
  M blk = 0, tgm = 0;
  uint64_t tgt_key = 0;
  bool mc = false, mc_can_win = false;
  __device__ __forceinline__ bool won(uint64_t key, M occ) const { return mc ? (mc_can_win && key == tgt_key) : occ == tgm; }
};
template <int S>
__device__ __forceinline__ RLevel<S> load_rlevel(const uint32_t *blk, const uint8_t *tgt, int64_t N, int64_t n, int T, int Tt, bool mc) {
  using M = typename RLevel<S>::M;
  RLevel<S> L;
  L.blk = ts::load_obstacles<S>(blk, N, n);
  uint64_t mul = 1;
  for (int j = 0; j < Tt; ++j) {
    const uint32_t tj = ts::clamp_cell(tgt[(int64_t)j * N + n], RLevel<S>::C);
    L.tgm |= M(1) << tj;
    if (j < T) {
      L.tgt_key += tj * mul;
      mul *= RLevel<S>::C;
    }
  }
  L.mc = mc, L.mc_can_win = T == Tt;
  return L;
}
// the cells of a key, each below C whatever bits the key holds: the key splits into two halves of four tiles
template <int S>
__device__ __forceinline__ void decode_key(uint64_t key, int T, uint32_t (&p)[kTiles], typename RLevel<S>::M &occ) {
  using M = typename RLevel<S>::M;
  constexpr uint32_t C = RLevel<S>::C;
  constexpr uint64_t C4 = (uint64_t)C * C * C * C;
  using Hi = std::conditional_t<(S <= 3), uint64_t, uint32_t>;  // key / C^4 of any 48-bit key: below 2^32 from 4x4 on
  uint32_t lo = (uint32_t)(key % C4);
  Hi hi = (Hi)(key / C4);
  occ = 0;
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    p[t] = 0;
    if (t < T) {
      if (t < 4) p[t] = lo % C, lo /= C;
      else p[t] = (uint32_t)(hi % C), hi /= C;
      occ |= M(1) << p[t];
    }
  }
}
// the key and the occupancy of the board one slide on
template <int S>
__device__ __forceinline__ uint64_t slide_key(const uint32_t (&p)[kTiles], typename RLevel<S>::M occ, typename RLevel<S>::M blk, int T, int dir,
                                               typename RLevel<S>::M &occ2) {
  using M = typename RLevel<S>::M;
  uint64_t key = 0, mul = 1;
  occ2 = 0;
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    if (t < T) {
      const uint32_t q = (uint32_t)ts::slide_cell<S>((int)p[t], occ, blk, dir);
      key += q * mul;
      mul *= RLevel<S>::C;
      occ2 |= M(1) << q;
    }
  }
  return key;
}
// the key of the root cells of board n as they lie in memory (clamped), and whether it is won
template <int S>
__device__ __forceinline__ uint64_t root_key(const RLevel<S> &L, const uint8_t *cells, int64_t N, int64_t n, int T, bool &won) {
  using M = typename RLevel<S>::M;
  uint64_t key = 0, mul = 1;
  M occ = 0;
  for (int t = 0; t < T; ++t) {
    const uint32_t c = ts::clamp_cell(cells[(int64_t)t * N + n], RLevel<S>::C);
    key += c * mul;
    mul *= RLevel<S>::C;
    occ |= M(1) << c;
  }
  won = L.won(key, occ);
  return key;
}
// succ of the live slot `i` holding `key` under move `dir` <= 3: kWon, or a slot of the row
template <int S>
__device__ __forceinline__ uint32_t succ_of(const RLevel<S> &L, const uint64_t *row, uint32_t slots, uint32_t slots_log2, uint32_t i, uint64_t key,
                                            int dir, int T) {
  using M = typename RLevel<S>::M;
  uint32_t p[kTiles];
  M occ, occ2;
  decode_key<S>(key, T, p, occ);
  const uint64_t next = slide_key<S>(p, occ, L.blk, T, dir, occ2);
  // (where nothing slid the probe finds i itself in a built row; over arbitrary bits the definition is still the probe's answer)
  if (L.won(next, occ2)) return kWon;
  bool held;
  const uint32_t slot = probe_row(row, slots, slots_log2, next, held);
  return held ? slot : i;
}

// the ticket of every lane that votes: one LDS atomic per wave, the lanes' offsets from the ballot; every lane of the wave calls it
__device__ __forceinline__ uint32_t ticket_of(bool vote, uint32_t *counter, uint32_t lane) {
  const uint64_t votes = __ballot(vote);
  if (votes == 0) return 0;  // the same for every lane of the wave
  uint32_t start = 0;
  if (lane == 0) start = atomicAdd(counter, (uint32_t)__popcll(votes));
  start = (uint32_t)__shfl((int)start, 0);
  return start + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
}

// ---- 1. the actions ----

struct AArgs {
  static constexpr bool kValue = false;  // no value head
  const uint8_t *tgt;
  const uint32_t *blk;
  const float *w1, *b1, *w2, *b2;
  const uint64_t *table;
  const int32_t *count;
  uint8_t *act;
  float *logits;  // may be NULL
  int64_t N;
  int32_t T, Tt, mc;
  int32_t H, slots, staged, wt_floats;  // slots: the tile-plane features T' * S*S of ts_mlp.h
  uint32_t row_slots;
};

template <int S>
__global__ __launch_bounds__(kMaxThreads) void k_rptable_actions(const AArgs a) {
  using M = typename ts::Bitboard<S>::mask_t;
  constexpr int C = S * S, MT = max_tiles<S>();
  stage_weights(a, C);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, threads = blockDim.x;
  float *hs_base = g_lds + head_floats<AArgs::kValue>(a.H) + a.wt_floats;
  Hs hs(hs_base + tid, (int)threads);
  uint32_t *list = reinterpret_cast<uint32_t *>(hs_base + a.H * (int)threads);
  uint32_t *ctl = list + kListWords;  // [0], [1]: the tickets of even and odd passes
  const uint32_t slots = a.row_slots;

  for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
    Level<S> b;
    load_level<S>(a, n, b);
    static_preact<S>(a, hs, b.blk, b.tgm, b.tg);
    const bool open = a.count[n] >= 0;
    const uint64_t *row = a.table + n * (int64_t)slots;
    uint8_t *act = a.act + n * (int64_t)slots;
    float4 *logits = a.logits ? reinterpret_cast<float4 *>(a.logits) + n * (int64_t)slots : nullptr;

    // the network on the state of a live slot
    auto evaluate = [&](uint32_t slot) {
      uint32_t p[kTiles];
      M occ;
      decode_key<S>(row[slot] & kKeyMask, a.T, p, occ);  // cells < C whatever the key: every weight read stays inside
      uint32_t pc[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) pc[t] = p[t];
      float z[4];
      logits_of<S, MT>(a, hs, pc, z);
      // TS_POLICY_GREEDY: the lowest action among the largest logits; <= 3 whatever z holds
      const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
      const uint32_t e = z[0] == m ? 0u : z[1] == m ? 1u : z[2] == m ? 2u : 3u;
      act[slot] = (uint8_t)e;
      if (logits) logits[slot] = make_float4(z[0], z[1], z[2], z[3]);
    };

    if (tid == 0) ctl[0] = 0u, ctl[1] = 0u;
    __syncthreads();
    uint32_t held = 0;  // states in the list, the same in every lane; below `threads` between two passes
    for (uint32_t base = 0, pass = 0; base < slots; base += kPass, ++pass) {
      uint32_t *tickets = &ctl[pass & 1u];
      for (uint32_t i = tid; i < kPass; i += threads) {
        const uint32_t slot = base + i;
        const bool in = slot < slots;
        const bool live = open && in && (row[slot] & kOcc) != 0;
        if (in && !live) {
          act[slot] = (uint8_t)TS_RPTABLE_NO_ACTION;
          if (logits) logits[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        const uint32_t ticket = ticket_of(live, tickets, lane);
        if (live) list[held + ticket] = slot;  // held + ticket < threads + kPass
      }
      __syncthreads();
      held += *tickets;
      if (tid == 0) ctl[(pass + 1u) & 1u] = 0u;  // the next pass's: last read before the second barrier of the pass before
      while (held >= threads) {
        held -= threads;
        evaluate(list[held + tid]);
      }
      __syncthreads();  // the list above `held` is the next pass's
    }
    if (tid < held) evaluate(list[tid]);
    __syncthreads();  // list and ctl are the next level's
  }
}

// ---- 2. the walk ----

struct WArgs {
  const uint8_t *root, *tgt;  // cell_t = uint8 (S <= 8); root: st->init or st->pos, NULL where root_moves is not asked for
  const uint32_t *blk;
  const uint64_t *table;
  const int32_t *count;
  const uint8_t *act;
  uint64_t *out;
  int16_t *root_moves;  // may be NULL
  int32_t *deepest;     // may be NULL
  int64_t N;
  uint32_t slots, slots_log2;
  int32_t T, Tt, mc, max_depth;
};

// the walk's LDS: the list's tickets and the counters of rounds d % 3 == 0, 1, 2; in the LDS form also the list of the live slots,
// succ by position in the list, and the entries by slot
template <bool GLOBAL>
struct WalkLds {
  uint32_t ctl[4];
  uint16_t lst[kLdsSlots], suc[kLdsSlots];
  uint8_t ent[kLdsSlots];
};
template <>
struct WalkLds<true> {
  uint32_t ctl[4];
};
constexpr uint32_t kWalkLdsBytes = 16u + 5u * kLdsSlots;
static_assert(sizeof(WalkLds<false>) == kWalkLdsBytes);

template <int S, bool GLOBAL>
__global__ __launch_bounds__(kBlockThreads) void k_rptable_walk(const WArgs a) {
  __shared__ WalkLds<GLOBAL> lds;
  uint32_t(&ctl)[4] = lds.ctl;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  (void)lane;
  const uint32_t slots = a.slots, log2 = a.slots_log2;
  const int T = a.T;
  const int64_t N = a.N;
  constexpr uint64_t kEntryMask = 0xffull << kEntryShift;
  constexpr uint64_t kFresh = kOcc | ((uint64_t)kNone << kEntryShift);

  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const uint64_t *row = a.table + n * (int64_t)slots;
    const uint8_t *act = a.act + n * (int64_t)slots;
    uint64_t *out = a.out + n * (int64_t)slots;
    const bool open = a.count[n] >= 0;
    const RLevel<S> L = load_rlevel<S>(a.blk, a.tgt, N, n, T, a.Tt, a.mc != 0);
    if (tid == 0) ctl[0] = 0u, ctl[1 + 1 % 3] = 0u;  // round 1 counts in ctl[1 + 1 % 3]
    __syncthreads();

    // ---- the live slots and their successors
    uint32_t m = 0;
    uint32_t left = 0;  // LDS form: this lane's unresolved states, at positions tid, tid + 256, ... of the list
    (void)left;
    if constexpr (GLOBAL) {
      for (uint32_t base = 0; base < slots; base += kBlockThreads) {  // slots > kLdsSlots: a multiple of the block
        const uint32_t i = base + tid;
        const uint64_t w = row[i];
        uint64_t pair = 0;
        if (open && (w & kOcc)) {
          const uint32_t dir = act[i];
          pair = kFresh | (dir <= 3u ? succ_of<S>(L, row, slots, log2, i, w & kKeyMask, (int)dir, T) : i);
        }
        st64(&out[i], pair);
      }
      block_sync();
    } else {
      for (uint32_t base = 0; base < slots; base += kBlockThreads) {
        const uint32_t i = base + tid;
        const bool live = open && i < slots && (row[i] & kOcc) != 0;
        const uint32_t ticket = ticket_of(live, &ctl[0], lane);
        if (live) lds.lst[ticket] = (uint16_t)i, lds.ent[i] = (uint8_t)kNone;  // a slot takes one ticket: below slots
      }
      __syncthreads();
      m = ctl[0];
      for (uint32_t k = tid; k < m; k += kBlockThreads) {
        const uint32_t i = lds.lst[k], dir = act[i];
        uint32_t s = i;
        if (dir <= 3u) s = succ_of<S>(L, row, slots, log2, i, row[i] & kKeyMask, (int)dir, T);
        lds.suc[k] = (uint16_t)(s == kWon ? kWon16 : s);
      }
      __syncthreads();
      left = tid < m ? (m - tid + kBlockThreads - 1u) / kBlockThreads : 0u;
    }

    // ---- the rounds (ts_rtable.hip's, one successor)
    bool exhausted = false;
    int32_t d = 1;
    for (; d <= a.max_depth; ++d) {
      uint32_t *const resolved = &ctl[1 + d % 3];
      if (tid == 0) ctl[1 + (d + 1) % 3] = 0u;  // the next round's counter: last read behind the barrier of round d - 2
      uint32_t mine = 0;
      if constexpr (GLOBAL) {
        for (uint32_t base = 0; base < slots; base += kBlockThreads) {
          const uint32_t i = base + tid;
          const uint64_t e = ld64(&out[i]);
          if (!(e & kOcc) || entry_of(e) != kNone) continue;
          const uint32_t s = (uint32_t)e;
          const bool hit = s == kWon ? d == 1 : (d > 1 && entry_of(ld64(&out[s & (slots - 1u)])) == (uint32_t)(d - 1));
          if (hit) {
            st64(&out[i], (e & ~kEntryMask) | ((uint64_t)d << kEntryShift));
            ++mine;
          }
        }
      } else {
        // a lane owns every 256th position of the list and keeps its own unresolved states packed at the front of them: no
        // other lane reads or writes those positions, so the list shrinks without a barrier
        uint32_t kept = 0;
        for (uint32_t j = 0; j < left; ++j) {
          const uint32_t k = tid + j * kBlockThreads;
          const uint32_t i = lds.lst[k], s = lds.suc[k];
          const bool hit = s == kWon16 ? d == 1 : (d > 1 && lds.ent[s] == (uint32_t)(d - 1));
          if (hit) {
            lds.ent[i] = (uint8_t)d;
            ++mine;
          } else {
            const uint32_t w = tid + kept * kBlockThreads;
            lds.lst[w] = (uint16_t)i, lds.suc[w] = (uint16_t)s;
            ++kept;
          }
        }
        left = kept;
      }
      if (mine) atomicAdd(resolved, mine);
      block_sync();
      if (*resolved == 0u) {
        exhausted = true;
        break;
      }
    }
    const uint32_t fill = exhausted ? kNone : kDeep;

    // ---- the row: the keys are re-read from the table
    for (uint32_t base = 0; base < slots; base += kBlockThreads) {
      const uint32_t i = base + tid;
      if (i >= slots) break;
      const uint64_t w = row[i];
      uint64_t word = 0;
      if (open && (w & kOcc)) {
        uint32_t e;
        if constexpr (GLOBAL) e = entry_of(ld64(&out[i]));
        else e = lds.ent[i];
        word = kOcc | ((uint64_t)(e == kNone ? fill : e) << kEntryShift) | (w & kKeyMask);
      }
      if constexpr (GLOBAL) st64(&out[i], word);
      else out[i] = word;
    }
    if constexpr (GLOBAL) block_sync();  // the root's entry is read from the row
    if (tid == 0) {
      if (a.deepest) a.deepest[n] = d - 1;  // the last round that resolved a state
      if (a.root_moves) {
        bool won;
        const uint64_t key = root_key<S>(L, a.root, N, n, T, won);
        int32_t moves = 0;
        if (!won) {
          moves = TS_REACH_FULL;
          if (open) {
            bool held;
            const uint32_t slot = probe_row(row, slots, log2, key, held);
            uint32_t e = kNone;
            if (held) {
              if constexpr (GLOBAL) e = entry_of(ld64(&out[slot]));
              else e = lds.ent[slot];
            }
            moves = held ? moves_of(e == kNone ? fill : e) : TS_RTABLE_ABSENT;
          }
        }
        a.root_moves[n] = (int16_t)moves;
      }
    }
    block_sync();  // ent, lst, suc and ctl are the next level's
  }
}

// ---- 3. the score ----

struct SArgs {
  const uint8_t *tgt;
  const uint32_t *blk;
  const uint64_t *ptable, *table;
  const uint8_t *act;
  const int32_t *count;
  int32_t *score;
  int64_t N;
  uint32_t slots, slots_log2;
  int32_t T, Tt, mc;
};

template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_rptable_score(const SArgs a) {
  using M = typename RLevel<S>::M;
  __shared__ int32_t part[kBlockThreads / ts::kWave][kScoreColumns];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t slots = a.slots, log2 = a.slots_log2;
  const int T = a.T;
  const int64_t N = a.N;

  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const uint64_t *row = a.table + n * (int64_t)slots, *prow = a.ptable + n * (int64_t)slots;
    const uint8_t *act = a.act + n * (int64_t)slots;
    int32_t c[kScoreColumns];
#pragma unroll
    for (int k = 0; k < kScoreColumns; ++k) c[k] = 0;
    if (a.count[n] >= 0) {  // block-uniform
      const RLevel<S> L = load_rlevel<S>(a.blk, a.tgt, N, n, T, a.Tt, a.mc != 0);
      for (uint32_t i = tid; i < slots; i += kBlockThreads) {
        const uint64_t w = row[i];
        if (!(w & kOcc)) continue;
        const uint32_t o = entry_of(w), p = entry_of(prow[i]), dir = act[i];
        const bool solvable = o >= 1u && o <= kMaxDepth, solved = p >= 1u && p <= kMaxDepth;
        bool agree = false;
        if (solvable && dir <= 3u) {
          const uint64_t key = w & kKeyMask;
          uint32_t cell[kTiles];
          M occ, occ2;
          decode_key<S>(key, T, cell, occ);
          const uint64_t next = slide_key<S>(cell, occ, L.blk, T, (int)dir, occ2);
          if (L.won(next, occ2)) {
            agree = o == 1u;
          } else {
            bool held;
            const uint32_t slot = probe_row(row, slots, log2, next, held);
            agree = held && entry_of(row[slot]) == o - 1u;
          }
        }
        c[0] += 1;
        c[1] += solvable ? 1 : 0;
        c[2] += solved ? 1 : 0;
        c[3] += (solved && p == o) ? 1 : 0;
        c[4] += agree ? 1 : 0;
        c[5] += (solved && solvable) ? (int32_t)p - (int32_t)o : 0;
        c[6] += p == kDeep ? 1 : 0;
        c[7] += p == 0u ? 1 : 0;
      }
    }
#pragma unroll
    for (int k = 0; k < kScoreColumns; ++k) {
      for (int o = ts::kWave / 2; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o);
      if (lane == 0) part[wave][k] = c[k];
    }
    __syncthreads();
    if (tid < (uint32_t)kScoreColumns) a.score[n * kScoreColumns + tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
    __syncthreads();  // part is the next level's
  }
}

// ---- the host side ----

using ActionsKernel = void (*)(const AArgs);
using WalkKernel = void (*)(const WArgs);
using ScoreKernel = void (*)(const SArgs);

ActionsKernel actions_kernel(int S) {
  return ts::by_size<ActionsKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> ActionsKernel { return k_rptable_actions<s>; });
}
template <bool GLOBAL>
WalkKernel walk_kernel(int S) {
  return ts::by_size<WalkKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> WalkKernel { return k_rptable_walk<s, GLOBAL>; });
}
ScoreKernel score_kernel(int S) {
  return ts::by_size<ScoreKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> ScoreKernel { return k_rptable_score<s>; });
}

bool reach_shape(const ts_dims *d) { return d->size <= TS_REACH_MAX_SIZE && d->n_tiles <= TS_REACH_MAX_TILES; }
bool slots_ok(int64_t slots) { return slots >= 2 && slots <= (1ll << 31) && !(slots & (slots - 1)); }
uint32_t log2_of(int64_t slots) {
  uint32_t l = 0;
  while ((1ll << l) < slots) ++l;
  return l;
}

// the slots and the shape of a call whose dims have passed the shared check: TS_ERR_ARG
int32_t check_table(const ts_dims *d, int32_t hidden, int64_t slots) {
  return slots_ok(slots) && reach_shape(d) && shape_supported(d, hidden) ? TS_OK : TS_ERR_ARG;
}

using MlpPlan = Plan<AArgs, ts_rptable_desc>;

// plan_forward_block (ts_mlp.h) with the list beside the hs columns: the most waves (four, two, one) that leave room for the
// tile-plane weights; where not even one wave's do, the weights stay in global memory
void plan_actions_block(const ts_dims *d, int32_t H, MlpPlan &p) {
  const int C = d->size * d->size;
  p.slots = (d->multi_color ? d->n_tiles : 1) * C;
  const size_t wt_bytes = d->n_tiles > 0 ? ((size_t)H * p.slots * 4u + 15u) & ~(size_t)15u : 0u;
  const size_t hs_bytes = (size_t)H * kHsLdsBytesPerUnit;  // per thread
  const size_t fixed = (size_t)head_floats<AArgs::kValue>(H) * 4u + kListBytes;
  p.threads = 0;
  for (const uint32_t threads : {256u, 128u, 64u}) {
    if (wt_bytes > 0 && fixed + wt_bytes + hs_bytes * threads <= ts::kMaxBlockLds) {
      p.threads = threads, p.staged = 1, p.wt_floats = (int32_t)(wt_bytes / 4u);
      break;
    }
  }
  if (!p.threads) {
    p.staged = 0, p.wt_floats = 0;
    p.threads = fixed + hs_bytes * 256u <= ts::kMaxBlockLds ? 256u : fixed + hs_bytes * 128u <= ts::kMaxBlockLds ? 128u : 64u;
  }
  p.lds = fixed + (size_t)p.wt_floats * 4u + hs_bytes * p.threads;
}

int32_t plan_actions(const ts_dims *d, int32_t hidden, int64_t slots, MlpPlan &p) {
  if (const int32_t rc = check_table(d, hidden, slots); rc != TS_OK) return rc;
  plan_actions_block(d, hidden, p);
  ts_rptable_desc &desc = p.desc;
  desc.threads_per_block = (int32_t)p.threads, desc.lds_bytes = (int32_t)p.lds, desc.weights_in_lds = p.staged;
  if (d->n_boards == 0) return TS_OK;
  p.kernel = actions_kernel(d->size);
  if (!p.kernel) return TS_ERR_ARG;
  p.blocks = (uint32_t)std::min(d->n_boards, kMaxBlocks);
  desc.form = TS_RPTABLE_FORM_LDS, desc.blocks = p.blocks;
  snprintf(desc.name, sizeof desc.name, "k_rptable_actions<%d>", d->size);
  return TS_OK;
}

struct WalkPlan {
  WalkKernel kernel = nullptr;
  ts_rptable_desc desc{};
};
int32_t plan_walk(const ts_dims *d, int64_t slots, WalkPlan &p) {
  if (const int32_t rc = check_table(d, 1, slots); rc != TS_OK) return rc;
  const bool global = slots > (int64_t)kLdsSlots;
  p.desc.threads_per_block = kBlockThreads;
  p.desc.lds_slots = (int32_t)kLdsSlots;
  p.desc.lds_bytes = (int32_t)(global ? 16u : kWalkLdsBytes);
  if (d->n_boards == 0) return TS_OK;
  p.kernel = global ? walk_kernel<true>(d->size) : walk_kernel<false>(d->size);
  if (!p.kernel) return TS_ERR_ARG;
  p.desc.form = global ? TS_RPTABLE_FORM_GLOBAL : TS_RPTABLE_FORM_LDS;
  p.desc.blocks = std::min(d->n_boards, kMaxBlocks);
  snprintf(p.desc.name, sizeof p.desc.name, "k_rptable_walk<%d, %s>", d->size, global ? "true" : "false");
  return TS_OK;
}

struct ScorePlan {
  ScoreKernel kernel = nullptr;
  ts_rptable_desc desc{};
};
int32_t plan_score(const ts_dims *d, int64_t slots, ScorePlan &p) {
  if (const int32_t rc = check_table(d, 1, slots); rc != TS_OK) return rc;
  p.desc.threads_per_block = kBlockThreads;
  p.desc.lds_bytes = (int32_t)(4u * (kBlockThreads / ts::kWave) * kScoreColumns);
  if (d->n_boards == 0) return TS_OK;
  p.kernel = score_kernel(d->size);
  if (!p.kernel) return TS_ERR_ARG;
  p.desc.form = TS_RPTABLE_FORM_LDS;
  p.desc.blocks = std::min(d->n_boards, kMaxBlocks);
  snprintf(p.desc.name, sizeof p.desc.name, "k_rptable_score<%d>", d->size);
  return TS_OK;
}

// [p, p + n) and [q, q + m) share a byte
bool overlaps(const void *p, int64_t n, const void *q, int64_t m) {
  if (!p || !q || n <= 0 || m <= 0) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

}  // namespace

extern "C" {

int32_t ts_rptable_abi_version(void) { return TS_RPTABLE_ABI_VERSION; }
int32_t ts_rptable_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_rptable_supported(const ts_dims *dims, int32_t hidden) {
  const int32_t rc = supported(dims, hidden);
  return rc == 1 ? (reach_shape(dims) ? 1 : 0) : rc;
}

int32_t ts_describe_rptable_actions(const ts_dims *dims, int32_t hidden, int64_t slots, ts_rptable_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  MlpPlan p;
  if (const int32_t rc = plan_actions(dims, hidden, slots, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_describe_rptable_walk(const ts_dims *dims, int64_t slots, ts_rptable_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  WalkPlan p;
  if (const int32_t rc = plan_walk(dims, slots, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_describe_rptable_score(const ts_dims *dims, int64_t slots, ts_rptable_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  ScorePlan p;
  if (const int32_t rc = plan_score(dims, slots, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_rptable_actions(const ts_dims *dims, const ts_state *st, const ts_mlp *mlp, const uint64_t *table, int64_t slots,
                           const int32_t *count, uint8_t *act, float *logits, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!mlp) return TS_ERR_NULL;
  MlpPlan p;
  if (const int32_t rc = plan_actions(dims, mlp->hidden, slots, p); rc != TS_OK) return rc;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no further pointer is looked at
  if (!st || !table || !count || !act || !mlp_complete(mlp) || !st->blk || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  if ((uintptr_t)logits & 15u) return TS_ERR_ARG;
  AArgs a{};
  a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  a.w1 = mlp->w1, a.b1 = mlp->b1, a.w2 = mlp->w2, a.b2 = mlp->b2;
  a.table = table, a.count = count, a.act = act, a.logits = logits;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color;
  a.H = mlp->hidden, a.slots = p.slots, a.staged = p.staged, a.wt_floats = p.wt_floats;
  a.row_slots = (uint32_t)slots;
  hipLaunchKernelGGL(p.kernel, dim3(p.blocks), dim3(p.threads), p.lds, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_rptable_walk(const ts_dims *dims, const ts_state *st, const uint64_t *table, int64_t slots, const int32_t *count,
                        const uint8_t *act, const ts_rptable_cfg *cfg, const ts_rptable_out *out, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!cfg || !out) return TS_ERR_NULL;
  WalkPlan p;
  if (const int32_t rc = plan_walk(dims, slots, p); rc != TS_OK) return rc;
  if (cfg->max_depth < 0 || cfg->max_depth > TS_TABLE_MAX_DEPTH) return TS_ERR_ARG;
  if (cfg->root != TS_RTABLE_ROOT_INIT && cfg->root != TS_RTABLE_ROOT_POS) return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no further pointer is looked at
  if (!st || !table || !count || !act || !out->table || !st->blk || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  const void *root = cfg->root == TS_RTABLE_ROOT_INIT ? st->init : st->pos;
  if (out->root_moves && dims->n_tiles > 0 && !root) return TS_ERR_NULL;
  const int64_t words = dims->n_boards * slots;
  if (overlaps(out->table, 8 * words, table, 8 * words) || overlaps(out->table, 8 * words, act, words)) return TS_ERR_ARG;
  WArgs a{};
  a.root = static_cast<const uint8_t *>(root), a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  a.table = table, a.count = count, a.act = act;
  a.out = out->table, a.root_moves = out->root_moves, a.deepest = out->deepest;
  a.N = dims->n_boards, a.slots = (uint32_t)slots, a.slots_log2 = log2_of(slots);
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.max_depth = cfg->max_depth;
  hipLaunchKernelGGL(p.kernel, dim3((uint32_t)p.desc.blocks), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_rptable_score(const ts_dims *dims, const ts_state *st, const uint64_t *ptable, const uint8_t *act, const uint64_t *table,
                         int64_t slots, const int32_t *count, int32_t *score, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  ScorePlan p;
  if (const int32_t rc = plan_score(dims, slots, p); rc != TS_OK) return rc;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !ptable || !act || !table || !count || !score || !st->blk || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  if ((uintptr_t)score & 3u) return TS_ERR_ARG;
  SArgs a{};
  a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  a.ptable = ptable, a.table = table, a.act = act, a.count = count, a.score = score;
  a.N = dims->n_boards, a.slots = (uint32_t)slots, a.slots_log2 = log2_of(slots);
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color;
  hipLaunchKernelGGL(p.kernel, dim3((uint32_t)p.desc.blocks), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
