// ts_rtable.hip — reachable distance tables: the distance to the win of every placement that play can reach from a level's root,
// in a hash table in the caller's memory, and the lookup that reads it (include/tiler_slider_rtable.h, which defines both).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_rtable.so): no existing code object is rebuilt.  It
// shares ts_core.h (the slide arithmetic) and ts_launch.h (dims check, error tail) with the other libraries and keys of 64 bits
// with the hashed solver (ts_reach.hip): ts_index.h's are 32-bit and stop at five tiles.
//
// Build: one launch of k_rtable_build<S> for any N.  A block of four waves builds level n directly into row n of the table and
// owns slice blockIdx.x of the workspace; it builds levels blockIdx.x, blockIdx.x + gridDim.x, ... through it.  A slice is
//     log   [capacity]      uint32   the slot of every state of R in the order it was claimed: the compact list of R; entries
//                                    V(d - 1) .. V(d) - 1 are the frontier of depth d
//     succ  [capacity * 4]  uint32   the slots of the four successors of state i of the log; kWon for a won successor
// and five control words in LDS: V (claims so far), the "count is above capacity" flag, three round counters in rotation.
//
// Phase 1, the closure (ts_reach.hip's expansion without the early stop and without first-move bits).  The row is cleared, the
// root claims its home slot.  Depth by depth the 4 * |frontier| (state, move) pairs are dealt over the 256 lanes: decode, T
// calls of ts::slide_cell<S>, encode, win test.  A won successor is noted as kWon.  Any other is looked up: an empty slot is
// claimed by compare-and-swap with the entry TS_TABLE_NONE, the claim takes a ticket from V and writes its slot into
// log[ticket]; either way the slot goes into succ.  A level whose count passes `capacity` is FULL and ends there (claims beyond
// the capacity take tickets and are not logged; the row has more slots than capacity, so a probe only fails once the count is
// above it).  At most `capacity` depths: every depth but the last claims a state.
//
// Phase 2, the rounds, over the log and not over the slots.  In round d a lane reads its state's entry; where that is still
// TS_TABLE_NONE it gathers the entries of the four successor slots and, if one of them is d - 1 (d = 1: kWon), writes d into its
// OWN entry.  A round only tests for d - 1 and only writes d, and neither NONE nor d is d - 1: no second copy of the distances
// is needed.  A round that resolves nothing ends the level, the unresolved entries are TS_TABLE_NONE as they stand; behind round
// max_depth they are rewritten to TS_TABLE_DEEP.
//
// Memory model (ts_reach.hip's reading).  A row and a slice are touched by one block only, but by four waves of it, and a CU's
// vector L1 is not refreshed by another wave's atomic, which is performed at the L2.  So EVERY access to them is a relaxed
// agent-scope atomic (loads and stores bypass the L1, read-modify-writes are performed at the L2), and every barrier is
// preceded by s_waitcnt vmcnt(0): what a wave stored has arrived before any wave passes.
//
// Lookup: k_rtable_lookup<S>, one board per lane, plain loads, no LDS; a probe takes at most `slots` steps and stays in its row.
#include "ts_launch.h"

#include "../../include/tiler_slider_rtable.h"

namespace {

using ts::kBlockThreads;
constexpr int kTiles = TS_REACH_MAX_TILES;
// Blocks of a launch, hence slices in use, at most: four blocks of four waves on each of 256 CUs.
constexpr int64_t kMaxInFlight = 1024;

constexpr uint64_t kOcc = 1ull << 63, kKeyMask = (1ull << 48) - 1;
constexpr int kEntryShift = 48;
constexpr uint32_t kWon = 0xffffffffu;     // succ: the successor is won
constexpr uint32_t kNoSlot = 0xfffffffeu;  // succ: no slot was found (only in a level that ends FULL)

__device__ __forceinline__ uint64_t ld64(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st64(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ld32(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st32(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
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
  return entry >= 1u && entry <= (uint32_t)TS_TABLE_MAX_DEPTH ? (int32_t)entry : entry == (uint32_t)TS_TABLE_DEEP ? TS_SOLVE_DEPTH : TS_SOLVE_NONE;
}

// A level as every lane of a block, or the one lane of a lookup, holds it: obstacles and the win test on a 64-bit key.
template <int S>
struct Level {
  using M = typename ts::Bitboard<S>::mask_t;
  static constexpr uint32_t C = ts::Bitboard<S>::C;
  M blk = 0, tgm = 0;
  uint64_t tgt_key = 0;
  bool mc = false, mc_can_win = false;
  // win test (state.py:172-186): multi-colour: the state IS the targets' index and T == Tt; single colour: the sets of cells
  __device__ __forceinline__ bool won(uint64_t key, M occ) const { return mc ? (mc_can_win && key == tgt_key) : occ == tgm; }
};
template <int S>
__device__ __forceinline__ Level<S> load_level(const uint32_t *blk, const uint8_t *tgt, int64_t N, int64_t n, int T, int Tt, bool mc) {
  using M = typename Level<S>::M;
  Level<S> L;
  L.blk = ts::load_obstacles<S>(blk, N, n);
  uint64_t mul = 1;
  for (int j = 0; j < Tt; ++j) {
    const uint32_t tj = ts::clamp_cell(tgt[(int64_t)j * N + n], Level<S>::C);
    L.tgm |= M(1) << tj;
    if (j < T) {
      L.tgt_key += tj * mul;
      mul *= Level<S>::C;
    }
  }
  L.mc = mc, L.mc_can_win = T == Tt;
  return L;
}
// the key and the occupancy of the cells of board n as they lie in memory (clamped), with the cells
template <int S>
__device__ __forceinline__ uint64_t encode_cells(const uint8_t *cells, int64_t N, int64_t n, int T, uint32_t (&p)[kTiles], typename Level<S>::M &occ) {
  using M = typename Level<S>::M;
  uint64_t key = 0, mul = 1;
  occ = 0;
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    p[t] = 0;
    if (t < T) {
      p[t] = ts::clamp_cell(cells[(int64_t)t * N + n], Level<S>::C);
      key += p[t] * mul;
      mul *= Level<S>::C;
      occ |= M(1) << p[t];
    }
  }
  return key;
}
// the cells and the occupancy of a key: the key splits into two halves of four tiles, one 64-bit division per decode
template <int S>
__device__ __forceinline__ void decode_key(uint64_t s, int T, uint32_t (&p)[kTiles], typename Level<S>::M &occ) {
  using M = typename Level<S>::M;
  constexpr uint32_t C = Level<S>::C, C4 = C * C * C * C;
  uint32_t lo = (uint32_t)(s % C4), hi = (uint32_t)(s / C4);
  occ = 0;
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    p[t] = 0;
    if (t < T) {
      uint32_t &r = t < 4 ? lo : hi;
      p[t] = r % C;
      r /= C;
      occ |= M(1) << p[t];
    }
  }
}
// the key and the occupancy of the board one slide on
template <int S>
__device__ __forceinline__ uint64_t slide_key(const uint32_t (&p)[kTiles], typename Level<S>::M occ, typename Level<S>::M blk, int T, int dir,
                                               typename Level<S>::M &occ2) {
  using M = typename Level<S>::M;
  uint64_t key = 0, mul = 1;
  occ2 = 0;
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    if (t < T) {
      const uint32_t q = (uint32_t)ts::slide_cell<S>((int)p[t], occ, blk, dir);
      key += q * mul;
      mul *= Level<S>::C;
      occ2 |= M(1) << q;
    }
  }
  return key;
}

struct BArgs {
  const uint8_t *root, *tgt;  // cell_t = uint8 (S <= 8); root: st->init or st->pos
  const uint32_t *blk;
  uint64_t *table;
  int32_t *count;
  int16_t *root_moves;  // may be NULL
  int32_t *deepest;     // may be NULL
  uint32_t *ws;
  int64_t N;
  uint64_t slice_words;  // uint32 words per slice
  uint32_t slots, slots_log2, capacity;
  int32_t T, Tt, mc, max_depth;
};

template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_rtable_build(const BArgs a) {
  using M = typename Level<S>::M;
  __shared__ uint32_t ctl[5];  // V, count above capacity, the counters of rounds d % 3 == 0, 1, 2

  const uint32_t tid = threadIdx.x;
  const int64_t N = a.N;
  const int T = a.T;
  const uint32_t slots = a.slots, mask = slots - 1u, cap = a.capacity;
  uint32_t *log = a.ws + (uint64_t)blockIdx.x * a.slice_words;
  uint32_t *succ = log + ((cap + 1u) & ~1u);  // (the log a whole number of 8-byte words; capacity <= 2^30)
  constexpr uint64_t kFresh = kOcc | ((uint64_t)TS_TABLE_NONE << kEntryShift);

  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    uint64_t *row = a.table + (uint64_t)n * slots;
    for (uint32_t i = tid; i < slots; i += kBlockThreads) st64(&row[i], 0);
    // the level and the root, by every lane
    const Level<S> L = load_level<S>(a.blk, a.tgt, N, n, T, a.Tt, a.mc != 0);
    uint32_t p[kTiles];
    M occ;
    const uint64_t root = encode_cells<S>(a.root, N, n, T, p, occ);
    int32_t count = 0, root_moves = 0, deepest = 0;
    if (!L.won(root, occ)) {  // block-uniform
      block_sync();           // the row is clear
      const uint32_t root_slot = home_of(root, a.slots_log2);
      if (tid == 0) {
        st64(&row[root_slot], kFresh | root);
        st32(&log[0], root_slot);
        ctl[0] = 1u, ctl[1] = 0u, ctl[2 + 1] = 0u;  // round 1 counts in ctl[2 + 1 % 3]
      }
      block_sync();
      // ---- phase 1: the closure
      uint32_t v_prev = 0, v = 1;  // the frontier is log[v_prev .. v)
      bool full = false;
      for (uint32_t depth = 0; depth < cap && v > v_prev; ++depth) {
        const uint32_t items = 4u * (v - v_prev);  // v - v_prev <= capacity <= 2^30
        for (uint32_t w = tid; w < items; w += kBlockThreads) {
          if (__hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;  // FULL: nothing of this level is used
          const int dir = (int)(w & 3u);
          const uint32_t i = v_prev + (w >> 2);
          const uint32_t own = ld32(&log[i]) & mask;
          const uint64_t s = ld64(&row[own]) & kKeyMask;
          decode_key<S>(s, T, p, occ);
          M occ2;
          const uint64_t key = slide_key<S>(p, occ, L.blk, T, dir, occ2);
          uint32_t found = kNoSlot;
          if (key == s) {
            found = own;  // nothing slid
          } else if (L.won(key, occ2)) {
            found = kWon;
          } else {
            uint32_t slot = home_of(key, a.slots_log2);
            for (uint32_t probe = 0; probe < slots; ++probe, slot = (slot + 1u) & mask) {
              uint64_t seen = ld64(&row[slot]);
              if (seen == 0) {
                if (__hip_atomic_compare_exchange_strong(&row[slot], &seen, kFresh | key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                  const uint32_t ticket = atomicAdd(&ctl[0], 1u);
                  if (ticket < cap)
                    st32(&log[ticket], slot);
                  else
                    __hip_atomic_store(&ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                  found = slot;
                  break;
                }
                // lost the race: `seen` is the entry that won it
              }
              if ((seen & kKeyMask) == key) {
                found = slot;
                break;
              }
            }
          }
          st32(&succ[4u * i + (uint32_t)dir], found);
        }
        block_sync();
        const uint32_t v_new = ctl[0];
        __syncthreads();  // every lane has read V before the next depth adds to it
        if (v_new > cap) {
          full = true;
          break;
        }
        v_prev = v, v = v_new;
      }
      full = full || v > v_prev;  // (cannot be: `capacity` non-empty frontiers hold `capacity` states, the next one is above it)
      if (full) {
        count = root_moves = TS_REACH_FULL;
      } else {
        count = (int32_t)v;
        // ---- phase 2: the rounds over the log
        bool exhausted = false;
        int32_t d = 1;
        for (; d <= a.max_depth; ++d) {
          uint32_t *const resolved = &ctl[2 + d % 3];
          if (tid == 0) ctl[2 + (d + 1) % 3] = 0u;  // the next round's counter: last read behind the barrier of round d - 2
          uint32_t mine = 0;
          for (uint32_t i = tid; i < v; i += kBlockThreads) {
            const uint32_t own = ld32(&log[i]) & mask;
            const uint64_t e = ld64(&row[own]);
            if (entry_of(e) != (uint32_t)TS_TABLE_NONE) continue;
            bool hit = false;
#pragma unroll
            for (int dir = 0; dir < 4; ++dir) {
              const uint32_t q = ld32(&succ[4u * i + (uint32_t)dir]);
              if (q == kWon)
                hit = hit || d == 1;
              else if (q < slots && d > 1)
                hit = hit || entry_of(ld64(&row[q])) == (uint32_t)(d - 1);
            }
            if (hit) {
              st64(&row[own], (e & ~(0xffull << kEntryShift)) | ((uint64_t)d << kEntryShift));
              ++mine;
            }
          }
          if (mine) atomicAdd(resolved, mine);
          block_sync();
          if (*resolved == 0u) {
            exhausted = true;
            break;
          }
        }
        deepest = d - 1;  // the last round that resolved a state
        if (!exhausted) {
          for (uint32_t i = tid; i < v; i += kBlockThreads) {
            const uint32_t own = ld32(&log[i]) & mask;
            const uint64_t e = ld64(&row[own]);
            if (entry_of(e) == (uint32_t)TS_TABLE_NONE) st64(&row[own], (e & ~(0xffull << kEntryShift)) | ((uint64_t)TS_TABLE_DEEP << kEntryShift));
          }
          block_sync();
        }
        root_moves = moves_of(entry_of(ld64(&row[root_slot])));
      }
      block_sync();  // every lane has read ctl and the root's entry: the next level writes both
    }
    if (tid == 0) {
      a.count[n] = count;
      if (a.root_moves) a.root_moves[n] = (int16_t)root_moves;
      if (a.deepest) a.deepest[n] = deepest;
    }
  }
}

struct LArgs {
  const uint8_t *pos, *tgt;
  const uint32_t *blk;
  const uint64_t *table;
  const int32_t *count;
  const int32_t *rows;  // may be NULL
  int16_t *moves;       // each output may be NULL
  uint8_t *best, *action;
  int64_t N, n_rows;
  uint32_t slots, slots_log2;
  int32_t T, Tt, mc;
};

// the entry of `key` in a row, 0 where the row does not hold it: at most `slots` reads, all inside the row
__device__ __forceinline__ uint32_t probe_row(const uint64_t *row, uint32_t slots, uint32_t slots_log2, uint64_t key, bool &held) {
  const uint32_t mask = slots - 1u;
  uint32_t slot = home_of(key, slots_log2) & mask;
  held = false;
  for (uint32_t probe = 0; probe < slots; ++probe, slot = (slot + 1u) & mask) {
    const uint64_t e = row[slot];
    if (e == 0) return 0;
    if ((e & kOcc) && (e & kKeyMask) == key) {
      held = true;
      return entry_of(e);
    }
  }
  return 0;
}

template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_rtable_lookup(const LArgs a) {
  using M = typename Level<S>::M;
  const int64_t n = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (n >= a.N) return;
  const int64_t N = a.N;
  const int T = a.T;
  const int64_t r = a.rows ? (int64_t)a.rows[n] : n;
  int32_t moves = TS_SOLVE_NONE;
  uint32_t best = 0;
  if (r >= 0 && r < a.n_rows) {
    const Level<S> L = load_level<S>(a.blk, a.tgt, N, n, T, a.Tt, a.mc != 0);
    uint32_t p[kTiles];
    M occ;
    const uint64_t key = encode_cells<S>(a.pos, N, n, T, p, occ);
    if (L.won(key, occ)) {
      moves = 0;
    } else if (a.count[r] == TS_REACH_FULL) {
      moves = TS_REACH_FULL;
    } else {
      const uint64_t *row = a.table + (uint64_t)r * a.slots;
      bool held;
      const uint32_t d0 = probe_row(row, a.slots, a.slots_log2, key, held);
      if (!held) {
        moves = TS_RTABLE_ABSENT;
      } else {
        moves = moves_of(d0);
        if (moves >= 1 && (a.best || a.action)) {
          for (int dir = 0; dir < 4; ++dir) {
            M occ2;
            const uint64_t next = slide_key<S>(p, occ, L.blk, T, dir, occ2);
            uint32_t d;
            if (L.won(next, occ2)) {
              d = 0;
            } else {
              bool there;
              d = probe_row(row, a.slots, a.slots_log2, next, there);
              if (!there || d == 0) d = (uint32_t)TS_TABLE_NONE;  // (an entry 0 is never stored: it is no distance)
            }
            best |= (d == d0 - 1u ? 1u : 0u) << dir;
          }
        }
      }
    }
  }
  if (a.moves) a.moves[n] = (int16_t)moves;
  if (a.best) a.best[n] = (uint8_t)best;
  if (a.action) a.action[n] = (uint8_t)ts::lowest_move(best);
}

using BuildKernel = void (*)(const BArgs);
using LookupKernel = void (*)(const LArgs);

BuildKernel build_kernel(int S) {
  return ts::by_size<BuildKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> BuildKernel { return k_rtable_build<s>; });
}
LookupKernel lookup_kernel(int S) {
  return ts::by_size<LookupKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> LookupKernel { return k_rtable_lookup<s>; });
}

struct BuildPlan {
  BuildKernel kernel = nullptr;
  BArgs a{};
  ts_rtable_desc desc{};
};

// dims: NULL or DIMS, then the shape: LIMIT
int32_t check_shape(const ts_dims *d) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (d->size > TS_REACH_MAX_SIZE || d->n_tiles > TS_REACH_MAX_TILES) return TS_ERR_LIMIT;
  return TS_OK;
}

bool capacity_ok(int32_t capacity) { return capacity >= 1 && capacity <= TS_REACH_MAX_CAPACITY; }

// the row and the slice of one level; `capacity` is in range
void sizes_of(int32_t capacity, ts_rtable_desc &desc, uint32_t &slots_log2) {
  slots_log2 = 1;
  while ((1ll << slots_log2) < 2ll * capacity) ++slots_log2;
  desc.slots = 1ll << slots_log2;
  desc.table_bytes = 8 * desc.slots;
  desc.workspace_bytes = 8 * (((int64_t)capacity + 1) / 2) + 16ll * capacity;  // the log, a whole number of 8-byte words, and succ
}

// Everything ts_rtable_build decides before it launches; touches no device and looks at no pointer but dims and cfg.
int32_t plan_build(const ts_dims *d, const ts_rtable_cfg *cfg, BuildPlan &p) {
  if (const int32_t rc = check_shape(d); rc != TS_OK) return rc;
  if (!cfg) return TS_ERR_NULL;
  if (cfg->max_depth < 0 || cfg->max_depth > TS_TABLE_MAX_DEPTH || !capacity_ok(cfg->capacity)) return TS_ERR_ARG;
  if (cfg->root != TS_RTABLE_ROOT_INIT && cfg->root != TS_RTABLE_ROOT_POS) return TS_ERR_ARG;
  BArgs &a = p.a;
  sizes_of(cfg->capacity, p.desc, a.slots_log2);
  p.desc.threads_per_block = kBlockThreads;
  if (d->n_boards == 0) return TS_OK;
  const int64_t fit = cfg->workspace_bytes / p.desc.workspace_bytes;
  if (cfg->workspace_bytes < 0 || fit < 1) return TS_ERR_ARG;
  p.desc.levels_in_flight = p.desc.blocks = std::min(std::min(d->n_boards, fit), kMaxInFlight);
  snprintf(p.desc.name, sizeof p.desc.name, "k_rtable_build<%d>", d->size);
  p.kernel = build_kernel(d->size);
  if (!p.kernel) return TS_ERR_LIMIT;
  a.N = d->n_boards, a.T = d->n_tiles, a.Tt = d->n_targets, a.mc = d->multi_color, a.max_depth = cfg->max_depth;
  a.slots = (uint32_t)p.desc.slots, a.capacity = (uint32_t)cfg->capacity;
  a.slice_words = (uint64_t)p.desc.workspace_bytes / 4u;
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_rtable_abi_version(void) { return TS_RTABLE_ABI_VERSION; }
int32_t ts_rtable_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_rtable_supported(const ts_dims *dims) {
  const int32_t rc = check_shape(dims);
  return rc == TS_OK ? 1 : rc == TS_ERR_LIMIT && ts::check_dims(dims) == TS_OK ? 0 : rc;
}

int64_t ts_rtable_slots(int32_t capacity) {
  if (!capacity_ok(capacity)) return TS_ERR_ARG;
  ts_rtable_desc desc{};
  uint32_t slots_log2;
  sizes_of(capacity, desc, slots_log2);
  return desc.slots;
}

int64_t ts_rtable_workspace_bytes(const ts_dims *dims, int32_t capacity, int64_t levels_in_flight) {
  if (const int32_t rc = check_shape(dims); rc != TS_OK) return rc;
  if (!capacity_ok(capacity) || levels_in_flight < 1) return TS_ERR_ARG;
  ts_rtable_desc desc{};
  uint32_t slots_log2;
  sizes_of(capacity, desc, slots_log2);
  if (levels_in_flight > INT64_MAX / desc.workspace_bytes) return TS_ERR_ARG;
  return levels_in_flight * desc.workspace_bytes;
}

int32_t ts_describe_rtable_build(const ts_dims *dims, const ts_rtable_cfg *cfg, ts_rtable_desc *desc) {
  if (!dims) return TS_ERR_NULL;
  BuildPlan p;
  if (const int32_t rc = plan_build(dims, cfg, p); rc != TS_OK) return rc;
  if (!desc) return TS_ERR_NULL;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_rtable_build(const ts_dims *dims, const ts_state *st, const ts_rtable_cfg *cfg, const ts_rtable_out *out, void *stream) {
  if (!dims) return TS_ERR_NULL;
  BuildPlan p;
  if (const int32_t rc = plan_build(dims, cfg, p); rc != TS_OK) return rc;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !out || !out->table || !out->count || !cfg->workspace || !st->blk) return TS_ERR_NULL;
  const void *root = cfg->root == TS_RTABLE_ROOT_INIT ? st->init : st->pos;
  if ((dims->n_tiles > 0 && !root) || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  p.a.root = static_cast<const uint8_t *>(root), p.a.tgt = static_cast<const uint8_t *>(st->tgt), p.a.blk = st->blk;
  p.a.table = out->table, p.a.count = out->count, p.a.root_moves = out->root_moves, p.a.deepest = out->deepest;
  p.a.ws = static_cast<uint32_t *>(cfg->workspace);
  hipLaunchKernelGGL(p.kernel, dim3((uint32_t)p.desc.blocks), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), p.a);
  return ts::finish_launch();
}

int32_t ts_rtable_lookup(const ts_dims *dims, const ts_state *st, const uint64_t *table, int64_t slots, const int32_t *count,
                         int64_t n_rows, const int32_t *rows, int16_t *moves, uint8_t *best, uint8_t *action, void *stream) {
  if (const int32_t rc = check_shape(dims); rc != TS_OK) return rc;
  if (n_rows < 0 || slots < 2 || slots > (1ll << 31) || (slots & (slots - 1))) return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !st->blk || (dims->n_tiles > 0 && !st->pos) || (dims->n_targets > 0 && !st->tgt) || (n_rows > 0 && (!table || !count)) ||
      (!moves && !best && !action))
    return TS_ERR_NULL;
  const int64_t blocks = (dims->n_boards + kBlockThreads - 1) / kBlockThreads;
  LookupKernel k = lookup_kernel(dims->size);
  if (!k || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  LArgs a{};
  a.pos = static_cast<const uint8_t *>(st->pos), a.tgt = static_cast<const uint8_t *>(st->tgt), a.blk = st->blk;
  a.table = table, a.count = count, a.rows = rows, a.moves = moves, a.best = best, a.action = action;
  a.N = dims->n_boards, a.n_rows = n_rows, a.slots = (uint32_t)slots;
  while ((1ll << a.slots_log2) < slots) ++a.slots_log2;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color;
  hipLaunchKernelGGL(k, dim3((uint32_t)blocks), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
