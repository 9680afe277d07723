// ts_reach.hip — hashed breadth-first solver: optimal move counts, first moves and reached-state counts of boards whose index
// space does not fit LDS (include/tiler_slider_reach.h, which defines the search).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_reach.so): no existing code object is rebuilt.  It
// shares ts_core.h (the slide arithmetic) and ts_launch.h (dims check, error tail) with the search library and brings its own
// 64-bit keys: ts_index.h is 32-bit and stops at five tiles.
//
// One launch of k_reach<S> for any N.  A block of four waves owns slice blockIdx.x of the workspace and plays boards
// blockIdx.x, blockIdx.x + gridDim.x, ... through it.  A slice is
//     table     [slots]     uint64   open addressing, linear probing; slots = pow2ceil(2 * capacity)
//     frontier  [capacity]  uint64   the compacted frontier F(d - 1): key and first-move bits of every state to expand
//     log       [capacity]  uint32   the slot of every state in the order it was claimed; entries V(d - 1) .. V(d) - 1 are F(d)
// and three control words in LDS: V (claims so far), the found mask, the "count is above capacity" flag.
//
// An entry:  bit 63 occupied | bit 62 FRESH (claimed in the depth being built) | bits 48 .. 51 first moves | bits 0 .. 47 key.
// 0 is an empty slot.  Depth d deals the 4 * |F(d - 1)| (state, move) pairs evenly over the 256 lanes: decode, T calls of
// ts::slide_cell<S>, encode, win test.  A won successor ORs its parent's first-move bits into the found mask.  Any other
// successor is looked up: an empty slot is claimed by compare-and-swap (FRESH, the parent's bits), the claim takes a ticket
// from V and writes its slot into log[ticket]; a FRESH entry of the same key gets the parent's bits ORed in (a state reached
// twice in one depth collects the first moves of both parents, so the depth runs to its end); an entry that is not FRESH was
// reached at an earlier depth and is left alone.  After the depth's barrier every lane reads V and the found mask and takes
// the same decision (the header's order: won, FULL, NONE, DEPTH); to go on, the lanes walk log[V(d - 1) .. V(d)), clear FRESH
// with a fetch-and - which returns the entry with its final bits - and write it into the frontier.
//
// FULL follows from the count: claims beyond `capacity` take tickets too and are not logged; a lane stops inserting only once
// the flag says the count is above capacity, and the table has more slots than capacity, so a probe sequence can only fail to
// find an empty slot once every slot is claimed, i.e. with the count above capacity.  Won successors are still collected after
// that: rule 1 comes before rule 2.
//
// Between boards the block clears what it used: the logged slots, or the whole table after FULL; the whole table once at
// the start, so the caller never zeroes anything.
//
// Memory model.  A slice is touched by its own block only, but by four waves of it, and a CU's vector L1 is not refreshed by
// another wave's atomic, which is performed at the L2.  So EVERY access to a slice is a relaxed agent-scope atomic (loads and
// stores bypass the L1, read-modify-writes are performed at the L2), and every barrier is preceded by s_waitcnt vmcnt(0):
// what a wave stored has arrived before any wave passes.  Not measured against a cheaper form.
#include "ts_launch.h"

#include "../../include/tiler_slider_reach.h"

namespace {

using ts::kBlockThreads;
constexpr int kReachTiles = TS_REACH_MAX_TILES;
// Blocks of a launch, hence slices in use, at most: four blocks of four waves on each of 256 CUs.
constexpr int64_t kMaxInFlight = 1024;

constexpr uint64_t kOcc = 1ull << 63, kFresh = 1ull << 62, kKeyMask = (1ull << 48) - 1;
constexpr int kFirstShift = 48;

struct RArgs {
  const uint8_t *pos, *tgt;  // cell_t = uint8 (S <= 8)
  const uint32_t *blk;
  int16_t *moves;
  uint8_t *best;    // may be NULL
  int32_t *states;  // may be NULL
  uint64_t *ws;
  int64_t N;
  uint64_t slice_words;  // uint64 words per slice
  uint32_t slots, slots_log2, capacity;
  int32_t T, Tt, mc, max_depth;
};

__device__ __forceinline__ uint64_t ld64(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st64(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ld32(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st32(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// what this wave stored has arrived, then the block's barrier
__device__ __forceinline__ void block_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_reach(const RArgs a) {
  using BB = ts::Bitboard<S>;
  using M = typename BB::mask_t;
  constexpr uint32_t C = BB::C;
  constexpr uint32_t C4 = C * C * C * C;  // the key splits into two halves of four tiles: one 64-bit division per decode
  __shared__ uint32_t ctl[3];              // V, found mask, count above capacity

  const uint32_t tid = threadIdx.x;
  const int64_t N = a.N;
  const int T = a.T, Tt = a.Tt;
  const uint32_t slots = a.slots, mask = slots - 1u, cap = a.capacity;
  uint64_t *table = a.ws + (uint64_t)blockIdx.x * a.slice_words;
  uint64_t *frontier = table + slots;
  uint32_t *log = reinterpret_cast<uint32_t *>(frontier + cap);

  for (uint32_t i = tid; i < slots; i += kBlockThreads) st64(&table[i], 0);
  block_sync();

  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    // the level and the root, by every lane (cell ids clamped as the step kernels clamp them)
    M blk = (M)a.blk[n];
    if constexpr (BB::wide) blk |= (M)a.blk[N + n] << 32;
    uint64_t root = 0;
    M occ_root = 0;
    {
      uint64_t mul = 1;
#pragma unroll
      for (int t = 0; t < kReachTiles; ++t) {
        if (t < T) {
          const uint32_t p = min((uint32_t)a.pos[(int64_t)t * N + n], C - 1u);
          root += p * mul;
          mul *= C;
          occ_root |= M(1) << p;
        }
      }
    }
    // win test (state.py:172-186): multi-colour: the state IS the targets' index and T == Tt; single colour: the sets of cells
    M tgm = 0;
    uint64_t tgt_key = 0;
    {
      uint64_t mul = 1;
      for (int j = 0; j < Tt; ++j) {
        const uint32_t tj = min((uint32_t)a.tgt[(int64_t)j * N + n], C - 1u);
        tgm |= M(1) << tj;
        if (j < T) {
          tgt_key += tj * mul;
          mul *= C;
        }
      }
    }
    const bool mc = a.mc != 0, mc_can_win = T == Tt;
    auto is_won = [&](uint64_t key, M occ) { return mc ? (mc_can_win && key == tgt_key) : occ == tgm; };
    auto home = [&](uint64_t key) { return (uint32_t)((key * 0x9e3779b97f4a7c15ull) >> 32) >> (32u - a.slots_log2) & mask; };

    int32_t result = 0, expanded = 0;
    uint32_t best = 0;
    if (!is_won(root, occ_root)) {  // block-uniform
      if (tid == 0) {
        const uint32_t h = home(root);
        st64(&table[h], kOcc | root);
        st32(&log[0], h);
        st64(&frontier[0], root);
        ctl[0] = 1u, ctl[1] = 0u, ctl[2] = 0u;
      }
      block_sync();
      uint32_t v_prev = 0, v = 1;  // V(d - 1), V(d)
      int32_t d = 0;
      for (;;) {
        if (d >= a.max_depth) {
          result = TS_SOLVE_DEPTH;
          break;
        }
        ++d;
        const uint32_t items = 4u * (v - v_prev);  // v - v_prev < capacity <= 2^30
        for (uint32_t w = tid; w < items; w += kBlockThreads) {
          const int dir = (int)(w & 3u);
          const uint64_t e = ld64(&frontier[w >> 2]);
          const uint64_t s = e & kKeyMask;
          const uint32_t f = d == 1 ? (1u << dir) : (uint32_t)(e >> kFirstShift) & 15u;
          uint32_t p[kReachTiles];
          M occ = 0;
          {
            uint32_t lo = (uint32_t)(s % C4), hi = (uint32_t)(s / C4);
#pragma unroll
            for (int t = 0; t < kReachTiles; ++t) {
              p[t] = 0;
              if (t < T) {
                uint32_t &r = t < 4 ? lo : hi;
                p[t] = r % C;
                r /= C;
                occ |= M(1) << p[t];
              }
            }
          }
          uint64_t key = 0, mul = 1;
          M occ2 = 0;
#pragma unroll
          for (int t = 0; t < kReachTiles; ++t) {
            if (t < T) {
              const uint32_t q = (uint32_t)ts::slide_cell<S>((int)p[t], occ, blk, dir);
              key += q * mul;
              mul *= C;
              occ2 |= M(1) << q;
            }
          }
          if (key == s) continue;  // nothing slid: never on a shortest path
          if (is_won(key, occ2)) {
            atomicOr(&ctl[1], f);
            continue;
          }
          if (__hip_atomic_load(&ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;  // the count is above capacity: FULL unless a win turns up
          const uint64_t fresh = kOcc | kFresh | ((uint64_t)f << kFirstShift) | key;
          uint32_t slot = home(key);
          for (uint32_t probe = 0; probe < slots; ++probe, slot = (slot + 1u) & mask) {
            uint64_t seen = ld64(&table[slot]);
            if (seen == 0) {
              if (__hip_atomic_compare_exchange_strong(&table[slot], &seen, fresh, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                const uint32_t ticket = atomicAdd(&ctl[0], 1u);
                if (ticket < cap)
                  st32(&log[ticket], slot);
                else
                  __hip_atomic_store(&ctl[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                break;
              }
              // lost the race: `seen` is the entry that won it
            }
            if ((seen & kKeyMask) == key) {
              if ((seen & kFresh) && (((uint64_t)f << kFirstShift) & ~seen))
                __hip_atomic_fetch_or(&table[slot], (uint64_t)f << kFirstShift, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              break;
            }
          }
        }
        block_sync();
        expanded = (int32_t)v;  // every state of V(d - 1) has been expanded
        const uint32_t v_new = ctl[0], found = ctl[1];
        if (found) {
          result = d;
          best = found;
          break;
        }
        if (v_new > cap) {
          result = TS_REACH_FULL;
          break;
        }
        if (v_new == v) {
          result = TS_SOLVE_NONE;
          break;
        }
        // F(d) becomes the frontier: FRESH cleared, the first-move bits final
        for (uint32_t i = tid; i < v_new - v; i += kBlockThreads) {
          const uint32_t slot = ld32(&log[v + i]);
          const uint64_t e = __hip_atomic_fetch_and(&table[slot], ~kFresh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          st64(&frontier[i], e & ~(kFresh | kOcc));
        }
        v_prev = v, v = v_new;
        block_sync();
      }
      // Clear what the board used.  Every lane has read ctl; it is written next behind the barrier below.
      const uint32_t claimed = ctl[0];
      if (claimed > cap) {
        for (uint32_t i = tid; i < slots; i += kBlockThreads) st64(&table[i], 0);
      } else {
        for (uint32_t i = tid; i < claimed; i += kBlockThreads) st64(&table[ld32(&log[i])], 0);
      }
      block_sync();
    }
    if (tid == 0) {
      a.moves[n] = (int16_t)result;
      if (a.best) a.best[n] = (uint8_t)best;
      if (a.states) a.states[n] = expanded;
    }
  }
}

using ReachKernel = void (*)(const RArgs);

ReachKernel reach_kernel(int S) {
  return ts::by_size<ReachKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> ReachKernel { return k_reach<s>; });
}

struct ReachPlan {
  ReachKernel kernel = nullptr;
  RArgs a{};
  ts_reach_desc desc{};
};

// dims: NULL or DIMS, then the shape: LIMIT
int32_t check_shape(const ts_dims *d) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (d->size > TS_REACH_MAX_SIZE || d->n_tiles > TS_REACH_MAX_TILES) return TS_ERR_LIMIT;
  return TS_OK;
}

// the slice of one board; `capacity` is in range
void slice_of(int32_t capacity, ts_reach_desc &desc, uint32_t &slots_log2) {
  slots_log2 = 1;
  while ((1ll << slots_log2) < 2ll * capacity) ++slots_log2;
  desc.slots_per_board = 1ll << slots_log2;
  desc.table_bytes = 8 * desc.slots_per_board;
  desc.frontier_bytes = 8ll * capacity;
  desc.log_bytes = 8 * (((int64_t)capacity + 1) / 2);  // uint32 entries, the slice a whole number of 8-byte words
  desc.bytes_per_board = desc.table_bytes + desc.frontier_bytes + desc.log_bytes;
}

// Everything ts_reach_solve decides before it launches; touches no device and looks at no pointer but dims and cfg.
int32_t plan_reach(const ts_dims *d, const ts_reach_cfg *cfg, ReachPlan &p) {
  if (const int32_t rc = check_shape(d); rc != TS_OK) return rc;
  if (!cfg) return TS_ERR_NULL;
  if (cfg->max_depth < 0 || cfg->max_depth > TS_REACH_MAX_DEPTH || cfg->capacity < 1 || cfg->capacity > TS_REACH_MAX_CAPACITY) return TS_ERR_ARG;
  RArgs &a = p.a;
  slice_of(cfg->capacity, p.desc, a.slots_log2);
  p.desc.threads_per_block = kBlockThreads;
  if (d->n_boards == 0) return TS_OK;
  const int64_t fit = cfg->workspace_bytes / p.desc.bytes_per_board;
  if (cfg->workspace_bytes < 0 || fit < 1) return TS_ERR_ARG;
  p.desc.boards_in_flight = p.desc.blocks = std::min(std::min(d->n_boards, fit), kMaxInFlight);
  snprintf(p.desc.name, sizeof p.desc.name, "k_reach<%d>", d->size);
  p.kernel = reach_kernel(d->size);
  if (!p.kernel) return TS_ERR_LIMIT;
  a.N = d->n_boards, a.T = d->n_tiles, a.Tt = d->n_targets, a.mc = d->multi_color, a.max_depth = cfg->max_depth;
  a.slots = (uint32_t)p.desc.slots_per_board, a.capacity = (uint32_t)cfg->capacity;
  a.slice_words = (uint64_t)p.desc.bytes_per_board / 8u;
  return TS_OK;
}

}  // namespace

extern "C" {

int32_t ts_reach_abi_version(void) { return TS_REACH_ABI_VERSION; }
int32_t ts_reach_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_reach_supported(const ts_dims *dims) {
  const int32_t rc = check_shape(dims);
  return rc == TS_OK ? 1 : rc == TS_ERR_LIMIT && ts::check_dims(dims) == TS_OK ? 0 : rc;
}

int64_t ts_reach_workspace_bytes(const ts_dims *dims, int32_t capacity, int64_t boards_in_flight) {
  if (const int32_t rc = check_shape(dims); rc != TS_OK) return rc;
  if (capacity < 1 || capacity > TS_REACH_MAX_CAPACITY || boards_in_flight < 1) return TS_ERR_ARG;
  ts_reach_desc desc{};
  uint32_t slots_log2;
  slice_of(capacity, desc, slots_log2);
  if (boards_in_flight > INT64_MAX / desc.bytes_per_board) return TS_ERR_ARG;
  return boards_in_flight * desc.bytes_per_board;
}

int32_t ts_describe_reach(const ts_dims *dims, const ts_reach_cfg *cfg, ts_reach_desc *desc) {
  if (!dims) return TS_ERR_NULL;
  ReachPlan p;
  if (const int32_t rc = plan_reach(dims, cfg, p); rc != TS_OK) return rc;
  if (!desc) return TS_ERR_NULL;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_reach_solve(const ts_dims *dims, const ts_state *st, const ts_reach_cfg *cfg, const ts_reach_out *out, void *stream) {
  if (!dims) return TS_ERR_NULL;
  ReachPlan p;
  if (const int32_t rc = plan_reach(dims, cfg, p); rc != TS_OK) return rc;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || !out || !out->moves || !cfg->workspace || !st->blk || (dims->n_tiles > 0 && !st->pos) || (dims->n_targets > 0 && !st->tgt)) return TS_ERR_NULL;
  p.a.pos = static_cast<const uint8_t *>(st->pos), p.a.tgt = static_cast<const uint8_t *>(st->tgt), p.a.blk = st->blk;
  p.a.moves = out->moves, p.a.best = out->best, p.a.states = out->states, p.a.ws = static_cast<uint64_t *>(cfg->workspace);
  hipLaunchKernelGGL(p.kernel, dim3((uint32_t)p.desc.blocks), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), p.a);
  return ts::finish_launch();
}

}  // extern "C"
