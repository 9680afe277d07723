// ts_rstarts.hip — reach-table curricula: a sorted band index of every level of a reachable distance table, and the placement of
// boards a chosen distance from the win that reads it (include/tiler_slider_rstarts.h, which defines both).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_rstarts.so): no existing code object is rebuilt.  It
// shares ts_core.h (the draw) and ts_launch.h (dims check, error tail) with the other libraries, restates the slot format of
// tiler_slider_rtable.h, and never decodes a key in the index kernel: that one is not templated on the board size.
//
// Index: one launch of k_rstarts_index<GLOBAL> for any number of levels, a block of four waves per level, block b taking levels
// b, b + gridDim.x, ... as k_rtable_build does.  Per level:
//   1. scan    the row is read once, 16 bytes a lane where the row is 16-byte aligned;
//   2. compact an occupied word (bit 63) takes a ticket - one LDS atomic per wave and pass, the lanes' offsets from the ballot -
//              and goes to position `ticket` of the sort buffer; tickets at or above the buffer's size are dropped, which a row
//              that ts_rtable_build wrote never sees (count <= W);
//   3. sort    a bitonic network in its all-ascending form over P = pow2ceil(m) positions, m the words kept: the first step of
//              the merge of blocks of 2k pairs i with i ^ (2k - 1), the later steps pair i with i ^ j, the minimum always goes
//              to the lower index, and a comparator whose partner is >= m is skipped - the padding with +infinity, which never
//              moves.  The words of a table are distinct, so the order of the tickets leaves no trace;
//   4. write   `first` is 256 binary searches, one per lane, `sorted` the buffer and zeros behind it.
// The sort buffer is LDS for a level of at most kLdsStates states (k_rstarts_index<false> knows no other; 32 KiB and four blocks
// a CU - not measured against 8,192 states and two), and the level's own `sorted` row above that (k_rstarts_index<true>, chosen
// by the width W; a level takes the row only if its count is above kLdsStates).  Every step of the network in the row is a
// step in global memory: staging the steps with j below the LDS tile in LDS was not built.
//
// Memory model of the sort in the row (ts_rtable.hip's reading).  The row is touched by one block only, but by four waves of it,
// and a CU's vector L1 is not refreshed by another wave's store.  So every access to it between the scan and the last step is a
// relaxed agent-scope atomic, and every barrier is preceded by s_waitcnt vmcnt(0).
//
// Placement: k_rstarts_place<S>, one board per lane, plain loads: two or three words of `first`, one or two of `sorted`; the key
// is decoded with the constant divisors of its size.  No LDS, no atomics, no barrier.
#include "ts_launch.h"

#include "../../include/tiler_slider_rstarts.h"
#include "ts_core.h"

namespace {

using ts::kBlockThreads;
constexpr int kTiles = TS_REACH_MAX_TILES;
constexpr int64_t kMaxBlocks = 1024;  // of the index launch: four blocks of four waves on each of 256 CUs
constexpr uint32_t kLdsStates = 4096;
constexpr uint32_t kFirst = TS_RSTARTS_FIRST;
static_assert(kFirst == kBlockThreads, "a lane per word of `first`");

constexpr uint64_t kOcc = 1ull << 63, kKeyMask = (1ull << 48) - 1;
constexpr int kEntryShift = 48;

__device__ __forceinline__ uint64_t ld64(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st64(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// what this wave stored has arrived, then the block's barrier
__device__ __forceinline__ void block_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

struct IArgs {
  const uint64_t *table;
  const int32_t *count;
  uint64_t *sorted;
  int32_t *first;
  int64_t L;
  uint32_t slots, W;
};

// The network over positions 0 .. m - 1 of a buffer read by ld(i) and written by st(i, v); sync() separates two steps.  Every
// lane of the block calls it with the same m.
template <class Ld, class St, class Sync>
__device__ __forceinline__ void sort_ascending(uint32_t m, uint32_t tid, Ld ld, St st, Sync sync) {
  if (m < 2u) return;
  const uint32_t P = 1u << (32 - __builtin_clz(m - 1u));  // pow2ceil(m), at most 2^30
  const uint32_t half = P >> 1;
  for (uint32_t k = 1; k < P; k <<= 1) {
    for (uint32_t j = k; j > 0u; j >>= 1) {
      for (uint32_t c = tid; c < half; c += kBlockThreads) {
        const uint32_t i = ((c & ~(j - 1u)) << 1) | (c & (j - 1u));  // comparator c: bit j of i is clear
        const uint32_t p = j == k ? i ^ (2u * k - 1u) : i | j;        // > i
        if (p < m) {
          const uint64_t x = ld(i), y = ld(p);
          if (x > y) st(i, y), st(p, x);
        }
      }
      sync();
    }
  }
}

// first[d] for the lane's d: the kept words below d << 48, bit 63 aside
template <class Ld>
__device__ __forceinline__ int32_t lower_bound_of(uint32_t d, uint32_t m, Ld ld) {
  const uint64_t edge = (uint64_t)d << kEntryShift;
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((ld(mid) & ~kOcc) < edge) lo = mid + 1u;
    else hi = mid;
  }
  return (int32_t)lo;
}

template <bool GLOBAL>
__global__ __launch_bounds__(kBlockThreads) void k_rstarts_index(const IArgs a) {
  __shared__ uint64_t s[kLdsStates];
  __shared__ uint32_t ctl[4];  // [0]: tickets given
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t slots = a.slots, W = a.W;
  for (int64_t l = blockIdx.x; l < a.L; l += gridDim.x) {
    const uint64_t *row = a.table + l * (int64_t)slots;
    uint64_t *out = a.sorted + l * (int64_t)W;
    int32_t *first = a.first + l * (int64_t)kFirst;
    const int32_t cnt = a.count[l];
    if (cnt < 0 || (uint32_t)cnt > W) {  // FULL, or not a level of this width: an empty index
      for (uint32_t i = tid; i < W; i += kBlockThreads) out[i] = 0;
      first[tid] = 0;
      continue;
    }
    const bool in_row = GLOBAL && (uint32_t)cnt > kLdsStates;
    const uint32_t keep = in_row ? W : (W < kLdsStates ? W : kLdsStates);
    if (tid == 0) ctl[0] = 0;
    __syncthreads();

    // scan and compact: two slots a lane and pass (slots is even)
    const bool wide = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
    const uint32_t pairs = slots >> 1;
    for (uint32_t base = 0; base < pairs; base += kBlockThreads) {
      const uint32_t q = base + tid;
      uint64_t w[2] = {0, 0};
      if (q < pairs) {
        if (wide) {
          const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(row + 2u * q);
          w[0] = v.x, w[1] = v.y;
        } else {
          w[0] = row[2u * q], w[1] = row[2u * q + 1u];
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool occ = (w[h] & kOcc) != 0;
        const uint64_t votes = __ballot(occ);
        if (votes == 0) continue;  // the same for every lane of the wave
        uint32_t start = 0;
        if (lane == 0) start = atomicAdd(&ctl[0], (uint32_t)__popcll(votes));
        start = (uint32_t)__shfl((int)start, 0);
        const uint32_t ticket = start + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
        if (occ && ticket < keep) {
          if (in_row) st64(out + ticket, w[h]);
          else s[ticket] = w[h];
        }
      }
    }
    block_sync();
    const uint32_t given = ctl[0];
    const uint32_t m = given < keep ? given : keep;

    if (in_row) {
      for (uint32_t i = m + tid; i < W; i += kBlockThreads) out[i] = 0;  // never a position of the network
      sort_ascending(m, tid, [&](uint32_t i) { return ld64(out + i); }, [&](uint32_t i, uint64_t v) { st64(out + i, v); }, [] { block_sync(); });
      first[tid] = lower_bound_of(tid, m, [&](uint32_t i) { return ld64(out + i); });
    } else {
      sort_ascending(m, tid, [&](uint32_t i) { return s[i]; }, [&](uint32_t i, uint64_t v) { s[i] = v; }, [] { __syncthreads(); });
      first[tid] = lower_bound_of(tid, m, [&](uint32_t i) { return s[i]; });
      for (uint32_t i = tid; i < W; i += kBlockThreads) out[i] = i < m ? s[i] : 0;
    }
    __syncthreads();  // s and ctl are the next level's
  }
}

struct PArgs {
  const uint64_t *sorted;
  const int32_t *first;
  const int32_t *rows;     // may be NULL
  const uint8_t *band;     // may be NULL
  const uint8_t *done_in;  // TS_STARTS_DONE: the flags that select; else NULL
  uint8_t *pos, *init;     // NULL where not written
  int32_t *step_count;
  uint8_t *done;
  int32_t *count;          // each output may be NULL
  uint8_t *dist, *deepest;
  int64_t N, n_rows;
  uint64_t key;            // mix64(seed ^ step_index * kBoardMul)
  uint64_t board_offset;
  uint32_t W, lo, hi;
  int32_t T;
};

template <int S>
__global__ __launch_bounds__(kBlockThreads) void k_rstarts_place(const PArgs a) {
  constexpr uint32_t C = S * S;
  constexpr uint64_t C4 = (uint64_t)C * C * C * C;
  using Hi = std::conditional_t<(S <= 3), uint64_t, uint32_t>;  // key / C^4 of any 48-bit key: below 2^32 from 4x4 on
  const int64_t N = a.N, n = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (n >= N) return;
  const uint32_t W = a.W;

  uint32_t lo = a.lo, hi = a.hi;
  if (a.band) lo = a.band[n], hi = a.band[N + n];
  hi = hi < (uint32_t)TS_TABLE_MAX_DEPTH ? hi : (uint32_t)TS_TABLE_MAX_DEPTH;
  const bool selected = a.done_in ? a.done_in[n] != 0 : true;
  const int64_t r = a.rows ? (int64_t)a.rows[n] : n;
  const bool has_row = r >= 0 && r < a.n_rows;

  uint32_t from = 0, count = 0, deep = 255;
  const uint64_t *row = a.sorted + (has_row ? r : 0) * (int64_t)W;
  if (has_row) {
    const int32_t *f = a.first + r * (int64_t)kFirst;
    const auto clamp = [W](int32_t v) -> uint32_t { return v < 0 ? 0u : (uint32_t)v > W ? W : (uint32_t)v; };
    from = clamp(f[lo]);                    // lo <= 255
    const uint32_t to = clamp(f[hi + 1u]);  // hi + 1 <= 253
    count = to > from ? to - from : 0u;
    if (a.deepest) {
      const uint32_t finite = clamp(f[TS_TABLE_MAX_DEPTH + 1]);
      if (finite) deep = (uint32_t)(row[finite - 1u] >> kEntryShift) & 0xffu;
    }
  }
  const bool placed = selected && count > 0u;  // count > 0 only where the row exists
  if (a.count) a.count[n] = (int32_t)count;
  if (a.deepest) a.deepest[n] = (uint8_t)deep;
  if (!placed) {
    if (a.dist) a.dist[n] = 255;
    return;
  }
  const uint64_t R = ts::mix64(a.key + (a.board_offset + (uint64_t)n) * ts::kDrawMul);
  const uint32_t j = (uint32_t)(((R >> 32) * (uint64_t)count) >> 32);  // < count: from + j < to <= W
  const uint64_t w = row[from + j];
  if (a.dist) a.dist[n] = (uint8_t)((w >> kEntryShift) & 0xffu);
  const uint64_t key = w & kKeyMask;
  uint32_t low = (uint32_t)(key % C4);
  Hi high = (Hi)(key / C4);
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    if (t < a.T) {
      uint8_t cell;
      if (t < 4) cell = (uint8_t)(low % C), low /= C;
      else cell = (uint8_t)(high % C), high /= C;
      if (a.pos) a.pos[(int64_t)t * N + n] = cell;
      if (a.init) a.init[(int64_t)t * N + n] = cell;
    }
  }
  if (a.step_count) a.step_count[n] = 0;
  if (a.done) a.done[n] = 0;
}

using PlaceKernel = void (*)(const PArgs);
PlaceKernel place_kernel(int S) {
  return ts::by_size<PlaceKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> PlaceKernel { return k_rstarts_place<s>; });
}

// dims: NULL or DIMS (or the shared LIMIT), then the shape: LIMIT
int32_t check_shape(const ts_dims *d) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (d->size > TS_REACH_MAX_SIZE || d->n_tiles > TS_REACH_MAX_TILES) return TS_ERR_LIMIT;
  return TS_OK;
}

bool width_ok(int64_t W) { return W >= 1 && W <= TS_REACH_MAX_CAPACITY; }

// refusal 1 of ts_rstarts_index and what it would launch; touches no device
int32_t plan_index(int64_t n_levels, int64_t slots, int64_t W, ts_rstarts_desc &desc) {
  if (n_levels < 0 || slots < 2 || slots > (1ll << 31) || (slots & (slots - 1)) || !width_ok(W)) return TS_ERR_ARG;
  desc = ts_rstarts_desc{};
  desc.threads_per_block = kBlockThreads;
  desc.lds_bytes = (int32_t)(8u * kLdsStates + 16u);
  desc.lds_states = (int32_t)kLdsStates;
  desc.bytes = 8 * W + 4 * (int64_t)kFirst;
  if (n_levels == 0) return TS_OK;
  const bool global = W > (int64_t)kLdsStates;
  desc.form = global ? TS_RSTARTS_FORM_GLOBAL : TS_RSTARTS_FORM_LDS;
  desc.blocks = std::min(n_levels, kMaxBlocks);
  snprintf(desc.name, sizeof desc.name, "k_rstarts_index<%s>", global ? "true" : "false");
  return TS_OK;
}

// refusals 1 and 3 of ts_rstarts_place and what it would launch; touches no device
int32_t plan_place(const ts_dims *d, ts_rstarts_desc &desc, PlaceKernel &kernel) {
  if (const int32_t rc = check_shape(d); rc != TS_OK) return rc;
  desc = ts_rstarts_desc{};
  desc.threads_per_block = kBlockThreads;
  kernel = place_kernel(d->size);
  const int64_t blocks = (d->n_boards + kBlockThreads - 1) / kBlockThreads;
  if (!kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  desc.blocks = blocks;
  if (blocks) snprintf(desc.name, sizeof desc.name, "k_rstarts_place<%d>", d->size);
  return TS_OK;
}

// [p, p + n) and [q, q + m) share a byte (an absent or empty region shares none)
bool overlaps(const void *p, int64_t n, const void *q, int64_t m) {
  if (!p || !q || n <= 0 || m <= 0) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

}  // namespace

extern "C" {

int32_t ts_rstarts_abi_version(void) { return TS_RSTARTS_ABI_VERSION; }
int32_t ts_rstarts_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_rstarts_supported(const ts_dims *dims) {
  const int32_t rc = check_shape(dims);
  return rc == TS_OK ? 1 : rc == TS_ERR_LIMIT && ts::check_dims(dims) == TS_OK ? 0 : rc;
}

int32_t ts_describe_rstarts_index(int64_t n_levels, int64_t slots, int64_t W, ts_rstarts_desc *desc) {
  if (!desc) return TS_ERR_NULL;
  ts_rstarts_desc d;
  if (const int32_t rc = plan_index(n_levels, slots, W, d); rc != TS_OK) return rc;
  *desc = d;
  return TS_OK;
}

int32_t ts_describe_rstarts_place(const ts_dims *dims, ts_rstarts_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  ts_rstarts_desc d;
  PlaceKernel k = nullptr;
  if (const int32_t rc = plan_place(dims, d, k); rc != TS_OK) return rc;
  *desc = d;
  return TS_OK;
}

int32_t ts_rstarts_index(const uint64_t *table, int64_t slots, const int32_t *count, int64_t n_levels, int64_t W, uint64_t *sorted,
                         int32_t *first, void *stream) {
  ts_rstarts_desc d;
  if (const int32_t rc = plan_index(n_levels, slots, W, d); rc != TS_OK) return rc;
  if (n_levels == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!table || !count || !sorted || !first) return TS_ERR_NULL;
  const int64_t tb = 8 * slots * n_levels, cb = 4 * n_levels, sb = 8 * W * n_levels, fb = 4 * (int64_t)kFirst * n_levels;
  if (overlaps(sorted, sb, table, tb) || overlaps(sorted, sb, count, cb) || overlaps(first, fb, table, tb) || overlaps(first, fb, count, cb) ||
      overlaps(sorted, sb, first, fb))
    return TS_ERR_ARG;
  IArgs a{};
  a.table = table, a.count = count, a.sorted = sorted, a.first = first, a.L = n_levels, a.slots = (uint32_t)slots, a.W = (uint32_t)W;
  const auto kernel = d.form == TS_RSTARTS_FORM_GLOBAL ? k_rstarts_index<true> : k_rstarts_index<false>;
  hipLaunchKernelGGL(kernel, dim3((uint32_t)d.blocks), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

int32_t ts_rstarts_place(const ts_dims *dims, const ts_state *st, const uint64_t *sorted, const int32_t *first, int64_t W,
                         int64_t n_rows, const int32_t *rows, const ts_starts_cfg *cfg, const ts_starts_out *out, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!cfg || !out) return TS_ERR_NULL;
  ts_rstarts_desc d;
  PlaceKernel kernel = nullptr;
  if (const int32_t rc = plan_place(dims, d, kernel); rc != TS_OK) return rc;
  const auto flag = [](int32_t v) { return v == 0 || v == 1; };
  if (cfg->lo < 0 || cfg->lo > TS_TABLE_MAX_DEPTH || cfg->hi < 0 || cfg->hi > TS_TABLE_MAX_DEPTH) return TS_ERR_ARG;
  if ((cfg->where != TS_STARTS_ALL && cfg->where != TS_STARTS_DONE) || !flag(cfg->write_pos) || !flag(cfg->write_init) || n_rows < 0 || !width_ok(W))
    return TS_ERR_ARG;
  const int64_t N = dims->n_boards, T = dims->n_tiles;
  if (N == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || (n_rows > 0 && (!sorted || !first))) return TS_ERR_NULL;
  if (cfg->write_pos && ((T > 0 && !st->pos) || !st->step_count || !st->done)) return TS_ERR_NULL;
  if (cfg->write_init && T > 0 && !st->init) return TS_ERR_NULL;
  if (cfg->where == TS_STARTS_DONE && !st->done) return TS_ERR_NULL;
  if (!cfg->write_pos && !cfg->write_init && !out->count && !out->dist && !out->deepest) return TS_ERR_NULL;
  if (cfg->band) {
    const int64_t B = 2 * N;
    const bool hit = (cfg->write_pos && (overlaps(cfg->band, B, st->pos, T * N) || overlaps(cfg->band, B, st->step_count, 4 * N) ||
                                         overlaps(cfg->band, B, st->done, N))) ||
                     (cfg->write_init && overlaps(cfg->band, B, st->init, T * N)) || overlaps(cfg->band, B, out->count, 4 * N) ||
                     overlaps(cfg->band, B, out->dist, N) || overlaps(cfg->band, B, out->deepest, N);
    if (hit) return TS_ERR_ARG;
  }
  if (n_rows == 0) return TS_OK;  // no board has a row: nothing to launch, nothing is written
  PArgs a{};
  a.sorted = sorted, a.first = first, a.rows = rows, a.band = cfg->band;
  a.done_in = cfg->where == TS_STARTS_DONE ? static_cast<const uint8_t *>(st->done) : nullptr;
  if (cfg->write_pos) a.pos = static_cast<uint8_t *>(st->pos), a.step_count = st->step_count, a.done = static_cast<uint8_t *>(st->done);
  if (cfg->write_init) a.init = static_cast<uint8_t *>(const_cast<void *>(st->init));  // const for the libraries that only read it
  a.count = out->count, a.dist = out->dist, a.deepest = out->deepest;
  a.N = N, a.n_rows = n_rows;
  a.key = ts::mix64(cfg->seed ^ ((uint64_t)cfg->step_index * ts::kBoardMul));
  a.board_offset = (uint64_t)cfg->board_offset;
  a.W = (uint32_t)W, a.lo = (uint32_t)cfg->lo, a.hi = (uint32_t)cfg->hi;
  a.T = dims->n_tiles;
  hipLaunchKernelGGL(kernel, dim3((uint32_t)d.blocks), dim3(kBlockThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
