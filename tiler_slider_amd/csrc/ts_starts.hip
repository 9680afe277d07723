// ts_starts.hip — curriculum starts: place boards a chosen distance from the win (include/tiler_slider_starts.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_starts.so): the other eleven libraries are pinned symbol
// by symbol and kernel by kernel, and nothing here touches any of them.
//
// One read of the distance table.  k_starts_place<S> takes the wave form of ts_table.hip: a block is ONE wave, cut into groups
// of G = 1 .. 64 lanes (ts::group_of<false>), a board per group.  Lane g of a group reads the ALIGNED 16-byte pieces g, g + G,
// ... of its board's row - one coalesced request per group and pass -, masks the bytes before the row's head and after its
// tail (rows are C^T bytes and start wherever the one before ends), and turns each piece into two 16-bit masks: the bytes in
// the band, and the bytes that are distances at all.  Counts are summed and prefix-summed across the group with wave
// shuffles; the lane whose piece holds the j-th match decodes the index and stores the cells.  No LDS, no atomics, no barrier.
//
// The byte arithmetic is SWAR on the four words of a piece and lives in ts_bytes.h, TS_HD, so that tests/native/starts_bytes_check.cpp
// runs it on the host over every byte value; the host side of a launch is ts_launch.h's.
#include "../../include/tiler_slider_starts.h"
#include "ts_launch.h"  // first: hip_runtime.h defines what TS_HD needs
#include "ts_bytes.h"

namespace {

using ts::kMaxTiles, ts::kWave, ts::Piece;
constexpr uint32_t kPiece = TS_STARTS_PIECE_BYTES;
static_assert(TS_STARTS_FORM_NONE == ts::kFormNone && TS_STARTS_FORM_WAVE == ts::kFormWave);
static_assert(kPiece == ts::kPieceBytes && TS_TABLE_MAX_DEPTH == ts::kMaxDistance);

struct PArgs {
  const uint8_t *table;
  const int32_t *rows;  // may be NULL
  const uint8_t *band;  // may be NULL
  const uint8_t *done_in;  // TS_STARTS_DONE: the flags that select; else NULL
  uint8_t *pos, *init;  // NULL where not written
  int32_t *step_count;
  uint8_t *done;
  int32_t *count;       // each output may be NULL
  uint8_t *dist, *deepest;
  int64_t N, n_rows;
  uint64_t key;          // mix64(seed ^ step_index * kBoardMul)
  uint64_t board_offset;
  uint32_t states, lo, hi;
  int32_t T;
  uint32_t lanes_log2;
};

// The sixteen bytes at table + rel, an address that is 16-byte aligned.  A piece that lies inside the table's `len` bytes is one
// load; one that the table's first or last byte cuts is read byte by byte, and only inside the table.  (Offsets from the kernel
// argument, not addresses made from integers: the loads stay global loads.)
__device__ __forceinline__ void load_piece(Piece &pc, const uint8_t *table, int64_t rel, int64_t len) {
  if (rel >= 0 && rel + (int64_t)kPiece <= len) {
    const uint4 v = *reinterpret_cast<const uint4 *>(table + rel);
    pc.w[0] = v.x, pc.w[1] = v.y, pc.w[2] = v.z, pc.w[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int64_t at = rel + 4 * i + b;
        if (at >= 0 && at < len) w |= (uint32_t)table[at] << (8 * b);
      }
      pc.w[i] = w;
    }
  }
}

template <int S>
__global__ __launch_bounds__(kWave) void k_starts_place(const PArgs a) {
  constexpr uint32_t C = ts::Bitboard<S>::C;
  const auto [G, g, grp, n, nl, live] = ts::group_of<false>(threadIdx.x, blockIdx.x, a.lanes_log2, a.N);
  (void)grp;
  const int64_t N = a.N;
  const uint32_t states = a.states;

  // the band of this board, and whether it holds anything; hi is cut at the largest distance
  uint32_t lo = a.lo, hi = a.hi;
  if (a.band) lo = a.band[nl], hi = a.band[N + nl];
  hi = hi < (uint32_t)TS_TABLE_MAX_DEPTH ? hi : (uint32_t)TS_TABLE_MAX_DEPTH;
  const bool banded = lo <= hi;  // an empty band matches nothing; the row's deepest distance is reported all the same
  const bool selected = a.done_in ? a.done_in[nl] != 0 : true;

  const int64_t r = a.rows ? (int64_t)a.rows[nl] : nl;
  const bool has_row = r >= 0 && r < a.n_rows;

  // the aligned pieces that cover the row: piece p is the sixteen bytes at table + base + 16 p, byte k of it is entry
  // 16 p + k - off of the row
  const int64_t len = a.n_rows * (int64_t)states, row = (has_row ? r : 0) * (int64_t)states;
  const uint32_t off = (uint32_t)((reinterpret_cast<uintptr_t>(a.table) + (uintptr_t)row) & (kPiece - 1u));
  const int64_t base = row - off;  // -15 at the least
  const uint32_t pieces = has_row ? (off + states + kPiece - 1u) / kPiece : 0u;
  const uint32_t passes = (pieces + G - 1u) >> a.lanes_log2;  // the same for every lane of the group
  const auto row_bits = [&](uint32_t p) -> uint32_t {  // the bytes of piece p that are entries of the row
    const uint32_t first = p * kPiece < off ? off - p * kPiece : 0u;
    const uint32_t end = off + states - p * kPiece;  // > 0 for p < pieces
    return (end >= kPiece ? 0xffffu : (1u << end) - 1u) & ~((1u << first) - 1u);
  };
  const auto fetch = [&](Piece &pc, uint32_t p) {
    pc.w[0] = pc.w[1] = pc.w[2] = pc.w[3] = 0u, pc.in_band = pc.is_dist = 0u;
    if (p < pieces) {
      load_piece(pc, a.table, base + (int64_t)p * kPiece, len);
      ts::classify(pc, banded ? lo : 0u, banded ? hi : 0u, row_bits(p));
      if (!banded) pc.in_band = 0u;
    }
  };

  // the first walk: matches and the deepest distance; a row of one pass stays in `pc`
  Piece pc;
  uint32_t mine = 0, deep = 0;
  for (uint32_t pass = 0; pass < passes; ++pass) {
    fetch(pc, pass * G + g);
    mine += (uint32_t)ts::popc(pc.in_band);
    const uint32_t d = ts::deepest_plus_one(pc);
    deep = d > deep ? d : deep;
  }
  uint32_t count = mine;
  for (uint32_t o = 1; o < G; o <<= 1) {  // the lanes of a group are a power of two, aligned in the wave: xor stays inside
    count += (uint32_t)__shfl_xor((int)count, (int)o);
    const uint32_t other = (uint32_t)__shfl_xor((int)deep, (int)o);
    deep = other > deep ? other : deep;
  }
  const bool placed = live && selected && count > 0u;  // count > 0 only where the row exists

  if (live && g == 0) {
    if (a.count) a.count[n] = (int32_t)count;
    if (a.deepest) a.deepest[n] = (uint8_t)(deep ? deep - 1u : 255u);
    if (a.dist && !placed) a.dist[n] = 255;
  }
  if (!placed) return;  // the whole group leaves: no shuffle below waits for it

  const uint64_t R = ts::mix64(a.key + (a.board_offset + (uint64_t)n) * ts::kDrawMul);
  const uint32_t j = (uint32_t)(((R >> 32) * (uint64_t)count) >> 32);  // < count

  // the second walk, up to the pass that holds the j-th match
  uint32_t before = 0;  // matches in the passes walked so far
  for (uint32_t pass = 0; pass < passes; ++pass) {
    const uint32_t p = pass * G + g;
    if (passes > 1u) fetch(pc, p);
    const uint32_t c = (uint32_t)ts::popc(pc.in_band);
    uint32_t incl = c;
    for (uint32_t o = 1; o < G; o <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, o, (int)G);
      if (g >= o) incl += up;
    }
    const uint32_t in_pass = (uint32_t)__shfl((int)incl, (int)(G - 1u), (int)G);
    if (j < before + in_pass) {
      const uint32_t excl = before + incl - c;
      if (j >= excl && j < excl + c) {  // one lane of the group
        const uint32_t k = ts::nth_set_bit(pc.in_band, j - excl);
        uint32_t idx = p * kPiece + k - off;  // < states: bit k is a byte of the row
        if (a.dist) a.dist[n] = (uint8_t)ts::byte_of(pc, k);
#pragma unroll
        for (int t = 0; t < kMaxTiles; ++t) {
          if (t < a.T) {
            const uint8_t cell = (uint8_t)(idx % C);
            idx /= C;
            if (a.pos) a.pos[(int64_t)t * N + n] = cell;
            if (a.init) a.init[(int64_t)t * N + n] = cell;
          }
        }
        if (a.step_count) a.step_count[n] = 0;
        if (a.done) a.done[n] = 0;
      }
      break;
    }
    before += in_pass;
  }
}

using PlaceKernel = void (*)(const PArgs);
PlaceKernel place_kernel(int S) {
  return ts::by_size<PlaceKernel, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> PlaceKernel { return k_starts_place<s>; });
}

struct PlacePlan {
  ts::FormPlan<PlaceKernel> f;
  ts_starts_desc desc{};
};

// Everything ts_starts_place decides before it launches; touches no device (ts_describe_starts_place reports it).  `d` has
// passed ts::check_dims.
int32_t plan_place(const ts_dims *d, PlacePlan &p) {
  // the wave form always; a board would like a lane for each piece of its row
  const auto choose = [&](int64_t states, uint32_t) -> ts::FormChoice<PlaceKernel> {
    return {nullptr, place_kernel(d->size), (states + kPiece - 1) / kPiece};
  };
  if (const int32_t rc = ts::plan_forms(d, 0, 0, "k_starts", choose, p.f); rc != TS_OK) return rc;
  ts_starts_desc &desc = p.desc;
  desc.form = p.f.form, desc.lanes_per_board = p.f.lanes_per_board, desc.boards_per_block = p.f.boards_per_block;
  desc.threads_per_block = (int32_t)p.f.threads;
  desc.states = p.f.states, desc.blocks = p.f.n_blocks;
  if (p.f.form != ts::kFormNone) {
    const int64_t pieces = (p.f.states + kPiece - 1) / kPiece;
    desc.bytes_per_lane = (int32_t)kPiece;
    desc.passes = (int32_t)((pieces + p.f.lanes_per_board - 1) / p.f.lanes_per_board);
    snprintf(desc.name, sizeof desc.name, "k_starts_place<%d>", d->size);
  }
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

int32_t ts_starts_abi_version(void) { return TS_STARTS_ABI_VERSION; }
int32_t ts_starts_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_starts_supported(const ts_dims *dims) {
  const int64_t states = ts::checked_states(dims);
  return states < 0 ? (int32_t)states : states > 0 ? 1 : 0;
}

int32_t ts_describe_starts_place(const ts_dims *dims, ts_starts_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  PlacePlan p;
  const int32_t rc = plan_place(dims, p);
  if (rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_starts_place(const ts_dims *dims, const ts_state *st, const uint8_t *table, int64_t n_rows, const int32_t *rows,
                        const ts_starts_cfg *cfg, const ts_starts_out *out, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!cfg || !out) return TS_ERR_NULL;
  PlacePlan p;
  if (const int32_t rc = plan_place(dims, p); rc != TS_OK) return rc;
  const auto flag = [](int32_t v) { return v == 0 || v == 1; };
  if (cfg->lo < 0 || cfg->lo > TS_TABLE_MAX_DEPTH || cfg->hi < 0 || cfg->hi > TS_TABLE_MAX_DEPTH) return TS_ERR_ARG;
  if ((cfg->where != TS_STARTS_ALL && cfg->where != TS_STARTS_DONE) || !flag(cfg->write_pos) || !flag(cfg->write_init) || n_rows < 0) return TS_ERR_ARG;
  const int64_t N = dims->n_boards, T = dims->n_tiles;
  if (N == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  if (!st || (n_rows > 0 && !table)) return TS_ERR_NULL;
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
  a.table = table, a.rows = rows, a.band = cfg->band;
  a.done_in = cfg->where == TS_STARTS_DONE ? static_cast<const uint8_t *>(st->done) : nullptr;
  if (cfg->write_pos) a.pos = static_cast<uint8_t *>(st->pos), a.step_count = st->step_count, a.done = static_cast<uint8_t *>(st->done);
  if (cfg->write_init) a.init = static_cast<uint8_t *>(const_cast<void *>(st->init));  // const for the libraries that only read it
  a.count = out->count, a.dist = out->dist, a.deepest = out->deepest;
  a.N = N, a.n_rows = n_rows;
  a.key = ts::mix64(cfg->seed ^ ((uint64_t)cfg->step_index * ts::kBoardMul));
  a.board_offset = (uint64_t)cfg->board_offset;
  a.states = (uint32_t)p.f.states, a.lo = (uint32_t)cfg->lo, a.hi = (uint32_t)cfg->hi;
  a.T = dims->n_tiles, a.lanes_log2 = p.f.lanes_log2;
  hipLaunchKernelGGL(p.f.kernel, dim3(p.f.blocks), dim3(p.f.threads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
