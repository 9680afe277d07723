// ts_launch.h — the host side shared by the search, table and rollout libraries: what every entry point checks before it plans,
// the wave-or-block plan of the two libraries that keep bitmaps in LDS, and the tail of every launch.
//
// Each library is a translation unit and a shared library of its own and includes this header for itself; everything here has
// internal linkage (one thread-local error word and one copy of each function per library, no new exported symbol).  The measured
// policy - which form a shape takes - stays in the .hip it was measured for and reaches plan_forms as a callable.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <type_traits>

#include "../../include/tiler_slider_search.h"
#include "ts_index.h"

namespace ts {
namespace {

// Dynamic LDS a block may ask for: the bound the step library allows itself (ts_kernels.hip: kMaxBlockLds), and what a block
// gets without asking, so that no launch here needs hipFuncSetAttribute.
constexpr size_t kMaxBlockLds = 64 * 1024;

thread_local int32_t t_last_hip_error = 0;  // ts_*_last_hip_error of the including library

inline int32_t check_dims(const ts_dims *d) {
  if (!d) return TS_ERR_NULL;
  if (d->n_boards < 0 || d->size < 1 || d->n_tiles < 0 || d->n_targets < 0 || (d->multi_color != 0 && d->multi_color != 1)) return TS_ERR_DIMS;
  if (d->size > TS_MAX_SIZE || d->n_tiles > TS_MAX_TILES || d->n_targets > TS_MAX_TILES) return TS_ERR_LIMIT;
  if (d->n_tiles > d->size * d->size) return TS_ERR_DIMS;
  return TS_OK;
}

// (S * S)^T, the size of the index space (ts_index.h), where it is held: boards up to TS_SOLVE_MAX_SIZE and at most
// TS_SOLVE_MAX_STATES entries; 0 beyond that.  `d` has passed check_dims.
inline int64_t index_states(const ts_dims *d) {
  if (d->size > TS_SOLVE_MAX_SIZE) return 0;
  const int64_t C = (int64_t)d->size * d->size;
  int64_t states = 1;
  for (int t = 0; t < d->n_tiles; ++t) {
    states *= C;
    if (states > TS_SOLVE_MAX_STATES) return 0;
  }
  return states;
}
// ts_solve_states / ts_table_states: a negative status for bad dims, else index_states
inline int64_t checked_states(const ts_dims *d) {
  if (const int32_t rc = check_dims(d); rc != TS_OK) return rc;
  return index_states(d);
}

// f(integral_constant<int, V>) for the V of Vs... that equals v, as a K; nullptr where none does
template <class K, int... Vs, class F>
K by_size(int v, F f) {
  K k = nullptr;
  (void)((v == Vs && (k = f(std::integral_constant<int, Vs>{}), true)) || ...);
  return k;
}

// Launch forms of a kernel that keeps `bitmaps` bitmaps over the index space and `ctl_words` control words per board in LDS.
// The values are those of TS_SOLVE_FORM_* and TS_TABLE_FORM_*.
enum : int32_t { kFormNone = 0, kFormWave = 1, kFormBlock = 2 };

template <class K>
struct FormPlan {
  K kernel = nullptr;
  uint32_t blocks = 0, threads = 0;
  size_t lds = 0;             // dynamic LDS of a block
  uint32_t words = 0;         // uint32 words per bitmap
  uint32_t board_words = 0;   // LDS words per board
  uint32_t lanes_log2 = 0;    // wave form: log2 of the lanes per board
  int32_t form = kFormNone, lanes_per_board = 0, boards_per_block = 0;
  int64_t states = 0, n_blocks = 0;
  char name[64] = "";
};
template <class K>
struct FormChoice {
  K block;       // the block kernel where the shape takes the block form, else nullptr
  K wave;        // the wave kernel otherwise
  int64_t want;  // wave form: lanes a board would like (rounded up to a power of two, at most 64)
};

// One board per block of four waves, or 64 / lanes boards per block of one wave: everything a launch decides before it is made;
// touches no device.  choose(states, words) -> FormChoice<K> is the library's policy; `stem`: "k_solve" -> "k_solve_wave<4>".
// An empty batch plans no launch (kFormNone, the sizes filled in).
template <class K, class Choose>
int32_t plan_forms(const ts_dims *d, int bitmaps, int ctl_words, const char *stem, Choose choose, FormPlan<K> &p) {
  const int64_t states = checked_states(d);
  if (states < 0) return (int32_t)states;
  if (states == 0) return TS_ERR_LIMIT;
  p.states = states;
  p.words = (uint32_t)((states + 31) / 32);
  p.board_words = (uint32_t)bitmaps * p.words + (uint32_t)ctl_words;
  if (d->n_boards == 0) return TS_OK;
  const FormChoice<K> c = choose(states, p.words);
  if (c.block) {
    p.kernel = c.block;
    p.threads = kBlockThreads;
    p.form = kFormBlock, p.lanes_per_board = kBlockThreads, p.boards_per_block = 1;
  } else {
    p.kernel = c.wave;
    while ((1 << p.lanes_log2) < kWave && (1 << p.lanes_log2) < c.want) ++p.lanes_log2;
    p.threads = kWave;
    p.form = kFormWave, p.lanes_per_board = 1 << p.lanes_log2, p.boards_per_block = kWave / p.lanes_per_board;
  }
  p.n_blocks = (d->n_boards + p.boards_per_block - 1) / p.boards_per_block;
  snprintf(p.name, sizeof p.name, "%s_%s<%d>", stem, c.block ? "block" : "wave", d->size);
  p.lds = (size_t)p.boards_per_block * p.board_words * 4u;
  if (!p.kernel || p.lds > kMaxBlockLds || p.n_blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)p.n_blocks;
  return TS_OK;
}

// the fields every ts_*_desc of a FormPlan shares
template <class Desc, class K>
void describe_forms(const FormPlan<K> &p, Desc &desc) {
  desc.form = p.form, desc.lanes_per_board = p.lanes_per_board, desc.boards_per_block = p.boards_per_block;
  desc.threads_per_block = (int32_t)p.threads;
  desc.bitmap_words = (int32_t)p.words;
  desc.lds_bytes_board = (int32_t)(p.board_words * 4u);
  desc.lds_bytes_block = (int32_t)p.lds;
  desc.states = p.states, desc.blocks = p.n_blocks;
  snprintf(desc.name, sizeof desc.name, "%s", p.name);
}

// after every launch: TS_OK, or TS_ERR_HIP with the error kept for ts_*_last_hip_error
inline int32_t finish_launch() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    t_last_hip_error = (int32_t)e;
    return TS_ERR_HIP;
  }
  return TS_OK;
}

// ts_*_tuning: value >= 0 sets the knob and returns what it was, a negative value reads it; -1 for a key without a knob
inline int64_t tune(std::atomic<int64_t> *knob, int64_t value) {
  if (!knob) return -1;
  return value >= 0 ? knob->exchange(value, std::memory_order_relaxed) : knob->load(std::memory_order_relaxed);
}

}  // namespace
}  // namespace ts
