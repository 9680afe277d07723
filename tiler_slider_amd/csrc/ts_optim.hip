// ts_optim.hip — the fused optimiser: global-norm clip, AdamW and the zeroing of the gradients over up to 32 small tensors in
// one launch (include/tiler_slider_optim.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_optim.so): the other ten libraries are pinned symbol
// by symbol and kernel by kernel, and nothing here touches any of them.  The library knows no board: no ts_dims.
//
// NO FLOAT ATOMICS.  The sum of squares is float64 all the way: lanes -> wave (wave_sum) -> block (LDS) -> in the multi-block
// form one partial per block in the caller's workspace, which every block of k_optim_apply (and k_optim_finish) adds up again
// by ONE function, sum_partials, on 256 threads: the same bits in every block, from run to run.
//
// The tensors reach the kernels as arrays in the kernel argument (1,648 bytes); every index into them is uniform over a chunk's threads, so a
// pointer is a scalar load from the argument segment and no array is copied anywhere.  The element space is cut into CHUNKS of
// four elements a thread, none across two tensors; chunk ids run through the tensors in order and a block takes every
// gridDim.x-th (in the one block a chunk is one WAVE's, 256 elements, and each of the sixteen waves takes every sixteenth),
// finding a chunk's tensor by walking `cend` forward - ids only ascend.  Where a tensor's
// four pointers are 16-byte aligned a thread's four elements are consecutive and move as one dwordx4 (a ragged last vector
// falls back to dwords); otherwise they lie a block's width apart and every access of the wave is one coalesced dword.  Every
// access is guarded by its element index against the tensor's numel.
//
// What is uniform over a call - c, the two bias corrections, lr, the skip flag - is worked out by thread 0 of each block from
// the total and counters[0] (make_uniform: float64, rounded to float32 once) and handed to the block through LDS.
// counters[0] is read there and written by thread 0 of k_optim_one after its last barrier, or by k_optim_finish, a launch of
// its own behind k_optim_apply: stream order puts the write after every block's read.
#include "../../include/tiler_slider_optim.h"
#include "ts_launch.h"

#include <cmath>

namespace {

using ts::kWave;
constexpr int kThreads = TS_OPTIM_THREADS;         // the multi-block kernels: four waves
constexpr int kOneThreads = TS_OPTIM_ONE_THREADS;  // the one block: sixteen waves, a whole CU's worth of loads in flight
constexpr int kPerThread = 4;
constexpr int64_t kMaxBlocks = TS_OPTIM_MAX_BLOCKS;
constexpr int kMaxTensors = TS_OPTIM_MAX_TENSORS;
static_assert(TS_OPTIM_CHUNK == kThreads * kPerThread, "a chunk is four elements a thread");
static_assert(TS_OPTIM_ONE_CHUNK == kWave * kPerThread, "the one block's chunk is a wave's");

namespace policy {
// Calls of at most this many elements take the one-block form (ts_optim_tuning(TS_OPTIM_TUNE_ONE_BLOCK_MAX)).
// Measured, MI355X, us per FusedAdam.step() with the clip on and the gradients zeroed, one tensor, one block / multi-block
// (profiles/optim_timing.log, tools/optim_timing.py):
//     1,024: 19.6 / 24.7    4,096: 30.2 / 37.7    16,384: 29.3 / 36.4    32,768: 28.6 / 37.3    65,536: 47.5 / 37.9    131,072: 88.2 / 24.6
// Up to 32,768 elements both forms cost the host's call and the one launch is 5 to 9 us ahead of the three; from 65,536 on the
// one block's trips (sixteen waves, 256 elements each, two passes) are longer than the two launches it saves.  The project's
// networks (2,757 parameters for 4x4 boards at H = 32, 20,869 for 8x8 at H = 64: 24 / 29 us either) lie below.
constexpr int64_t kOneBlockMax = 32768;
}  // namespace policy

std::atomic<int64_t> g_one_block_max{policy::kOneBlockMax};

struct OArgs {
  float *p[kMaxTensors], *g[kMaxTensors], *m[kMaxTensors], *v[kMaxTensors];
  int64_t numel[kMaxTensors];
  int64_t cend[kMaxTensors];  // chunks up to and including tensor i
  int64_t chunks;             // cend[n - 1]
  int64_t *counters;
  float *grad_norm;
  const float *lr_dev;
  double *partials;
  double max_norm;            // 0: no clip
  uint32_t vec;               // bit i: tensor i moves 16 bytes at a time
  uint32_t n_partials;
  int32_t norm, skip_nonfinite, zero_grad;
  float lr, eps, wd;
  float beta1, beta2, omb1, omb2;  // float32(beta), float32(1 - beta)
  double beta1d, beta2d;
};

struct Uniform {
  float c, bc1, bc2, lr;
  int32_t skip, pad;  // 24 bytes: what the block's LDS is counted with (kLdsOne, kLdsMulti)
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// lanes -> wave -> LDS -> thread 0, the waves in order; the result is thread 0's alone
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double *sh) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    t = sh[0];
#pragma unroll
    for (int w = 1; w < THREADS / kWave; ++w) t += sh[w];
  }
  return t;
}

// the partials in a fixed order, on kThreads threads: partial j is thread j mod kThreads', each thread's in index order
__device__ __forceinline__ double sum_partials(const OArgs &a, double *sh) {
  double t = 0.0;
  for (uint32_t j = threadIdx.x; j < a.n_partials; j += kThreads) t += a.partials[j];
  return block_sum<kThreads>(t, sh);
}

__device__ __forceinline__ double powi(double b, int64_t e) {  // b^e by squaring: at most 126 float64 roundings
  double r = 1.0;
  for (; e > 0; e >>= 1, b *= b)
    if (e & 1) r *= b;
  return r;
}

// thread 0 only: what the call's elements share.  `total` is the sum of squares (ignored without the norm pass).
__device__ __forceinline__ Uniform make_uniform(const OArgs &a, double total, double &gn) {
  Uniform u;
  gn = a.norm ? sqrt(total) : 0.0;
  const bool finite = total - total == 0.0;  // false for an infinity and for a NaN
  u.skip = (a.norm && a.skip_nonfinite && !finite) ? 1 : 0;
  double c = 1.0;
  if (a.norm && a.max_norm > 0.0) {
    c = a.max_norm / (gn + 1e-6);
    c = c < 1.0 ? c : 1.0;
  }
  u.c = (float)c;
  const int64_t t1 = a.counters[0] + 1;
  u.bc1 = (float)(1.0 - powi(a.beta1d, t1));
  u.bc2 = (float)(1.0 - powi(a.beta2d, t1));
  u.lr = a.lr_dev ? *a.lr_dev : a.lr;
  return u;
}

// A thread's four elements of the chunk that starts at element e0 of a tensor of n: consecutive from e0 + 4 tid (vec), or
// THREADS apart from e0 + tid.  THREADS threads share a chunk: a block of the multi-block forms, ONE WAVE of the one block.
template <int THREADS>
struct Lane {
  int64_t first, n;
  int step;
  bool full;  // all four inside and vec: one dwordx4
  __device__ __forceinline__ Lane(bool vec, int64_t e0, int64_t n_, int tid) : n(n_) {
    first = vec ? e0 + kPerThread * (int64_t)tid : e0 + tid;
    step = vec ? 1 : THREADS;
    full = vec && first + kPerThread <= n;
  }
  __device__ __forceinline__ void load(const float *base, float (&x)[kPerThread]) const {
    if (full) {
      const float4 q = *reinterpret_cast<const float4 *>(base + first);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) {
        const int64_t i = first + (int64_t)j * step;
        x[j] = i < n ? base[i] : 0.0f;
      }
    }
  }
  __device__ __forceinline__ void store(float *base, const float (&x)[kPerThread]) const {
    if (full) {
      *reinterpret_cast<float4 *>(base + first) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) {
        const int64_t i = first + (int64_t)j * step;
        if (i < n) base[i] = x[j];
      }
    }
  }
};

// Who shares a chunk, and which chunks are theirs: a block of kThreads takes every gridDim.x-th from blockIdx.x on; in the one
// block every wave is such a team of its own and takes every 16th, so sixteen chunks are in flight at once and the six tensors
// of the project's networks are one trip, not six.
template <int THREADS>
struct Team {
  int tid;
  int64_t first, stride;
  __device__ __forceinline__ Team() {
    if constexpr (THREADS == kWave) tid = threadIdx.x & (kWave - 1), first = threadIdx.x / kWave, stride = kOneThreads / kWave;
    else tid = threadIdx.x, first = blockIdx.x, stride = gridDim.x;
  }
};

// the chunks of this team, in ascending order: f(tensor, first element of the chunk)
template <int THREADS, class F>
__device__ __forceinline__ void for_chunks(const OArgs &a, const Team<THREADS> &team, F f) {
  int ti = 0;
  int64_t c0 = 0;  // the first chunk id of tensor ti
  for (int64_t c = team.first; c < a.chunks; c += team.stride) {  // uniform over the team
    while (c >= a.cend[ti]) c0 = a.cend[ti], ++ti;              // c < chunks = cend[n - 1]: ti stays below n
    f(ti, (c - c0) * (int64_t)(THREADS * kPerThread));
  }
}

template <int THREADS>
__device__ __forceinline__ double norm_pass(const OArgs &a) {
  double acc = 0.0;
  const Team<THREADS> team;
  for_chunks<THREADS>(a, team, [&](int ti, int64_t e0) {
    const Lane<THREADS> lane((a.vec >> ti) & 1u, e0, a.numel[ti], team.tid);
    float g[kPerThread];
    lane.load(a.g[ti], g);  // 0 beyond the tensor
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) acc += (double)g[j] * (double)g[j];
  });
  return acc;
}

template <int THREADS>
__device__ __forceinline__ void apply_pass(const OArgs &a, const Uniform u) {
  const float decay = 1.0f - u.lr * a.wd;
  const bool zero = a.zero_grad != 0;
  const float zeros[kPerThread] = {0.0f, 0.0f, 0.0f, 0.0f};
  const Team<THREADS> team;
  if (u.skip) {  // uniform over the call
    if (zero)
      for_chunks<THREADS>(a, team, [&](int ti, int64_t e0) { Lane<THREADS>((a.vec >> ti) & 1u, e0, a.numel[ti], team.tid).store(a.g[ti], zeros); });
    return;
  }
  for_chunks<THREADS>(a, team, [&](int ti, int64_t e0) {
    const Lane<THREADS> lane((a.vec >> ti) & 1u, e0, a.numel[ti], team.tid);
    float g[kPerThread], p[kPerThread], m[kPerThread], v[kPerThread];
    lane.load(a.g[ti], g), lane.load(a.p[ti], p), lane.load(a.m[ti], m), lane.load(a.v[ti], v);  // all before the first use
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
      const float gh = u.c * g[j];
      m[j] = a.beta1 * m[j] + a.omb1 * gh;
      v[j] = a.beta2 * v[j] + a.omb2 * (gh * gh);
      p[j] = p[j] * decay - u.lr * (m[j] / u.bc1) / (sqrtf(v[j] / u.bc2) + a.eps);
    }
    lane.store(a.p[ti], p), lane.store(a.m[ti], m), lane.store(a.v[ti], v);
    if (zero) lane.store(a.g[ti], zeros);
  });
}

// thread 0, once per call, after every read of counters[0]
__device__ __forceinline__ void write_state(const OArgs &a, const Uniform &u, double gn) {
  if (u.skip) a.counters[1] += 1;
  else a.counters[0] += 1;
  if (a.grad_norm) a.grad_norm[0] = (float)gn;
}

// ------------------------------------------------------------------------------------------------------ the one-block form
__global__ __launch_bounds__(kOneThreads) void k_optim_one(const OArgs a) {
  __shared__ double sh[kOneThreads / kWave];
  __shared__ Uniform shu;
  double total = 0.0, gn = 0.0;
  if (a.norm) total = block_sum<kOneThreads>(norm_pass<kWave>(a), sh);  // uniform; thread 0's
  Uniform u{};
  if (threadIdx.x == 0) shu = u = make_uniform(a, total, gn);
  __syncthreads();
  apply_pass<kWave>(a, shu);
  __syncthreads();
  if (threadIdx.x == 0) write_state(a, u, gn);
}

// --------------------------------------------------------------------------------------------------- the multi-block forms
__global__ __launch_bounds__(kThreads) void k_optim_norm(const OArgs a) {
  __shared__ double sh[kThreads / kWave];
  const double t = block_sum<kThreads>(norm_pass<kThreads>(a), sh);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = t;  // gridDim.x == n_partials
}

__global__ __launch_bounds__(kThreads) void k_optim_apply(const OArgs a) {
  __shared__ double sh[kThreads / kWave];
  __shared__ Uniform shu;
  double total = 0.0, gn;
  if (a.norm) total = sum_partials(a, sh);
  if (threadIdx.x == 0) shu = make_uniform(a, total, gn);
  __syncthreads();
  apply_pass<kThreads>(a, shu);
}

__global__ __launch_bounds__(kThreads) void k_optim_finish(const OArgs a) {
  __shared__ double sh[kThreads / kWave];
  double total = 0.0, gn;
  if (a.norm) total = sum_partials(a, sh);  // the same function on the same 256 threads: the same bits as every applying block's
  if (threadIdx.x == 0) {
    const Uniform u = make_uniform(a, total, gn);
    write_state(a, u, gn);
  }
}

// ---------------------------------------------------------------------------------------------------------------------- host
constexpr uint32_t kWhatAll = TS_OPTIM_NORM | TS_OPTIM_ZERO_GRAD;
constexpr int32_t kLdsOne = (int32_t)(sizeof(double) * (kOneThreads / kWave) + sizeof(Uniform));
constexpr int32_t kLdsMulti = (int32_t)(sizeof(double) * (kThreads / kWave) + sizeof(Uniform));

struct Plan {
  int32_t form = TS_OPTIM_FORM_NONE, launches = 0, threads = 0;
  int64_t total = 0, chunks = 0, blocks = 0, ws_bytes = 0;
  int64_t cend[kMaxTensors] = {};
};

// n and every numel have been checked
Plan plan_step(int32_t n, const int64_t *numel, bool norm) {
  Plan p;
  for (int i = 0; i < n; ++i) p.total += numel[i];
  if (p.total == 0) return p;
  const bool one = p.total <= g_one_block_max.load(std::memory_order_relaxed);
  p.form = one ? TS_OPTIM_FORM_ONE : norm ? TS_OPTIM_FORM_MULTI : TS_OPTIM_FORM_APPLY;
  p.launches = one ? 1 : norm ? 3 : 2;
  p.threads = one ? kOneThreads : kThreads;
  const int64_t chunk = (int64_t)(one ? kWave : kThreads) * kPerThread;  // a wave's in the one block, a block's otherwise
  for (int i = 0; i < n; ++i) p.cend[i] = (p.chunks += (numel[i] + chunk - 1) / chunk);
  p.blocks = one ? 1 : std::min(p.chunks, kMaxBlocks);
  p.ws_bytes = p.form == TS_OPTIM_FORM_MULTI ? 8 * p.blocks : 0;
  return p;
}

struct Range {
  uintptr_t lo, hi;
  bool written;
};
// two ranges overlap and at least one of them is written: a sweep over the ranges in the order of their starts
bool hazard(Range *r, int count) {
  std::sort(r, r + count, [](const Range &x, const Range &y) { return x.lo < y.lo; });
  uintptr_t end_any = 0, end_written = 0;
  for (int i = 0; i < count; ++i) {
    if (r[i].lo < (r[i].written ? end_any : end_written)) return true;
    end_any = std::max(end_any, r[i].hi);
    if (r[i].written) end_written = std::max(end_written, r[i].hi);
  }
  return false;
}
bool misaligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }
bool bad(float x) { return !(x >= 0.0f); }                  // negative or NaN
bool bad_beta(double b) { return !(b >= 0.0 && b < 1.0); }  // outside [0, 1) or NaN

}  // namespace

extern "C" {

int32_t ts_optim_abi_version(void) { return TS_OPTIM_ABI_VERSION; }
int32_t ts_optim_last_hip_error(void) { return ts::t_last_hip_error; }

int64_t ts_optim_tuning(int32_t key, int64_t value) { return ts::tune(key == TS_OPTIM_TUNE_ONE_BLOCK_MAX ? &g_one_block_max : nullptr, value); }

int64_t ts_optim_workspace_bytes(int64_t total_numel) { return total_numel < 0 ? (int64_t)TS_ERR_ARG : total_numel == 0 ? 0 : 8 * kMaxBlocks; }

int32_t ts_describe_adam_step(int32_t n_tensors, const int64_t *numel, uint32_t what, ts_optim_desc *desc) {
  if (!desc || (n_tensors > 0 && !numel)) return TS_ERR_NULL;
  if (n_tensors < 0 || n_tensors > kMaxTensors || (what & ~kWhatAll)) return TS_ERR_ARG;
  for (int i = 0; i < n_tensors; ++i)
    if (numel[i] < 0) return TS_ERR_ARG;
  const bool norm = (what & TS_OPTIM_NORM) != 0, zero = (what & TS_OPTIM_ZERO_GRAD) != 0;
  const Plan p = plan_step(n_tensors, numel, norm);
  ts_optim_desc d{};
  d.form = p.form, d.launches = p.launches, d.threads_per_block = p.threads;
  d.total_numel = p.total;
  if (p.form != TS_OPTIM_FORM_NONE) {
    const bool one = p.form == TS_OPTIM_FORM_ONE;
    d.lds_bytes = one ? kLdsOne : kLdsMulti;
    d.blocks = p.blocks, d.chunks = p.chunks, d.workspace_bytes = p.ws_bytes;
    d.bytes_read = p.total * (16 + (norm ? 4 : 0));
    d.bytes_written = p.total * (12 + (zero ? 4 : 0)) + 16 + (norm ? 4 : 0);
    snprintf(d.name, sizeof d.name, one ? "k_optim_one" : "k_optim_apply");
    if (p.form == TS_OPTIM_FORM_MULTI) snprintf(d.norm_name, sizeof d.norm_name, "k_optim_norm");
    if (!one) snprintf(d.finish_name, sizeof d.finish_name, "k_optim_finish");
  }
  *desc = d;
  return TS_OK;
}

int32_t ts_adam_step(const ts_optim_tensors *tensors, const ts_adam_cfg *cfg, const ts_optim_out *out, void *stream) {
  if (!tensors || !cfg || !out) return TS_ERR_NULL;
  const int32_t n = tensors->n_tensors;
  if (n < 0 || n > kMaxTensors) return TS_ERR_ARG;
  for (int i = 0; i < n; ++i)
    if (tensors->numel[i] < 0) return TS_ERR_ARG;
  if (bad(cfg->lr) || bad(cfg->eps) || bad(cfg->weight_decay) || bad(cfg->max_grad_norm) || bad_beta(cfg->beta1) || bad_beta(cfg->beta2))
    return TS_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool norm = cfg->max_grad_norm > 0.0f || cfg->skip_nonfinite || out->grad_norm;
  const bool zero = cfg->zero_grad != 0;
  const Plan p = plan_step(n, tensors->numel, norm);
  if (p.form == TS_OPTIM_FORM_NONE) {  // nothing to launch, no further pointer is looked at
    if (!out->grad_norm) return TS_OK;
    if (const hipError_t e = hipMemsetAsync(out->grad_norm, 0, sizeof(float), s); e != hipSuccess) {
      ts::t_last_hip_error = (int32_t)e;
      return TS_ERR_HIP;
    }
    return TS_OK;
  }
  if (!out->counters || (p.ws_bytes && !out->workspace)) return TS_ERR_NULL;
  for (int i = 0; i < n; ++i)
    if (tensors->numel[i] > 0 && (!tensors->param[i] || !tensors->grad[i] || !tensors->m[i] || !tensors->v[i])) return TS_ERR_NULL;
  if (misaligned(out->counters, 8) || misaligned(out->workspace, 8) || misaligned(out->grad_norm, 4) || misaligned(cfg->lr_dev, 4)) return TS_ERR_ARG;
  Range ranges[4 * kMaxTensors + 4];
  int count = 0;
  const auto add = [&](const void *ptr, int64_t bytes, bool written) {
    if (ptr && bytes > 0) ranges[count++] = Range{(uintptr_t)ptr, (uintptr_t)ptr + (uintptr_t)bytes, written};
  };
  OArgs a{};
  for (int i = 0; i < n; ++i) {
    const int64_t ne = tensors->numel[i];
    a.numel[i] = ne, a.cend[i] = p.cend[i];
    if (ne == 0) continue;  // its pointers are not looked at, and no chunk is its
    float *const arr[4] = {tensors->param[i], tensors->grad[i], tensors->m[i], tensors->v[i]};
    bool vec = true;
    for (int k = 0; k < 4; ++k) {
      if (misaligned(arr[k], 4)) return TS_ERR_ARG;
      vec = vec && !misaligned(arr[k], 16);
      add(arr[k], 4 * ne, k != 1 || zero);
    }
    a.p[i] = arr[0], a.g[i] = arr[1], a.m[i] = arr[2], a.v[i] = arr[3];
    if (vec) a.vec |= 1u << i;
  }
  add(out->counters, 16, true), add(out->grad_norm, 4, true), add(cfg->lr_dev, 4, false);
  if (p.ws_bytes) add(out->workspace, p.ws_bytes, true);
  if (hazard(ranges, count)) return TS_ERR_ARG;
  a.chunks = p.chunks;
  a.counters = out->counters, a.grad_norm = out->grad_norm, a.lr_dev = cfg->lr_dev;
  a.partials = static_cast<double *>(out->workspace);
  a.n_partials = p.form == TS_OPTIM_FORM_MULTI ? (uint32_t)p.blocks : 0u;
  a.max_norm = (double)cfg->max_grad_norm;
  a.norm = norm ? 1 : 0, a.skip_nonfinite = cfg->skip_nonfinite ? 1 : 0, a.zero_grad = zero ? 1 : 0;
  a.lr = cfg->lr, a.eps = cfg->eps, a.wd = cfg->weight_decay;
  a.beta1d = cfg->beta1, a.beta2d = cfg->beta2;
  a.beta1 = (float)cfg->beta1, a.beta2 = (float)cfg->beta2;
  a.omb1 = (float)(1.0 - cfg->beta1), a.omb2 = (float)(1.0 - cfg->beta2);
  if (p.form == TS_OPTIM_FORM_ONE) {
    hipLaunchKernelGGL(k_optim_one, dim3(1), dim3(kOneThreads), 0, s, a);
    return ts::finish_launch();
  }
  if (p.form == TS_OPTIM_FORM_MULTI) {
    hipLaunchKernelGGL(k_optim_norm, dim3((uint32_t)p.blocks), dim3(kThreads), 0, s, a);
    if (const int32_t rc = ts::finish_launch(); rc != TS_OK) return rc;
  }
  hipLaunchKernelGGL(k_optim_apply, dim3((uint32_t)p.blocks), dim3(kThreads), 0, s, a);
  if (const int32_t rc = ts::finish_launch(); rc != TS_OK) return rc;
  hipLaunchKernelGGL(k_optim_finish, dim3(1), dim3(kThreads), 0, s, a);
  return ts::finish_launch();
}

}  // extern "C"
