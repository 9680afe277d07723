// ts_loss.hip — the fused actor-critic loss: PPO, A2C or cross-entropy, with its gradient, in one pass over the samples
// (include/tiler_slider_loss.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_loss.so): the other nine libraries are pinned symbol
// by symbol and kernel by kernel, and nothing here touches any of them.  The library knows no board: M samples, no ts_dims.
//
// NO FLOAT ATOMICS.  Every sum over samples goes lanes -> wave (wave_sum, ts_mlp.h's idiom) -> block (LDS) -> one partial per
// block in the caller's workspace -> k_loss_finish, ONE block, which adds the partials in a fixed order.  The grid is bounded
// at kMaxBlocks blocks, which fixes the number of partials; results are identical bit for bit from run to run.
//
// k_loss_stats: the first pass.  count, sum adv and sum adv^2 over the live samples, from act, mask and adv alone (2 or 6 bytes a
// sample).  The count is an integer; the two sums are float64 (the pass is bound by its loads, and sigma from float32 sums of
// squares would cancel).  k_loss_finish(phase 0) turns them into the header of the workspace: count, c, mu, sigma + 1e-8.
//
// k_loss_main: ONE SAMPLE PER LANE, grid-stride.  No address depends on loaded data, so a step's loads - the logits and the old
// logits as one 16-byte load each, act and mask as bytes, adv, values and ret as dwords - are all issued before the first is
// consumed; lanes past the batch read the LAST sample and write nothing.  The four uniform questions (old_logits? a value term?
// adv? mask?) are template constants of the body, asked once at the top of the kernel (ts_targets.hip's device), so that a
// step is one straight run of code.  One 16-byte store and one 4-byte store per sample.  k_loss_finish(phase 1) writes the
// eight scalars.
//
// Workspace, in 32-bit words: [0, 8) the header; [8, 8 + 6 B) the stats partials of B blocks (count, sum, sum of squares, 64 bits
// each, stored as two words: the workspace is only 4-byte aligned); [8 + 6 B, 8 + 11 B) the main partials (five floats a block).
#include "../../include/tiler_slider_loss.h"
#include "ts_launch.h"

#include <cmath>

namespace {

using ts::kWave;
constexpr int kThreads = TS_LOSS_THREADS;  // four waves per block
constexpr int kWaves = kThreads / kWave;
constexpr int64_t kMaxBlocks = TS_LOSS_MAX_BLOCKS;
constexpr int kHeaderWords = 8, kStatWords = 6, kMainWords = 5;
enum { kHdrCount = 0, kHdrC = 1, kHdrMu = 2, kHdrSigmaEps = 3 };
enum { kSumPi = 0, kSumV = 1, kSumH = 2, kSumKl = 3, kSumCut = 4 };

struct LArgs {
  const float4 *logits, *old_logits;
  const uint8_t *act, *mask;
  const float *adv, *values, *ret;
  float4 *dlogits;
  float *dvalues, *scalars;
  uint32_t *ws;
  int64_t M;
  uint32_t blocks;
  int32_t normalize, phase;
  float clip, value_coef, entropy_coef;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

__device__ __forceinline__ void store64(uint32_t *w, double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  w[0] = (uint32_t)b, w[1] = (uint32_t)(b >> 32);
}
__device__ __forceinline__ double load64(const uint32_t *w) {
  return __longlong_as_double((long long)((unsigned long long)w[0] | ((unsigned long long)w[1] << 32)));
}

// ---------------------------------------------------------------------------------------------------------------- first pass
template <bool ADV, bool MASK>
__device__ __forceinline__ void stats_body(const LArgs &a, double (&sh)[kWaves][3]) {
  const int64_t M = a.M, stride = (int64_t)gridDim.x * kThreads;
  double cnt = 0.0, s1 = 0.0, s2 = 0.0;  // a lane's count is a small integer: exact
  for (int64_t base = (int64_t)blockIdx.x * kThreads; base < M; base += stride) {  // block-uniform
    const int64_t i = base + threadIdx.x;
    const bool in = i < M;
    const int64_t il = in ? i : M - 1;
    const uint32_t act = a.act[il];
    uint32_t m = 1u;
    if constexpr (MASK) m = a.mask[il];
    float adv = 0.0f;
    if constexpr (ADV) adv = a.adv[il];
    const bool live = in & (act <= 3u) & (m != 0u);  // & not &&: the mask byte is loaded whatever the action byte holds
    cnt += live ? 1.0 : 0.0;
    if constexpr (ADV) {
      const double d = live ? (double)adv : 0.0;  // a select: whatever a sample that is not live holds
      s1 += d;
      s2 += d * d;
    }
  }
  cnt = wave_sum(cnt), s1 = wave_sum(s1), s2 = wave_sum(s2);
  const int wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][0] = cnt, sh[wave][1] = s1, sh[wave][2] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t *part = a.ws + kHeaderWords + (int64_t)blockIdx.x * kStatWords;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double t = sh[0][q];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) t += sh[w][q];
      store64(part + 2 * q, t);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_loss_stats(const LArgs a) {
  __shared__ double sh[kWaves][3];  // one array for the four bodies
  if (a.adv) {
    if (a.mask) stats_body<true, true>(a, sh);
    else stats_body<true, false>(a, sh);
  } else {
    if (a.mask) stats_body<false, true>(a, sh);
    else stats_body<false, false>(a, sh);
  }
}

// ------------------------------------------------------------------------------------------------- the one-block finishing kernel
__global__ __launch_bounds__(kThreads) void k_loss_finish(const LArgs a) {
  __shared__ double shd[kWaves][3];
  __shared__ float shf[kWaves][kMainWords];
  const int wave = threadIdx.x / kWave;
  const bool first = (threadIdx.x & (kWave - 1)) == 0;
  float *hdr = reinterpret_cast<float *>(a.ws);
  if (a.phase == 0) {  // uniform
    double t[3] = {0.0, 0.0, 0.0};
    for (uint32_t b = threadIdx.x; b < a.blocks; b += kThreads) {  // a fixed order: block b is always this thread's
      const uint32_t *part = a.ws + kHeaderWords + (int64_t)b * kStatWords;
#pragma unroll
      for (int q = 0; q < 3; ++q) t[q] += load64(part + 2 * q);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      t[q] = wave_sum(t[q]);
      if (first) shd[wave][q] = t[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double r[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        r[q] = shd[0][q];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) r[q] += shd[w][q];
      }
      const double n = r[0] > 1.0 ? r[0] : 1.0;
      const double mu = r[1] / n;
      double var = r[2] / n - mu * mu;
      var = var > 0.0 ? var : 0.0;
      hdr[kHdrCount] = (float)r[0];
      hdr[kHdrC] = (float)(1.0 / n);
      hdr[kHdrMu] = (float)mu;
      hdr[kHdrSigmaEps] = (float)(sqrt(var) + 1e-8);
    }
    return;
  }
  float t[kMainWords];
#pragma unroll
  for (int q = 0; q < kMainWords; ++q) t[q] = 0.0f;
  const float *parts = reinterpret_cast<const float *>(a.ws + kHeaderWords + (int64_t)a.blocks * kStatWords);
  for (uint32_t b = threadIdx.x; b < a.blocks; b += kThreads) {
#pragma unroll
    for (int q = 0; q < kMainWords; ++q) t[q] += parts[(int64_t)b * kMainWords + q];
  }
#pragma unroll
  for (int q = 0; q < kMainWords; ++q) {
    t[q] = wave_sum(t[q]);
    if (first) shf[wave][q] = t[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float r[kMainWords];
#pragma unroll
    for (int q = 0; q < kMainWords; ++q) {
      r[q] = shf[0][q];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) r[q] += shf[w][q];
    }
    const float c = hdr[kHdrC];
    float *s = a.scalars;
    s[0] = c * (r[kSumPi] + a.value_coef * r[kSumV] - a.entropy_coef * r[kSumH]);
    s[1] = c * r[kSumPi];
    s[2] = c * r[kSumV];
    s[3] = c * r[kSumH];
    s[4] = c * r[kSumKl];
    s[5] = c * r[kSumCut];
    s[6] = hdr[kHdrCount];
    s[7] = a.adv ? hdr[kHdrMu] : 0.0f;
  }
}

// ----------------------------------------------------------------------------------------------------------------- main pass
struct LogSoftmax {
  float lp[4], e[4], s;
};
// through the max: every exponent is <= 0 and one of them is 0, so 1 <= s <= 4 and every lp is finite for finite logits
__device__ __forceinline__ LogSoftmax log_softmax(const float4 z) {
  LogSoftmax o;
  const float mx = fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w));
  const float x[4] = {z.x - mx, z.y - mx, z.z - mx, z.w - mx};
#pragma unroll
  for (int j = 0; j < 4; ++j) o.e[j] = __expf(x[j]);
  o.s = (o.e[0] + o.e[1]) + (o.e[2] + o.e[3]);
  const float ls = __logf(o.s);
#pragma unroll
  for (int j = 0; j < 4; ++j) o.lp[j] = x[j] - ls;
  return o;
}
__device__ __forceinline__ float pick(const float (&v)[4], uint32_t a) {
  return a == 0u ? v[0] : a == 1u ? v[1] : a == 2u ? v[2] : v[3];
}

template <bool OLD, bool VAL, bool ADV, bool MASK>
__device__ __forceinline__ void main_body(const LArgs &a, float (&sh)[kWaves][kMainWords]) {
  const int64_t M = a.M, stride = (int64_t)gridDim.x * kThreads;
  const float *hdr = reinterpret_cast<const float *>(a.ws);
  const float c = hdr[kHdrC], mu = hdr[kHdrMu], sigma_eps = hdr[kHdrSigmaEps];
  const bool normalize = a.normalize != 0;
  const float beta = a.entropy_coef, lo = 1.0f - a.clip, hi = 1.0f + a.clip;
  const float k2 = 2.0f * c * a.value_coef;
  float sum[kMainWords];
#pragma unroll
  for (int q = 0; q < kMainWords; ++q) sum[q] = 0.0f;

  for (int64_t base = (int64_t)blockIdx.x * kThreads; base < M; base += stride) {  // block-uniform
    const int64_t i = base + threadIdx.x;
    const bool in = i < M;
    const int64_t il = in ? i : M - 1;
    // ---- the step's loads, all before the first use
    const float4 z = a.logits[il];
    float4 zo = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (OLD) zo = a.old_logits[il];
    const uint32_t act = a.act[il];
    uint32_t m = 1u;
    if constexpr (MASK) m = a.mask[il];
    float adv = 1.0f, v = 0.0f, rt = 0.0f;
    if constexpr (ADV) adv = a.adv[il];
    if constexpr (VAL) v = a.values[il], rt = a.ret[il];
    const bool live = in & (act <= 3u) & (m != 0u);  // & not &&: no load waits for another

    const LogSoftmax ls = log_softmax(z);
    const float inv = 1.0f / ls.s;
    float p[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = ls.e[j] * inv;
    const float H = -((p[0] * ls.lp[0] + p[1] * ls.lp[1]) + (p[2] * ls.lp[2] + p[3] * ls.lp[3]));
    float A = adv;
    if constexpr (ADV) {
      if (normalize) A = (adv - mu) / sigma_eps;  // uniform
    }
    const float lpa = pick(ls.lp, act);
    float lpi, g, kl = 0.0f, cut = 0.0f;
    if constexpr (OLD) {
      const LogSoftmax was = log_softmax(zo);
      const float d = lpa - pick(was.lp, act);  // log r
      const float r = __expf(d);
      const float u1 = r * A, u2 = fminf(fmaxf(r, lo), hi) * A;
      const bool unclipped = u1 <= u2;
      lpi = unclipped ? -u1 : -u2;
      g = unclipped ? -u1 : 0.0f;
      kl = (r - 1.0f) - d;
      cut = unclipped ? 0.0f : 1.0f;
    } else {
      lpi = -A * lpa;
      g = -A;
    }
    float4 dz;
    dz.x = c * (g * ((act == 0u ? 1.0f : 0.0f) - p[0]) + beta * p[0] * (ls.lp[0] + H));
    dz.y = c * (g * ((act == 1u ? 1.0f : 0.0f) - p[1]) + beta * p[1] * (ls.lp[1] + H));
    dz.z = c * (g * ((act == 2u ? 1.0f : 0.0f) - p[2]) + beta * p[2] * (ls.lp[2] + H));
    dz.w = c * (g * ((act == 3u ? 1.0f : 0.0f) - p[3]) + beta * p[3] * (ls.lp[3] + H));
    const float dv = v - rt;
    // ---- selects, not products: a sample that is not live gives exact zeros whatever it holds
    sum[kSumPi] += live ? lpi : 0.0f;
    sum[kSumH] += live ? H : 0.0f;
    if constexpr (VAL) sum[kSumV] += live ? dv * dv : 0.0f;
    if constexpr (OLD) sum[kSumKl] += live ? kl : 0.0f, sum[kSumCut] += live ? cut : 0.0f;
    if (in) {
      a.dlogits[i] = live ? dz : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if constexpr (VAL) a.dvalues[i] = live ? k2 * dv : 0.0f;
    }
  }

  const int wave = threadIdx.x / kWave;
#pragma unroll
  for (int q = 0; q < kMainWords; ++q) {
    sum[q] = wave_sum(sum[q]);
    if ((threadIdx.x & (kWave - 1)) == 0) sh[wave][q] = sum[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float *part = reinterpret_cast<float *>(a.ws + kHeaderWords + (int64_t)gridDim.x * kStatWords) + (int64_t)blockIdx.x * kMainWords;
#pragma unroll
    for (int q = 0; q < kMainWords; ++q) {
      float t = sh[0][q];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) t += sh[w][q];
      part[q] = t;
    }
  }
}

template <bool OLD, bool VAL>
__device__ __forceinline__ void main_inputs(const LArgs &a, float (&sh)[kWaves][kMainWords]) {
  if (a.adv) {
    if (a.mask) main_body<OLD, VAL, true, true>(a, sh);
    else main_body<OLD, VAL, true, false>(a, sh);
  } else {
    if (a.mask) main_body<OLD, VAL, false, true>(a, sh);
    else main_body<OLD, VAL, false, false>(a, sh);
  }
}

__global__ __launch_bounds__(kThreads) void k_loss_main(const LArgs a) {
  __shared__ float sh[kWaves][kMainWords];  // one array for the sixteen bodies
  if (a.old_logits) {
    if (a.values) main_inputs<true, true>(a, sh);
    else main_inputs<true, false>(a, sh);
  } else {
    if (a.values) main_inputs<false, true>(a, sh);
    else main_inputs<false, false>(a, sh);
  }
}

// ---------------------------------------------------------------------------------------------------------------------- host
constexpr uint32_t kWhatAll = TS_LOSS_OLD_LOGITS | TS_LOSS_VALUES | TS_LOSS_ADV | TS_LOSS_MASK;
constexpr int32_t kLdsBytes = (int32_t)(sizeof(float) * kWaves * kMainWords);

int64_t blocks_of(int64_t M) { return std::min<int64_t>((M + kThreads - 1) / kThreads, kMaxBlocks); }
int64_t workspace_bytes(int64_t M) { return M == 0 ? 0 : 4 * (kHeaderWords + (int64_t)(kStatWords + kMainWords) * blocks_of(M)); }

struct Range {
  const void *p;
  int64_t bytes;
};
bool overlap(const Range &x, const Range &y) {
  if (!x.p || !y.p || x.bytes <= 0 || y.bytes <= 0) return false;
  const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
  return a < b + (uintptr_t)y.bytes && b < a + (uintptr_t)x.bytes;
}
bool misaligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

}  // namespace

extern "C" {

int32_t ts_loss_abi_version(void) { return TS_LOSS_ABI_VERSION; }
int32_t ts_loss_last_hip_error(void) { return ts::t_last_hip_error; }

int64_t ts_loss_workspace_bytes(int64_t n_samples) { return n_samples < 0 ? (int64_t)TS_ERR_ARG : workspace_bytes(n_samples); }

int32_t ts_describe_loss(int64_t n_samples, uint32_t what, ts_loss_desc *desc) {
  if (!desc) return TS_ERR_NULL;
  if (n_samples < 0 || (what & ~kWhatAll)) return TS_ERR_ARG;
  ts_loss_desc d{};
  d.threads_per_block = kThreads;
  d.lds_bytes = kLdsBytes;
  d.samples = n_samples;
  if (n_samples > 0) {
    const auto bit = [&](uint32_t b) -> int64_t { return (what & b) ? 1 : 0; };
    const int64_t old = bit(TS_LOSS_OLD_LOGITS), val = bit(TS_LOSS_VALUES), adv = bit(TS_LOSS_ADV), mask = bit(TS_LOSS_MASK);
    d.launches = 4;
    d.blocks = d.partials = blocks_of(n_samples);
    d.workspace_bytes = workspace_bytes(n_samples);
    const int64_t first = 1 + mask + 4 * adv;                                // act, mask, adv
    const int64_t main = 16 + 16 * old + 1 + mask + 4 * adv + 8 * val;        // logits, old logits, act, mask, adv, values and ret
    d.bytes_read = n_samples * (first + main);
    d.bytes_written = n_samples * (16 + 4 * val) + 4 * TS_LOSS_SCALARS;
    snprintf(d.name, sizeof d.name, "k_loss_main");
    snprintf(d.stats_name, sizeof d.stats_name, "k_loss_stats");
    snprintf(d.finish_name, sizeof d.finish_name, "k_loss_finish");
  }
  *desc = d;
  return TS_OK;
}

int32_t ts_actor_critic_loss(const ts_loss_in *in, const ts_loss_out *out, void *stream) {
  if (!in || !out) return TS_ERR_NULL;
  const bool value_term = in->values && in->ret;
  if (in->n_samples < 0 || !(in->clip >= 0.0f) || (in->old_logits && in->clip == 0.0f) || (!in->values != !in->ret) ||
      (out->dvalues && !in->values) || (in->normalize_adv && !in->adv) || std::isnan(in->value_coef) || std::isnan(in->entropy_coef))
    return TS_ERR_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t M = in->n_samples;
  if (M == 0) {  // nothing to launch, no further pointer is looked at
    if (!out->scalars) return TS_OK;
    if (const hipError_t e = hipMemsetAsync(out->scalars, 0, sizeof(float) * TS_LOSS_SCALARS, s); e != hipSuccess) {
      ts::t_last_hip_error = (int32_t)e;
      return TS_ERR_HIP;
    }
    return TS_OK;
  }
  if (!in->logits || !in->act || !out->dlogits || !out->scalars || !out->workspace || (value_term && !out->dvalues)) return TS_ERR_NULL;
  if (misaligned(in->logits, 16) || misaligned(in->old_logits, 16) || misaligned(out->dlogits, 16) || misaligned(in->adv, 4) ||
      misaligned(in->values, 4) || misaligned(in->ret, 4) || misaligned(out->dvalues, 4) || misaligned(out->scalars, 4) ||
      misaligned(out->workspace, 4))
    return TS_ERR_ARG;
  const Range outs[4] = {{out->dlogits, 16 * M}, {out->dvalues, 4 * M}, {out->scalars, 4 * TS_LOSS_SCALARS}, {out->workspace, workspace_bytes(M)}};
  const Range ins[7] = {{in->logits, 16 * M}, {in->old_logits, 16 * M}, {in->act, M}, {in->mask, M}, {in->adv, 4 * M}, {in->values, 4 * M}, {in->ret, 4 * M}};
  for (int x = 0; x < 4; ++x) {
    for (int y = 0; y < 7; ++y)
      if (overlap(outs[x], ins[y])) return TS_ERR_ARG;
    for (int y = x + 1; y < 4; ++y)
      if (overlap(outs[x], outs[y])) return TS_ERR_ARG;
  }
  LArgs a{};
  a.logits = reinterpret_cast<const float4 *>(in->logits), a.old_logits = reinterpret_cast<const float4 *>(in->old_logits);
  a.act = in->act, a.mask = in->mask, a.adv = in->adv, a.values = in->values, a.ret = in->ret;
  a.dlogits = reinterpret_cast<float4 *>(out->dlogits), a.dvalues = out->dvalues, a.scalars = out->scalars;
  a.ws = static_cast<uint32_t *>(out->workspace);
  a.M = M, a.blocks = (uint32_t)blocks_of(M);
  a.normalize = in->normalize_adv ? 1 : 0;
  a.clip = in->clip, a.value_coef = in->value_coef, a.entropy_coef = in->entropy_coef;
  hipLaunchKernelGGL(k_loss_stats, dim3(a.blocks), dim3(kThreads), 0, s, a);
  if (const int32_t rc = ts::finish_launch(); rc != TS_OK) return rc;
  a.phase = 0;
  hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(kThreads), 0, s, a);
  if (const int32_t rc = ts::finish_launch(); rc != TS_OK) return rc;
  hipLaunchKernelGGL(k_loss_main, dim3(a.blocks), dim3(kThreads), 0, s, a);
  if (const int32_t rc = ts::finish_launch(); rc != TS_OK) return rc;
  a.phase = 1;
  hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(kThreads), 0, s, a);
  return ts::finish_launch();
}

}  // extern "C"
