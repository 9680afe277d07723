// ts_vtrace.hip — V-trace targets: off-policy returns and advantages of a logged trajectory (include/tiler_slider_vtrace.h).
//
// A translation unit and a shared library of its own (lib/libtiler_slider_vtrace.so): the other twenty libraries are pinned symbol
// by symbol and kernel by kernel, and nothing here touches any of them.  The flag rules, the reward rule and the Manhattan reward -
// manhattan, reward_of - are RESTATED from ts_targets.hip (which copied the latter from ts_rollout.hip), not shared through a
// header: moving device code between files changes the pinned kernels.  tests/test_gpu_vtrace.py holds this
// copy to trajectory_returns() bit for bit.
//
// k_traj_vtrace<S>: ONE BOARD PER LANE, the log walked BACKWARDS in chunks of kChunk steps, as k_traj_returns walks it.  No address
// depends on loaded data, so a chunk's loads - per step two 16-byte logits rows (one where pi_logits is NULL), up to three bytes
// (flags, action, expert's move), a value and, in the kernels that read them, T cell bytes - are all issued before the first is
// consumed.  Across lanes every read and write is contiguous: a byte, a dword or 16 bytes per lane.
//
// NOTHING IN w DEPENDS ON THE RECURSION.  So a chunk runs in two parts: first, for each of its steps independently, both
// softmaxes, mu, w, rho, the reward and delta = rho (r + gamma V+ - V), kept as three floats a step - delta, gc = gamma c and
// rg = gamma rho; then the sequential part, two multiply-adds a step on the carry:
// D = gc D+ + delta and adv = rg D+ + delta.  Only V+ crosses steps in the first part, and it is a load, not a result.
//
// S = 0 is the kernel that reads NO CELLS, one for every board size: the question "are the cells read" is a template parameter,
// so that kernel holds no reward code and none of its registers.  The other uniform questions that decide LOADS - are there
// values, is there a pi_logits - are template constants of the body, asked once at the top of the kernel (ts_targets.hip's
// device), so that a chunk's loads are one straight run of code; those that decide arithmetic alone (select, beta, the expert)
// are selects.  No LDS, no barrier, no atomics: results are reproducible bit for bit.
#include "../../include/tiler_slider_vtrace.h"
#include "ts_launch.h"

#include <cmath>

namespace {

using ts::kWave;
constexpr int kThreads = 256;  // four waves per block; waves never interact
constexpr int kChunk = 4;      // steps of a board whose loads are in flight together
constexpr int kMaxTargets = TS_ROLLOUT_MAX_TILES;

struct VArgs {
  const uint8_t *first, *pos_log, *flags_log, *tgt;  // cell_t = uint8 (S <= 8)
  const uint8_t *act_log, *expert_log;               // expert_log is never NULL here: act_log stands in, `expert` says so
  const float *values, *last_value;
  const float4 *mu_logits, *pi_logits;
  float *reward, *adv, *ret, *weight, *log_mu;
  uint8_t *mask;
  int64_t N;
  int32_t T, Tt, mc, steps, vstride;
  int32_t progress;  // uniform: m(c[k]) is needed beside m(pos_log[k])
  int32_t greedy;    // uniform: TS_POLICY_GREEDY
  int32_t expert;    // uniform: beta_threshold != 0 and expert_log was given
  float eps4, one_eps, beta, one_beta;  // eps / 4, 1 - eps, beta, 1 - beta
  float gamma, lam, rho_bar, c_bar;
  float w_step, w_win, w_timeout, w_invalid, w_dist, w_progress;
};

template <int S>
constexpr int vtrace_tiles() {
  return S == 0 ? 1 : (S * S < TS_ROLLOUT_MAX_TILES ? S * S : TS_ROLLOUT_MAX_TILES);
}

__device__ __forceinline__ float pick4(const float (&v)[4], uint32_t a) {  // selects: a runtime index would go through scratch
  return a == 0u ? v[0] : a == 1u ? v[1] : a == 2u ? v[2] : v[3];
}

// e[j] = exp(z[j] - max z) and their sum: through the max, so 1 <= s <= 4
__device__ __forceinline__ float softmax_parts(const float4 z, float (&e)[4]) {
  const float mx = fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w));
  e[0] = __expf(z.x - mx), e[1] = __expf(z.y - mx), e[2] = __expf(z.z - mx), e[3] = __expf(z.w - mx);
  return (e[0] + e[1]) + (e[2] + e[3]);
}

template <int S, bool VALUES, bool PI>
__device__ __forceinline__ void vtrace_body(const VArgs &a) {
  constexpr bool CELLS = S > 0;
  constexpr int SS = CELLS ? S : 1, C = SS * SS, MT = vtrace_tiles<S>();
  const int64_t N = a.N;
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n - (int64_t)(threadIdx.x & (kWave - 1)) >= N) return;  // wave-uniform
  // lanes past the batch walk a copy of the LAST board and write nothing
  const bool live = n < N;
  const int64_t nl = live ? n : N - 1;
  const int T = a.T, Tt = a.Tt, K = a.steps;
  const bool mc = a.mc != 0, progress = a.progress != 0;

  uint32_t tg[kMaxTargets];
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) tg[j] = 0;
  if (CELLS && Tt > 0) {
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j) tg[j] = a.tgt[(int64_t)min(j, Tt - 1) * N + nl];
  }
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) tg[j] = min(tg[j], (uint32_t)(C - 1));

  // ---- restated from ts_targets.hip: the build-defined Manhattan reward of the cells c[] (include/tiler_slider.h: ts_reward) ----
  auto manhattan = [](uint32_t x, uint32_t y) -> int {
    return abs((int)(x / SS) - (int)(y / SS)) + abs((int)(x % SS) - (int)(y % SS));
  };
  auto reward_of = [&](const uint32_t (&c)[MT]) -> int32_t {
    int sum = 0;
    if (mc) {
      const int m = T < Tt ? T : Tt;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < m) sum += manhattan(c[t], tg[t]);
    } else if (Tt > 0) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (t < T) {
          int best = 1 << 30;
#pragma unroll
          for (int j = 0; j < kMaxTargets; ++j)
            if (j < Tt) best = min(best, manhattan(c[t], tg[j]));
          sum += best;
        }
      }
    }
    return -sum;
  };
  // ---- end of the restatement ----

  // a row of cells as it lies in memory: rows past the tile count read the last row, results unused
  auto load_row = [&](const uint8_t *src, uint32_t (&c)[MT]) {
#pragma unroll
    for (int t = 0; t < MT; ++t) c[t] = src[(int64_t)min(t, T - 1) * N + nl];
  };
  auto m_of = [&](uint32_t (&c)[MT]) -> int32_t {
#pragma unroll
    for (int t = 0; t < MT; ++t) c[t] = min(c[t], (uint32_t)(C - 1));
    return reward_of(c);
  };
  // c[k]: `first`, or the row below in the log (without w_progress m(c[0]) is not used: any row that can be read)
  auto row_before = [&](int k) -> const uint8_t * {
    return k > 0 ? a.pos_log + (int64_t)(k - 1) * T * N : (progress ? a.first : a.pos_log);
  };

  const float gamma = a.gamma;
  const bool greedy = a.greedy != 0, expert = a.expert != 0;
  int32_t m_carry = 0;  // m(pos_log[k]) of the step about to be walked
  if constexpr (CELLS) {
    uint32_t c[MT];
    load_row(a.pos_log + (int64_t)(K - 1) * T * N, c);
    m_carry = m_of(c);
  }
  float v_carry = a.last_value ? a.last_value[nl] : 0.0f;  // V_(k + 1)
  float d_carry = 0.0f;                                     // D+

  for (int k0 = K - 1; k0 >= 0; k0 -= kChunk) {
    // ---- the chunk's loads, all before the first use: steps k0, k0 - 1, ...; steps below 0 read step 0 again, results unused
    uint32_t f[kChunk], act[kChunk], xp[kChunk], c[kChunk][MT];
    float v[kChunk];
    float4 zm[kChunk], zp[kChunk];
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
      const int k = max(k0 - kk, 0);
      const int64_t i = (int64_t)k * N + nl;
      f[kk] = a.flags_log[i];
      act[kk] = a.act_log[i];
      xp[kk] = a.expert_log[i];
      zm[kk] = a.mu_logits[i];
      zp[kk] = zm[kk];
      if constexpr (PI) zp[kk] = a.pi_logits[i];
      v[kk] = 0.0f;
      if constexpr (VALUES) v[kk] = a.values[i * a.vstride];
      if constexpr (CELLS) {
        load_row(row_before(k), c[kk]);
      } else {
#pragma unroll
        for (int t = 0; t < MT; ++t) c[kk][t] = 0;
      }
    }
    // ---- the part that does not depend on the carry: weights, reward, delta
    float w[kChunk], lmu[kChunk], r[kChunk], delta[kChunk], gc[kChunk], rg[kChunk];
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
      const uint32_t fl = f[kk];
      const bool end = (fl & (TS_FLAG_SUCCESS | TS_FLAG_TIMEOUT)) != 0;
      const uint32_t ac = min(act[kk], 3u);
      // the behaviour policy: p_e[a], the expert's share, the random draw's share
      float e[4];
      const float s = softmax_parts(zm[kk], e);
      const float p_sample = pick4(e, ac) / s;  // IEEE division
      const float4 z = zm[kk];
      const float mx = fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w));
      const uint32_t amax = z.x == mx ? 0u : z.y == mx ? 1u : z.z == mx ? 2u : 3u;  // the lowest argmax
      const float pe = greedy ? (ac == amax ? 1.0f : 0.0f) : p_sample;
      const bool taught = expert && xp[kk] != 255u;
      const float inner = taught ? fmaf(a.beta, ac == xp[kk] ? 1.0f : 0.0f, a.one_beta * pe) : pe;
      const float mu = fmaf(a.one_eps, inner, a.eps4);
      // the target policy: where pi_logits is NULL pi IS p_sample, one value from one expression (identity 1 of the header)
      float pi = p_sample;
      if constexpr (PI) {
        float e2[4];
        const float s2 = softmax_parts(zp[kk], e2);
        pi = pick4(e2, ac) / s2;
      }
      const bool some = mu > 0.0f;
      w[kk] = some ? pi / mu : INFINITY;
      lmu[kk] = some ? __logf(mu) : -INFINITY;
      const float rho = fminf(a.rho_bar, w[kk]);
      const float cw = a.lam * fminf(a.c_bar, w[kk]);
      // the reward, ts_traj_returns' rule
      float rr = a.w_step;
      rr += (fl & TS_FLAG_SUCCESS) ? a.w_win : 0.0f;
      rr += (fl & TS_FLAG_TIMEOUT) ? a.w_timeout : 0.0f;
      rr += (fl & TS_FLAG_INVALID_MOVE) ? a.w_invalid : 0.0f;
      if constexpr (CELLS) {
        const int32_t m_after = m_carry;
        const int32_t m_before = m_of(c[kk]);
        m_carry = m_before;
        rr = fmaf(a.w_dist, (float)m_after, rr);
        if (progress) rr = fmaf(a.w_progress, (float)(m_after - m_before), rr);
      }
      r[kk] = rr;
      const float v_plus = end ? 0.0f : v_carry;
      v_carry = v[kk];
      delta[kk] = rho * (fmaf(gamma, v_plus, rr) - v[kk]);
      gc[kk] = gamma * cw;
      rg[kk] = gamma * rho;
    }
    // ---- the recursion: two multiply-adds a step
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk) {
      const int k = k0 - kk;
      if (k < 0) break;  // uniform
      const bool is_void = (f[kk] & (TS_FLAG_STEPPED_DONE | TS_FLAG_AUTORESET | TS_FLAG_BAD_ACTION)) != 0;
      const bool end = (f[kk] & (TS_FLAG_SUCCESS | TS_FLAG_TIMEOUT)) != 0;  // a select, not a zero factor: the carry may be infinite
      const float d = end ? delta[kk] : fmaf(gc[kk], d_carry, delta[kk]);
      const float adv = end ? delta[kk] : fmaf(rg[kk], d_carry, delta[kk]);
      if (!is_void) d_carry = d;
      if (live) {
        const int64_t i = (int64_t)k * N + n;
        if (a.reward) a.reward[i] = is_void ? 0.0f : r[kk];
        if (a.adv) a.adv[i] = is_void ? 0.0f : adv;
        if (a.ret) a.ret[i] = is_void ? 0.0f : v[kk] + d;
        if (a.weight) a.weight[i] = is_void ? 0.0f : w[kk];
        if (a.log_mu) a.log_mu[i] = is_void ? 0.0f : lmu[kk];
        if (a.mask) a.mask[i] = is_void ? (uint8_t)0 : (uint8_t)1;
      }
    }
  }
}

template <int S>
__global__ __launch_bounds__(kThreads) void k_traj_vtrace(const VArgs a) {
  if (a.values) {
    if (a.pi_logits) vtrace_body<S, true, true>(a);
    else vtrace_body<S, true, false>(a);
  } else {
    if (a.pi_logits) vtrace_body<S, false, true>(a);
    else vtrace_body<S, false, false>(a);
  }
}

using VtraceKernel = void (*)(const VArgs);

// S = 0: the kernel without cells
VtraceKernel vtrace_kernel(int S) {
  return ts::by_size<VtraceKernel, 0, 1, 2, 3, 4, 5, 6, 7, 8>(S, [](auto s) -> VtraceKernel { return k_traj_vtrace<s>; });
}

// valid dims: ts_targets_supported(dims, TS_TARGETS_RETURNS)'s rule, which is ts_rollout_supported(dims, TS_ROLLOUT_RANDOM)'s
bool vtrace_supported(const ts_dims *d) {
  return d->size <= TS_ROLLOUT_MAX_SIZE && d->n_tiles <= TS_ROLLOUT_MAX_TILES && d->n_targets <= TS_ROLLOUT_MAX_TILES;
}

bool valid_steps(int32_t steps) { return steps >= 1 && steps <= TS_ROLLOUT_MAX_STEPS; }
bool unit_interval(float x) { return x >= 0.0f && x <= 1.0f; }  // false for a NaN
bool valid_bar(float x) { return x >= 0.0f; }                   // false for a NaN, true for +infinity

constexpr uint32_t kOut = TS_VTRACE_OUT_REWARD | TS_VTRACE_OUT_ADV | TS_VTRACE_OUT_RET | TS_VTRACE_OUT_MASK | TS_VTRACE_OUT_WEIGHT | TS_VTRACE_OUT_LOG_MU;
constexpr uint32_t kIn = TS_VTRACE_IN_CELLS | TS_VTRACE_IN_FIRST | TS_VTRACE_IN_VALUES | TS_VTRACE_IN_LAST_VALUE | TS_VTRACE_IN_EXPERT | TS_VTRACE_IN_PI;
constexpr uint64_t kTwo32 = 1ull << 32;

struct Plan {
  uint32_t blocks = 0;  // 0: nothing is launched
  int kernel_size = 0;  // the S of k_traj_vtrace<S>
  ts_vtrace_desc desc{};
};

// Every check that needs no pointer, after dims, and the launch a call would make
int32_t plan(const ts_dims *d, int32_t steps, uint32_t what, Plan &p) {
  if (!vtrace_supported(d)) return TS_ERR_LIMIT;
  if (!valid_steps(steps)) return TS_ERR_ARG;
  if ((what & ~(kOut | kIn)) || !(what & kOut)) return TS_ERR_ARG;
  const auto bit = [&](uint32_t b) -> int64_t { return (what & b) ? 1 : 0; };
  const int64_t N = d->n_boards, K = steps, T = d->n_tiles;
  const int64_t cells = bit(TS_VTRACE_IN_CELLS) | bit(TS_VTRACE_IN_FIRST);
  p.kernel_size = cells && T > 0 ? d->size : 0;
  p.desc.threads_per_block = kThreads;
  p.desc.lds_bytes = 0;
  p.desc.chunk_steps = kChunk;
  p.desc.cells_kernel = p.kernel_size ? 1 : 0;
  p.desc.samples = K * N;
  if (N == 0) return TS_OK;  // nothing is launched
  const int64_t blocks = (N + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  p.desc.blocks = blocks;
  p.desc.bytes_read = K * N * (1 + 1 + 16 + bit(TS_VTRACE_IN_EXPERT) + 16 * bit(TS_VTRACE_IN_PI) + 4 * bit(TS_VTRACE_IN_VALUES)) +
                      cells * ((K + bit(TS_VTRACE_IN_FIRST)) * T * N + (int64_t)d->n_targets * N) + 4 * N * bit(TS_VTRACE_IN_LAST_VALUE);
  p.desc.bytes_written = K * N * (4 * (bit(TS_VTRACE_OUT_REWARD) + bit(TS_VTRACE_OUT_ADV) + bit(TS_VTRACE_OUT_RET) + bit(TS_VTRACE_OUT_WEIGHT) +
                                       bit(TS_VTRACE_OUT_LOG_MU)) + bit(TS_VTRACE_OUT_MASK));
  snprintf(p.desc.name, sizeof p.desc.name, "k_traj_vtrace<%d>", p.kernel_size);
  return TS_OK;
}

bool misaligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

}  // namespace

extern "C" {

int32_t ts_vtrace_abi_version(void) { return TS_VTRACE_ABI_VERSION; }
int32_t ts_vtrace_last_hip_error(void) { return ts::t_last_hip_error; }

int32_t ts_vtrace_supported(const ts_dims *dims) {
  const int32_t rc = ts::check_dims(dims);
  if (rc == TS_ERR_LIMIT) return 0;
  if (rc != TS_OK) return rc;
  return vtrace_supported(dims) ? 1 : 0;
}

int32_t ts_describe_traj_vtrace(const ts_dims *dims, int32_t steps, uint32_t what, ts_vtrace_desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  Plan p;
  if (const int32_t rc = plan(dims, steps, what, p); rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

int32_t ts_traj_vtrace(const ts_dims *dims, const ts_state *st, const ts_vtrace_in *in, const ts_vtrace_out *out, void *stream) {
  if (const int32_t rc = ts::check_dims(dims); rc != TS_OK) return rc;
  if (!in || !out) return TS_ERR_NULL;
  if (!vtrace_supported(dims)) return TS_ERR_LIMIT;
  if (!valid_steps(in->steps) || (in->select != TS_POLICY_GREEDY && in->select != TS_POLICY_SAMPLE) || in->explore_threshold > kTwo32 ||
      in->beta_threshold > kTwo32 || !unit_interval(in->gamma) || !unit_interval(in->lam) || !valid_bar(in->rho_bar) || !valid_bar(in->c_bar) ||
      (in->value_stride != 1 && in->value_stride != 4))
    return TS_ERR_ARG;
  if (dims->n_boards == 0) return TS_OK;  // nothing to launch, no pointer is looked at
  const bool progress = in->w_progress != 0.0f, cells = progress || in->w_dist != 0.0f;
  const bool tiles = dims->n_tiles > 0;
  if (!in->flags_log || (cells && tiles && !in->pos_log) || (progress && tiles && !in->first) ||
      (cells && tiles && dims->n_targets > 0 && (!st || !st->tgt)) || !in->act_log || !in->mu_logits ||
      (!out->reward && !out->adv && !out->ret && !out->weight && !out->log_mu && !out->mask))
    return TS_ERR_NULL;
  if (misaligned(in->mu_logits, 16) || misaligned(in->pi_logits, 16) || misaligned(in->values, 4) || misaligned(in->last_value, 4) ||
      misaligned(out->reward, 4) || misaligned(out->adv, 4) || misaligned(out->ret, 4) || misaligned(out->weight, 4) || misaligned(out->log_mu, 4))
    return TS_ERR_ARG;
  const uint32_t what = (out->reward ? TS_VTRACE_OUT_REWARD : 0u) | (out->adv ? TS_VTRACE_OUT_ADV : 0u) | (out->ret ? TS_VTRACE_OUT_RET : 0u) |
                        (out->mask ? TS_VTRACE_OUT_MASK : 0u) | (out->weight ? TS_VTRACE_OUT_WEIGHT : 0u) | (out->log_mu ? TS_VTRACE_OUT_LOG_MU : 0u) |
                        (cells ? TS_VTRACE_IN_CELLS : 0u);
  Plan p;
  if (const int32_t rc = plan(dims, in->steps, what, p); rc != TS_OK) return rc;
  VtraceKernel k = vtrace_kernel(p.kernel_size);
  if (!k) return TS_ERR_LIMIT;
  const bool read_cells = p.kernel_size != 0;
  VArgs a{};
  a.first = static_cast<const uint8_t *>(in->first), a.pos_log = static_cast<const uint8_t *>(in->pos_log), a.flags_log = in->flags_log;
  a.tgt = read_cells && st ? static_cast<const uint8_t *>(st->tgt) : nullptr;
  a.act_log = in->act_log;
  a.expert = in->beta_threshold != 0 && in->expert_log ? 1 : 0;
  a.expert_log = in->expert_log ? in->expert_log : in->act_log;  // a byte that can be read; `expert` = 0 ignores it
  a.values = in->values, a.last_value = in->last_value;
  a.mu_logits = reinterpret_cast<const float4 *>(in->mu_logits), a.pi_logits = reinterpret_cast<const float4 *>(in->pi_logits);
  a.reward = out->reward, a.adv = out->adv, a.ret = out->ret, a.weight = out->weight, a.log_mu = out->log_mu, a.mask = out->mask;
  a.N = dims->n_boards;
  a.T = dims->n_tiles, a.Tt = dims->n_targets, a.mc = dims->multi_color, a.steps = in->steps, a.vstride = in->value_stride;
  a.progress = progress ? 1 : 0;
  a.greedy = in->select == TS_POLICY_GREEDY ? 1 : 0;
  // the thresholds times 2^-32 in double (exact), rounded to float32 once; 1 - x likewise
  const double eps = (double)in->explore_threshold / (double)kTwo32, beta = (double)in->beta_threshold / (double)kTwo32;
  a.eps4 = (float)(eps / 4.0), a.one_eps = (float)(1.0 - eps), a.beta = (float)beta, a.one_beta = (float)(1.0 - beta);
  a.gamma = in->gamma, a.lam = in->lam, a.rho_bar = in->rho_bar, a.c_bar = in->c_bar;
  a.w_step = in->w_step, a.w_win = in->w_win, a.w_timeout = in->w_timeout, a.w_invalid = in->w_invalid;
  a.w_dist = in->w_dist, a.w_progress = in->w_progress;
  hipLaunchKernelGGL(k, dim3(p.blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return ts::finish_launch();
}

}  // extern "C"
