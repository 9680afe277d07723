// ts_mlp.h — the network shared by the policy, train and actor-critic libraries: the sparse first layer and the heads on the
// device, the backward over a logged trajectory, and the host's block plans.
//
// Each library is a translation unit and a shared library of its own and includes this header for itself; everything here has
// internal linkage, as in ts_launch.h.  The device functions are templates on the library's argument struct A (PArgs, TArgs),
// which holds the fields they read and one constant, A::kValue: whether a value head (wv, bv; v = bv + sum_j wv[j] h_j) rides
// on the hidden layer beside the four logits.  Every statement of the value head is under `if constexpr (A::kValue)`, so each
// library compiles the code it had when these functions were written out in it (profiles/mlp_core_codegen.md, DESIGN.md
// section 19).  The __global__ kernels stay in their .hip files.
#pragma once
#include "../../include/tiler_slider_policy.h"
#include "ts_launch.h"

namespace {

using ts::kWave;
constexpr int kMaxThreads = 256;  // forward: at most four waves per block; waves interact only through the staged weights
constexpr int kMaxTargets = TS_ROLLOUT_MAX_TILES;
constexpr int kMaxTilesLane = TS_ROLLOUT_MAX_TILES;
constexpr int kChunk = 4;           // backward: steps of a board held in registers
constexpr int kCus = 256;           // backward: the grid's bound is the one-wave blocks whose LDS fits a CU's 160 KiB, at most
constexpr int kMaxBlocksPerCu = 8;  // eight, on each of 256 CUs
constexpr size_t kCuLds = 160 * 1024;

template <int S>
constexpr int max_tiles() {
  return S * S < kMaxTilesLane ? S * S : kMaxTilesLane;
}

// hs, the static pre-activations of a lane's board: the lane's column of [j][thread] in LDS
struct Hs {
  float *p;
  int stride;
  __device__ __forceinline__ Hs(float *base, int threads) : p(base), stride(threads) {}
  __device__ __forceinline__ float &at(int j) { return p[j * stride]; }
};
constexpr int kHsLdsBytesPerUnit = 4;

// LDS of a block: [w2 [H][4] | b2 [4] | with a value head: wv [H] | bv, rounded up to 16 bytes]
//                 [w1t [H][slots], where staged, rounded up to 16 bytes] [hs [H][threads]]
// and in the backward: [sd [H][64]] [gw2 [H][4] | gb1 [H] | gb2 [4] | with a value head: gwv [H] | gbv]
//                      [the w1 accumulator [H][acc_stride]]
__host__ __device__ constexpr int actor_floats(int H) { return 4 * H + 4; }  // wv starts here
template <bool V>
__host__ __device__ constexpr int head_floats(int H) {
  return V ? actor_floats(H) + ((H + 1 + 3) & ~3) : actor_floats(H);
}
template <bool V>
__host__ __device__ constexpr int small_floats(int H) {
  return V ? 6 * H + 5 : 5 * H + 4;
}

extern __shared__ float g_lds[];

// the second layer, and the tile-plane rows of w1 (features C .. C + slots - 1) transposed into [j][slot]; global reads are contiguous
template <class A>
__device__ __forceinline__ void stage_weights(const A &a, int C) {
  const int nh = 4 * a.H;
  for (int i = threadIdx.x; i < nh; i += blockDim.x) g_lds[i] = a.w2[i];
  if (threadIdx.x < 4) g_lds[nh + threadIdx.x] = a.b2[threadIdx.x];
  if constexpr (A::kValue) {
    float *wvs = g_lds + actor_floats(a.H);
    for (int i = threadIdx.x; i < a.H; i += blockDim.x) wvs[i] = a.wv[i];
    if (threadIdx.x == 0) wvs[a.H] = a.bv[0];
  }
  if (a.staged) {
    float *wt = g_lds + head_floats<A::kValue>(a.H);
    const int total = a.H * a.slots;
    const float *src = a.w1 + (int64_t)C * a.H;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int slot = i / a.H, j = i - slot * a.H;
      wt[j * a.slots + slot] = src[i];
    }
  }
  __syncthreads();
}

// the prologue: everything of the first layer that the tiles cannot change
template <int S, class A, class M>
__device__ __forceinline__ void static_preact(const A &a, Hs &hs, M blk, M tgm, const uint32_t (&tg)[kMaxTargets]) {
  constexpr int C = S * S;
  const int H = a.H;
  for (int j = 0; j < H; ++j) hs.at(j) = a.b1[j];
  // one feature per lane and round: the lowest bit left of the lane's mask, until no lane of the wave has one
  auto add_bits = [&](M m, int plane) {
    while (__builtin_amdgcn_ballot_w64(m != 0) != 0) {
      const bool has = m != 0;
      const int p = has ? ts::lsb(m) : 0;
      m &= m - 1;
      const float *row = a.w1 + (int64_t)(plane * C + p) * H;
      for (int j = 0; j < H; ++j) hs.at(j) += has ? row[j] : 0.0f;
    }
  };
  add_bits(blk, 0);
  if (a.mc) {
#pragma unroll
    for (int t = 0; t < kMaxTargets; ++t) {
      if (t < a.Tt) {
        const float *row = a.w1 + (int64_t)((1 + a.T + t) * C + (int)tg[t]) * H;
        for (int j = 0; j < H; ++j) hs.at(j) += row[j];
      }
    }
  } else {
    add_bits(tgm, 2);
  }
}

// the logits, and with a value head the value, of the board whose clamped cells are pc[]
template <int S, int MT, class A, class... V>
__device__ __forceinline__ void logits_of(const A &a, Hs &hs, const uint32_t (&pc)[MT], float (&z)[4], V &...v) {
  static_assert(sizeof...(V) == (A::kValue ? 1 : 0), "the value is returned exactly where the network has a value head");
  using M = typename ts::Bitboard<S>::mask_t;
  constexpr int C = S * S;
  const int H = a.H, T = a.T;
  uint32_t slot[MT];
  bool inc[MT];  // single colour: a cell counts once
  M seen = 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    slot[t] = a.mc ? (uint32_t)(t * C) + pc[t] : pc[t];
    inc[t] = a.mc || !((seen >> pc[t]) & 1);
    if (t < T) seen |= M(1) << pc[t];
  }
  const float4 *w2 = reinterpret_cast<const float4 *>(g_lds);
  const float4 b2 = w2[H];
  z[0] = b2.x, z[1] = b2.y, z[2] = b2.z, z[3] = b2.w;
  const float *wvs = g_lds + actor_floats(H);
  if constexpr (A::kValue) ((v = wvs[H]), ...);
  const float *tile_rows = a.w1 + (int64_t)C * H;
  for (int j = 0; j < H; ++j) {
    float acc = hs.at(j);
    if (a.staged) {
      const float *row = g_lds + head_floats<A::kValue>(H) + j * a.slots;
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < T) acc += inc[t] ? row[slot[t]] : 0.0f;
    } else {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        if (t < T) acc += inc[t] ? tile_rows[(int64_t)slot[t] * H + j] : 0.0f;
    }
    const float h = fmaxf(acc, 0.0f);
    const float4 w = w2[j];  // one address for the whole wave: a broadcast
    z[0] = fmaf(h, w.x, z[0]), z[1] = fmaf(h, w.y, z[1]), z[2] = fmaf(h, w.z, z[2]), z[3] = fmaf(h, w.w, z[3]);
    if constexpr (A::kValue) ((v = fmaf(h, wvs[j], v)), ...);
  }
}
// the level of lane nl: obstacles, clamped targets and (single colour) their mask
template <int S>
struct Level {
  using M = typename ts::Bitboard<S>::mask_t;
  M blk, tgm;
  uint32_t tg[kMaxTargets];
};

template <int S, class A>
__device__ __forceinline__ void load_level(const A &a, int64_t nl, Level<S> &b) {
  using M = typename Level<S>::M;
  constexpr int C = S * S;
  constexpr M kFull = C == 64 ? ~M(0) : (M(1) << (C & 63)) - 1;
  const int64_t N = a.N;
  b.blk = ts::load_obstacles<S>(a.blk, N, nl) & kFull;
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) b.tg[j] = 0;
  if (a.Tt > 0) {
#pragma unroll
    for (int j = 0; j < kMaxTargets; ++j) b.tg[j] = a.tgt[(int64_t)min(j, a.Tt - 1) * N + nl];
  }
  b.tgm = 0;
#pragma unroll
  for (int j = 0; j < kMaxTargets; ++j) {
    b.tg[j] = min(b.tg[j], (uint32_t)(C - 1));
    if (j < a.Tt) b.tgm |= M(1) << b.tg[j];
  }
}

// row t of sample k's cells: c[0] is `first`, c[k] is pos_log[k - 1]
template <class A>
__device__ __forceinline__ const uint8_t *cells_of(const A &a, int k) {
  return k == 0 ? a.first : a.pos_log + (int64_t)(k - 1) * a.T * a.N;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// The whole backward for one answer of the plan (the design: ts_train.hip's file comment).  STAGED and MODE are constants of the
// body so that only the addresses of the path taken are kept across the loop over the hidden units (with both kept the kernel
// spilled); the kernels dispatch on a.staged / a.mode themselves (from a shared function all 16 backward kernels came out
// different).  The value head adds dv to the chunk (8 registers per step instead of 7), a sixth running sum per unit and gwv, gbv.
template <int S, bool STAGED, int MODE, class A>
__device__ __forceinline__ void backward_body(const A &a) {
  using M = typename Level<S>::M;
  constexpr bool V = A::kValue;
  constexpr int C = S * S, MT = max_tiles<S>();
  const int H = a.H, T = a.T, K = a.steps;
  const int64_t N = a.N;
  const int lane = threadIdx.x;
  const bool mc = a.mc != 0;

  stage_weights(a, C);
  float *wt = g_lds + head_floats<V>(H);
  float *hs_base = wt + a.wt_floats;
  float *sd = hs_base + H * kWave + lane;  // the lane's column of sum_k dp_j
  float *gsm = hs_base + 2 * H * kWave;    // gw2 [H][4] | gb1 [H] | gb2 [4] | gwv [H] | gbv
  float *acc = gsm + small_floats<V>(H);   // mode 2: [H][acc_stride] over all features; mode 1: over the tile slots
  const int acc_floats = MODE != 0 ? H * a.acc_stride : 0;
  for (int i = lane; i < small_floats<V>(H) + acc_floats; i += kWave) gsm[i] = 0.0f;
  __syncthreads();

  Hs hs(hs_base + lane, kWave);
  const float4 *w2 = reinterpret_cast<const float4 *>(g_lds);
  const float *wvs = g_lds + actor_floats(H);
  const float *tile_rows = a.w1 + (int64_t)C * H;
  float gb2x = 0.0f, gb2y = 0.0f, gb2z = 0.0f, gb2w = 0.0f, gbv = 0.0f;
  const int64_t groups = (N + kWave - 1) / kWave;

  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t n = g * kWave + lane;
    const bool live = n < N;
    const int64_t nl = live ? n : N - 1;
    Level<S> b;
    load_level<S>(a, nl, b);
    static_preact<S>(a, hs, b.blk, b.tgm, b.tg);
    for (int j = 0; j < H; ++j) sd[j * kWave] = 0.0f;

    for (int k0 = 0; k0 < K; k0 += kChunk) {
      // ---- the chunk: cells (a byte per tile), the mask of the tiles that count, dz, dv; dead lanes and steps past K hold dz = dv = 0
      uint64_t cells[kChunk];
      uint32_t inc[kChunk];
      float4 dz[kChunk];
      float dv[kChunk];
#pragma unroll
      for (int kk = 0; kk < kChunk; ++kk) {
        const int k = k0 + kk;
        const bool valid = live && k < K;
        const int kc = k < K ? k : K - 1;
        uint32_t pc[MT];  // written out here and in the forward kernels: as a function, every form tried changed the kernels of both
#pragma unroll
        for (int t = 0; t < MT; ++t) pc[t] = 0;
        if (T > 0) {
          const uint8_t *src = cells_of(a, kc);
#pragma unroll
          for (int t = 0; t < MT; ++t) pc[t] = src[(int64_t)min(t, T - 1) * N + nl];
        }
        uint64_t packed = 0;
        uint32_t m = 0;
        M seen = 0;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          pc[t] = min(pc[t], (uint32_t)(C - 1));
          packed |= (uint64_t)pc[t] << (8 * t);
          if (t < T) {
            if (mc || !((seen >> pc[t]) & 1)) m |= 1u << t;
            seen |= M(1) << pc[t];
          }
        }
        cells[kk] = packed;
        inc[kk] = valid ? m : 0u;
        const float4 d = reinterpret_cast<const float4 *>(a.dz)[(int64_t)kc * N + nl];
        dz[kk] = valid ? d : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (V) dv[kk] = valid ? a.dv[(int64_t)kc * N + nl] : 0.0f;
        gb2x += dz[kk].x, gb2y += dz[kk].y, gb2z += dz[kk].z, gb2w += dz[kk].w;
        if constexpr (V) gbv += dv[kk];
      }

      // ---- unit outside, step inside
      for (int j = 0; j < H; ++j) {
        const float4 w = w2[j];
        float wvj = 0.0f;
        if constexpr (V) wvj = wvs[j];
        const float hsj = hs.at(j);
        const float *row = wt + j * a.slots;
        float *acc_row = acc + j * a.acc_stride + (MODE == 2 ? C : 0);
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, sv = 0.0f, sdp = 0.0f;
#pragma unroll
        for (int kk = 0; kk < kChunk; ++kk) {
          float pre = hsj;
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            if (t < T) {
              const uint32_t cell = (uint32_t)(cells[kk] >> (8 * t)) & 0xffu;
              const uint32_t slot = mc ? (uint32_t)(t * C) + cell : cell;
              const bool on = (inc[kk] >> t) & 1u;
              const float wt_v = STAGED ? row[slot] : tile_rows[slot * (uint32_t)H + (uint32_t)j];
              pre += on ? wt_v : 0.0f;
            }
          }
          const float h = fmaxf(pre, 0.0f);
          // two expressions on purpose: with a zero for wvj * dv the first is not the second for signed zeros
          float dh;
          if constexpr (V)
            dh = fmaf(w.x, dz[kk].x, fmaf(w.y, dz[kk].y, fmaf(w.z, dz[kk].z, fmaf(w.w, dz[kk].w, wvj * dv[kk]))));
          else
            dh = fmaf(w.x, dz[kk].x, fmaf(w.y, dz[kk].y, fmaf(w.z, dz[kk].z, w.w * dz[kk].w)));
          const float dp = pre > 0.0f ? dh : 0.0f;
          s0 = fmaf(h, dz[kk].x, s0), s1 = fmaf(h, dz[kk].y, s1), s2 = fmaf(h, dz[kk].z, s2), s3 = fmaf(h, dz[kk].w, s3);
          if constexpr (V) sv = fmaf(h, dv[kk], sv);
          sdp += dp;
          if (dp != 0.0f) {  // the tile features of this sample
#pragma unroll
            for (int t = 0; t < MT; ++t) {
              if (t < T && ((inc[kk] >> t) & 1u)) {
                const uint32_t cell = (uint32_t)(cells[kk] >> (8 * t)) & 0xffu;
                const uint32_t slot = mc ? (uint32_t)(t * C) + cell : cell;
                if constexpr (MODE != 0)
                  atomicAdd(acc_row + slot, dp);
                else
                  atomicAdd(a.gw1 + ((uint32_t)C + slot) * (uint32_t)H + (uint32_t)j, dp);
              }
            }
          }
        }
        sd[j * kWave] += sdp;
        s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2), s3 = wave_sum(s3);
        if constexpr (V) sv = wave_sum(sv);
        if (lane == 0) {
          float4 *gw2 = reinterpret_cast<float4 *>(gsm) + j;
          float4 v = *gw2;
          v.x += s0, v.y += s1, v.z += s2, v.w += s3;
          *gw2 = v;
          if constexpr (V) gsm[5 * H + 4 + j] += sv;
        }
      }
    }

    // ---- once per board and unit: b1 and the constant features (obstacles, targets) receive sum_k dp_j
    for (int j = 0; j < H; ++j) {
      const float s = wave_sum(sd[j * kWave]);
      if (lane == 0) gsm[4 * H + j] += s;
    }
    auto scatter = [&](int feature, bool has) {
      if constexpr (MODE == 2) {
        for (int j = 0; j < H; ++j) {
          const float v = sd[j * kWave];
          if (has && v != 0.0f) atomicAdd(acc + j * a.acc_stride + feature, v);
        }
      } else {
        float *row = a.gw1 + (int64_t)feature * H;
        for (int j = 0; j < H; ++j) {
          const float v = sd[j * kWave];
          if (has && v != 0.0f) atomicAdd(row + j, v);
        }
      }
    };
    auto scatter_bits = [&](M m, int plane) {
      if (!live) m = 0;
      while (__builtin_amdgcn_ballot_w64(m != 0) != 0) {
        const bool has = m != 0;
        const int p = has ? ts::lsb(m) : 0;
        m &= m - 1;
        scatter(plane * C + p, has);
      }
    };
    scatter_bits(b.blk, 0);
    if (mc) {
#pragma unroll
      for (int t = 0; t < kMaxTargets; ++t)
        if (t < a.Tt) scatter((1 + T + t) * C + (int)b.tg[t], live);
    } else {
      scatter_bits(b.tgm, 2);
    }
  }

  gb2x = wave_sum(gb2x), gb2y = wave_sum(gb2y), gb2z = wave_sum(gb2z), gb2w = wave_sum(gb2w);
  if constexpr (V) gbv = wave_sum(gbv);
  if (lane == 0) {
    gsm[5 * H] = gb2x, gsm[5 * H + 1] = gb2y, gsm[5 * H + 2] = gb2z, gsm[5 * H + 3] = gb2w;
    if constexpr (V) gsm[6 * H + 4] = gbv;
  }
  __syncthreads();

  // ---- the flush, once per block: contiguous rows, exact zeros skipped
  auto flush = [&](float *dst, const float *src, int count) {
    for (int i = lane; i < count; i += kWave) {
      const float v = src[i];
      if (v != 0.0f) atomicAdd(dst + i, v);
    }
  };
  flush(a.gw2, gsm, 4 * H);
  flush(a.gb1, gsm + 4 * H, H);
  flush(a.gb2, gsm + 5 * H, 4);
  if constexpr (V) {
    flush(a.gwv, gsm + 5 * H + 4, H);
    flush(a.gbv, gsm + 6 * H + 4, 1);
  }
  if constexpr (MODE != 0) {
    const int first_feature = MODE == 2 ? 0 : C;
    const int count = (MODE == 2 ? a.D : a.slots) * H;
    float *dst = a.gw1 + (int64_t)first_feature * H;
    for (int i = lane; i < count; i += kWave) {
      const int f = i / H, j = i - f * H;
      const float v = acc[j * a.acc_stride + f];
      if (v != 0.0f) atomicAdd(dst + i, v);
    }
  }
}

// ---- the host side ----

// valid dims: the random rollout's shapes (a board's dynamic and static state stays in registers), every allowed width
inline bool shape_supported(const ts_dims *d, int32_t hidden) {
  return d->size <= TS_ROLLOUT_MAX_SIZE && d->n_tiles <= TS_ROLLOUT_MAX_TILES && d->n_targets <= TS_ROLLOUT_MAX_TILES && hidden >= 1 &&
         hidden <= TS_POLICY_MAX_HIDDEN;
}
// ts_policy_supported, ts_train_supported, ts_ac_supported
inline int32_t supported(const ts_dims *dims, int32_t hidden) {
  const int32_t rc = ts::check_dims(dims);
  if (rc == TS_ERR_LIMIT) return 0;
  if (rc != TS_OK) return rc;
  return shape_supported(dims, hidden) ? 1 : 0;
}

inline bool mlp_complete(const ts_mlp *mlp) { return mlp->w1 && mlp->b1 && mlp->w2 && mlp->b2; }

inline int features_of(const ts_dims *d) { return (d->multi_color ? 1 + d->n_tiles + d->n_targets : 3) * d->size * d->size; }

// what a launch decides before it is made; D, mode and acc_stride are the backward's
template <class A, class Desc>
struct Plan {
  using Kernel = void (*)(const A);
  Kernel kernel = nullptr;
  uint32_t blocks = 0, threads = 0;
  size_t lds = 0;
  int32_t slots = 0, staged = 0, wt_floats = 0, D = 0, mode = 0, acc_stride = 0;
  Desc desc{};
};

// The forward's block of a supported shape: the most waves (four, two, one) whose hs columns leave room, behind the second
// layer, for the tile-plane weights in the LDS a block may ask for; where not even one wave's do, the weights stay in global
// memory.
template <class A, class Desc>
void plan_forward_block(const ts_dims *d, int32_t H, Plan<A, Desc> &p) {
  const int C = d->size * d->size;
  p.slots = (d->multi_color ? d->n_tiles : 1) * C;
  const size_t wt_bytes = d->n_tiles > 0 ? ((size_t)H * p.slots * 4u + 15u) & ~(size_t)15u : 0u;
  const size_t hs_bytes = (size_t)H * kHsLdsBytesPerUnit;             // per thread
  const size_t head_bytes = (size_t)head_floats<A::kValue>(H) * 4u;  // the second layer, always staged
  p.threads = 0;
  for (const uint32_t threads : {256u, 128u, 64u}) {
    if (wt_bytes > 0 && head_bytes + wt_bytes + hs_bytes * threads <= ts::kMaxBlockLds) {
      p.threads = threads, p.staged = 1, p.wt_floats = (int32_t)(wt_bytes / 4u);
      break;
    }
  }
  if (!p.threads) {
    p.staged = 0, p.wt_floats = 0;
    p.threads = head_bytes + hs_bytes * 256u <= ts::kMaxBlockLds ? 256u : head_bytes + hs_bytes * 128u <= ts::kMaxBlockLds ? 128u : 64u;
  }
  p.lds = head_bytes + (size_t)p.wt_floats * 4u + hs_bytes * p.threads;
}

// The backward's block, one wave: the second layer, hs and sd columns and the small accumulators always; then, in this order
// of preference, the whole w1 accumulator (2), its tile planes (1), or none (0); then the staged tile-plane weights if they
// still fit.
template <class A, class Desc>
void plan_backward_block(const ts_dims *d, int32_t H, Plan<A, Desc> &p) {
  constexpr bool V = A::kValue;
  const int C = d->size * d->size;
  p.slots = (d->multi_color ? d->n_tiles : 1) * C;
  p.D = features_of(d);
  p.threads = kWave;
  const size_t wt_bytes = d->n_tiles > 0 ? ((size_t)H * p.slots * 4u + 15u) & ~(size_t)15u : 0u;
  const size_t fixed = (size_t)head_floats<V>(H) * 4u + 2u * (size_t)H * kHsLdsBytesPerUnit * kWave + (size_t)small_floats<V>(H) * 4u;
  const size_t whole = (size_t)H * (p.D | 1) * 4u, tiles = (size_t)H * (p.slots | 1) * 4u;
  size_t acc_bytes = 0;
  if (fixed + whole <= ts::kMaxBlockLds) {
    p.mode = 2, p.acc_stride = p.D | 1, acc_bytes = whole;
  } else if (d->n_tiles > 0 && fixed + tiles <= ts::kMaxBlockLds) {
    p.mode = 1, p.acc_stride = p.slots | 1, acc_bytes = tiles;
  } else {
    p.mode = 0, p.acc_stride = 0;
  }
  p.staged = wt_bytes > 0 && fixed + acc_bytes + wt_bytes <= ts::kMaxBlockLds ? 1 : 0;
  p.wt_floats = p.staged ? (int32_t)(wt_bytes / 4u) : 0;
  p.lds = fixed + acc_bytes + (size_t)p.wt_floats * 4u;
}

// what tells the train and the actor-critic library apart on the host
template <class A>
struct TrainKernels {
  using Kernel = void (*)(const A);
  const char *forward_stem, *backward_stem;  // "k_train_forward" -> "k_train_forward<4>"
  Kernel (*forward)(int S), (*backward)(int S);
  int sample_bytes;  // what the forward writes per sample
};

// Every check of a forward or backward over a trajectory that needs no pointer, and the launch the call would make
template <class A, class Desc>
int32_t plan_train(const ts_dims *d, int32_t hidden, int32_t steps, bool backward, const TrainKernels<A> &lib, Plan<A, Desc> &p) {
  if (const int32_t rc = ts::check_dims(d); rc != TS_OK) return rc;
  if (!shape_supported(d, hidden)) return TS_ERR_LIMIT;
  if (steps < 1 || steps > TS_ROLLOUT_MAX_STEPS) return TS_ERR_ARG;
  if (backward)
    plan_backward_block(d, hidden, p);
  else
    plan_forward_block(d, hidden, p);
  p.desc.threads_per_block = (int32_t)p.threads;
  p.desc.lds_bytes = (int32_t)p.lds;
  p.desc.weights_in_lds = p.staged;
  p.desc.grads_in_lds = p.mode;
  p.desc.chunk_steps = backward ? kChunk : 0;
  p.desc.samples = (int64_t)steps * d->n_boards;
  if (d->n_boards == 0) return TS_OK;  // nothing is launched
  const int64_t groups = (d->n_boards + p.threads - 1) / p.threads;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kMaxBlocksPerCu, (int64_t)(kCuLds / p.lds)));
  const int64_t blocks = backward ? std::min<int64_t>(groups, kCus * per_cu) : groups;
  p.kernel = backward ? lib.backward(d->size) : lib.forward(d->size);
  if (!p.kernel || blocks > 0x7fffffffll) return TS_ERR_LIMIT;
  p.blocks = (uint32_t)blocks;
  p.desc.blocks = blocks;
  if (backward) {
    const int64_t w1_floats = p.mode == 2 ? (int64_t)p.D * hidden : p.mode == 1 ? (int64_t)p.slots * hidden : 0;
    p.desc.flush_bytes = blocks * 4 * (small_floats<A::kValue>(hidden) + w1_floats);
  } else {
    p.desc.flush_bytes = lib.sample_bytes * p.desc.samples;
  }
  snprintf(p.desc.name, sizeof p.desc.name, "%s<%d>", backward ? lib.backward_stem : lib.forward_stem, d->size);
  return TS_OK;
}

template <class A, class Desc>
int32_t describe_train(const ts_dims *dims, int32_t hidden, int32_t steps, bool backward, const TrainKernels<A> &lib, Desc *desc) {
  if (!dims || !desc) return TS_ERR_NULL;
  Plan<A, Desc> p;
  const int32_t rc = plan_train(dims, hidden, steps, backward, lib, p);
  if (rc != TS_OK) return rc;
  *desc = p.desc;
  return TS_OK;
}

}  // namespace
