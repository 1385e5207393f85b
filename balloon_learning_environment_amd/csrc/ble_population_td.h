// ble_population_td.h -- training a population of replay learners: what the off-policy grouped update
// (ble_qnet_td_step_grouped_f32) has and the on-policy one (ble_population_train.h) does not -- the two TD loss heads, the replay draw
// over one ring of P R columns and epsilon-greedy per member.  The target pass, the online forward, dW, the slab reduction, dX and Adam
// are §3q's and §3r's grouped kernels as they stand.
//
// Every kernel is a sibling of a plain one (ble_train.h, ble_explore.h) with one more coordinate, the member, in an instantiation of its
// own; the plain kernels keep their instructions.  Member p's part of every result holds the bytes the plain entry point gives member p
// alone: the statements of the losses in their order, the Philox keys and the draw's arithmetic are the plain kernels'.  No
// floating-point atomics.
#pragma once
#include "ble_explore.h"
#include "ble_train.h"

namespace ble {

// ble_qr_loss_kernel for a population, one wave per row b of the P B rows; member p = b / B.  kappa is read at [p], the divisor is
// (float) B, the member's rows.  The arithmetic is the plain kernel's, statement for statement.
__global__ __launch_bounds__(kTrainLossBlock) void ble_qr_loss_grouped_kernel(
    const float* __restrict__ logits, const float* __restrict__ tlogits, int64_t ld, int actions, int atoms, const float* __restrict__ ret,
    const float* __restrict__ discount, const uint8_t* __restrict__ action, const float* __restrict__ kappa_of, int64_t rows_per_member,
    float* __restrict__ targets, float* __restrict__ dlogits, float* __restrict__ loss, uint32_t* __restrict__ err_flags) {
  __shared__ float s_t[kQnetMaxAtoms];
  __shared__ float s_rho[kQnetMaxAtoms];
  __shared__ int s_best;
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const float kappa = kappa_of[b / rows_per_member];
  const float* __restrict__ zt = tlogits + b * ld;
  const float* __restrict__ z = logits + b * ld;
  const int act = action[b];
  if (lane == 0) {
    int best = 0;
    float qb = 0.0f;
    for (int a = 0; a < actions; ++a) {
      float s = 0.0f;
      for (int j = 0; j < atoms; ++j) s += zt[a * atoms + j];
      const float qa = s / (float)atoms;
      if (a == 0 || (qb == qb && (qa != qa || qa > qb))) { best = a; qb = qa; }      // (the rule: ble_qnet_head_kernel states it)
    }
    s_best = best;
    if (act >= actions && err_flags != nullptr) atomicOr(err_flags, kFlagTrainAction);
  }
  __syncthreads();
  const int best = s_best;
  const float r = ret[b], d = discount[b];
  for (int j = lane; j < atoms; j += kTrainLossBlock) {
    const float p = d * zt[best * atoms + j];
    const float tj = r + p;
    s_t[j] = tj;
    targets[b * atoms + j] = tj;
  }
  __syncthreads();
  float* __restrict__ dl = dlogits + b * ld;
  for (int c = lane; c < ld; c += kTrainLossBlock) dl[c] = 0.0f;
  __syncthreads();
  const bool valid = act < actions;
  for (int i = lane; i < atoms; i += kTrainLossBlock) {
    const float theta = valid ? z[act * atoms + i] : 0.0f;
    const float tau = ((float)i + 0.5f) / (float)atoms;
    float rho = 0.0f, grad = 0.0f;
    for (int j = 0; j < atoms; ++j) {
      const float u = s_t[j] - theta;
      const float w = fabsf(tau - (u < 0.0f ? 1.0f : 0.0f));
      const float au = fabsf(u);
      const float h = au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa);
      const float cl = au <= kappa ? u : (u < 0.0f ? -kappa : kappa);
      const float wh = w * h, wc = w * cl;
      rho += wh;
      grad += wc;
    }
    s_rho[i] = valid ? rho / (float)atoms : 0.0f;
    if (valid) dl[act * atoms + i] = -((grad / (float)atoms) / (float)rows_per_member);
  }
  __syncthreads();
  if (lane == 0) {
    float l = 0.0f;
    for (int i = 0; i < atoms; ++i) l += s_rho[i];
    loss[b] = l;
  }
}

// ble_td_loss_kernel<kTdDqnMse | kTdDqnHuber> for a population, one wave per row b of the P B rows: the divisor is (float) B, the
// member's rows (the DQN losses have no per-member coefficient).  SARSA has no grouped form.
template <int kKind>
__global__ __launch_bounds__(kTrainLossBlock) void ble_td_loss_grouped_kernel(
    const float* __restrict__ logits, const float* __restrict__ other, int64_t ld, int actions, const float* __restrict__ ret,
    const float* __restrict__ discount, const uint8_t* __restrict__ action, int64_t rows_per_member, float* __restrict__ targets,
    float* __restrict__ dlogits, float* __restrict__ loss, uint32_t* __restrict__ err_flags) {
  static_assert(kKind == kTdDqnMse || kKind == kTdDqnHuber, "the grouped TD loss is DQN's");
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  float* __restrict__ dl = dlogits + b * ld;
  for (int c = lane; c < ld; c += kTrainLossBlock) dl[c] = 0.0f;
  __syncthreads();
  if (lane != 0) return;
  const float* __restrict__ z = logits + b * ld;
  const float* __restrict__ zo = other + b * ld;
  const int act = action[b];
  const bool valid = act < actions;
  if (!valid && err_flags != nullptr) atomicOr(err_flags, kFlagTrainAction);
  const float r = ret[b];
  const float fb = (float)rows_per_member;
  float l = 0.0f;
  int best = 0;
  float qb = 0.0f;
  for (int a = 0; a < actions; ++a) {
    const float qa = zo[a];
    if (a == 0 || (qb == qb && (qa != qa || qa > qb))) { best = a; qb = qa; }      // (the rule: ble_qnet_head_kernel states it)
  }
  const float p = discount[b] * zo[best];
  const float t = r + p;
  targets[b] = t;
  if (valid) {
    const float u = t - z[act];
    if (kKind == kTdDqnMse) {
      const float u2 = 2.0f * u;
      l = u * u;
      dl[act] = -(u2 / fb);
    } else {
      const float au = fabsf(u);
      l = au <= 1.0f ? 0.5f * u * u : au - 0.5f;
      const float cl = au <= 1.0f ? u : (u < 0.0f ? -1.0f : 1.0f);
      dl[act] = -(cl / fb);
    }
  }
  loss[b] = l;
}

// ble_replay_sample_kernel over ONE ring of N = P R columns, columns [p R, (p + 1) R) member p's; one workgroup per batch row, P B of
// them.  Workgroup p B + b draws from replay_stream(seed[p], b, *counter): tt over the plain kernel's span, ee = (e32 R) >> 32 -- the
// draws member p's own sampler makes on a ring of its R columns -- and tests, emits and gathers at column p R + ee.
__global__ __launch_bounds__(kReplayBlock) void ble_replay_sample_grouped_kernel(ble_replay_f32 rp, ble_train_batch_f32 bt,
                                                                                const unsigned long long* __restrict__ seed_of,
                                                                                int64_t rows_per_member, int64_t envs_per_member,
                                                                                uint32_t* __restrict__ err_flags) {
  __shared__ int64_t s_t, s_env;
  __shared__ int s_m;
  const int64_t row = blockIdx.x;
  if (threadIdx.x == 0) {
    const int64_t p = row / rows_per_member, b = row - p * rows_per_member;
    const int64_t count = *rp.count;
    const int64_t lo = count > rp.capacity ? count - rp.capacity : 0;
    const int64_t span = count - rp.update_horizon - lo;            // candidates t: t + n <= count - 1
    Philox g = replay_stream((uint64_t)seed_of[p], b, *rp.counter);
    int64_t t = -1, env = -1;
    int m = 0, term = 0;
    for (int tries = 0; span > 0 && tries < rp.max_tries; ++tries) {
      const uint64_t hi = philox_u32(g), lo32 = philox_u32(g), e32 = philox_u32(g);
      const int64_t tt = lo + (int64_t)__umul64hi((hi << 32) | lo32, (uint64_t)span);
      const int64_t ee = p * envs_per_member + (int64_t)(((uint64_t)e32 * (uint64_t)envs_per_member) >> 32);
      if (replay_window(rp, tt, ee, &m, &term)) { t = tt; env = ee; break; }
    }
    if (t < 0) { m = 0; term = 0; }
    replay_emit(rp, bt, row, t, env, m, term, err_flags);
    s_t = t; s_env = env; s_m = m;
  }
  __syncthreads();
  replay_gather(rp, bt, row, s_t, s_env, s_m);
}

// ble_explore_kernel for a population of P members of R rows: row p R + r draws from the stream of (seed[p], r, step) and takes the
// random action when u < epsilon[p] -- member p's own epsilon-greedy on its R rows.
__global__ __launch_bounds__(256) void ble_explore_grouped_kernel(uint8_t* __restrict__ action, int64_t n, int64_t rows_per_member,
                                                                  const float* __restrict__ epsilon_of,
                                                                  const unsigned long long* __restrict__ seed_of, uint64_t step) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t p = i / rows_per_member, r = i - p * rows_per_member;
  Philox g = philox_init((uint64_t)seed_of[p], (uint64_t)r, (uint32_t)step);
  g.key1 ^= (uint32_t)(step >> 32);
  const uint32_t u = philox_u32(g), rnd = philox_u32(g);
  const float uf = (float)(u >> 8) * (1.0f / 16777216.0f);             // [0, 1), 24 bits
  if (uf < epsilon_of[p]) action[i] = (uint8_t)(((uint64_t)rnd * 3u) >> 32);
}

}  // namespace ble
