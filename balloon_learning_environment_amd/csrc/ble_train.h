// ble_train.h -- the QR-DQN update of Dopamine 4.0.0's JaxQuantileAgent on the device: the n-step replay sampler, the
// quantile Huber loss and its dL/dlogits, the backward pass of the Dense stack on v_mfma_f32_32x32x2_f32 and optax 0.0.9's Adam; for
// one-atom networks also DQN's TD losses (JaxDQNAgent), the reference MLP agent's SARSA loss and optax's plain SGD.
//
// Determinism: no floating-point atomics anywhere.  Every sum below runs in one order fixed by the shapes (B, the layer widths, the
// number of batch slabs, itself a function of B): an update is a pure function of its inputs, and a captured graph computes the bits
// eager launches compute.
//
// Backward layout.  dW = X^T dY is a GEMM over the batch: the MFMA's K dimension is the batch row, A[i][k] = X[b][k0 + i] and
// B[k][j] = dY[b][m0 + j], both read row-major and coalesced.  The accumulator of a wave covering k0 .. k0 + 31 (k0 a multiple of 32)
// and m0 .. m0 + 63 holds, in register r of tile t, k = k0 + (r & 3) + 8 (r >> 2) + 4 half and m = m0 + 32 t + (lane & 31): registers
// 4q .. 4q + 3 are exactly the float4 (g = m0 / 64, c = k0 / 8 + q, t, lane) of the packed layout (ble_qnet.h), so the gradient is
// stored straight into a packed image, one aligned float4 per (q, t).
// dX = dY W^T reads W transposed.  The packed image is ordered for W's columns, so a lane would gather four scattered floats per MFMA
// step; instead the trainer keeps weights_t, the packed image of W^T (layer l >= 1 as a K' = M_l by M' = K_l layer, no bias), which the
// Adam kernel rewrites with every update.  dX is then the forward's own tiling over that image, with 1{X > 0} in the epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ble_qnet.h"
#include "ble_reset.h"

namespace ble {

constexpr int kTrainLossBlock = 64;       // one wave per batch row
constexpr int kReplayBlock = 256;         // one workgroup per batch row
constexpr int kAdamBlock = 256;
constexpr int kWgradSlabRows = 256;       // batch rows per dW slab (B > 256: B / 256 slabs, at most kWgradMaxSlabs)
constexpr int kWgradMaxSlabs = 16;
constexpr uint32_t kFlagReplayEmpty = 2048u, kFlagTrainAction = 4096u;

// Batch slabs of the dW reduction: a function of B alone.
inline int wgrad_slabs(int64_t b) {
  const int64_t s = b / kWgradSlabRows;
  return (int)(s < 1 ? 1 : (s > kWgradMaxSlabs ? kWgradMaxSlabs : s));
}

// ------------------------------------------------------------------------------------------------------------ replay sampling
// The n-step window that starts at step t of environment env: valid when, among t .. t + n - 1, no episode end comes before the first
// terminal (a time-limit end without a terminal invalidates it); m = n, or 1 + the position of the first terminal (term = 1).
__device__ inline bool replay_window(const ble_replay_f32& rp, int64_t t, int64_t env, int* m, int* term) {
  int mm = rp.update_horizon, tm = 0;
  for (int k = 0; k < rp.update_horizon; ++k) {
    const int64_t at = ((t + k) % rp.capacity) * rp.num_envs + env;
    if (rp.terminal[at]) { mm = k + 1; tm = 1; break; }
    if (rp.episode_end[at]) return false;
  }
  *m = mm; *term = tm;
  return true;
}

// Lane 0: row b's return, discount, action and index (t < 0: a failed draw -- zeros, index (-1, -1), BLE_FLAG_REPLAY_EMPTY).
__device__ inline void replay_emit(const ble_replay_f32& rp, const ble_train_batch_f32& bt, int64_t b, int64_t t, int64_t env, int m,
                                   int term, uint32_t* __restrict__ err_flags) {
  float ret = 0.0f, disc = 0.0f;
  uint8_t act = 0;
  if (t < 0) {
    if (err_flags != nullptr) atomicOr(err_flags, kFlagReplayEmpty);
  } else {
    for (int k = 0; k < m; ++k) {                                      // Dopamine: np.sum(float32 gamma^k table * rewards), k ascending
      const float gk = (float)pow(rp.gamma, (double)k);
      ret = __fadd_rn(ret, __fmul_rn(gk, rp.reward[((t + k) % rp.capacity) * rp.num_envs + env]));     // (rounded apart: no fma)
    }
    disc = term ? 0.0f : (float)pow(rp.gamma, (double)rp.update_horizon);
    act = rp.action[(t % rp.capacity) * rp.num_envs + env];
  }
  bt.ret[b] = ret;
  bt.discount[b] = disc;
  bt.action[b] = act;
  if (bt.index != nullptr) { bt.index[2 * b] = t; bt.index[2 * b + 1] = env; }
}

// The whole workgroup: state row b = obs[t], next_state row b = obs[t + m] (zeros when t < 0; columns >= BLE_OBS_DIM zero).
__device__ inline void replay_gather(const ble_replay_f32& rp, const ble_train_batch_f32& bt, int64_t b, int64_t t, int64_t env, int m) {
  const int quads = (int)(bt.state_stride / 4);
  float4* __restrict__ so = reinterpret_cast<float4*>(bt.state + b * bt.state_stride);
  float4* __restrict__ no = reinterpret_cast<float4*>(bt.next_state + b * bt.state_stride);
  const float4* si = t < 0 ? nullptr : reinterpret_cast<const float4*>(rp.obs + ((t % rp.capacity) * rp.num_envs + env) * rp.obs_stride);
  const float4* ni = t < 0 ? nullptr : reinterpret_cast<const float4*>(rp.obs + (((t + m) % rp.capacity) * rp.num_envs + env) * rp.obs_stride);
  for (int q = threadIdx.x; q < quads; q += blockDim.x) {
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = a;
    if (si != nullptr && 4 * q < BLE_OBS_DIM) {                      // (obs_stride is a multiple of 4 >= BLE_OBS_DIM: quad q is in the row)
      a = si[q]; c = ni[q];
      if (4 * q + 3 >= BLE_OBS_DIM) { a.w = 0.0f; c.w = 0.0f; }       // column 1099 (the last quad holds 1096 .. 1099)
    }
    so[q] = a;
    no[q] = c;
  }
}

// The Philox stream of batch row b: keyed by (seed, b, the update counter).
__device__ inline Philox replay_stream(uint64_t seed, int64_t b, uint64_t counter) {
  Philox g = philox_init(seed, (uint64_t)b, (uint32_t)counter);
  g.c3 = (uint32_t)(counter >> 32);                                  // (b < 2^32: the env key's high word is free)
  return g;
}

// One workgroup per batch row: lane 0 draws (t, env) uniformly until the window is valid, then the workgroup gathers obs[t] and obs[t + m].
__global__ __launch_bounds__(kReplayBlock) void ble_replay_sample_kernel(ble_replay_f32 rp, ble_train_batch_f32 bt, uint64_t seed,
                                                                        uint32_t* __restrict__ err_flags) {
  __shared__ int64_t s_t, s_env;
  __shared__ int s_m;
  const int64_t b = blockIdx.x;
  if (threadIdx.x == 0) {
    const int64_t count = *rp.count;
    const int64_t lo = count > rp.capacity ? count - rp.capacity : 0;
    const int64_t span = count - rp.update_horizon - lo;            // candidates t: t + n <= count - 1
    Philox g = replay_stream(seed, b, *rp.counter);
    int64_t t = -1, env = -1;
    int m = 0, term = 0;
    for (int tries = 0; span > 0 && tries < rp.max_tries; ++tries) {
      const uint64_t hi = philox_u32(g), lo32 = philox_u32(g), e32 = philox_u32(g);
      const int64_t tt = lo + (int64_t)__umul64hi((hi << 32) | lo32, (uint64_t)span);
      const int64_t ee = (int64_t)(((uint64_t)e32 * (uint64_t)rp.num_envs) >> 32);
      if (replay_window(rp, tt, ee, &m, &term)) { t = tt; env = ee; break; }
    }
    if (t < 0) { m = 0; term = 0; }
    replay_emit(rp, bt, b, t, env, m, term, err_flags);
    s_t = t; s_env = env; s_m = m;
  }
  __syncthreads();
  replay_gather(rp, bt, b, s_t, s_env, s_m);
}

// ------------------------------------------------------------------------------------------------------------ counters
__global__ void ble_train_advance_kernel(unsigned long long* __restrict__ counter) { *counter += 1ull; }

// adam_step += 1, then optax's bias corrections 1 - b^t (fp64 power rounded to fp32)
__global__ void ble_adam_prologue_kernel(unsigned long long* __restrict__ step, double b1, double b2, float* __restrict__ corr) {
  const unsigned long long t = *step + 1ull;
  *step = t;
  corr[0] = (float)(1.0 - pow(b1, (double)t));
  corr[1] = (float)(1.0 - pow(b2, (double)t));
}

// ------------------------------------------------------------------------------------------------------------ loss
// Dopamine 4.0.0 quantile_agent.train, one wave per row b:
//   a* = argmax_a mean_j z'[a, j] (ble_qnet_head_kernel's rule), T_j = ret + discount z'[a*, j], theta_i = z[action, i],
//   u_ij = T_j - theta_i, rho_ij = |tau_i - 1{u_ij < 0}| H(u_ij), tau_i = (i + 1/2) / A,
//   H(u) = u^2 / 2 if |u| <= kappa else kappa (|u| - kappa / 2) (a select: no 0 * inf),
//   L_b = sum_i (sum_j rho_ij) / A, objective mean_b L_b,
//   dL/dtheta_i = -((sum_j |tau_i - 1{u_ij < 0}| clip(u_ij, -kappa, kappa)) / A) / B  (the indicator's derivative is 0, as JAX's).
// Sums in ascending j, then ascending i.
__global__ __launch_bounds__(kTrainLossBlock) void ble_qr_loss_kernel(const float* __restrict__ logits, const float* __restrict__ tlogits,
                                                                     int64_t ld, int actions, int atoms, const float* __restrict__ ret,
                                                                     const float* __restrict__ discount, const uint8_t* __restrict__ action,
                                                                     float kappa, int64_t batch, float* __restrict__ targets,
                                                                     float* __restrict__ dlogits, float* __restrict__ loss,
                                                                     uint32_t* __restrict__ err_flags) {
  __shared__ float s_t[kQnetMaxAtoms];
  __shared__ float s_rho[kQnetMaxAtoms];
  __shared__ int s_best;
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
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
    if (valid) dl[act * atoms + i] = -((grad / (float)atoms) / (float)batch);
  }
  __syncthreads();
  if (lane == 0) {
    float l = 0.0f;
    for (int i = 0; i < atoms; ++i) l += s_rho[i];
    loss[b] = l;
  }
}

// ------------------------------------------------------------------------------------------------------------ TD losses (one atom)
// The logits [B, 3] of a one-atom network are its Q-values.  One wave per row b; lane 0 evaluates, in the order written:
//   DQN (Dopamine 4.0.0 dqn_agent.train; `other` = the target network's logits on next_state):
//     a* = argmax_a q'(s')[a] (ble_qnet_head_kernel's rule), T = ret + discount q'(s')[a*], u = T - q(s)[action],
//     kTdDqnMse:   L_b = u^2,                                            dL/dq = -((2 u) / B)
//     kTdDqnHuber: L_b = u^2 / 2 if |u| <= 1 else |u| - 1/2 (a select),  dL/dq = -(clip(u, -1, 1) / B)
//   kTdSarsaMse (the reference's mlp_agent.train; logits holds 2 B rows, the online network on state then on next_state, and so does
//   dlogits; `other` = logits + B ld):
//     T = ret + gamma q(s')[next_action], delta = q(s)[action] - T, L_b = delta^2,
//     dL/dq(s)[action] = (2 delta) / B, dL/dq(s')[next_action] = -((gamma (2 delta)) / B); mask[b] != 0: L_b and both rows are 0.
// An action >= actions (either one, for SARSA) sets BLE_FLAG_TRAIN_ACTION and zeroes the row.  targets[b] = T.
enum : int { kTdDqnMse = 0, kTdDqnHuber = 1, kTdSarsaMse = 2 };

template <int kKind>
__global__ __launch_bounds__(kTrainLossBlock) void ble_td_loss_kernel(const float* __restrict__ logits, const float* __restrict__ other,
                                                                     int64_t ld, int actions, const float* __restrict__ ret,
                                                                     const float* __restrict__ discount, const uint8_t* __restrict__ action,
                                                                     const uint8_t* __restrict__ next_action, const uint8_t* __restrict__ mask,
                                                                     float gamma, int64_t batch, float* __restrict__ targets,
                                                                     float* __restrict__ dlogits, float* __restrict__ loss,
                                                                     uint32_t* __restrict__ err_flags) {
  constexpr bool kSarsa = kKind == kTdSarsaMse;
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  float* __restrict__ dl = dlogits + b * ld;
  float* __restrict__ dn = dlogits + (batch + b) * ld;                // (SARSA: the next_state branch's row)
  for (int c = lane; c < ld; c += kTrainLossBlock) {
    dl[c] = 0.0f;
    if (kSarsa) dn[c] = 0.0f;
  }
  __syncthreads();
  if (lane != 0) return;
  const float* __restrict__ z = logits + b * ld;
  const float* __restrict__ zo = other + b * ld;
  const int act = action[b];
  const int nact = kSarsa ? (int)next_action[b] : 0;
  const bool valid = act < actions && nact < actions;
  if (!valid && err_flags != nullptr) atomicOr(err_flags, kFlagTrainAction);
  const bool live = valid && !(kSarsa && mask != nullptr && mask[b] != 0);
  const float r = ret[b];
  const float fb = (float)batch;
  float l = 0.0f;
  if (kSarsa) {
    const float qn = valid ? zo[nact] : 0.0f;
    const float p = gamma * qn;
    const float t = r + p;
    targets[b] = t;
    if (live) {
      const float delta = z[act] - t;
      const float d2 = 2.0f * delta;
      const float gd = gamma * d2;
      l = delta * delta;
      dl[act] = d2 / fb;
      dn[nact] = -(gd / fb);
    }
  } else {
    int best = 0;
    float qb = 0.0f;
    for (int a = 0; a < actions; ++a) {
      const float qa = zo[a];
      if (a == 0 || (qb == qb && (qa != qa || qa > qb))) { best = a; qb = qa; }      // (the rule: ble_qnet_head_kernel states it)
    }
    const float p = discount[b] * zo[best];
    const float t = r + p;
    targets[b] = t;
    if (live) {
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
  }
  loss[b] = l;
}

// ------------------------------------------------------------------------------------------------------------ backward
// dW (+ db) of one layer over the batch rows of slab `blockIdx.z`, one wave per (32 k) x (64 m) tile: out is the layer's packed block
// (kp x mp kernel then mp bias) of the gradient, or of the slab's partial sums.  k >= K or m >= M is written as 0.0.
__global__ __launch_bounds__(64) void ble_qnet_wgrad_kernel(const float* __restrict__ x, int64_t ldx, int k_in, int kp,
                                                            const float* __restrict__ dy, int64_t ldy, int m_out, int mp,
                                                            int64_t batch, int64_t slab_rows, float* __restrict__ out,
                                                            int64_t slab_stride) {
  const int lane = threadIdx.x, half = lane >> 5, l31 = lane & 31;
  const int k0 = blockIdx.x * 32, g = blockIdx.y;
  const int m0 = g * kQnetCols;
  const int64_t rb = (int64_t)blockIdx.z * slab_rows;
  const int64_t re = rb + slab_rows < batch ? rb + slab_rows : batch;
  float* __restrict__ o = out + blockIdx.z * slab_stride;
  const int kk = k0 + l31;
  const bool kin = kk < k_in;
  qnet_f32x16 acc0, acc1;
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
  float sb0 = 0.0f, sb1 = 0.0f;
  const bool bias = blockIdx.x == 0;
  for (int64_t b = rb; b < re; b += 8) {
    float a[4], y0[4], y1[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t row = b + 2 * s + half;
      const bool rin = row < re;
      a[s] = rin && kin ? x[row * ldx + kk] : 0.0f;
      y0[s] = rin ? dy[row * ldy + m0 + l31] : 0.0f;
      y1[s] = rin ? dy[row * ldy + m0 + 32 + l31] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], y0[s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], y1[s], acc1, 0, 0, 0);
      if (bias) { sb0 += y0[s]; sb1 += y1[s]; }
    }
  }
  const int chunks = kp / kQnetChunk;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = k0 / kQnetChunk + q;
    if (c >= chunks) break;
    const int kb = kQnetChunk * c + 4 * half;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const qnet_f32x16& acc = t == 0 ? acc0 : acc1;
      const bool min_ = m0 + 32 * t + l31 < m_out;
      float4 v;
      v.x = min_ && kb + 0 < k_in ? acc[4 * q + 0] : 0.0f;
      v.y = min_ && kb + 1 < k_in ? acc[4 * q + 1] : 0.0f;
      v.z = min_ && kb + 2 < k_in ? acc[4 * q + 2] : 0.0f;
      v.w = min_ && kb + 3 < k_in ? acc[4 * q + 3] : 0.0f;
      reinterpret_cast<float4*>(o)[((int64_t)(g * chunks + c) * 2 + t) * 64 + lane] = v;
    }
  }
  if (bias) {                                  // db: even rows (lanes 0..31) + odd rows (lanes 32..63)
    const float o0 = __shfl_down(sb0, 32), o1 = __shfl_down(sb1, 32);
    if (half == 0) {
      float* __restrict__ ob = o + (int64_t)kp * mp + m0;
      ob[l31] = m0 + l31 < m_out ? sb0 + o0 : 0.0f;
      ob[32 + l31] = m0 + 32 + l31 < m_out ? sb1 + o1 : 0.0f;
    }
  }
}

// grad[e] = partial[0][e] + partial[1][e] + ... in slab order
__global__ __launch_bounds__(256) void ble_wgrad_reduce_kernel(const float* __restrict__ partial, int slabs, int64_t stride, int64_t n,
                                                               float* __restrict__ grad) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float s = partial[e];
  for (int k = 1; k < slabs; ++k) s += partial[k * stride + e];
  grad[e] = s;
}

// dX[r][0 .. mp') = (dY[r] . W^T) * 1{X[r] > 0}: the forward's tiling (ble_qnet_dense_kernel, kObs = false) over the transposed image
// (kp' = round8(M), mp' = round64(K), no bias).  X: the layer's input activations (ReLU outputs: X > 0 iff the pre-activation is).
__global__ __launch_bounds__(kQnetBlock) void ble_qnet_dgrad_kernel(const float* __restrict__ dy, int64_t ld, int kp,
                                                                    const float* __restrict__ wt, const float* __restrict__ xin,
                                                                    float* __restrict__ dx, int groups, int64_t n) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t tile = blockIdx.x;
  const int g = (int)(tile % groups);
  const int64_t r0 = (tile / groups) * kQnetRows + (threadIdx.x >> 6) * 32;
  if (r0 >= n) return;
  const int half = lane >> 5;
  const int64_t row = min(r0 + (lane & 31), n - 1);
  const float* __restrict__ xr = dy + row * ld;
  const float4* __restrict__ wg = reinterpret_cast<const float4*>(wt + (int64_t)g * kp * kQnetCols) + lane;
  const int chunks = kp / kQnetChunk;
  qnet_f32x16 acc0, acc1;
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
  float4 a = qnet_load_a<false>(xr, 4 * half, 0);
  float4 b0 = wg[0], b1 = wg[64];
  for (int c = 0; c < chunks; ++c) {
    const int cn = c + 1 < chunks ? c + 1 : c;
    const float4 an = qnet_load_a<false>(xr, cn * kQnetChunk + 4 * half, 0);
    const float4 b0n = wg[(int64_t)cn * 128], b1n = wg[(int64_t)cn * 128 + 64];
    qnet_mfma4(a, b0, b1, acc0, acc1);
    a = an; b0 = b0n; b1 = b1n;
  }
  const int col = g * kQnetCols + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t rr = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (rr < n) {
      dx[rr * ld + col] = xin[rr * ld + col] > 0.0f ? acc0[r] : 0.0f;
      dx[rr * ld + col + 32] = xin[rr * ld + col + 32] > 0.0f ? acc1[r] : 0.0f;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ Adam
// The optimisers' common end: element e of the packed image has become nw; when e is a kernel element (k, m) of a layer l >= 1 it
// also goes to its slot of weights_t.
__device__ __forceinline__ void mirror_weight_t(float* __restrict__ wt, int64_t e, float nw, const TrainDims& dims) {
  int l = 0;
  while (l + 1 < dims.layers && e >= dims.offset[l + 1]) ++l;
  const int64_t r = e - dims.offset[l];
  if (l == 0 || r >= (int64_t)dims.kp[l] * dims.mp[l]) return;
  int k, mm;
  qnet_slot_km(r, dims.kp[l], &k, &mm);
  if (k < dims.k[l] && mm < dims.m[l]) wt[dims.toffset[l] + qnet_transposed_index(k, mm, (int)qnet_round_up(dims.m[l], kQnetChunk))] = nw;
}

// optax.adam (scale_by_adam, then scale(-lr)): m = (1 - b1) g + b1 m, v = (1 - b2) g^2 + b2 v,
// w += -lr (m / c1) / (sqrt(v / c2) + eps), omb = 1 - b (float64, then rounded, as optax's Python float); a kernel element also goes
// to weights_t.
__global__ __launch_bounds__(kAdamBlock) void ble_adam_kernel(float* __restrict__ w, float* __restrict__ wt, const float* __restrict__ grad,
                                                              float* __restrict__ mom, float* __restrict__ vel, const float* __restrict__ corr,
                                                              float lr, float b1, float omb1, float b2, float omb2, float eps,
                                                              TrainDims dims) {
  const int64_t e = (int64_t)blockIdx.x * kAdamBlock + threadIdx.x;
  if (e >= dims.offset[dims.layers]) return;
  const float g = grad[e];
  const float gg = g * g;
  const float m = omb1 * g + b1 * mom[e];
  const float v = omb2 * gg + b2 * vel[e];
  mom[e] = m;
  vel[e] = v;
  const float mh = m / corr[0], vh = v / corr[1];
  const float step = lr * (mh / (sqrtf(vh) + eps));
  const float nw = w[e] - step;
  w[e] = nw;
  mirror_weight_t(wt, e, nw, dims);
}

// ------------------------------------------------------------------------------------------------------------ SGD
// optax.sgd(lr) without momentum: w += -lr g, the product rounded before the sum; a kernel element also goes to weights_t, as in Adam.
// The gradient's padding is zero, so the image's stays zero.
__global__ __launch_bounds__(kAdamBlock) void ble_sgd_kernel(float* __restrict__ w, float* __restrict__ wt, const float* __restrict__ grad,
                                                             float lr, TrainDims dims) {
  const int64_t e = (int64_t)blockIdx.x * kAdamBlock + threadIdx.x;
  if (e >= dims.offset[dims.layers]) return;
  const float step = lr * grad[e];
  const float nw = w[e] - step;
  w[e] = nw;
  mirror_weight_t(wt, e, nw, dims);
}

}  // namespace ble
