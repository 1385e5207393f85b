// ble_actor.h -- on-policy training on the device: a two-atom network read as actor and critic (policy logit of action a
// = z[2a], state value = z[1]; z[3] and z[5] are not read), its sampling head, generalised advantage estimation over a [T][N] block,
// the advantage normalisation and the PPO loss head that emits dL/dlogits for ble_train.h's backward pass.
//
// Everything is fp32 with one rounding per operation written (the build contracts a * b + c only inside one expression, so every
// product and sum below is its own statement); every branch is a select, never a product with a 0/1 mask, so a NaN or inf of the
// branch not taken cannot leak.  No floating-point atomics: every reduction order is fixed by the shapes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ble_qnet.h"
#include "ble_reset.h"
#include "ble_train.h"

namespace ble {

constexpr uint64_t kActorStream = 0x4143544F52ull;      // "ACTOR": apart from the epsilon-greedy stream of the same seed
constexpr int kAdvNormBlock = 256;

struct AcSoftmax {
  float lp[3], p[3];
};

// log-softmax and softmax of three logits, used by both heads so that their bits agree.  Finite logits give finite lp.
__device__ __forceinline__ AcSoftmax ac_log_softmax(float z0, float z1, float z2) {
  AcSoftmax r;
  const float m = fmaxf(fmaxf(z0, z1), z2);
  const float d0 = z0 - m, d1 = z1 - m, d2 = z2 - m;
  const float e0 = expf(d0), e1 = expf(d1), e2 = expf(d2);
  const float s01 = e0 + e1;
  const float s = s01 + e2;
  const float ls = logf(s);
  r.lp[0] = d0 - ls; r.lp[1] = d1 - ls; r.lp[2] = d2 - ls;
  r.p[0] = e0 / s; r.p[1] = e1 / s; r.p[2] = e2 / s;
  return r;
}

// One lane per row of the last layer's output.  Greedy (step == nullptr): argmax over z[0], z[2], z[4] with ble_qnet_head_kernel's rule.
// Sampled: the inverse CDF of the softmax at u = (w >> 8) 2^-24, w the first word of the Philox stream of
// (seed ^ kActorStream, env_offset + i, *step) -- ble_explore_kernel's keying, so the draw of an environment at a step does not depend
// on n or on the row's position.
__global__ __launch_bounds__(kQnetHeadBlock) void ble_ac_head_kernel(const float* __restrict__ logits, int64_t ld, uint64_t seed,
                                                                     int64_t env_offset, const unsigned long long* __restrict__ step,
                                                                     uint8_t* __restrict__ action, float* __restrict__ logp,
                                                                     float* __restrict__ value, float* __restrict__ probs, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kQnetHeadBlock + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ z = logits + i * ld;
  const float z0 = z[0], z1 = z[2], z2 = z[4];
  const AcSoftmax sm = ac_log_softmax(z0, z1, z2);
  int act;
  if (step == nullptr) {
    const float q[3] = {z0, z1, z2};
    act = 0;
    float qb = q[0];
    for (int a = 1; a < 3; ++a) {
      if (qb == qb && (q[a] != q[a] || q[a] > qb)) { act = a; qb = q[a]; }      // (the rule: ble_qnet_head_kernel states it)
    }
  } else {
    const uint64_t st = *step;
    Philox g = philox_init(seed ^ kActorStream, (uint64_t)(env_offset + i), (uint32_t)st);
    g.key1 ^= (uint32_t)(st >> 32);
    const uint32_t w = philox_u32(g);
    const float u = (float)(w >> 8) * (1.0f / 16777216.0f);             // [0, 1), 24 bits
    const float c0 = sm.p[0];
    const float c1 = sm.p[0] + sm.p[1];
    act = u < c0 ? 0 : (u < c1 ? 1 : 2);
  }
  action[i] = (uint8_t)act;
  logp[i] = act == 0 ? sm.lp[0] : (act == 1 ? sm.lp[1] : sm.lp[2]);
  value[i] = z[1];
  if (probs != nullptr) {
    probs[3 * i + 0] = sm.p[0]; probs[3 * i + 1] = sm.p[1]; probs[3 * i + 2] = sm.p[2];
  }
}

// Generalised advantage estimation, one lane per environment over arrays laid out [T][N], t descending.  A terminal step bootstraps
// nothing; a step cut by the time limit (episode_end without terminal), whose next observation already belongs to the new episode,
// bootstraps from its own value; both cut the trace.
__global__ __launch_bounds__(256) void ble_gae_kernel(const float* __restrict__ reward, const float* __restrict__ value,
                                                      const float* __restrict__ boot_value, const uint8_t* __restrict__ terminal,
                                                      const uint8_t* __restrict__ episode_end, float gamma, float lambda,
                                                      float* __restrict__ advantage, float* __restrict__ ret, int64_t steps, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const float gl = __fmul_rn(gamma, lambda);
  float a_next = 0.0f;
  float nv = boot_value[e];
  for (int64_t t = steps - 1; t >= 0; --t) {
    const int64_t at = t * n + e;
    const float v = value[at];
    const bool term = terminal[at] != 0, end = episode_end[at] != 0;
    const float boot = term ? 0.0f : (end ? v : nv);
    const float p = gamma * boot;
    const float s = reward[at] + p;
    const float delta = s - v;
    const float carry = end ? 0.0f : a_next;
    const float q = gl * carry;
    const float a = delta + q;
    advantage[at] = a;
    ret[at] = a + v;
    a_next = a;
    nv = v;
  }
}

// In place A <- (A - mean) / (sqrt(var) + 1e-8) over m advantages, float64, one workgroup: thread k sums elements k, k + 256, ...
// ascending, thread 0 adds the 256 partials ascending; the variance (/ m) by a second pass of the same shape.
__global__ __launch_bounds__(kAdvNormBlock) void ble_adv_normalize_kernel(float* __restrict__ adv, int64_t m) {
  __shared__ double s_part[kAdvNormBlock];
  __shared__ double s_stat;
  const int k = threadIdx.x;
  double s = 0.0;
  for (int64_t i = k; i < m; i += kAdvNormBlock) s += (double)adv[i];
  s_part[k] = s;
  __syncthreads();
  if (k == 0) {
    double t = 0.0;
    for (int j = 0; j < kAdvNormBlock; ++j) t += s_part[j];
    s_stat = t / (double)m;
  }
  __syncthreads();
  const double mean = s_stat;
  s = 0.0;
  for (int64_t i = k; i < m; i += kAdvNormBlock) {
    const double d = (double)adv[i] - mean;
    const double d2 = d * d;
    s += d2;
  }
  __syncthreads();
  s_part[k] = s;
  __syncthreads();
  if (k == 0) {
    double t = 0.0;
    for (int j = 0; j < kAdvNormBlock; ++j) t += s_part[j];
    s_stat = sqrt(t / (double)m) + 1e-8;
  }
  __syncthreads();
  const double den = s_stat;
  for (int64_t i = k; i < m; i += kAdvNormBlock) {
    const double d = (double)adv[i] - mean;
    adv[i] = (float)(d / den);
  }
}

// The clipped PPO objective of row b, one wave per row (launched as ble_td_loss_kernel is); lane 0 evaluates, in the order written:
//   (lp, p) = ac_log_softmax(z[0], z[2], z[4]), H = -((p0 lp0 + p1 lp1) + p2 lp2), rho = exp(lp[act] - old_logp),
//   s1 = rho A, s2 = clamp(rho, 1 - clip, 1 + clip) A, active = s1 <= s2, L_pi = -(active ? s1 : s2), dv = z[1] - R,
//   L_v = c_v dv^2, L_b = (L_pi + L_v) - c_e H;
//   dL/dz[2a] = ((active ? -(A rho ((a == act) - p_a)) : 0) + c_e p_a (lp_a + H)) / B, dL/dz[1] = (2 c_v dv) / B.
// aux[b] = (lp[act], H).  An action >= 3 sets BLE_FLAG_TRAIN_ACTION and zeroes the row.
__global__ __launch_bounds__(kTrainLossBlock) void ble_ppo_loss_kernel(const float* __restrict__ logits, int64_t ld,
                                                                      const float* __restrict__ ret, const uint8_t* __restrict__ action,
                                                                      const float* __restrict__ old_logp, const float* __restrict__ advantage,
                                                                      float clip, float value_coef, float entropy_coef, int64_t batch,
                                                                      float* __restrict__ aux, float* __restrict__ dlogits,
                                                                      float* __restrict__ loss, uint32_t* __restrict__ err_flags) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  float* __restrict__ dl = dlogits + b * ld;
  for (int c = lane; c < ld; c += kTrainLossBlock) dl[c] = 0.0f;
  __syncthreads();
  if (lane != 0) return;
  const int act = action[b];
  if (act >= 3) {
    if (err_flags != nullptr) atomicOr(err_flags, kFlagTrainAction);
    loss[b] = 0.0f;
    aux[2 * b] = 0.0f; aux[2 * b + 1] = 0.0f;
    return;
  }
  const float* __restrict__ z = logits + b * ld;
  const AcSoftmax sm = ac_log_softmax(z[0], z[2], z[4]);
  const float t0 = sm.p[0] * sm.lp[0];
  const float t1 = sm.p[1] * sm.lp[1];
  const float t2 = sm.p[2] * sm.lp[2];
  const float t01 = t0 + t1;
  const float h = -(t01 + t2);
  const float lpa = act == 0 ? sm.lp[0] : (act == 1 ? sm.lp[1] : sm.lp[2]);
  const float adv = advantage[b];
  const float d = lpa - old_logp[b];
  const float rho = expf(d);
  const float s1 = rho * adv;
  const float lo = 1.0f - clip, hi = 1.0f + clip;
  const float rc = fminf(fmaxf(rho, lo), hi);
  const float s2 = rc * adv;
  const bool active = s1 <= s2;
  const float lpi = -(active ? s1 : s2);
  const float dv = z[1] - ret[b];
  const float dv2 = dv * dv;
  const float lv = value_coef * dv2;
  const float lsum = lpi + lv;
  const float eh = entropy_coef * h;
  loss[b] = lsum - eh;
  const float w = adv * rho;
  const float fb = (float)batch;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ind = a == act ? 1.0f : 0.0f;
    const float dp = ind - sm.p[a];
    const float wg = w * dp;
    const float g = active ? -wg : 0.0f;
    const float lh = sm.lp[a] + h;
    const float plh = sm.p[a] * lh;
    const float ha = entropy_coef * plh;
    const float gh = g + ha;
    dl[2 * a] = gh / fb;
  }
  const float c2 = 2.0f * value_coef;
  const float gv = c2 * dv;
  dl[1] = gv / fb;
  aux[2 * b] = lpa;
  aux[2 * b + 1] = h;
}

}  // namespace ble
