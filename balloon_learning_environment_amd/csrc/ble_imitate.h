// ble_imitate.h -- supervised imitation on the device: the behaviour-cloning loss head of the two-atom actor-critic of
// ble_actor.h (policy logit of action a = z[2a], state value = z[1]), which emits dL/dlogits for ble_train.h's backward pass, and the
// DAgger mixture of the learner's and the expert's actions.
//
// §3m's arithmetic rules: fp32 with one rounding per operation written (every product and sum below is its own statement), every
// branch a select, no floating-point atomics.  Both heads of ble_actor.h and this one call ac_log_softmax, so their bits agree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ble_actor.h"
#include "ble_plan.h"

namespace ble {

constexpr uint64_t kDaggerStream = 0x444147474552ull;      // "DAGGER": apart from the actor and epsilon-greedy streams of the same seed
constexpr int kDaggerMixBlock = 256;

// The smoothed cross-entropy of row b against the expert's label act = action[b], one wave per row (launched as ble_ppo_loss_kernel
// is); lane 0 evaluates, in the order written:
//   (lp, p) = ac_log_softmax(z[0], z[2], z[4]), s3 = s / 3, hi = (1 - s) + s3, q_a = (a == act) ? hi : s3,
//   CE = -((q0 lp0 + q1 lp1) + q2 lp2), dv = z[1] - R, L_b = CE + c_v dv^2;
//   dL/dz[2a] = (p_a - q_a) / B, dL/dz[1] = (2 c_v dv) / B.
// c_v == 0: ret is not read (it may be NULL), dL/dz[1] is exactly 0 and L_b = CE.  aux[b] = (lp[act], agree), agree = 1.0f when the
// greedy action of these logits (ble_ac_head_kernel's rule) is act.  An action >= 3 sets BLE_FLAG_TRAIN_ACTION and zeroes the row.
__global__ __launch_bounds__(kTrainLossBlock) void ble_bc_loss_kernel(const float* __restrict__ logits, int64_t ld,
                                                                     const float* __restrict__ ret, const uint8_t* __restrict__ action,
                                                                     float smoothing, float value_coef, int64_t batch,
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
  const float z0 = z[0], z1 = z[2], z2 = z[4];
  const AcSoftmax sm = ac_log_softmax(z0, z1, z2);
  const float s3 = smoothing / 3.0f;
  const float keep = 1.0f - smoothing;
  const float hi = keep + s3;
  const float q0 = act == 0 ? hi : s3, q1 = act == 1 ? hi : s3, q2 = act == 2 ? hi : s3;
  const float t0 = q0 * sm.lp[0];
  const float t1 = q1 * sm.lp[1];
  const float t2 = q2 * sm.lp[2];
  const float t01 = t0 + t1;
  const float ce = -(t01 + t2);
  const bool has_value = value_coef != 0.0f;
  const float r = has_value ? ret[b] : 0.0f;
  const float dv = z[1] - r;
  const float dv2 = dv * dv;
  const float lv = value_coef * dv2;
  const float lsum = ce + lv;
  loss[b] = has_value ? lsum : ce;
  const float fb = (float)batch;
  const float g0 = sm.p[0] - q0, g1 = sm.p[1] - q1, g2 = sm.p[2] - q2;
  dl[0] = g0 / fb;
  dl[2] = g1 / fb;
  dl[4] = g2 / fb;
  const float c2 = 2.0f * value_coef;
  const float gv = c2 * dv;
  const float gvb = gv / fb;
  dl[1] = has_value ? gvb : 0.0f;
  const float q[3] = {z0, z1, z2};
  int best = 0;
  float qb = q[0];
  for (int a = 1; a < 3; ++a) {
    if (qb == qb && (q[a] != q[a] || q[a] > qb)) { best = a; qb = q[a]; }      // (the rule: ble_qnet_head_kernel states it)
  }
  aux[2 * b] = act == 0 ? sm.lp[0] : (act == 1 ? sm.lp[1] : sm.lp[2]);
  aux[2 * b + 1] = best == act ? 1.0f : 0.0f;
}

// The soft cross-entropy of row b against the distribution its per-action values q = target_q[b] give, launched as
// ble_bc_loss_kernel is; lane 0 evaluates, in the order written:
//   valid_a = isfinite(q_a), y_a = valid_a ? q_a beta : -Inf, (lt, t) = ac_log_softmax(y0, y1, y2)  -- an invalid action: t_a = 0 exactly;
//   s3 = s / 3, u_a = (1 - s) t_a, t'_a = u_a + s3, (lp, p) = ac_log_softmax(z[0], z[2], z[4]),
//   CE = -((t'0 lp0 + t'1 lp1) + t'2 lp2), dv = z[1] - R, L_b = CE + c_v dv^2;
//   dL/dz[2a] = (p_a - t'_a) / B, dL/dz[1] = (2 c_v dv) / B.
// aux[b] = (lp[a*], agree): a* the valid action first in the selection's order (plan_key, then a ascending).  No valid action: loss, aux
// and the row's gradient are 0 and no flag is set (a dead environment is legitimate).  One valid action a: t = one-hot, t'_a = (1 - s) +
// s3 and t' = s3 elsewhere -- ble_bc_loss_kernel with the label a, operation for operation.
__global__ __launch_bounds__(kTrainLossBlock) void ble_soft_bc_loss_kernel(const float* __restrict__ logits, int64_t ld,
                                                                          const float* __restrict__ ret, const float* __restrict__ target_q,
                                                                          float beta, float smoothing, float value_coef, int64_t batch,
                                                                          float* __restrict__ aux, float* __restrict__ dlogits,
                                                                          float* __restrict__ loss) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  float* __restrict__ dl = dlogits + b * ld;
  for (int c = lane; c < ld; c += kTrainLossBlock) dl[c] = 0.0f;
  __syncthreads();
  if (lane != 0) return;
  const float tq0 = target_q[3 * b], tq1 = target_q[3 * b + 1], tq2 = target_q[3 * b + 2];
  const uint32_t k0 = plan_key(tq0), k1 = plan_key(tq1), k2 = plan_key(tq2);
  const bool v0 = k0 != kPlanKeyNonFinite, v1 = k1 != kPlanKeyNonFinite, v2 = k2 != kPlanKeyNonFinite;
  const bool any = v0 || v1 || v2;
  const float sy0 = tq0 * beta;
  const float sy1 = tq1 * beta;
  const float sy2 = tq2 * beta;
  const float y0 = v0 ? sy0 : -INFINITY, y1 = v1 ? sy1 : -INFINITY, y2 = v2 ? sy2 : -INFINITY;
  const AcSoftmax tm = ac_log_softmax(y0, y1, y2);
  const float* __restrict__ z = logits + b * ld;
  const float z0 = z[0], z1 = z[2], z2 = z[4];
  const AcSoftmax sm = ac_log_softmax(z0, z1, z2);
  const float s3 = smoothing / 3.0f;
  const float keep = 1.0f - smoothing;
  const float u0 = keep * tm.p[0];
  const float u1 = keep * tm.p[1];
  const float u2 = keep * tm.p[2];
  const float q0 = u0 + s3;
  const float q1 = u1 + s3;
  const float q2 = u2 + s3;
  const float t0 = q0 * sm.lp[0];
  const float t1 = q1 * sm.lp[1];
  const float t2 = q2 * sm.lp[2];
  const float t01 = t0 + t1;
  const float ce = -(t01 + t2);
  const bool has_value = value_coef != 0.0f;
  const float r = has_value ? ret[b] : 0.0f;
  const float dv = z[1] - r;
  const float dv2 = dv * dv;
  const float lv = value_coef * dv2;
  const float lsum = ce + lv;
  const float row_loss = has_value ? lsum : ce;
  loss[b] = any ? row_loss : 0.0f;
  const float fb = (float)batch;
  const float g0 = sm.p[0] - q0, g1 = sm.p[1] - q1, g2 = sm.p[2] - q2;
  const float d0 = g0 / fb;
  const float d1 = g1 / fb;
  const float d2 = g2 / fb;
  dl[0] = any ? d0 : 0.0f;
  dl[2] = any ? d1 : 0.0f;
  dl[4] = any ? d2 : 0.0f;
  const float c2 = 2.0f * value_coef;
  const float gv = c2 * dv;
  const float gvb = gv / fb;
  dl[1] = (has_value && any) ? gvb : 0.0f;
  // a*: the first of the three in the selection's order
  int star = 0;
  uint32_t ks = k0;
  if (plan_before(k1, 1, ks, star)) { star = 1; ks = k1; }
  if (plan_before(k2, 2, ks, star)) { star = 2; ks = k2; }
  const float q[3] = {z0, z1, z2};
  int best = 0;
  float qb = q[0];
  for (int a = 1; a < 3; ++a) {
    if (qb == qb && (q[a] != q[a] || q[a] > qb)) { best = a; qb = q[a]; }      // (the rule: ble_qnet_head_kernel states it)
  }
  const float lps = star == 0 ? sm.lp[0] : (star == 1 ? sm.lp[1] : sm.lp[2]);
  aux[2 * b] = any ? lps : 0.0f;
  aux[2 * b + 1] = (any && best == star) ? 1.0f : 0.0f;
}

// One lane per environment: action[i] = u < beta ? expert[i] : learner[i], u = (w >> 8) 2^-24, w the first word of the Philox stream of
// (seed ^ kDaggerStream, env_offset + i, *step) -- ble_ac_head_kernel's keying under its own constant, so the draw of an environment at
// a step does not depend on n or on the row's position.  beta = 0 copies the learner; beta = 1 the expert (u < 1 always).  action may
// alias learner: a lane reads its own element before it writes it.
__global__ __launch_bounds__(kDaggerMixBlock) void ble_dagger_mix_kernel(const uint8_t* learner, const uint8_t* __restrict__ expert,
                                                                        float beta, uint64_t seed, int64_t env_offset,
                                                                        const unsigned long long* __restrict__ step, uint8_t* action,
                                                                        uint8_t* __restrict__ took_expert, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kDaggerMixBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t st = *step;
  Philox g = philox_init(seed ^ kDaggerStream, (uint64_t)(env_offset + i), (uint32_t)st);
  g.key1 ^= (uint32_t)(st >> 32);
  const uint32_t w = philox_u32(g);
  const float u = (float)(w >> 8) * (1.0f / 16777216.0f);             // [0, 1), 24 bits
  const bool took = u < beta;
  const uint8_t mine = learner[i], theirs = expert[i];
  action[i] = took ? theirs : mine;
  if (took_expert != nullptr) took_expert[i] = took ? 1 : 0;
}

}  // namespace ble
