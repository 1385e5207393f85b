// ble_plan.h -- plan on the device: sample K piecewise-constant action plans per environment (ble_plan_sample_u8) and, once
// the look-ahead kernels have flown them, pick the best one (ble_plan_select_f32).  The flights themselves are ble_rollout_f32 /
// ble_rollout_belief_f32, unchanged.
//
// The sampler is one lane per (environment e, plan k), lane index j = e K + k as in ble_rollout_kernel, so the stores of a wave to
// plans [H][n][K] are consecutive bytes.  Integers only: a NumPy restatement reproduces it bit for bit (tests/plan_host.py).
// The selection is one wavefront per environment: the K returns become sort keys in LDS, every lane counts the predecessors of its
// plans (lanes stride over K; K <= 1024: at most 16 plans per lane), the plans of rank < max(elite, 1) are listed in rank order, and
// the rest reads that list.  No atomics, no cross-lane arithmetic: the order is a function of the returns alone.
//
// Expert iteration adds a prior to iteration 0 of the sampler (ble_plan_prior_u16 -> ble_plan_sample_prior_u8: counts made
// from a policy's probabilities where iteration 0 has zeros) and the best return among the plans that begin with each action
// (ble_plan_action_values_f32: one wavefront per environment, the selection's own order).
//
// The lane functions below build for the host as well (tests/emul/plan_emul.cpp, exit_emul.cpp); the kernels need hipcc.
#pragma once
#include "ble_reset.h"

namespace ble {

constexpr int kPlanMaxPlans = 1024;              // BLE_PLAN_MAX_PLANS
constexpr int kPlanMaxIterations = 16;           // BLE_PLAN_MAX_ITERATIONS
constexpr unsigned long long kPlanKey = 0x504C414E53ull;      // "PLANS": the sampler's streams are not the reset's or the noise's
constexpr uint32_t kPlanKeyNonFinite = 0xFFFFFFFFu;
constexpr int kPlanStay = 1;

// The generator of plan k of an environment in iteration `iteration` of decision `decision`, at its first block.
// Segment s takes word s % 4 of block s / 4 (256 blocks per plan: 1024 segments, and a plan has at most 960 entries).
BLE_FN Philox plan_stream(uint64_t seed, uint64_t key, uint64_t decision, int iteration, int k) {
  Philox g = philox_init(seed ^ kPlanKey, key, (uint32_t)decision);
  g.key1 ^= (uint32_t)(decision >> 32);
  g.c0 = (uint32_t)((iteration * kPlanMaxPlans + k) * 256);
  return g;
}

// One action from one 32-bit word and the segment's elite counts: Laplace-smoothed, P(a) = (c_a + 1) / (E + 3); zero counts: thirds.
BLE_FN int plan_draw(uint32_t word, int c0, int c1, int c2) {
  const uint32_t r = (uint32_t)(((uint64_t)word * (uint64_t)(uint32_t)(c0 + c1 + c2 + 3)) >> 32);      // mulhi32: uniform in [0, E + 3)
  return r < (uint32_t)(c0 + 1) ? 0 : (r < (uint32_t)(c0 + c1 + 2) ? 1 : 2);
}

// Plan k of one environment: entry h goes to out[h * out_stride].  counts: the environment's elite counts [segments][3] (read when
// iteration > 0); prev: its previous best plan, entry h at prev[h * prev_stride] (read by the warm start: iteration 0, k == 3).
BLE_FN void plan_sample_lane(uint64_t seed, uint64_t key, uint64_t decision, int iteration, int k, int n_entries, int segment,
                             const uint16_t* counts, const uint8_t* prev, int64_t prev_stride, uint8_t* out, int64_t out_stride) {
  if (iteration == 0 && k < 4) {                 // the fixed slots: STAY, DOWN, UP, the previous best plan shifted left by one entry
    for (int h = 0; h < n_entries; ++h) {
      const int hn = h + 1 < n_entries ? h + 1 : n_entries - 1;
      out[h * out_stride] = k == 0 ? (uint8_t)kPlanStay : (k == 1 ? (uint8_t)0 : (k == 2 ? (uint8_t)2 : prev[hn * prev_stride]));
    }
    return;
  }
  Philox g = plan_stream(seed, key, decision, iteration, k);
  int a = kPlanStay, left = 0, s = 0;
#pragma unroll 1
  for (int h = 0; h < n_entries; ++h) {
    if (left == 0) {                             // entry h opens segment s
      const int w = s & 3;
      if (w == 0) philox_refill(g);              // block s / 4 (the refill moves the counter on by one)
      const uint32_t word = w == 0 ? g.out[0] : (w == 1 ? g.out[1] : (w == 2 ? g.out[2] : g.out[3]));
      int c0 = 0, c1 = 0, c2 = 0;
      if (iteration > 0) { c0 = counts[3 * s]; c1 = counts[3 * s + 1]; c2 = counts[3 * s + 2]; }
      a = plan_draw(word, c0, c1, c2);
      ++s; left = segment;
    }
    --left;
    out[h * out_stride] = (uint8_t)a;
  }
}

// The sort key of a return: smaller is better.  Finite returns in descending order (-0 counts as +0), every non-finite one after
// them, all equal (kPlanKeyNonFinite: no finite return maps to it).
BLE_FN uint32_t plan_key(float ret) {
  union { float f; uint32_t u; } b;
  b.f = ret;
  if ((b.u & 0x7F800000u) == 0x7F800000u) return kPlanKeyNonFinite;
  if (b.u == 0x80000000u) b.u = 0u;
  return (b.u & 0x80000000u) ? b.u : ~(b.u | 0x80000000u);     // ~(ascending key)
}
// plan j comes before plan k: the better key, then the smaller index
BLE_FN bool plan_before(uint32_t key_j, int j, uint32_t key_k, int k) { return key_j < key_k || (key_j == key_k && j < k); }
// the number of plans in front of plan k
BLE_FN int plan_rank(const uint32_t* keys, int n_plans, int k) {
  const uint32_t mine = keys[k];
  int rank = 0;
#pragma unroll 4
  for (int j = 0; j < n_plans; ++j) rank += plan_before(keys[j], j, mine, k) ? 1 : 0;
  return rank;
}
// this iteration's best plan replaces the incumbent: it is finite and strictly better (a tie keeps the incumbent; a non-finite
// incumbent loses to any finite plan)
BLE_FN bool plan_replaces(uint32_t key_new, bool have_incumbent, uint32_t key_incumbent) {
  return key_new != kPlanKeyNonFinite && (!have_incumbent || key_new < key_incumbent);
}
// the elite counts of one segment: how many of the first `elite` plans in order took each action in the segment's first entry
// (a plan is constant over a segment).  entry: the environment's K actions of that entry.
BLE_FN void plan_elite_segment(const uint16_t* order, int elite, const uint8_t* entry, uint16_t* counts3) {
  int c0 = 0, c1 = 0, c2 = 0;
#pragma unroll 1
  for (int i = 0; i < elite; ++i) {
    const int a = entry[order[i]];
    c0 += a == 0; c1 += a == 1; c2 += a >= 2;
  }
  counts3[0] = (uint16_t)c0; counts3[1] = (uint16_t)c1; counts3[2] = (uint16_t)c2;
}

// ---- expert iteration: a prior for iteration 0, and the per-action values of the plans flown
constexpr int kPlanActions = 3;
constexpr int kPlanNoPlan = 0x7FFFFFFF;          // the index of "no plan yet": behind every real plan of the same key

// The prior count of one action in segment s: trunc(p * (strength >> s)), at most 65 535; the weight is zero from s = 16.  A NaN or
// negative p gives 0, and so does a NaN product.
BLE_FN uint16_t plan_prior_count(float p, int strength, int s) {
  const uint32_t w = s < 16 ? ((uint32_t)strength >> s) : 0u;
  const float v = p * (float)w;
  const uint32_t c = v >= 65535.0f ? 65535u : (v >= 1.0f ? (uint32_t)v : 0u);
  return p > 0.0f ? (uint16_t)c : (uint16_t)0;
}

// plan_sample_lane with a prior: iteration 0 draws its free plans (k >= 4) from `prior` [segments][3] where plan_sample_lane draws
// from zeros.  Everything else -- the fixed slots, the streams, the later iterations -- is plan_sample_lane itself.
BLE_FN void plan_sample_prior_lane(uint64_t seed, uint64_t key, uint64_t decision, int iteration, int k, int n_entries, int segment,
                                   const uint16_t* counts, const uint16_t* prior, const uint8_t* prev, int64_t prev_stride, uint8_t* out,
                                   int64_t out_stride) {
  if (iteration > 0 || k < 4) {
    plan_sample_lane(seed, key, decision, iteration, k, n_entries, segment, counts, prev, prev_stride, out, out_stride);
    return;
  }
  Philox g = plan_stream(seed, key, decision, iteration, k);
  int a = kPlanStay, left = 0, s = 0;
#pragma unroll 1
  for (int h = 0; h < n_entries; ++h) {
    if (left == 0) {                             // entry h opens segment s
      const int w = s & 3;
      if (w == 0) philox_refill(g);
      const uint32_t word = w == 0 ? g.out[0] : (w == 1 ? g.out[1] : (w == 2 ? g.out[2] : g.out[3]));
      a = plan_draw(word, prior[3 * s], prior[3 * s + 1], prior[3 * s + 2]);
      ++s; left = segment;
    }
    --left;
    out[h * out_stride] = (uint8_t)a;
  }
}

// The first plan in the selection's order among `n` plans (index k0, k0 + stride, ...) whose first action is a, as a (key, k) pair per
// action, and how many take a.  best_k starts at kPlanNoPlan with the non-finite key.
struct PlanActionBest {
  uint32_t key[kPlanActions];
  int k[kPlanActions], visits[kPlanActions];
};
BLE_FN void plan_action_best_init(PlanActionBest& b) {
  for (int a = 0; a < kPlanActions; ++a) { b.key[a] = kPlanKeyNonFinite; b.k[a] = kPlanNoPlan; b.visits[a] = 0; }
}
BLE_FN void plan_action_best_take(PlanActionBest& b, int a, uint32_t key, int k, int visits) {
  const bool better = plan_before(key, k, b.key[a], b.k[a]);
  b.key[a] = better ? key : b.key[a];
  b.k[a] = better ? k : b.k[a];
  b.visits[a] += visits;
}
// One action's entry from the best pair of this call: (q, q_k) as written; ret_best is ret[k] (read only when the key is finite).
// accumulate: the stored q stays unless plan_replaces says otherwise.
BLE_FN void plan_action_write(uint32_t key, int k, float ret_best, int visits, bool accumulate, float* q, int32_t* q_k, int32_t* n_visits) {
  const bool finite = key != kPlanKeyNonFinite;
  if (!accumulate) {
    union { uint32_t u; float f; } ninf;
    ninf.u = 0xFF800000u;
    *q = finite ? ret_best : ninf.f;
    *q_k = finite ? k : -1;
    *n_visits = visits;
    return;
  }
  const bool replace = plan_replaces(key, true, plan_key(*q));
  if (replace) *q = ret_best;
  *q_k = replace ? k : -1;
  *n_visits += visits;
}

// ---- a learned terminal value: ret + gamma^steps_flown * V(leaf)
// The score of one plan.  The discount is the rollout's own sequence -- 1.0 multiplied steps_flown times by gamma -- hence its `disc`
// bit for bit; the product and the sum are two statements (two roundings under -ffp-contract=on), rounded to fp32 once.  A leaf that
// is not OK keeps the plan's return: a select, so its value may hold anything.
BLE_FN float plan_bootstrap_lane(float ret, int steps_flown, uint8_t leaf_status, float value, double gamma) {
  double d = 1.0;
#pragma unroll 1
  for (int i = 0; i < steps_flown; ++i) d *= gamma;
  const double t = d * (double)value;
  const double s = (double)ret + t;
  return leaf_status == 0 ? (float)s : ret;
}

#if defined(__HIPCC__)
// struct ble_plan_bootstrap (include/ble_abi.h) as the kernel takes it; score may be ret (no __restrict__)
struct PlanBootstrapArgs {
  int64_t total;                               // n K
  double gamma;
  const float* ret;                            // [n][K]
  const int32_t* __restrict__ steps_flown;     // [n][K]
  const uint8_t* __restrict__ leaf_status;     // [n K]
  const float* __restrict__ value;             // [n K]
  float* score;                                // [n][K]
};

// One lane per (environment, plan).
__global__ __launch_bounds__(256) void ble_plan_bootstrap_kernel(PlanBootstrapArgs a) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.total) return;
  a.score[j] = plan_bootstrap_lane(a.ret[j], a.steps_flown[j], a.leaf_status[j], a.value[j], a.gamma);
}

// struct ble_plan_sample (include/ble_abi.h) as the kernel takes it
struct PlanSampleArgs {
  int64_t n, env_offset;
  int n_plans, n_entries, segment, iteration;
  const unsigned long long* __restrict__ decision;
  const uint16_t* __restrict__ counts;         // [n][segments][3]
  const uint8_t* __restrict__ best_plan;       // [H][n]
  uint8_t* __restrict__ plans;                 // [H][n][K]
};

// S: the seed source (ScalarSeed / EnvSeed, ble_kernels.hip)
template <class S>
__global__ __launch_bounds__(256) void ble_plan_sample_kernel(PlanSampleArgs a, S seed) {
  const int64_t lanes_total = a.n * (int64_t)a.n_plans;          // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= lanes_total) return;
  const int64_t e = (int64_t)((uint32_t)j / (uint32_t)a.n_plans);
  const int k = (int)(j - e * a.n_plans);
  const int segments = (a.n_entries + a.segment - 1) / a.segment;
  plan_sample_lane(seed.of(e), seed.key(e, a.env_offset), *a.decision, a.iteration, k, a.n_entries, a.segment,
                   a.counts ? a.counts + e * (int64_t)(3 * segments) : nullptr, a.best_plan + e, a.n, a.plans + j, lanes_total);
}

// struct ble_plan_select (include/ble_abi.h) as the kernel takes it
struct PlanSelectArgs {
  int64_t n;
  int n_plans, n_entries, segment, iteration, elite;
  const float* __restrict__ ret;               // [n][K]
  const uint8_t* __restrict__ plans;           // [H][n][K]
  float* __restrict__ best_return;             // [n]
  int32_t* __restrict__ best_k;                // [n]
  uint8_t* __restrict__ best_plan;             // [H][n]
  uint8_t* __restrict__ action;                // [n]
  uint16_t* __restrict__ counts;               // [n][segments][3]
  unsigned long long* advance;                 // optional: the decision counter, moved on by one
};

constexpr int kPlanSelectBlock = 64;             // one wavefront per environment

__global__ __launch_bounds__(kPlanSelectBlock) void ble_plan_select_kernel(PlanSelectArgs a) {
  __shared__ uint32_t keys[kPlanMaxPlans];
  __shared__ uint16_t order[kPlanMaxPlans];
  const int64_t e = blockIdx.x;
  const int lane = (int)threadIdx.x, K = a.n_plans;
  const int64_t lanes_total = a.n * (int64_t)K;
  // (the sampler, this decision's last reader of the counter, ran before this launch)
  if (a.advance != nullptr && e == 0 && lane == 0) *a.advance += 1ull;
  for (int k = lane; k < K; k += kPlanSelectBlock) keys[k] = plan_key(a.ret[e * K + k]);
  __syncthreads();
  const int listed = a.elite > 1 ? a.elite : 1;
  for (int k = lane; k < K; k += kPlanSelectBlock) {
    const int rank = plan_rank(keys, K, k);
    if (rank < listed) order[rank] = (uint16_t)k;                // (ranks are a permutation of 0 .. K - 1: every slot below `listed` is written)
  }
  __syncthreads();
  const int k_best = order[0];
  const uint32_t key_new = keys[k_best];
  const bool have = a.iteration > 0;
  const float incumbent = have ? a.best_return[e] : 0.0f;        // (every lane reads the same word, before lane 0 writes it below)
  const bool replace = plan_replaces(key_new, have, plan_key(incumbent));
  __syncthreads();
  if (replace) {
    for (int h = lane; h < a.n_entries; h += kPlanSelectBlock) a.best_plan[h * a.n + e] = a.plans[h * lanes_total + e * K + k_best];
    if (lane == 0) { a.best_return[e] = a.ret[e * K + k_best]; a.best_k[e] = k_best; a.action[e] = a.plans[e * K + k_best]; }
  } else if (!have) {                            // iteration 0 and no finite plan: all STAY
    for (int h = lane; h < a.n_entries; h += kPlanSelectBlock) a.best_plan[h * a.n + e] = (uint8_t)kPlanStay;
    if (lane == 0) { a.best_return[e] = -INFINITY; a.best_k[e] = -1; a.action[e] = (uint8_t)kPlanStay; }
  } else if (lane == 0) {                        // the incumbent stays
    a.best_k[e] = -1; a.action[e] = a.best_plan[e];
  }
  if (a.elite >= 1) {
    const int segments = (a.n_entries + a.segment - 1) / a.segment;
    for (int s = lane; s < segments; s += kPlanSelectBlock)
      plan_elite_segment(order, a.elite, a.plans + (int64_t)(s * a.segment) * lanes_total + e * K, a.counts + (e * segments + s) * 3);
  }
}
// ---- expert iteration
// One lane per (environment, segment): probs [n][3] -> counts [n][segments][3].
__global__ __launch_bounds__(256) void ble_plan_prior_kernel(const float* __restrict__ probs, int strength, int segments,
                                                             uint16_t* __restrict__ counts, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t e = (int64_t)((uint32_t)i / (uint32_t)segments);      // (total < 2^31: the entry point checks)
  const int s = (int)(i - e * segments);
  for (int a = 0; a < kPlanActions; ++a) counts[3 * i + a] = plan_prior_count(probs[3 * e + a], strength, s);
}

// ble_plan_sample_kernel with a prior: an instantiation of its own, so that the kernels without one keep their instructions.
template <class S>
__global__ __launch_bounds__(256) void ble_plan_sample_prior_kernel(PlanSampleArgs a, const uint16_t* __restrict__ prior, S seed) {
  const int64_t lanes_total = a.n * (int64_t)a.n_plans;          // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= lanes_total) return;
  const int64_t e = (int64_t)((uint32_t)j / (uint32_t)a.n_plans);
  const int k = (int)(j - e * a.n_plans);
  const int segments = (a.n_entries + a.segment - 1) / a.segment;
  plan_sample_prior_lane(seed.of(e), seed.key(e, a.env_offset), *a.decision, a.iteration, k, a.n_entries, a.segment,
                         a.counts ? a.counts + e * (int64_t)(3 * segments) : nullptr, prior + e * (int64_t)(3 * segments), a.best_plan + e,
                         a.n, a.plans + j, lanes_total);
}

// struct ble_plan_action_values (include/ble_abi.h) as the kernel takes it
struct PlanActionValuesArgs {
  int64_t n;
  int n_plans, accumulate;
  const float* __restrict__ ret;               // [n][K]
  const uint8_t* __restrict__ first;           // [n][K]
  float* q;                                    // [n][3]
  int32_t* q_k;                                // [n][3]
  int32_t* visits;                             // [n][3]
};

// One wavefront per environment: every lane folds its plans (k = lane, lane + 64, ...) into a (key, k) pair and a count per action,
// the 64 partial results meet in LDS, and lane a folds them for action a, in lane order.  Integer compares only; no atomics.
__global__ __launch_bounds__(kPlanSelectBlock) void ble_plan_action_values_kernel(PlanActionValuesArgs a) {
  __shared__ uint32_t s_key[kPlanActions][kPlanSelectBlock];
  __shared__ int s_k[kPlanActions][kPlanSelectBlock];
  __shared__ int s_visits[kPlanActions][kPlanSelectBlock];
  const int64_t e = blockIdx.x;
  const int lane = (int)threadIdx.x, K = a.n_plans;
  PlanActionBest mine;
  plan_action_best_init(mine);
  for (int k = lane; k < K; k += kPlanSelectBlock) {
    const uint32_t key = plan_key(a.ret[e * K + k]);
    const int first = a.first[e * K + k];
    const int act = first >= 2 ? 2 : first;
#pragma unroll
    for (int c = 0; c < kPlanActions; ++c) plan_action_best_take(mine, c, act == c ? key : kPlanKeyNonFinite, act == c ? k : kPlanNoPlan, act == c ? 1 : 0);
  }
#pragma unroll
  for (int c = 0; c < kPlanActions; ++c) { s_key[c][lane] = mine.key[c]; s_k[c][lane] = mine.k[c]; s_visits[c][lane] = mine.visits[c]; }
  __syncthreads();
  if (lane >= kPlanActions) return;
  uint32_t key = kPlanKeyNonFinite;
  int k = kPlanNoPlan, visits = 0;
  for (int l = 0; l < kPlanSelectBlock; ++l) {
    const bool better = plan_before(s_key[lane][l], s_k[lane][l], key, k);
    key = better ? s_key[lane][l] : key;
    k = better ? s_k[lane][l] : k;
    visits += s_visits[lane][l];
  }
  const float ret_best = key != kPlanKeyNonFinite ? a.ret[e * K + k] : 0.0f;      // (a finite key names a real plan: k < K)
  plan_action_write(key, k, ret_best, visits, a.accumulate != 0, a.q + 3 * e + lane, a.q_k + 3 * e + lane, a.visits + 3 * e + lane);
}
#endif  // __HIPCC__

}  // namespace ble
