// Host build of the expert-iteration lane functions of csrc/ble_plan.h for tests/test_exit_host.py.  TEST TOOLING: never
// loaded by the package.  The sampler and the action values are integer arithmetic; the prior count is one fp32 product and a
// truncation, which the host evaluates as the device does (no contraction: there is nothing to contract).
#include "../../balloon_learning_environment_amd/csrc/ble_plan.h"

using namespace ble;

constexpr int kMaxEntries = 960;      // BLE_ROLLOUT_MAX_STEPS

// plan_prior_count over probs [n][3]: counts [n][segments][3]
extern "C" void emul_plan_prior(const float* probs, int strength, int segments, int n, uint16_t* counts) {
  for (int e = 0; e < n; ++e)
    for (int s = 0; s < segments; ++s)
      for (int a = 0; a < 3; ++a) counts[(e * segments + s) * 3 + a] = plan_prior_count(probs[3 * e + a], strength, s);
}

// plan_sample_prior_lane for every plan of one environment: plans [H][K]; counts [segments][3] or NULL; prior [segments][3]; prev [H] or
// NULL (all STAY)
extern "C" void emul_plan_sample_prior(uint64_t seed, uint64_t key, uint64_t decision, int iteration, int n_plans, int n_entries, int segment,
                                       const uint16_t* counts, const uint16_t* prior, const uint8_t* prev, uint8_t* plans) {
  uint8_t stay[kMaxEntries];
  for (int h = 0; h < kMaxEntries; ++h) stay[h] = (uint8_t)kPlanStay;
  for (int k = 0; k < n_plans; ++k)
    plan_sample_prior_lane(seed, key, decision, iteration, k, n_entries, segment, counts, prior, prev ? prev : stay, 1, plans + k, n_plans);
}

// The action values of one environment with the kernel's lane functions, its steps in the kernel's order: 64 lanes fold their plans
// (k = lane, lane + 64, ...), then each action folds the 64 partial results in lane order.  ret [K], first [K]; q, q_k, visits [3].
extern "C" void emul_plan_action_values(int n_plans, int accumulate, const float* ret, const uint8_t* first, float* q, int32_t* q_k,
                                        int32_t* visits) {
  static PlanActionBest lanes[64];
  for (int lane = 0; lane < 64; ++lane) {
    plan_action_best_init(lanes[lane]);
    for (int k = lane; k < n_plans; k += 64) {
      const uint32_t key = plan_key(ret[k]);
      const int act = first[k] >= 2 ? 2 : first[k];
      for (int c = 0; c < kPlanActions; ++c)
        plan_action_best_take(lanes[lane], c, act == c ? key : kPlanKeyNonFinite, act == c ? k : kPlanNoPlan, act == c ? 1 : 0);
    }
  }
  for (int a = 0; a < kPlanActions; ++a) {
    uint32_t key = kPlanKeyNonFinite;
    int k = kPlanNoPlan, n_visits = 0;
    for (int l = 0; l < 64; ++l) {
      const bool better = plan_before(lanes[l].key[a], lanes[l].k[a], key, k);
      key = better ? lanes[l].key[a] : key;
      k = better ? lanes[l].k[a] : k;
      n_visits += lanes[l].visits[a];
    }
    plan_action_write(key, k, key != kPlanKeyNonFinite ? ret[k] : 0.0f, n_visits, accumulate != 0, q + a, q_k + a, visits + a);
  }
}
