// Host build of the planner's lane functions (csrc/ble_plan.h) for tests/test_plan_host.py.  TEST TOOLING: never loaded by the
// package.  Everything here is integer arithmetic, so the host build gives the device's bits.
#include "../../balloon_learning_environment_amd/csrc/ble_plan.h"

using namespace ble;

constexpr int kMaxEntries = 960;      // BLE_ROLLOUT_MAX_STEPS

// plan_sample_lane for every plan of one environment: plans [H][K]; counts [segments][3] or NULL; prev [H] or NULL (all STAY)
extern "C" void emul_plan_sample(uint64_t seed, uint64_t key, uint64_t decision, int iteration, int n_plans, int n_entries, int segment,
                                 const uint16_t* counts, const uint8_t* prev, uint8_t* plans) {
  uint8_t stay[kMaxEntries];
  for (int h = 0; h < kMaxEntries; ++h) stay[h] = (uint8_t)kPlanStay;
  for (int k = 0; k < n_plans; ++k)
    plan_sample_lane(seed, key, decision, iteration, k, n_entries, segment, counts, prev ? prev : stay, 1, plans + k, n_plans);
}

extern "C" int emul_plan_draw(uint32_t word, int c0, int c1, int c2) { return plan_draw(word, c0, c1, c2); }

// The selection of one environment with the kernel's lane functions, its steps in the kernel's order: keys, ranks and the list of the
// first max(elite, 1) plans, the incumbent rule, the elite counts.  ret [K], plans [H][K]; best_return / best_k / action: one word each;
// best_plan [H]; counts [segments][3] (elite >= 1).
extern "C" void emul_plan_select(int n_plans, int n_entries, int segment, int iteration, int elite, const float* ret, const uint8_t* plans,
                                 float* best_return, int32_t* best_k, uint8_t* best_plan, uint8_t* action, uint16_t* counts) {
  static uint32_t keys[kPlanMaxPlans];
  static uint16_t order[kPlanMaxPlans];
  for (int k = 0; k < n_plans; ++k) keys[k] = plan_key(ret[k]);
  const int listed = elite > 1 ? elite : 1;
  for (int k = 0; k < n_plans; ++k) {
    const int rank = plan_rank(keys, n_plans, k);
    if (rank < listed) order[rank] = (uint16_t)k;
  }
  const int k_best = order[0];
  const bool have = iteration > 0;
  const bool replace = plan_replaces(keys[k_best], have, plan_key(have ? *best_return : 0.0f));
  if (replace) {
    for (int h = 0; h < n_entries; ++h) best_plan[h] = plans[h * n_plans + k_best];
    *best_return = ret[k_best]; *best_k = k_best;
  } else if (!have) {
    for (int h = 0; h < n_entries; ++h) best_plan[h] = (uint8_t)kPlanStay;
    *best_return = -INFINITY; *best_k = -1;
  } else {
    *best_k = -1;
  }
  *action = best_plan[0];
  if (elite >= 1)
    for (int s = 0; s < (n_entries + segment - 1) / segment; ++s) plan_elite_segment(order, elite, plans + s * segment * n_plans, counts + 3 * s);
}
