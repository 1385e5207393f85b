// Host build of the beam search's select and finish lane functions (csrc/ble_tree.h) for tests/test_tree_host.py.  TEST TOOLING: never
// loaded by the package.  Everything here is integer arithmetic on the keys, so the host build gives the device's answers.
#include "../../balloon_learning_environment_amd/csrc/ble_tree.h"

using namespace ble;

// The selection of one environment, the kernel's steps in its order: keys, then every child's rank.  ret [C]; parent, choice [beam].
extern "C" void emul_tree_select(int n_children, int beam, const float* ret, int32_t* parent, int32_t* choice) {
  static uint32_t keys[kTreeMaxChildren];
  for (int c = 0; c < n_children; ++c) keys[c] = plan_key(ret[c]);
  const int n_keep = n_children < beam ? n_children : beam;
  for (int c = 0; c < n_children; ++c) tree_select_lane(keys, n_children, n_keep, c, parent, choice);
}

// The finish of one environment with the kernel's lane functions: ret, score [C] (score: the keys' values); choice [depth][beam];
// best_plan [depth * segment]; action, best_return: one word each; q, visits [3] or NULL.
extern "C" void emul_tree_finish(int n_children, int beam, int depth, int segment, const float* ret, const float* score, int source_ok,
                                 const int32_t* choice, uint8_t* best_plan, uint8_t* action, float* best_return, float* q, int32_t* visits) {
  static uint32_t keys[kTreeMaxChildren];
  static uint8_t path[kTreeMaxDepth];
  const int C = n_children, D = depth;
  for (int c = 0; c < C; ++c) keys[c] = plan_key(score[c]);
  int c_best = 0;
  for (int c = 0; c < C; ++c)
    if (plan_rank(keys, C, c) == 0) c_best = c;
  const bool flown = tree_finish_best(source_ok != 0, keys[c_best], score[c_best], best_return);
  if (flown) tree_backtrack(choice, beam, beam, D, c_best, path);
  for (int h = 0; h < D * segment; ++h) best_plan[h] = flown ? path[h / segment] : (uint8_t)kPlanStay;
  *action = flown ? path[0] : (uint8_t)kPlanStay;
  if (q == nullptr) return;
  PlanActionBest best;
  plan_action_best_init(best);
  for (int c = 0; c < C; ++c) {
    const int act = D > 1 ? tree_backtrack(choice, beam, beam, D - 1, tree_clamp(choice[(D - 2) * beam + c / 3], 3 * beam), nullptr) : c;
    const int counts = tree_void(ret[c]) ? 0 : 1;
    for (int k = 0; k < kPlanActions; ++k)
      plan_action_best_take(best, k, act == k ? keys[c] : kPlanKeyNonFinite, act == k ? c : kPlanNoPlan, act == k ? counts : 0);
  }
  for (int k = 0; k < kPlanActions; ++k) {
    int32_t q_k;
    plan_action_write(best.key[k], best.k[k], best.key[k] != kPlanKeyNonFinite ? score[best.k[k]] : 0.0f, best.visits[k], false, q + k, &q_k,
                      visits + k);
  }
}
