// Host build of the scenario tree's lane functions (csrc/ble_tree_scenarios.h) for tests/test_tree_scenarios_host.py: the fly / carry /
// void decision of an expand lane, and one level's risk -> select with the kernels' own lane functions.  TEST TOOLING: never loaded by
// the package.  The decision and the order are integer work, the score is plan_risk_score's fp64 sum: the host build gives the device's
// answers.
#include "../../balloon_learning_environment_amd/csrc/ble_tree_scenarios.h"

using namespace ble;

// status, acc: the parent group's num words (acc NULL: level 1, status[0] the environment's byte) -> kTreeLaneFly / Carry / Void
extern "C" int emul_tree_scenario_lane(const uint8_t* status, const double* acc, int num, int m, int act) {
  return tree_scenario_lane(status, acc, num, m, act);
}

// One level of one environment, the three launches' steps in their order: ret [C][num] -> score [C] (ble_plan_risk_kernel's lane), the
// keys of the scores, every child's rank (ble_tree_select_kernel's lanes).  parent, choice [beam].
extern "C" void emul_tree_scenarios_level(int n_children, int num, int tail, int beam, const float* ret, float* score, int32_t* parent,
                                          int32_t* choice) {
  static uint32_t keys[kTreeMaxChildren];
  for (int c = 0; c < n_children; ++c) score[c] = plan_risk_score(ret + (int64_t)c * num, 1, num, tail);
  for (int c = 0; c < n_children; ++c) keys[c] = plan_key(score[c]);
  const int n_keep = n_children < beam ? n_children : beam;
  for (int c = 0; c < n_children; ++c) tree_select_lane(keys, n_children, n_keep, c, parent, choice);
}
