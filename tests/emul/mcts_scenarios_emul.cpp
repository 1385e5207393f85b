// Host build of the group functions of the guided tree search in scenario winds (csrc/ble_mcts_scenarios.h) for
// tests/test_mcts_scenarios_host.py.  TEST TOOLING: never loaded by the package.  One environment (n = 1, e = 0): the pool's node arrays
// are [R][3L][M], group_status and group_g [R][3L], the statistics [cap].  Select and finish are mcts_emul.cpp's, fed group_status.
// Built with -ffp-contract=off: every statement rounds once, as the device's does under -ffp-contract=on.
#include "../../balloon_learning_environment_amd/csrc/ble_mcts_scenarios.h"

using namespace ble;

// the statistics of the one environment, in struct ble_mcts_pool's order (mcts_emul.cpp's EmulMctsStats)
struct EmulMctsStats {
  int32_t *parent, *first_child, *depth, *visits, *pending;
  double *value_sum, *g;
  float* prior;
  double* g_range;
};

// acc, disc, node_status: the pool's arrays [R][3L][M]; value [3L][M], probs [3L][M][3]: the round's rows, or NULL.
extern "C" void emul_mcts_backup_scenarios(const EmulMctsStats* st, int round, int leaves, int max_depth, int num, int tail, const double* acc,
                                           const double* disc, const uint8_t* node_status, const float* value, const float* probs,
                                           const int32_t* leaf, const int32_t* kind, uint8_t* group_status, double* group_g) {
  const MctsStats s{st->parent, st->first_child, st->depth, st->visits, st->pending, st->value_sum, st->g, st->prior, st->g_range};
  const int count = 1 + 3 * leaves * round, after = count + 3 * leaves;
  const int64_t at = (int64_t)round * 3 * leaves;
  for (int l = 0; l < leaves; ++l) {
    const int64_t node = (at + 3 * l) * num, row = (int64_t)3 * l * num;
    mcts_backup_group_slot(s, count, max_depth, count + 3 * l, tree_clamp(leaf[l], count), kind[l], acc + node, disc + node, node_status + node,
                           value != nullptr ? value + row : nullptr, probs != nullptr ? probs + 3 * row : nullptr, num, tail,
                           group_status + at + 3 * l, group_g + at + 3 * l);
  }
  for (int i = 0; i < after; ++i) s.pending[i] = 0;
}

// the group step alone, on one group's M nodes: -> G (NaN: void), prior [3], *spent
extern "C" double emul_mcts_group(const double* acc, const double* disc, const uint8_t* status, const float* value, const float* probs, int num,
                                  int tail, float* prior, uint8_t* spent) {
  mcts_group_prior(status, probs, num, prior);
  *spent = mcts_group_spent(status, acc, num) ? 1 : 0;
  return mcts_group_g(acc, disc, status, value, num, tail);
}

// the expand's rule for lane (m, act) from its parent group (acc NULL: the root)
extern "C" int emul_mcts_lane_rule(const uint8_t* status, const double* acc, int num, int m, int act) {
  return tree_scenario_lane(status, acc, num, m, act);
}
