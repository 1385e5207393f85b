// Host build of the guided tree search's select, backup and finish lane functions (csrc/ble_mcts.h) for tests/test_mcts_emul_host.py.
// TEST TOOLING: never loaded by the package.  One environment (n = 1, e = 0): the pool's node arrays are [R][3L], the statistics [cap].
// Built with -ffp-contract=off: every statement of the score rounds once, as the device's does under -ffp-contract=on.
#include "../../balloon_learning_environment_amd/csrc/ble_mcts.h"

using namespace ble;

// the statistics of the one environment, in struct ble_mcts_pool's order
struct EmulMctsStats {
  int32_t *parent, *first_child, *depth, *visits, *pending;
  double *value_sum, *g;
  float* prior;
  double* g_range;
};
static MctsStats stats_of(const EmulMctsStats* s) {
  return MctsStats{s->parent, s->first_child, s->depth, s->visits, s->pending, s->value_sum, s->g, s->prior, s->g_range};
}

// The kernel's steps in its order: round 0 initialises the root; then the L descents.  pool_status [R][3L]; leaf, kind [L].
extern "C" void emul_mcts_select(const EmulMctsStats* st, int round, int leaves, int max_depth, double c_puct, int source_status,
                                 const uint8_t* pool_status, const float* root_prior, int32_t* leaf, int32_t* kind) {
  const MctsStats s = stats_of(st);
  const int count = 1 + 3 * leaves * round;
  if (round == 0) mcts_root_init(s, root_prior);
  for (int i = 0; i < count; ++i) s.pending[i] = 0;
  const uint8_t source = (uint8_t)source_status;
  const MctsStatusOk ok{&source, pool_status, 1, 0, 3 * leaves};
  for (int l = 0; l < leaves; ++l) mcts_select_slot(s, count, max_depth, c_puct, l, leaf, kind, ok);
}

// acc, disc, pool_status: the pool's arrays [R][3L]; value [3L], probs [3L][3]: the round's rows, or NULL.
extern "C" void emul_mcts_backup(const EmulMctsStats* st, int round, int leaves, int max_depth, const double* acc, const double* disc,
                                 const uint8_t* pool_status, const float* value, const float* probs, const int32_t* leaf,
                                 const int32_t* kind) {
  const MctsStats s = stats_of(st);
  const int count = 1 + 3 * leaves * round, after = count + 3 * leaves;
  const int64_t at = (int64_t)round * 3 * leaves;
  for (int l = 0; l < leaves; ++l)
    mcts_backup_slot(s, count, max_depth, count + 3 * l, tree_clamp(leaf[l], count), kind[l], acc + at + 3 * l, disc + at + 3 * l,
                     pool_status + at + 3 * l, value != nullptr ? value + 3 * l : nullptr, probs != nullptr ? probs + 9 * l : nullptr);
  for (int i = 0; i < after; ++i) s.pending[i] = 0;
}

// best_plan [max_depth * segment]; q, visits [3]; action, best_return, pv_length: one word each.
extern "C" void emul_mcts_finish(const EmulMctsStats* st, int rounds, int leaves, int max_depth, int segment, int source_status, uint8_t* best_plan,
                                 uint8_t* action, float* best_return, float* q, int32_t* visits, int32_t* pv_length) {
  static uint8_t path[kTreeMaxDepth];
  const int length = mcts_finish_env(stats_of(st), 1 + 3 * leaves * rounds, max_depth, source_status == 0, q, visits, path, 1, action, best_return);
  for (int h = 0; h < max_depth * segment; ++h) best_plan[h] = h / segment < length ? path[h / segment] : (uint8_t)kPlanStay;
  *pv_length = length;
}

// the score alone (the c_puct = 0 and tie tests read it)
extern "C" double emul_mcts_score(double value_sum, int visits, int pending, double g_lo, double g_hi, double c_puct, float prior, int nv_node) {
  return mcts_score(value_sum, visits, pending, g_lo, g_hi, c_puct, prior, nv_node);
}
