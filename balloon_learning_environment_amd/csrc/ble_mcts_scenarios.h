// ble_mcts_scenarios.h -- the guided tree search in SAMPLED winds: §3v's node pool flown in §3l's M scenario winds.
//
// Node id i of environment e is a GROUP of M = scn->num scenario nodes: node (i, m) lies at mcts_node_index(i, e, n, 3L) M + m of the
// node arena, [R][n][3L][M], so the nodes born in one round are still one contiguous leaf arena, of 3L M leaves per environment.  Id 0
// is environment e itself for every m, with acc 0, disc 1, flown 0.  The statistics stay [n][cap] per GROUP; group_status (0 live,
// 1 spent) and group_g (fp64) are [R][n][3L], the layout §3v's pool_status has: ble_mcts_select_kernel and ble_mcts_finish_kernel
// take a pool view whose status array is group_status and run unchanged -- "status OK" of a group is "not spent".
//
//   ble_mcts_expand_scenarios_kernel   one lane per (e, l, a, m), lane index within the round's slice = destination node index:
//                                      expand_lane (ble_tree.h) with ble_mcts_expand_kernel's lane map times M.  An EXPAND slot's
//                                      lanes take their rule from tree_scenario_lane on the parent group's M status bytes
//                                      and acc words (a live node flies one edge in scenario m, a stopped node of a live group is
//                                      carried on unchanged under every action); any other slot's lanes store void nodes.  No arithmetic
//                                      of its own.
//   ble_mcts_backup_scenarios_kernel   one lane per environment, looping l, a, m: the group step -- M nodes to one G, one prior row, one
//                                      status byte (mcts_group_g, mcts_group_prior, mcts_group_spent) -- and then §3v's backup of that G
//                                      (mcts_newborn, ble_mcts.h).
//
// The group's G.  G_m = acc_m + disc_m V_m, fp64, two statements; V_m the guide's value of node (id, m) where there is one and the node's
// status is OK, else 0.  G: the mean of the `tail` smallest G_m in ble_plan_risk_f32's order -- G_m ascending with -0 equal to +0, then
// m ascending --, summed in that order in double from 0.0, divided by tail once, kept in fp64.  Any non-finite G_m: the group is void.
// The group's prior: the mean of the probs rows of its nodes whose status is OK, m ascending, each component summed in double from 0.0,
// divided by their number once, rounded to float once; uniform without a guide, without such a node, or when one of those rows fails
// mcts_prior_row's test.
//
// The group functions build for the host (tests/emul/mcts_scenarios_emul.cpp); the kernels need hipcc.  No array is indexed at run
// time but the memory the arguments point to: the M values of a group are held in registers, through fully unrolled loops (M <= 16).
// Included by ble_kernels.hip after ble_mcts.h and ble_tree_scenarios.h.
#pragma once
#include "ble_mcts.h"
#include "ble_tree_scenarios.h"

namespace ble {

BLE_FN uint64_t mcts_double_bits(double x) {
  union { double f; uint64_t u; } b;
  b.f = x;
  return b.u;
}
// The ascending sort key of a FINITE G (-0 counts as +0): key(a) < key(b) <=> a < b.  risk_key's, on 64 bits.
BLE_FN uint64_t mcts_group_key(double g) {
  uint64_t u = mcts_double_bits(g);
  if (u == 0x8000000000000000ull) u = 0ull;
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
BLE_FN bool mcts_group_finite(double g) { return (mcts_double_bits(g) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

// G_m of node m of a group: acc, disc, status point at the group's first node, value (NULL: no guide) at its first row.
BLE_FN double mcts_group_node_g(const double* acc, const double* disc, const uint8_t* status, const float* value, int m) {
  const float v_m = (value != nullptr && status[m] == 0) ? value[m] : 0.0f;          // a terminal keeps its return
  const double tail = disc[m] * (double)v_m;
  const double g_m = acc[m] + tail;
  return g_m;
}

// The group's G; NaN: void.  1 <= tail <= num <= 16.  The M values and their keys are formed once, 3L M node reads a round as the backup's
// own: g and key are indexed by fully unrolled loops alone, so they live in registers (no scratch), and the ranks in one 64-bit word.
BLE_FN double mcts_group_g(const double* acc, const double* disc, const uint8_t* status, const float* value, int num, int tail) {
  union { uint64_t u; double f; } nan;
  nan.u = 0x7FF8000000000000ull;
  double g[kScenarioMax];
  uint64_t key[kScenarioMax];
  bool finite = true;
#pragma unroll
  for (int m = 0; m < kScenarioMax; ++m) {
    g[m] = 0.0;
    if (m < num) g[m] = mcts_group_node_g(acc, disc, status, value, m);
    finite = finite && mcts_group_finite(g[m]);
    key[m] = mcts_group_key(g[m]);
  }
  if (!finite) return nan.f;
  // the ranks, four bits each: nibble m = the number of scenarios in front of m (risk_ranks' counting)
  uint64_t ranks = 0;
#pragma unroll
  for (int m = 0; m < kScenarioMax; ++m) {
    uint64_t rank = 0;
#pragma unroll
    for (int j = 0; j < kScenarioMax; ++j)
      if (j < num) rank += (key[j] < key[m] || (key[j] == key[m] && j < m)) ? 1u : 0u;
    if (m < num) ranks |= rank << (4 * m);
  }
  double sum = 0.0;
#pragma unroll 1
  for (int r = 0; r < tail; ++r) {
#pragma unroll
    for (int m = 0; m < kScenarioMax; ++m)
      if (m < num && (int)((ranks >> (4 * m)) & 15u) == r) sum += g[m];                                 // (a permutation: exactly one m)
  }
  const double mean = sum / (double)tail;
  return mean;
}

// whether all M nodes of the group are stopped
BLE_FN bool mcts_group_spent(const uint8_t* status, const double* acc, int num) {
  bool spent = true;
#pragma unroll 1
  for (int m = 0; m < num; ++m) spent = spent && tree_node_stopped(status[m], acc[m]);
  return spent;
}

// The group's prior row: probs (NULL: no guide) points at the group's first row, [num][3].
BLE_FN void mcts_group_prior(const uint8_t* status, const float* probs, int num, float* prior) {
  const float third = 1.0f / 3.0f;
  double sum0 = 0.0, sum1 = 0.0, sum2 = 0.0;
  int rows = 0;
  bool good = probs != nullptr;
  if (good) {
#pragma unroll 1
    for (int m = 0; m < num; ++m) {
      if (status[m] != 0) continue;
      const float* row = probs + 3 * m;
      for (int a = 0; a < 3; ++a) good = good && row[a] >= 0.0f && row[a] <= 3.4028234663852886e38f;      // mcts_prior_row's test
      sum0 += (double)row[0];
      sum1 += (double)row[1];
      sum2 += (double)row[2];
      ++rows;
    }
  }
  good = good && rows > 0;
  const double count = (double)(rows > 0 ? rows : 1);
  const double mean0 = sum0 / count, mean1 = sum1 / count, mean2 = sum2 / count;
  prior[0] = good ? (float)mean0 : third;
  prior[1] = good ? (float)mean1 : third;
  prior[2] = good ? (float)mean2 : third;
}

// Backup of slot l of a round, whose three GROUPS have ids first_id + a: acc, disc, status point at the first node of the first of them
// ([3][num] nodes next to each other), value (NULL: no guide) and probs at the slot's first row, group_status and group_g at the slot's
// first group.  The group step -- the newborn's G, prior and status from its M nodes -- and then mcts_backup_slot's own mcts_newborn.
BLE_FN void mcts_backup_group_slot(const MctsStats& s, int count, int max_depth, int first_id, int v, int what, const double* acc,
                                   const double* disc, const uint8_t* status, const float* value, const float* probs, int num, int tail,
                                   uint8_t* group_status, double* group_g) {
  union { uint64_t u; double f; } nan;
  nan.u = 0x7FF8000000000000ull;
  const bool grown = what == kMctsExpand;
  for (int a = 0; a < 3; ++a) {
    const int c = first_id + a, at = a * num;
    mcts_group_prior(status + at, probs != nullptr ? probs + 3 * at : nullptr, num, s.prior + 3 * c);
    group_status[a] = mcts_group_spent(status + at, acc + at, num) ? 1 : 0;
    const double G = grown ? mcts_group_g(acc + at, disc + at, status + at, value != nullptr ? value + at : nullptr, num, tail) : nan.f;
    group_g[a] = G;
    mcts_newborn(s, count, max_depth, c, v, grown, G != G, G);
  }
  if (grown) s.first_child[v] = first_id;
  if (what == kMctsRevisit) mcts_add_path(s, v, s.g[v], max_depth, count);
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(kMctsBlock) void ble_mcts_backup_scenarios_kernel(MctsPoolDev p, int round, int num, int tail, const float* value,
                                                                               const float* probs, uint8_t* group_status, double* group_g) {
  const int64_t e = (int64_t)blockIdx.x * kMctsBlock + threadIdx.x;
  if (e >= p.n) return;
  const int L = p.leaves, count = 1 + 3 * L * round;
  const MctsStats g = mcts_rows(p, e);
  const int64_t at = ((int64_t)round * p.n + e) * (3 * L), row = e * (3 * L);          // the round's first group: in the pool, in the slice
#pragma unroll 1
  for (int l = 0; l < L; ++l) {
    const int64_t node = (at + 3 * l) * num, leaf = (row + 3 * l) * num;
    mcts_backup_group_slot(g, count, p.max_depth, count + 3 * l, tree_clamp(p.leaf[e * L + l], count), p.kind[e * L + l], p.nodes.acc + node,
                           p.nodes.disc + node, p.nodes.s.status + node, value != nullptr ? value + leaf : nullptr,
                           probs != nullptr ? probs + 3 * leaf : nullptr, num, tail, group_status + at + 3 * l, group_g + at + 3 * l);
  }
  for (int i = 0; i < count; ++i) g.pending[i] = 0;
}

// expand_lane (ble_tree.h) under tree_scenario_lane's rule with the pool's lane map: lane j = ((e 3L + 3l + a) M + m) of the round's slice.
template <class V, class S>
__global__ __launch_bounds__(kStepBlock) void ble_mcts_expand_scenarios_kernel(StateDev st, MctsExpandArgs a, MctsPoolDev p, ScenariosDev b, S seed,
                                                                              ScenarioGen gen, uint32_t* err_flags, V veh) {
  using W = WindScenario<S>;
  __shared__ ScenarioRolloutShared shm;
  const int leaves3 = 3 * p.leaves;
  const int64_t groups_total = a.n * (int64_t)leaves3;
  const int64_t lanes_total = groups_total * b.num;              // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  const bool in_range = j < lanes_total;
  const int64_t ec = in_range ? (int64_t)((uint32_t)j / (uint32_t)b.num) : 0;
  const int sm = in_range ? (int)(j - ec * b.num) : 0;
  const int64_t e = (int64_t)((uint32_t)ec / (uint32_t)leaves3);
  const int slot = (int)(ec - e * leaves3);
  const int act = slot % 3;
  const int64_t dj = (int64_t)a.round * lanes_total + j;         // the child's index in the pool
  W wind{b, seed, gen, sm};
  bool from_pool = false;
  int rule = kTreeLaneVoid;
  int64_t pj = e;                                // the parent node's index: in st, or in the pool
  if (in_range) {
    const int64_t le = e * p.leaves + slot / 3;
    const int id = tree_clamp(p.leaf[le], 1 + leaves3 * a.round);           // ids born before this round
    const bool grow = p.kind[le] == kMctsExpand;
    from_pool = grow && id > 0;
    int64_t pg = e;                              // the parent group's first node
    if (from_pool) { pg = mcts_node_index(id, e, a.n, leaves3) * b.num; pj = pg + sm; }
    // fly or carry: from the parent group's M status bytes and M acc words, once per edge; a slot that does not grow: void
    if (grow) rule = tree_scenario_lane((from_pool ? p.nodes.s.status : st.status) + pg, from_pool ? p.nodes.acc + pg : nullptr, b.num, sm, act);
  }
  expand_lane(st, a, wind, shm, ExpandFromPool{st, p.nodes.s, from_pool}, pj, from_pool ? p.nodes.acc : nullptr, p.nodes.disc, p.nodes.flown,
              p.nodes, dj, e, in_range, act, rule, err_flags, veh);
}
#endif  // __HIPCC__

}  // namespace ble
