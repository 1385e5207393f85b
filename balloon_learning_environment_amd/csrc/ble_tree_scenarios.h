// ble_tree_scenarios.h -- the beam search in SAMPLED winds: §3s's shared-prefix tree flown in §3l's M scenario winds.
//
// A GROUP (e, c) is M scenario nodes, node (e, c, m) at index (e C_d + c) M + m of the level's arena: the same child of the same
// environment, flown in scenario m.  ble_tree_expand_scenarios_kernel flies one edge per lane, one lane per (e, r, a, m), lane index =
// destination node index: the lane loads node (e C_{d-1} + parent[e][r]) M + m of the previous level's arena (at level 1: environment e
// of the state itself) and flies the edge with the lane body of ble_rollout_scenarios_kernel (ble_lookahead.h with WindScenario: one
// text for both -- the same draws, the same noise and correction behind the same three value barriers, the single float add, the same
// order of the three return statements) and stores the child, both in ble_tree_expand_kernel's expand_lane.  Hence a node of a non-void group
// reached by (a_1 .. a_d) holds the bits ble_rollout_scenarios_f32 gives the plan a_1 x segment, .., a_d x segment in scenario m.
// The level's ret is [n][C_d][M]: ble_plan_risk_kernel maps it to [n][C_d], which ble_tree_select_kernel and ble_tree_finish_kernel
// take as their keys.  No arithmetic of its own.
//
// Stopped, spent, void.  A scenario node is STOPPED when its status is not OK or its acc is NaN: it flies nothing and is carried on
// unchanged -- state, acc, disc, flown -- under EVERY action, which is what a frozen lane of ble_rollout_scenarios_kernel holds.  A
// group whose M nodes are all stopped is SPENT: its a = 0 child group is the carry, its a = 1 and a = 2 child groups are VOID, the same
// copies with acc = NaN in all M nodes.  A void group is spent, so all its descendants are void.  (§3s's rule per node would give a NaN
// score to two of the three continuations of a group in which ONE scenario ended, though they differ in every other scenario.)
//
// tree_scenario_lane builds for the host as well (tests/emul/tree_scenarios_emul.cpp); the kernel needs hipcc.
// Included by ble_kernels.hip after ble_tree.h (TreeArenaDev, TreeExpandArgs) and ble_scenarios.h (ScenariosDev, ScenarioRolloutShared).
#pragma once
#include "ble_tree.h"
#include "ble_scenarios.h"

namespace ble {

BLE_FN bool tree_node_stopped(uint8_t status, double acc) { return status != 0 || acc != acc; }

// What the lane of scenario m under action act does, decided from its parent GROUP: status [num] and acc [num] are the group's M status
// bytes and M acc words (acc == nullptr: level 1 -- status[0] is the environment's own byte, the M nodes are that one environment with
// acc 0).  Fly: the node is live.  Carry: the node is stopped, the child is the node unchanged.  Void: the whole group is spent and
// act != 0, the child is the node with acc = NaN.
BLE_FN int tree_scenario_lane(const uint8_t* status, const double* acc, int num, int m, int act) {
  if (acc == nullptr) return status[0] == 0 ? kTreeLaneFly : (act == 0 ? kTreeLaneCarry : kTreeLaneVoid);
  if (!tree_node_stopped(status[m], acc[m])) return kTreeLaneFly;
  bool spent = true;
#pragma unroll 1
  for (int k = 0; k < num; ++k) spent = spent && tree_node_stopped(status[k], acc[k]);
  return spent && act != 0 ? kTreeLaneVoid : kTreeLaneCarry;
}

#if defined(__HIPCC__)
// src.acc == nullptr: level 1 -- src.s is the state itself, node e for every m, with acc 0, disc 1, flown 0.
template <class V, class S>
__global__ __launch_bounds__(kStepBlock) void ble_tree_expand_scenarios_kernel(StateDev st, TreeExpandArgs a, TreeArenaDev src, TreeArenaDev dst,
                                                                              ScenariosDev b, S seed, ScenarioGen gen, uint32_t* err_flags,
                                                                              V veh) {
  using W = WindScenario<S>;
  __shared__ ScenarioRolloutShared shm;
  const int n_children = 3 * a.n_parents;
  const int64_t groups_total = a.n * (int64_t)n_children;
  const int64_t lanes_total = groups_total * b.num;              // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  const bool in_range = j < lanes_total;
  const int64_t ec = in_range ? (int64_t)((uint32_t)j / (uint32_t)b.num) : 0;
  const int sm = in_range ? (int)(j - ec * b.num) : 0;
  const int64_t e = (int64_t)((uint32_t)ec / (uint32_t)n_children);
  const int child = (int)(ec - e * n_children);
  const int act = child % 3;
  const bool first = src.acc == nullptr;
  int64_t pg = e;                                // the parent group's first node in src (level 1: the environment)
  if (in_range && !first) pg = (e * a.parent_children + tree_clamp(a.parent[e * a.beam + child / 3], a.parent_children)) * b.num;
  const int64_t pj = first ? pg : pg + sm;       // the parent node
  W wind{b, seed, gen, sm};
  // fly, carry or void: from the parent group's M status bytes and M acc words, once per edge (the note above tree_scenario_lane)
  int rule = kTreeLaneCarry;
  if (in_range) rule = tree_scenario_lane(src.s.status + pg, first ? nullptr : src.acc + pg, b.num, sm, act);
  expand_lane(st, a, wind, shm, ExpandFromArena{src.s}, pj, src.acc, src.disc, src.flown, dst, j, e, in_range, act, rule, err_flags, veh);
}
#endif  // __HIPCC__

}  // namespace ble
