// ble_tree.h -- plan by beam search: a shared-prefix tree of action plans, level by level on the device.
//
// A level is two launches.  ble_tree_expand_kernel flies one EDGE -- one action for segment x action_repeat agent steps -- per lane, one
// lane per (environment e, parent rank r, action a), child index c = 3 r + a, lane index j = e C + c with C = 3 P children per
// environment: the lane loads node parent[e][r] of the previous level's arena (at level 1: environment e of the state itself), flies the
// edge in ENVIRONMENT e's wind -- its grid, its noise key, its belief slab, whatever the node -- and stores the child as a full state plus
// what the rollout lane keeps in registers across steps (acc, disc in fp64, flown) into index j of the other arena.  The load, the wind
// and the flown step are the rollouts' own (ble_lookahead.h: one text for all of them), the frozen rule is theirs -- hence, for a node
// reached by (a_1 .. a_d), the bits ble_rollout_leaves_f32 gives the plan a_1 x segment, .., a_d x segment: fp32 state and fp64 acc /
// disc pass through memory exactly.
// ble_tree_select_kernel then orders the C children of every environment by §3k's order (the key and rank lane functions of ble_plan.h,
// one wavefront per environment, no atomics) and lists the first min(C, B) as the next level's parents.  After the last level
// ble_tree_finish_kernel orders once more -- by the returns or by a caller's scores -- and walks the best child back through `choice`.
//
// Dead and void nodes: a parent whose status is not OK flies nothing; its a = 0 child carries it on unchanged (the plan "through" a dead
// node earns 0 from there on, as a frozen rollout lane does), its a = 1, 2 children are VOID: the same copy with acc = NaN.  A node whose
// acc is NaN is void however it got there (a flight in a NaN wind included): it is never flown again and all its children are void.
// Void nodes carry a non-finite return, so the order puts them last.
//
// The lane functions of select and finish build for the host as well (tests/emul/tree_emul.cpp); the kernels need hipcc.
// Included by ble_kernels.hip after ble_plan.h (the key and rank functions) and ble_gp_belief.h (BeliefDev, gp_belief_mean).
#pragma once
#include "ble_plan.h"

namespace ble {

constexpr int kTreeMaxBeam = 256;                        // BLE_TREE_MAX_BEAM
constexpr int kTreeMaxChildren = 3 * kTreeMaxBeam;       // 768 <= kPlanMaxPlans: at most 12 keys per lane of the rank count
static_assert(kTreeMaxChildren <= kPlanMaxPlans, "the rank code's bound");
constexpr int kTreeMaxDepth = 960;                       // BLE_ROLLOUT_MAX_STEPS at segment = action_repeat = 1

// a void node stands for nothing: its return is NaN
BLE_FN bool tree_void(float ret) { return ret != ret; }
// an index read from device memory, held to [0, bound): a corrupted list cannot send a load out of its array
BLE_FN int tree_clamp(int v, int bound) { return v < 0 ? 0 : (v >= bound ? bound - 1 : v); }

// Select, child c of one environment: its rank among the n_children keys; the first n_keep in rank order are the next level's parents.
// parent, choice: the environment's lists (ranks are a permutation: every slot below n_keep is written by exactly one child).
BLE_FN void tree_select_lane(const uint32_t* keys, int n_children, int n_keep, int c, int32_t* parent, int32_t* choice) {
  const int rank = plan_rank(keys, n_children, c);
  if (rank < n_keep) { parent[rank] = c; choice[rank] = c; }
}

// The path of child c of level `depth`, walked back to level 1: the child's action is c % 3 and its parent's rank c / 3, whose child
// index at the level above is choice[level - 2][rank] (choice_e: the environment's lists, level d at choice_e + (d - 1) * level_stride).
// path (optional): the action of level d goes to path[d - 1].  Returns the level-1 action.
BLE_FN int tree_backtrack(const int32_t* choice_e, int64_t level_stride, int beam, int depth, int c, uint8_t* path) {
  int a = c % 3;
#pragma unroll 1
  for (int d = depth; d >= 1; --d) {
    a = c % 3;
    if (path != nullptr) path[d - 1] = (uint8_t)a;
    if (d > 1) c = tree_clamp(choice_e[(int64_t)(d - 2) * level_stride + c / 3], 3 * beam);
  }
  return a;
}

// Finish, what one environment answers from its best child (rank 0 of the final order): source_ok false -> all STAY, +0.0f; no finite
// key -> all STAY, -Inf (ble_plan_select_f32's answer at iteration 0); otherwise the child's path.  Returns true when the path is flown.
BLE_FN bool tree_finish_best(bool source_ok, uint32_t key_best, float value_best, float* best_return) {
  union { uint32_t u; float f; } ninf;
  ninf.u = 0xFF800000u;
  if (!source_ok) { *best_return = 0.0f; return false; }
  if (key_best == kPlanKeyNonFinite) { *best_return = ninf.f; return false; }
  *best_return = value_best;
  return true;
}

// What an expand lane does with its parent node.  Fly: one edge.  Carry: the child is the node unchanged.  Void: the same with acc = NaN.
constexpr int kTreeLaneFly = 0, kTreeLaneCarry = 1, kTreeLaneVoid = 2;

#if defined(__HIPCC__)
// A node arena as the kernels take it: a leaf arena (every array leaf_store writes) and the rollout lane's registers
struct TreeArenaDev {
  StateDev s;
  double* acc;               // the discounted return so far, fp64; NaN: void
  double* disc;              // gamma^flown, the rollout's own product
  int32_t* flown;            // agent steps entered with status OK
  float* ret;                // (float)acc
};

// struct ble_tree_expand (include/ble_abi.h) as the kernel takes it
struct TreeExpandArgs {
  int64_t n;
  int n_parents;             // P of the level above (1 at level 1)
  int parent_children;       // C of the level above: node parent[e][r] lies at e * parent_children + parent[e][r] of src
  int beam;                  // the row length of parent
  int edge_steps;            // segment * action_repeat
  int substeps;
  double gamma;
  const float* __restrict__ wind_grid;
  int64_t grid_env_stride;
  const int32_t* __restrict__ parent;      // [n][beam]; level 1: not read
};

// A SOURCE tells expand_lane where its parent's state arrays lie, at each of its two uses.  The beam's: one arena (ble_mcts.h: the pool's).
struct ExpandFromArena {
  const StateDev& s;
  __device__ __forceinline__ const StateDev& state() const { return s; }
};

// THE edge of the two scenario expands (ble_tree_expand_scenarios_kernel, ble_mcts_expand_scenarios_kernel): the parent is node pj of
// src with the words acc / disc / flown [pj] (acc == nullptr: a node of the state itself, with acc 0, disc 1, flown 0), the per-episode
// cache environment e's; the child goes to index dj of dst.  rule: kTreeLaneFly, Carry or Void.  A lane that does not fly stores the
// parent's own words; the child's acc is NaN exactly where the rule is Void.  All lanes of the workgroup call it.  The two one-wind
// expands (below, ble_mcts.h) keep this shell as text: through it, with the rule decided by the loaded node, they were 0.9 - 2.2 % slower.
template <class W, class A, class Src, class V>
__device__ __forceinline__ void expand_lane(const StateDev& st, const A& a, W& wind, typename W::Shared& shm, const Src& src, int64_t pj,
                                            const double* acc, const double* disc, const int32_t* flown, const TreeArenaDev& dst, int64_t dj,
                                            int64_t e, bool in_range, int act, int rule, uint32_t* err_flags, const V& veh) {
  LookaheadLane l;
  bool live = false;
  if (in_range) {
    lookahead_load(l, src.state(), pj, st, a.n, e);
    if (acc != nullptr) { l.acc = acc[pj]; l.disc = disc[pj]; l.flown = flown[pj]; }
    wind.load(e);
    live = rule == kTreeLaneFly;                 // a stopped node flies nothing
  }
  const bool flew = live;                        // (edge_steps >= 1: a live parent enters its first step)
  lookahead_fill<W>(shm);
  __syncthreads();
  lookahead_begin(l, wind, shm, st, a, e, in_range, live, veh);
#pragma unroll 1
  for (int t = 0; t < a.edge_steps; ++t) {
    if (live) lookahead_step(l, wind, shm, a, act, veh);
    live = live && l.s.status == kOk;            // a scenario that went terminal: frozen, reward 0
  }
  if (in_range) {
    leaf_store(src.state(), dst.s, pj, dj, flew, l.s, l.c, act);
    if (rule == kTreeLaneVoid) l.acc = __builtin_nan("");
    dst.acc[dj] = l.acc; dst.disc[dj] = l.disc; dst.flown[dj] = l.flown;
    dst.ret[dj] = (float)l.acc;
  }
  report_flags(l.flags, err_flags);
}

// src.acc == nullptr: level 1 -- src.s is the state itself, node e, with acc 0, disc 1, flown 0.
template <int kWind, class V = VehicleDefault>
__global__ __launch_bounds__(kStepBlock) void ble_tree_expand_kernel(StateDev st, TreeExpandArgs a, TreeArenaDev src, TreeArenaDev dst,
                                                                     BeliefDev b, StepNoise gen, uint32_t* err_flags, V veh) {
  using W = LookaheadWind<kWind>;
  __shared__ typename W::Shared shm;
  W wind;
  if constexpr (kWind == kTreeWindNoise) wind.gen = gen;
  if constexpr (kWind == kTreeWindBelief) wind.b = b;
  const int n_children = 3 * a.n_parents;
  const int64_t lanes_total = a.n * (int64_t)n_children;         // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  const bool in_range = j < lanes_total;
  const int64_t e = in_range ? (int64_t)((uint32_t)j / (uint32_t)n_children) : 0;
  const int child = in_range ? (int)(j - e * n_children) : 0;
  const int act = child % 3;
  const bool first = src.acc == nullptr;
  int64_t pj = e;                                // the parent node's index in src
  if (in_range && !first) pj = e * a.parent_children + tree_clamp(a.parent[e * a.beam + child / 3], a.parent_children);
  LookaheadLane l;
  bool live = false;
  if (in_range) {
    // the parent node's state; the per-episode cache is environment e's: a node holds its environment's constants
    lookahead_load(l, src.s, pj, st, a.n, e);
    if (!first) { l.acc = src.acc[pj]; l.disc = src.disc[pj]; l.flown = src.flown[pj]; }
    wind.load(e);
    live = l.s.status == kOk && !(l.acc != l.acc);     // a dead or void parent flies nothing
  }
  const bool flew = live;                        // (edge_steps >= 1: a live parent enters its first step)
  lookahead_fill<W>(shm);
  __syncthreads();
  lookahead_begin(l, wind, shm, st, a, e, in_range, live, veh);
#pragma unroll 1
  for (int t = 0; t < a.edge_steps; ++t) {
    if (live) lookahead_step(l, wind, shm, a, act, veh);
    live = live && l.s.status == kOk;            // a plan that went terminal: frozen, reward 0
  }
  if (in_range) {
    // the child: what the lane holds after its last executed step, or -- a dead or void parent -- the parent's own words (leaf_store)
    leaf_store(src.s, dst.s, pj, j, flew, l.s, l.c, act);
    // a parent that flew nothing is carried on by its a = 0 child alone; the others, and every child of a void parent, are void
    if (!flew && act != 0) l.acc = __builtin_nan("");
    dst.acc[j] = l.acc; dst.disc[j] = l.disc; dst.flown[j] = l.flown;
    dst.ret[j] = (float)l.acc;
  }
  report_flags(l.flags, err_flags);
}

// struct ble_tree_select (include/ble_abi.h) as the kernel takes it
struct TreeSelectArgs {
  int64_t n;
  int n_children, beam;
  const float* __restrict__ ret;               // [n][C]
  int32_t* __restrict__ parent;                // [n][beam]
  int32_t* __restrict__ choice;                // [n][beam]: this level's lists
};

// One wavefront per environment: keys in LDS, every lane ranks its children (c = lane, lane + 64, ...: at most 12).
__global__ __launch_bounds__(kPlanSelectBlock) void ble_tree_select_kernel(TreeSelectArgs a) {
  __shared__ uint32_t keys[kTreeMaxChildren];
  const int64_t e = blockIdx.x;
  const int lane = (int)threadIdx.x, C = a.n_children;
  for (int c = lane; c < C; c += kPlanSelectBlock) keys[c] = plan_key(a.ret[e * C + c]);
  __syncthreads();
  const int n_keep = C < a.beam ? C : a.beam;
  for (int c = lane; c < C; c += kPlanSelectBlock) tree_select_lane(keys, C, n_keep, c, a.parent + e * a.beam, a.choice + e * a.beam);
}

// struct ble_tree_finish (include/ble_abi.h) as the kernel takes it
struct TreeFinishArgs {
  int64_t n;
  int n_children, beam, depth, segment;
  const float* __restrict__ ret;               // [n][C]: void where NaN
  const float* __restrict__ score;             // [n][C]: the keys' values (ret itself without a leaf value)
  const uint8_t* __restrict__ source_status;   // [n]
  const int32_t* __restrict__ choice;          // [depth][n][beam] (levels 1 .. depth - 1 are read)
  uint8_t* __restrict__ best_plan;             // [depth * segment][n]
  uint8_t* __restrict__ action;                // [n]
  float* __restrict__ best_return;             // [n]
  float* __restrict__ q;                       // optional [n][3]
  int32_t* __restrict__ visits;                // optional [n][3]
};

// One wavefront per environment: the final order's first child, its path, and per root action the best key and the non-void count.
__global__ __launch_bounds__(kPlanSelectBlock) void ble_tree_finish_kernel(TreeFinishArgs a) {
  __shared__ uint32_t keys[kTreeMaxChildren];
  __shared__ uint8_t root[kTreeMaxBeam];         // the level-1 action of the parents of the last level, by rank
  __shared__ uint8_t path[kTreeMaxDepth];
  __shared__ int s_best;
  __shared__ uint32_t s_key[kPlanActions][kPlanSelectBlock];
  __shared__ int s_k[kPlanActions][kPlanSelectBlock];
  __shared__ int s_visits[kPlanActions][kPlanSelectBlock];
  const int64_t e = blockIdx.x;
  const int lane = (int)threadIdx.x, C = a.n_children, D = a.depth;
  const int64_t level_stride = a.n * (int64_t)a.beam;
  const int32_t* const choice_e = a.choice + e * a.beam;
  for (int c = lane; c < C; c += kPlanSelectBlock) keys[c] = plan_key(a.score[e * C + c]);
  __syncthreads();
  for (int c = lane; c < C; c += kPlanSelectBlock)
    if (plan_rank(keys, C, c) == 0) s_best = c;                  // (ranks are a permutation: exactly one child writes)
  if (a.q != nullptr && D > 1)                                   // the parents' level-1 actions: parent r is child choice[D - 1][r] of level D - 1
    for (int r = lane; r < C / 3; r += kPlanSelectBlock)
      root[r] = (uint8_t)tree_backtrack(choice_e, level_stride, a.beam, D - 1, tree_clamp(choice_e[(int64_t)(D - 2) * level_stride + r], 3 * a.beam),
                                        nullptr);
  __syncthreads();
  const int c_best = s_best;
  float best_return;
  const bool flown = tree_finish_best(a.source_status[e] == 0, keys[c_best], a.score[e * C + c_best], &best_return);
  if (flown && lane == 0) tree_backtrack(choice_e, level_stride, a.beam, D, c_best, path);
  __syncthreads();
  for (int h = lane; h < D * a.segment; h += kPlanSelectBlock) a.best_plan[h * a.n + e] = flown ? path[h / a.segment] : (uint8_t)kPlanStay;
  if (lane == 0) { a.best_return[e] = best_return; a.action[e] = flown ? path[0] : (uint8_t)kPlanStay; }
  if (a.q == nullptr) return;                                    // (uniform over the workgroup)
  PlanActionBest mine;
  plan_action_best_init(mine);
  for (int c = lane; c < C; c += kPlanSelectBlock) {
    const int act = D > 1 ? (int)root[c / 3] : c;
    const int counts = tree_void(a.ret[e * C + c]) ? 0 : 1;
#pragma unroll
    for (int k = 0; k < kPlanActions; ++k)
      plan_action_best_take(mine, k, act == k ? keys[c] : kPlanKeyNonFinite, act == k ? c : kPlanNoPlan, act == k ? counts : 0);
  }
#pragma unroll
  for (int k = 0; k < kPlanActions; ++k) { s_key[k][lane] = mine.key[k]; s_k[k][lane] = mine.k[k]; s_visits[k][lane] = mine.visits[k]; }
  __syncthreads();
  if (lane >= kPlanActions) return;
  uint32_t key = kPlanKeyNonFinite;
  int k = kPlanNoPlan, n_visits = 0;
  for (int l = 0; l < kPlanSelectBlock; ++l) {
    const bool better = plan_before(s_key[lane][l], s_k[lane][l], key, k);
    key = better ? s_key[lane][l] : key;
    k = better ? s_k[lane][l] : k;
    n_visits += s_visits[lane][l];
  }
  const float value = key != kPlanKeyNonFinite ? a.score[e * C + k] : 0.0f;       // (a finite key names a real child: k < C)
  int32_t q_k;
  plan_action_write(key, k, value, n_visits, false, a.q + 3 * e + lane, &q_k, a.visits + 3 * e + lane);
}
#endif  // __HIPCC__

}  // namespace ble
