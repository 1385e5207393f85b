// ble_mcts.h -- guided tree search: PUCT over a persistent node pool, a prior and a value per node.
//
// Per environment a pool of cap = 1 + 3 L R node ids: id 0 is the root -- environment e of the simulator itself, never copied --, id
// 1 + r 3L + 3l + a the child under action a of the l-th leaf chosen in round r.  The nodes are ble_tree_arena entries stored round-major,
// [R][n][3L]: the nodes born in one round are one contiguous leaf arena of 3L leaves per environment (mcts_node_index).  The statistics
// lie [n][cap]: parent, first_child (0: not expanded), depth, visits, pending (int32), value_sum, g (fp64), prior [3] (fp32), and per
// environment g_range = (g_lo, g_hi).
//
// A round is three launches with the caller's network between the second and the third:
//   ble_mcts_select_kernel   L descents per environment by PUCT, in order, each seeing the pending visits of the ones before it
//   ble_mcts_expand_kernel   one lane per (e, l, a): the edge flown with the rollouts' own text (ble_lookahead.h), hence their bits
//   ble_mcts_backup_kernel   the newborn's statistics, G = acc + disc V along the path to the root, pending cleared
// and ble_mcts_finish_kernel reads the answer off the root's children.  Select, backup and finish: one lane per environment on the
// global arrays.  Measured against one wavefront per environment with the statistics staged in LDS (profiles/mcts_rate.jsonl:
// N = 4 096, R = 16, L = 8): the selects of a decision 1.91 ms against 3.29, the backups 1.61 against 1.54, the finish 0.02 against
// 0.03; the decision 8.46 ms against 9.81.  The faster is kept.
//
// The score is fp64, one operation per statement, + - x / sqrt only: every statement rounds once, on the device as on the host, so
// tests/mcts_host.py's NumPy twin is held to the bits.  The lane functions build for the host (tests/emul/mcts_emul.cpp).
// Included by ble_kernels.hip after ble_tree.h (TreeArenaDev, tree_clamp) and ble_gp_belief.h.
#pragma once
#include "ble_tree.h"

namespace ble {

constexpr int kMctsMaxLeaves = 256;                      // BLE_MCTS_MAX_LEAVES: L R at most
constexpr int kMctsMaxNodes = 1 + 3 * kMctsMaxLeaves;    // 769 ids per environment
constexpr int kMctsEmpty = 0, kMctsExpand = 1, kMctsRevisit = 2;      // BLE_MCTS_EMPTY / EXPAND / REVISIT

// One environment's statistics, wherever they lie (a row of the global arrays, a test's arrays)
struct MctsStats {
  int32_t *parent, *first_child, *depth, *visits, *pending;
  double *value_sum, *g;
  float* prior;              // [cap][3]
  double* g_range;           // g_lo, g_hi
};

// where node id >= 1 of environment e lies in the round-major node arrays
BLE_FN int64_t mcts_node_index(int id, int64_t e, int64_t n, int leaves3) {
  const int k = id - 1, r = k / leaves3;
  return ((int64_t)r * n + e) * leaves3 + (k - r * leaves3);
}

// whether a node's status is OK: the root's is the source's, any other's the pool's
struct MctsStatusOk {
  const uint8_t* source;     // [n]
  const uint8_t* pool;       // [R][n][3L]
  int64_t n, e;
  int leaves3;
};
BLE_FN bool mcts_status_ok(const MctsStatusOk& k, int id) {
  return (id == 0 ? k.source[k.e] : k.pool[mcts_node_index(id, k.e, k.n, k.leaves3)]) == 0;
}

// The root before round 0: no parent, not expanded, no visit; prior: the caller's row (sanitised as every row is) or uniform.
BLE_FN void mcts_prior_row(const float* row, float* prior) {
  const float third = 1.0f / 3.0f;
  bool good = row != nullptr;
  if (good)
    for (int a = 0; a < 3; ++a) good = good && row[a] >= 0.0f && row[a] <= 3.4028234663852886e38f;       // (a NaN fails both)
  for (int a = 0; a < 3; ++a) prior[a] = good ? row[a] : third;
}
BLE_FN void mcts_root_init(const MctsStats& s, const float* root_prior) {
  union { uint64_t u; double f; } inf;
  inf.u = 0x7FF0000000000000ull;
  s.parent[0] = -1; s.first_child[0] = 0; s.depth[0] = 0; s.visits[0] = 0; s.pending[0] = 0;
  s.value_sum[0] = 0.0; s.g[0] = 0.0;
  mcts_prior_row(root_prior, s.prior);
  s.g_range[0] = inf.f; s.g_range[1] = -inf.f;
}

// PUCT: Qn + c_puct prior sqrt(Nv(node)) / (1 + Nv(child)), Nv = visits + pending.  Qn: the child's mean, scaled to the range of G seen
// so far (0 while that range is empty), times visits / Nv -- a pending visit is a visit worth g_lo.  One rounding per statement.
BLE_FN double mcts_score(double value_sum, int visits, int pending, double g_lo, double g_hi, double c_puct, float prior, int nv_node) {
  const double n_visits = (double)visits;
  const double nv = (double)(visits + pending);
  const double mean = value_sum / n_visits;
  const double above = mean - g_lo;
  const double range = g_hi - g_lo;
  double qn = 0.0;
  if (range > 0.0) qn = above / range;
  const double share = n_visits / nv;
  qn = qn * share;
  const double root = d_sqrt((double)nv_node);
  double u = c_puct * (double)prior;
  u = u * root;
  const double below = 1.0 + nv;
  u = u / below;
  const double score = qn + u;
  return score;
}

// `add` pending visits on node v and every ancestor (a path has at most max_depth edges: a corrupted list cannot loop)
BLE_FN void mcts_pend_path(const MctsStats& s, int v, int add, int max_depth, int count) {
  for (int hop = 0; hop <= max_depth && v >= 0; ++hop) {
    s.pending[v] += add;
    v = s.parent[v] < count ? s.parent[v] : -1;
  }
}
// one visit worth G on node v and every ancestor
BLE_FN void mcts_add_path(const MctsStats& s, int v, double G, int max_depth, int count) {
  for (int hop = 0; hop <= max_depth && v >= 0; ++hop) {
    s.visits[v] += 1;
    s.value_sum[v] += G;
    v = s.parent[v] < count ? s.parent[v] : -1;
  }
}

// Descent l of a round: from the root by the largest score among the non-void children (visits > 0), ties to the lower action, to
//   EXPAND   a node that is not expanded, OK, above max_depth and not chosen by an earlier slot of this round: pending += 3 on its path
//   EMPTY    a node an earlier slot chose; also a root that is not OK or whose children are all void
//   REVISIT  a node that cannot grow -- status not OK, depth == max_depth, or expanded into three void children: pending += 1
// count: the ids born before this round (1 + 3L round).  leaf, kind: the environment's lists, slots < l already written.
BLE_FN void mcts_select_slot(const MctsStats& s, int count, int max_depth, double c_puct, int l, int32_t* leaf, int32_t* kind,
                             const MctsStatusOk& ok) {
  const double g_lo = s.g_range[0], g_hi = s.g_range[1];
  int v = 0, what = kMctsEmpty;
  if (mcts_status_ok(ok, 0)) {
    for (int level = 0; level <= max_depth; ++level) {
      const int fc = s.first_child[v];
      if (fc <= 0 || fc + 2 >= count) {          // not expanded
        bool chosen = false;
        for (int k = 0; k < l; ++k) chosen = chosen || (kind[k] == kMctsExpand && leaf[k] == v);
        what = chosen ? kMctsEmpty : ((!mcts_status_ok(ok, v) || s.depth[v] >= max_depth) ? kMctsRevisit : kMctsExpand);
        break;
      }
      const int nv_node = s.visits[v] + s.pending[v];
      int best = -1;
      double best_score = 0.0;
      for (int a = 0; a < 3; ++a) {
        const int c = fc + a;
        if (s.visits[c] <= 0) continue;          // void
        const double score = mcts_score(s.value_sum[c], s.visits[c], s.pending[c], g_lo, g_hi, c_puct, s.prior[3 * v + a], nv_node);
        if (best < 0 || score > best_score) { best = c; best_score = score; }
      }
      if (best < 0) { what = v == 0 ? kMctsEmpty : kMctsRevisit; break; }
      v = best;
    }
  }
  leaf[l] = v;
  kind[l] = what;
  if (what != kMctsEmpty) mcts_pend_path(s, v, what == kMctsExpand ? 3 : 1, max_depth, count);
}

// The newborn c of both backups (this file's and ble_mcts_scenarios.h's), born under node v by a slot that grew or not: its links, and
// -- unless it is void: no G, never selected -- one visit worth G on itself, in the range, and on v and every ancestor.
BLE_FN void mcts_newborn(const MctsStats& s, int count, int max_depth, int c, int v, bool grown, bool is_void, double G) {
  union { uint64_t u; double f; } nan;
  nan.u = 0x7FF8000000000000ull;
  s.parent[c] = grown ? v : -1;
  s.depth[c] = grown ? s.depth[v] + 1 : 0;
  s.first_child[c] = 0;
  s.pending[c] = 0;
  if (is_void) { s.visits[c] = 0; s.value_sum[c] = 0.0; s.g[c] = nan.f; return; }
  s.g[c] = G; s.visits[c] = 1; s.value_sum[c] = G;
  if (G < s.g_range[0]) s.g_range[0] = G;
  if (G > s.g_range[1]) s.g_range[1] = G;
  mcts_add_path(s, v, G, max_depth, count);
}

// Backup of slot l of a round, whose three nodes have ids first_id + a and lie next to each other in the pool: acc, disc, status point
// at the first of them, value (NULL: no guide, V = 0) and probs (NULL: uniform) at the slot's first row.  count: the ids born before
// this round.
BLE_FN void mcts_backup_slot(const MctsStats& s, int count, int max_depth, int first_id, int v, int what, const double* acc,
                             const double* disc, const uint8_t* status, const float* value, const float* probs) {
  const bool grown = what == kMctsExpand;
  for (int a = 0; a < 3; ++a) {
    const int c = first_id + a;
    const double acc_c = acc[a];
    mcts_prior_row(probs != nullptr ? probs + 3 * a : nullptr, s.prior + 3 * c);
    const bool is_void = !grown || acc_c != acc_c;
    double G = 0.0;
    if (!is_void) {
      const float v_c = (value != nullptr && status[a] == 0) ? value[a] : 0.0f;      // a terminal keeps its return
      const double tail = disc[a] * (double)v_c;
      G = acc_c + tail;
    }
    mcts_newborn(s, count, max_depth, c, v, grown, is_void, G);
  }
  if (grown) s.first_child[v] = first_id;
  if (what == kMctsRevisit) mcts_add_path(s, v, s.g[v], max_depth, count);
}

// The most visited child of an expanded node: ties to the larger mean (as fp32), then to the lower action; -1: none was visited.
// q, visits (optional): every child's mean as fp32 (-Inf: void) and its visits.
BLE_FN int mcts_best_child(const MctsStats& s, int fc, float* q, int32_t* visits) {
  union { uint32_t u; float f; } ninf;
  ninf.u = 0xFF800000u;
  int best = -1, best_n = 0;
  float best_q = ninf.f;
  for (int a = 0; a < 3; ++a) {
    const int n_a = s.visits[fc + a];
    float q_a = ninf.f;
    if (n_a > 0) {
      const double mean = s.value_sum[fc + a] / (double)n_a;
      q_a = (float)mean;
    }
    if (q != nullptr) { q[a] = q_a; visits[a] = n_a > 0 ? n_a : 0; }
    if (n_a > 0 && (best < 0 || n_a > best_n || (n_a == best_n && q_a > best_q))) { best = a; best_n = n_a; best_q = q_a; }
  }
  return best;
}

// Finish of one environment: q, visits [3] of the root's children, the action, its q, and the principal variation -- the most visited
// child followed down to a node without children -- into path (at most max_depth actions); returns its length.  A source that is not OK:
// STAY, +0.0f; a root without a visited child: STAY, -Inf; both with length 0.  count: every id born (1 + 3 L R).  Level d's action goes
// to path[d * path_stride].
BLE_FN int mcts_finish_env(const MctsStats& s, int count, int max_depth, bool source_ok, float* q, int32_t* visits, uint8_t* path,
                           int64_t path_stride, uint8_t* action, float* best_return) {
  union { uint32_t u; float f; } ninf;
  ninf.u = 0xFF800000u;
  for (int a = 0; a < 3; ++a) { q[a] = ninf.f; visits[a] = 0; }
  *action = (uint8_t)kPlanStay;
  if (!source_ok) { *best_return = 0.0f; return 0; }
  *best_return = ninf.f;
  int v = 0, length = 0;
  while (length < max_depth) {
    const int fc = s.first_child[v];
    if (fc <= 0 || fc + 2 >= count) break;
    const int a = mcts_best_child(s, fc, v == 0 ? q : nullptr, visits);
    if (a < 0) break;
    if (v == 0) { *action = (uint8_t)a; *best_return = q[a]; }
    path[(length++) * path_stride] = (uint8_t)a;
    v = fc + a;
  }
  return length;
}

#if defined(__HIPCC__)
constexpr int kMctsBlock = 64;                   // environments per workgroup of select, backup and finish

// struct ble_mcts_pool (include/ble_abi.h) as the kernels take it.  No __restrict__: the expand reads one round's nodes and writes
// another's through the same arrays (StateDev carries none either).
struct MctsPoolDev {
  int64_t n;
  int rounds, leaves, max_depth, segment;
  TreeArenaDev nodes;
  MctsStats stats;           // the global arrays, [n][cap]
  int32_t *leaf, *kind;      // [n][L]
};
__device__ __forceinline__ int mcts_cap(const MctsPoolDev& p) { return 1 + 3 * p.leaves * p.rounds; }
// environment e's rows of the global arrays
__device__ __forceinline__ MctsStats mcts_rows(const MctsPoolDev& p, int64_t e) {
  const int64_t at = e * mcts_cap(p);
  const MctsStats& g = p.stats;
  return MctsStats{g.parent + at, g.first_child + at, g.depth + at, g.visits + at, g.pending + at, g.value_sum + at, g.g + at,
                   g.prior + 3 * at, g.g_range + 2 * e};
}

// ---- select, backup, finish: one lane per environment on the global arrays
__global__ __launch_bounds__(kMctsBlock) void ble_mcts_select_kernel(MctsPoolDev p, int round, double c_puct, const uint8_t* source_status,
                                                                     const float* root_prior) {
  const int64_t e = (int64_t)blockIdx.x * kMctsBlock + threadIdx.x;
  if (e >= p.n) return;
  const int L = p.leaves, count = 1 + 3 * L * round;
  const MctsStats g = mcts_rows(p, e);
  if (round == 0) mcts_root_init(g, root_prior != nullptr ? root_prior + 3 * e : nullptr);
  const MctsStatusOk ok{source_status, p.nodes.s.status, p.n, e, 3 * L};
#pragma unroll 1
  for (int l = 0; l < L; ++l) mcts_select_slot(g, count, p.max_depth, c_puct, l, p.leaf + e * L, p.kind + e * L, ok);
}

__global__ __launch_bounds__(kMctsBlock) void ble_mcts_backup_kernel(MctsPoolDev p, int round, const float* value, const float* probs) {
  const int64_t e = (int64_t)blockIdx.x * kMctsBlock + threadIdx.x;
  if (e >= p.n) return;
  const int L = p.leaves, count = 1 + 3 * L * round;
  const MctsStats g = mcts_rows(p, e);
  const int64_t at = ((int64_t)round * p.n + e) * (3 * L), row = e * (3 * L);
#pragma unroll 1
  for (int l = 0; l < L; ++l)
    mcts_backup_slot(g, count, p.max_depth, count + 3 * l, tree_clamp(p.leaf[e * L + l], count), p.kind[e * L + l], p.nodes.acc + at + 3 * l,
                     p.nodes.disc + at + 3 * l, p.nodes.s.status + at + 3 * l, value != nullptr ? value + row + 3 * l : nullptr,
                     probs != nullptr ? probs + 3 * (row + 3 * l) : nullptr);
  for (int i = 0; i < count; ++i) g.pending[i] = 0;
}

// struct ble_mcts_finish (include/ble_abi.h) as the kernel takes it
struct MctsFinishArgs {
  const uint8_t* source_status;
  uint8_t* best_plan;        // [D * segment][n]
  uint8_t* action;
  float* best_return;
  float* q;                  // [n][3]
  int32_t* visits;           // [n][3]
  int32_t* pv_length;
};
__global__ __launch_bounds__(kMctsBlock) void ble_mcts_finish_kernel(MctsPoolDev p, MctsFinishArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kMctsBlock + threadIdx.x;
  if (e >= p.n) return;
  // the path goes through best_plan's own column -- level d at row d * segment -- and is spread over the segments from the last row down
  const MctsStats g = mcts_rows(p, e);
  const int64_t level_stride = (int64_t)p.segment * p.n;
  const int length = mcts_finish_env(g, mcts_cap(p), p.max_depth, a.source_status[e] == 0, a.q + 3 * e, a.visits + 3 * e, a.best_plan + e,
                                     level_stride, a.action + e, a.best_return + e);
  for (int h = p.max_depth * p.segment - 1; h >= 0; --h)
    a.best_plan[h * p.n + e] = h / p.segment < length ? a.best_plan[(h / p.segment) * level_stride + e] : (uint8_t)kPlanStay;
  a.pv_length[e] = length;
}

// struct ble_mcts_expand (include/ble_abi.h) as the kernel takes it: the members lookahead_begin / lookahead_step read of their `A`
struct MctsExpandArgs {
  int64_t n;
  int round, edge_steps, substeps;
  double gamma;
  const float* wind_grid;
  int64_t grid_env_stride;
};

// expand_lane's source in the pool: the pool, or -- id 0, a slot that does not grow -- the state itself.  The choice is formed again at
// each use: bound once to a `const StateDev&` it is a StateDev of its own, 584 bytes of scratch per lane.
struct ExpandFromPool {
  const StateDev &st, &pool;
  bool from_pool;
  __device__ __forceinline__ const StateDev& state() const { return from_pool ? pool : st; }
};

// ble_tree_expand_kernel's shell (text, as there: the note above expand_lane) with the pool's lane map: lane j = e 3L + 3l + a.  An EXPAND slot's lane loads
// node leaf[e][l] (id 0: environment e of st, with acc 0, disc 1, flown 0), flies the edge and stores the child; every other lane
// stores a void node (the source's words, acc NaN).
template <int kWind, class V = VehicleDefault>
__global__ __launch_bounds__(kStepBlock) void ble_mcts_expand_kernel(StateDev st, MctsExpandArgs a, MctsPoolDev p, BeliefDev b, StepNoise gen,
                                                                     uint32_t* err_flags, V veh) {
  using W = LookaheadWind<kWind>;
  __shared__ typename W::Shared shm;
  W wind;
  if constexpr (kWind == kTreeWindNoise) wind.gen = gen;
  if constexpr (kWind == kTreeWindBelief) wind.b = b;
  const int leaves3 = 3 * p.leaves;
  const int64_t lanes_total = a.n * (int64_t)leaves3;            // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  const bool in_range = j < lanes_total;
  const int64_t e = in_range ? (int64_t)((uint32_t)j / (uint32_t)leaves3) : 0;
  const int slot = in_range ? (int)(j - e * leaves3) : 0;
  const int act = slot % 3;
  const int64_t dj = (int64_t)a.round * lanes_total + j;         // the child's index in the pool
  LookaheadLane l;
  bool live = false, from_pool = false;
  int64_t pj = e;                                // the parent node's index: in st, or in the pool
  if (in_range) {
    const int64_t le = e * p.leaves + slot / 3;
    const int id = tree_clamp(p.leaf[le], 1 + leaves3 * a.round);           // ids born before this round
    const bool grow = p.kind[le] == kMctsExpand;
    from_pool = grow && id > 0;
    if (from_pool) pj = mcts_node_index(id, e, a.n, leaves3);
    // the parent node's state; the per-episode cache is environment e's: a node holds its environment's constants
    lookahead_load(l, from_pool ? p.nodes.s : st, pj, st, a.n, e);
    if (from_pool) { l.acc = p.nodes.acc[pj]; l.disc = p.nodes.disc[pj]; l.flown = p.nodes.flown[pj]; }
    wind.load(e);
    live = grow && l.s.status == kOk && !(l.acc != l.acc);       // (select chose an OK, non-void leaf: held again here)
  }
  const bool flew = live;                        // (edge_steps >= 1: a live parent enters its first step)
  lookahead_fill<W>(shm);
  __syncthreads();
  lookahead_begin(l, wind, shm, st, a, e, in_range, live, veh);
#pragma unroll 1
  for (int t = 0; t < a.edge_steps; ++t) {
    if (live) lookahead_step(l, wind, shm, a, act, veh);
    live = live && l.s.status == kOk;            // an edge that went terminal: frozen, reward 0
  }
  if (in_range) {
    leaf_store(from_pool ? p.nodes.s : st, p.nodes.s, pj, dj, flew, l.s, l.c, act);
    if (!flew) l.acc = __builtin_nan("");        // nothing was flown: void
    p.nodes.acc[dj] = l.acc; p.nodes.disc[dj] = l.disc; p.nodes.flown[dj] = l.flown;
    p.nodes.ret[dj] = (float)l.acc;
  }
  report_flags(l.flags, err_flags);
}
#endif  // __HIPCC__

}  // namespace ble
