// ble_replay.h -- prioritized n-step replay on the device: the sum tree of Dopamine 4.0.0's
// OutOfGraphPrioritizedReplayBuffer over the per-environment ring of ble_train.h, its stratified sampler and set_priority.
//
// The tree is a heap of fp64 nodes padded to a power of two P: nodes[1] is the root, nodes[P + i] leaf i, the padded leaves are 0.
// Leaf (t % T) N + env is the n-step window that starts at ring row t for that environment, so the leaves of one vector step form one
// contiguous block.  A parent is always recomputed as left + right from its children (never updated with += delta), so the tree is a
// pure function of its leaves.  No atomics: every kernel that writes the tree is one workgroup, level by level with a barrier between.
//
// When a window enters the tree: adding vector step s zeroes row s % T (its windows are being overwritten) and gives row (s - n) % T,
// whose windows have just become complete, the max recorded priority -- 0 for a window that crosses a time-limit end without a terminal
// (replay_window).  Every nonzero leaf is then a valid window; the sampler's validity check is only a guard.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ble_train.h"

namespace ble {

constexpr int kTreeBlock = 1024;                 // the one workgroup of the tree add and set-priority kernels
constexpr uint32_t kFlagReplayPriority = 8192u;

// Correctly rounded float32 sqrt and quotient (as NumPy / XLA's): through fp64, where the double rounding is innocuous (53 >= 2 x 24 + 2);
// __fsqrt_rn is 1 ulp off on gfx950.
__device__ inline float sqrt_f32_rn(float x) { return (float)sqrt((double)x); }
__device__ inline float div_f32_rn(float a, float b) { return (float)((double)a / (double)b); }

// Recomputes nodes lo .. hi (inclusive, at one level) from their children; skip_lo .. skip_hi are left to another pass of the loop.
__device__ inline void tree_sum_range(double* __restrict__ nodes, int64_t lo, int64_t hi, int64_t skip_lo, int64_t skip_hi) {
  for (int64_t i = lo + threadIdx.x; i <= hi; i += kTreeBlock)
    if (i < skip_lo || i > skip_hi) nodes[i] = nodes[2 * i] + nodes[2 * i + 1];
}

// After vector step s = count - 1 was added: zero row s % T, give row (s - n) % T the max recorded priority (valid windows) or 0,
// then the ancestors of both contiguous leaf ranges.
__global__ __launch_bounds__(kTreeBlock) void ble_tree_add_kernel(ble_replay_f32 rp, ble_sum_tree_f64 tr) {
  const int64_t s = *rp.count - 1;
  if (s < 0) return;
  const int64_t N = rp.num_envs, T = rp.capacity, P = tr.padded;
  const int n = rp.update_horizon;
  double* __restrict__ nodes = tr.nodes;
  const bool complete = s >= n;
  const int64_t z0 = P + (s % T) * N, c0 = complete ? P + ((s - n) % T) * N : z0;
  const double mx = *tr.max_priority;
  for (int64_t e = threadIdx.x; e < N; e += kTreeBlock) {
    nodes[z0 + e] = 0.0;
    int m, term;
    if (complete) nodes[c0 + e] = replay_window(rp, s - n, e, &m, &term) ? mx : 0.0;
  }
  __syncthreads();
  int64_t zl = z0, zh = z0 + N - 1, cl = c0, ch = c0 + N - 1;
  while (zl > 1) {
    zl >>= 1; zh >>= 1; cl >>= 1; ch >>= 1;
    tree_sum_range(nodes, zl, zh, 1, 0);
    tree_sum_range(nodes, cl, ch, zl, zh);          // (the two ranges may meet near the root: each node is written once)
    __syncthreads();
  }
}

// Dopamine's SumTree.sample walk from a query q in [0, total): left if q < left sum, else q -= left sum and right.  A child whose sum is
// 0 is never entered (rounding can point at an empty subtree): the walk takes the other child, so it ends on a nonzero leaf whenever the
// root is nonzero.  Returns the leaf index (node - P).
__device__ inline int64_t tree_find(const double* __restrict__ nodes, int64_t padded, double q) {
  int64_t node = 1;
  while (node < padded) {
    const double l = nodes[2 * node], r = nodes[2 * node + 1];
    bool left = q < l;
    if (left && !(l > 0.0)) left = false;
    else if (!left && !(r > 0.0)) left = true;
    if (left) {
      node = 2 * node;
    } else {
      q -= l;
      node = 2 * node + 1;
    }
  }
  return node - padded;
}

// Stratified prioritized draws, one workgroup per batch row: lane 0 draws q = total (b + u) / B (row b's stratum), walks the tree, and
// checks the window; a rejected draw is redrawn from the whole tree (q = total u), max_tries draws in all.  priority[b] = the leaf (fp32;
// 0 for a failed row).  The gather is the uniform sampler's.
__global__ __launch_bounds__(kReplayBlock) void ble_replay_sample_prio_kernel(ble_replay_f32 rp, ble_sum_tree_f64 tr, ble_train_batch_f32 bt,
                                                                             float* __restrict__ priority, uint64_t seed,
                                                                             uint32_t* __restrict__ err_flags) {
  __shared__ int64_t s_t, s_env;
  __shared__ int s_m;
  const int64_t b = blockIdx.x;
  if (threadIdx.x == 0) {
    const int64_t count = *rp.count, T = rp.capacity, N = rp.num_envs;
    const int64_t last = count - 1, lo = count > T ? count - T : 0;
    const double total = tr.nodes[1];
    const double seg = total / (double)bt.batch;
    Philox g = replay_stream(seed, b, *rp.counter);
    int64_t t = -1, env = -1;
    int m = 0, term = 0;
    double p = 0.0;
    for (int tries = 0; total > 0.0 && last >= 0 && tries < rp.max_tries; ++tries) {
      const double u = philox_uniform(g);
      const double q = tries == 0 ? seg * (double)b + u * seg : u * total;
      const int64_t leaf = tree_find(tr.nodes, tr.padded, q);
      if (leaf >= tr.leaves) continue;
      const int64_t row = leaf / N, ee = leaf - row * N;
      const int64_t tt = last - ((last % T) - row + T) % T;         // the newest step held in ring row `row`
      if (tt < lo || tt + rp.update_horizon > last) continue;
      if (replay_window(rp, tt, ee, &m, &term)) { t = tt; env = ee; p = tr.nodes[tr.padded + leaf]; break; }
    }
    if (t < 0) { m = 0; term = 0; }
    replay_emit(rp, bt, b, t, env, m, term, err_flags);
    priority[b] = (float)p;
    s_t = t; s_env = env; s_m = m;
  }
  __syncthreads();
  replay_gather(rp, bt, b, s_t, s_env, s_m);
}

// set_priority after an update (quantile_agent.py): leaf = sqrt(L_b + 1e-10) in fp32 (jnp's arithmetic), stored as fp64, in batch order
// so that the later row wins on a duplicate index; rows with index -1 are skipped; a non-finite or negative L_b leaves its leaf and sets
// kFlagReplayPriority (an index outside the ring is skipped too).  The max recorded priority rises to the largest new leaf.  weighted[b] = (w_b / max w) L_b with
// w_b = 1 / sqrt(p_b + 1e-10), the reported loss (the gradient is not weighted); 0 for a failed row, which is left out of the max.
__global__ __launch_bounds__(kTreeBlock) void ble_set_priority_kernel(int64_t T, int64_t N, ble_sum_tree_f64 tr, const int64_t* __restrict__ index,
                                                                      int64_t batch, const float* __restrict__ priority,
                                                                      const float* __restrict__ loss, float* __restrict__ weighted,
                                                                      uint32_t* __restrict__ err_flags) {
  __shared__ float s_max[kTreeBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wmax = 0.0f;
  for (int64_t b = threadIdx.x; b < batch; b += kTreeBlock)
    if (index[2 * b] >= 0) wmax = fmaxf(wmax, div_f32_rn(1.0f, sqrt_f32_rn(__fadd_rn(priority[b], 1e-10f))));
  for (int o = 32; o > 0; o >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, o));      // (a max: any order gives the same bits)
  if (lane == 0) s_max[wave] = wmax;
  __syncthreads();
  wmax = s_max[0];
  for (int w = 1; w < kTreeBlock / 64; ++w) wmax = fmaxf(wmax, s_max[w]);
  for (int64_t b = threadIdx.x; b < batch; b += kTreeBlock) {
    float v = 0.0f;
    if (index[2 * b] >= 0) {
      const float w = div_f32_rn(1.0f, sqrt_f32_rn(__fadd_rn(priority[b], 1e-10f)));
      v = __fmul_rn(div_f32_rn(w, wmax), loss[b]);
    }
    weighted[b] = v;
  }
  if (threadIdx.x == 0) {
    double mx = *tr.max_priority;
    bool bad = false;
    for (int64_t b = 0; b < batch; ++b) {
      const int64_t t = index[2 * b], env = index[2 * b + 1];
      if (t < 0 || env < 0 || env >= N) continue;
      const float l = loss[b];
      if (!(l >= 0.0f) || isinf(l)) { bad = true; continue; }
      const double v = (double)sqrt_f32_rn(__fadd_rn(l, 1e-10f));
      tr.nodes[tr.padded + (t % T) * N + env] = v;
      mx = fmax(mx, v);
    }
    *tr.max_priority = mx;
    if (bad && err_flags != nullptr) *err_flags |= kFlagReplayPriority;
  }
  __syncthreads();
  for (int64_t half = tr.padded >> 1, sh = 1; half >= 1; half >>= 1, ++sh) {   // one level per pass, leaves' parents first
    for (int64_t b = threadIdx.x; b < batch; b += kTreeBlock) {
      const int64_t t = index[2 * b], env = index[2 * b + 1];
      if (t < 0 || env < 0 || env >= N) continue;
      const int64_t node = (tr.padded + (t % T) * N + env) >> sh;
      tr.nodes[node] = tr.nodes[2 * node] + tr.nodes[2 * node + 1];   // (rows that share an ancestor write the same sum)
    }
    __syncthreads();
  }
}

}  // namespace ble
