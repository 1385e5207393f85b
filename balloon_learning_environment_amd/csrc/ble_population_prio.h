// ble_population_prio.h -- prioritized replay and Marco Polo exploration for a population of P replay learners: P sum
// trees over ONE ring of N = P R columns (columns [p R, (p + 1) R) member p's), a grouped stratified sampler, a grouped
// set_priority and a grouped Marco Polo.
//
// The contract is §3t's: member p's part of every result holds the bytes the plain kernel of ble_replay.h / ble_explore.h gives member
// p's own objects -- a ring of its R columns with its own tree and max priority, an explorer of R lanes with its own probability and
// seed.  Member p's tree is a solo tree image at nodes + p member_stride: an fp64 heap over T R leaves padded to a power of two, leaf
// (t % T) R + r the window of column p R + r.  Each kernel below is its plain sibling with the member coordinate added, in an
// instantiation of its own; the statements that round (the stratum's query, the weights, the leaves, every parent = left + right) are
// written as the plain kernels write them.  A workgroup writes member p's tree only, so every tree stays a pure function of its leaves
// with no floating-point atomics; the one word the workgroups share, err_flags, is set with an integer atomic OR.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ble_explore.h"
#include "ble_replay.h"

namespace ble {

// ble_tree_add_kernel, workgroup p on member p's tree: zero row s % T, give row (s - n) % T member p's max recorded priority (valid
// windows of its columns) or 0, then the ancestors of both leaf ranges inside that tree.
__global__ __launch_bounds__(kTreeBlock) void ble_tree_add_grouped_kernel(ble_replay_f32 rp, ble_sum_tree_grouped_f64 tr,
                                                                          int64_t envs_per_member) {
  const int64_t s = *rp.count - 1;
  if (s < 0) return;
  const int64_t p = blockIdx.x;
  const int64_t R = envs_per_member, T = rp.capacity, P = tr.padded;
  const int64_t col0 = p * R;
  const int n = rp.update_horizon;
  double* __restrict__ nodes = tr.nodes + p * tr.member_stride;
  const bool complete = s >= n;
  const int64_t z0 = P + (s % T) * R, c0 = complete ? P + ((s - n) % T) * R : z0;
  const double mx = tr.max_priority[p];
  for (int64_t e = threadIdx.x; e < R; e += kTreeBlock) {
    nodes[z0 + e] = 0.0;
    int m, term;
    if (complete) nodes[c0 + e] = replay_window(rp, s - n, col0 + e, &m, &term) ? mx : 0.0;
  }
  __syncthreads();
  int64_t zl = z0, zh = z0 + R - 1, cl = c0, ch = c0 + R - 1;
  while (zl > 1) {
    zl >>= 1; zh >>= 1; cl >>= 1; ch >>= 1;
    tree_sum_range(nodes, zl, zh, 1, 0);
    tree_sum_range(nodes, cl, ch, zl, zh);          // (the two ranges may meet near the root: each node is written once)
    __syncthreads();
  }
}

// ble_replay_sample_prio_kernel, one workgroup per batch row of P B: row p B + b draws from replay_stream(seed[p], b, *counter), walks
// member p's tree and tests, emits and gathers at column p R + ee, as the grouped uniform sampler does.  The walk's loads depend on one
// another level by level (log2(padded) steps of one aligned 16-byte pair): P B workgroups walk at once, and the trees are read-only
// here, so the latency overlaps across rows as in the plain kernel.
__global__ __launch_bounds__(kReplayBlock) void ble_replay_sample_prio_grouped_kernel(ble_replay_f32 rp, ble_sum_tree_grouped_f64 tr,
                                                                                     ble_train_batch_f32 bt, float* __restrict__ priority,
                                                                                     const unsigned long long* __restrict__ seed_of,
                                                                                     int64_t rows_per_member, int64_t envs_per_member,
                                                                                     uint32_t* __restrict__ err_flags) {
  __shared__ int64_t s_t, s_env;
  __shared__ int s_m;
  const int64_t row = blockIdx.x;
  if (threadIdx.x == 0) {
    const int64_t member = row / rows_per_member, b = row - member * rows_per_member;
    const int64_t count = *rp.count, T = rp.capacity, R = envs_per_member;
    const int64_t last = count - 1, lo = count > T ? count - T : 0;
    const double* __restrict__ nodes = tr.nodes + member * tr.member_stride;
    const double total = nodes[1];
    const double seg = total / (double)rows_per_member;
    Philox g = replay_stream((uint64_t)seed_of[member], b, *rp.counter);
    int64_t t = -1, env = -1;
    int m = 0, term = 0;
    double p = 0.0;
    for (int tries = 0; total > 0.0 && last >= 0 && tries < rp.max_tries; ++tries) {
      const double u = philox_uniform(g);
      const double q = tries == 0 ? seg * (double)b + u * seg : u * total;
      const int64_t leaf = tree_find(nodes, tr.padded, q);
      if (leaf >= tr.leaves) continue;
      const int64_t ring_row = leaf / R, ee = member * R + (leaf - ring_row * R);
      const int64_t tt = last - ((last % T) - ring_row + T) % T;    // the newest step held in ring row `ring_row`
      if (tt < lo || tt + rp.update_horizon > last) continue;
      if (replay_window(rp, tt, ee, &m, &term)) { t = tt; env = ee; p = nodes[tr.padded + leaf]; break; }
    }
    if (t < 0) { m = 0; term = 0; }
    replay_emit(rp, bt, row, t, env, m, term, err_flags);
    priority[row] = (float)p;
    s_t = t; s_env = env; s_m = m;
  }
  __syncthreads();
  replay_gather(rp, bt, row, s_t, s_env, s_m);
}

// ble_set_priority_kernel, workgroup p over rows [p B, (p + 1) B) and member p's tree: the largest weight is over member p's valid
// rows, lane 0 writes the leaves in batch order (the later row wins on a duplicate), rows whose index is -1 or whose column lies
// outside [p R, (p + 1) R) are skipped, max_priority[p] rises, then the ancestors one level per pass.  The serial leaf pass is B rows
// long per member, not P B: the members' passes run side by side.
__global__ __launch_bounds__(kTreeBlock) void ble_set_priority_grouped_kernel(int64_t T, int64_t R, ble_sum_tree_grouped_f64 tr,
                                                                              const int64_t* __restrict__ index_all, int64_t batch,
                                                                              const float* __restrict__ priority_all,
                                                                              const float* __restrict__ loss_all,
                                                                              float* __restrict__ weighted_all,
                                                                              uint32_t* __restrict__ err_flags) {
  __shared__ float s_max[kTreeBlock / 64];
  const int64_t member = blockIdx.x, col0 = member * R;
  const int64_t* __restrict__ index = index_all + 2 * member * batch;
  const float* __restrict__ priority = priority_all + member * batch;
  const float* __restrict__ loss = loss_all + member * batch;
  float* __restrict__ weighted = weighted_all + member * batch;
  double* __restrict__ nodes = tr.nodes + member * tr.member_stride;
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
    double mx = tr.max_priority[member];
    bool bad = false;
    for (int64_t b = 0; b < batch; ++b) {
      const int64_t t = index[2 * b], env = index[2 * b + 1] - col0;
      if (t < 0 || env < 0 || env >= R) continue;
      const float l = loss[b];
      if (!(l >= 0.0f) || isinf(l)) { bad = true; continue; }
      const double v = (double)sqrt_f32_rn(__fadd_rn(l, 1e-10f));
      nodes[tr.padded + (t % T) * R + env] = v;
      mx = fmax(mx, v);
    }
    tr.max_priority[member] = mx;
    if (bad && err_flags != nullptr) atomicOr(err_flags, kFlagReplayPriority);   // (P workgroups, one word: no other's bit is lost)
  }
  __syncthreads();
  for (int64_t half = tr.padded >> 1, sh = 1; half >= 1; half >>= 1, ++sh) {   // one level per pass, leaves' parents first
    for (int64_t b = threadIdx.x; b < batch; b += kTreeBlock) {
      const int64_t t = index[2 * b], env = index[2 * b + 1] - col0;
      if (t < 0 || env < 0 || env >= R) continue;
      const int64_t node = (tr.padded + (t % T) * R + env) >> sh;
      nodes[node] = nodes[2 * node] + nodes[2 * node + 1];           // (rows that share an ancestor write the same sum)
    }
    __syncthreads();
  }
}

// ble_marco_polo_kernel for P members of R lanes: lane p R + r draws from the stream of (seed[p], r, step) and tests its episode
// against probability[p] -- member p's own explorer on its R rows.
__global__ __launch_bounds__(256) void ble_marco_polo_grouped_kernel(ble_marco_polo_grouped_f32 mp, int64_t rows_per_member,
                                                                     uint8_t* __restrict__ action) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= mp.n) return;
  const int64_t p = i / rows_per_member, r = i - p * rows_per_member;
  const uint64_t step = *mp.step;
  Philox g = philox_init((uint64_t)mp.seed[p], (uint64_t)r, (uint32_t)step);
  g.key1 ^= (uint32_t)(step >> 32);
  if (mp.begin[i]) {
    const float ut = marco_polo_u24(philox_uniform(g)), ue = marco_polo_u24(philox_uniform(g));
    mp.walk_clock[i] = 0;
    mp.target[i] = (double)fmaxf(6500.0f, __fadd_rn(__fmul_rn(ut, 4900.0f), 6500.0f));
    mp.phase_clock[i] = 0;
    mp.exploratory_episode[i] = (double)ue <= mp.probability[p] ? 1 : 0;
    mp.exploratory_phase[i] = 0;
    return;
  }
  int clock = mp.phase_clock[i] + 1;
  uint8_t phase = mp.exploratory_phase[i];
  if (mp.exploratory_episode[i] && clock >= (phase ? kMarcoPoloExploreSteps : kMarcoPoloRlSteps)) { phase ^= 1; clock = 0; }
  mp.phase_clock[i] = clock;
  mp.exploratory_phase[i] = phase;
  if (!phase) return;
  const int walk = mp.walk_clock[i] + 1;
  mp.walk_clock[i] = walk;
  g.c0 = 1;
  const double z = philox_normal(g);
  const double target = mp.target[i] + ((double)walk * 180.0) * 0.1666 * z;
  mp.target[i] = target;
  const float pr = __fadd_rn(5000.0f, __fmul_rn(mp.obs[i * mp.obs_stride], 9000.0f));
  action[i] = (double)__fsub_rn(pr, 100.0f) > target ? 2 : ((double)__fadd_rn(pr, 100.0f) < target ? 0 : 1);
}

}  // namespace ble
