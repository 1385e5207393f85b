// ble_explore.h -- exploration on the device: epsilon-greedy over the agent's actions and the reference's Marco Polo
// exploration.  Both are one lane per environment and draw from the Philox stream of (seed, environment, step).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ble_reset.h"

namespace ble {

__global__ __launch_bounds__(256) void ble_explore_kernel(uint8_t* __restrict__ action, int64_t n, float epsilon, uint64_t seed,
                                                          uint64_t step) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Philox g = philox_init(seed, (uint64_t)i, (uint32_t)step);
  g.key1 ^= (uint32_t)(step >> 32);
  const uint32_t u = philox_u32(g), r = philox_u32(g);
  const float uf = (float)(u >> 8) * (1.0f / 16777216.0f);             // [0, 1), 24 bits
  if (uf < epsilon) action[i] = (uint8_t)(((uint64_t)r * 3u) >> 32);
}

// Marco Polo exploration (the reference's MarcoPoloExploration over a RandomWalkAgent, one step = 3 min), one lane per environment.
// The Philox stream of (seed, env, step): block 0 holds the begin-of-episode uniforms (target, then episode), block 1 on the normal.
constexpr int kMarcoPoloRlSteps = 80, kMarcoPoloExploreSteps = 40;     // 4 h and 2 h
__host__ __device__ inline float marco_polo_u24(double u) { return (float)(uint32_t)(u * 16777216.0) * (1.0f / 16777216.0f); }

__global__ __launch_bounds__(256) void ble_marco_polo_kernel(ble_marco_polo_f32 mp, uint8_t* __restrict__ action) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= mp.n) return;
  const uint64_t step = *mp.step;
  Philox g = philox_init(mp.seed, (uint64_t)i, (uint32_t)step);
  g.key1 ^= (uint32_t)(step >> 32);
  if (mp.begin[i]) {
    // RandomWalkAgent.begin_episode: clock 0, target U[6500, 11400) (jax.random.uniform in float32); then phase clock 0, the
    // episode is exploratory when u <= p, RL phase; the agent's action is kept.
    const float ut = marco_polo_u24(philox_uniform(g)), ue = marco_polo_u24(philox_uniform(g));
    mp.walk_clock[i] = 0;
    mp.target[i] = (double)fmaxf(6500.0f, __fadd_rn(__fmul_rn(ut, 4900.0f), 6500.0f));
    mp.phase_clock[i] = 0;
    mp.exploratory_episode[i] = (double)ue <= mp.exploratory_episode_probability ? 1 : 0;
    mp.exploratory_phase[i] = 0;
    return;
  }
  int clock = mp.phase_clock[i] + 1;
  uint8_t phase = mp.exploratory_phase[i];
  if (mp.exploratory_episode[i] && clock >= (phase ? kMarcoPoloExploreSteps : kMarcoPoloRlSteps)) { phase ^= 1; clock = 0; }
  mp.phase_clock[i] = clock;
  mp.exploratory_phase[i] = phase;
  if (!phase) return;
  // RandomWalkAgent.step: clock += 180 s, target += seconds * 0.1666 * z (float64), then the hysteresis rule on p = 5000 + 9000 f0
  // (float32, NamedPerciatelliFeatures.balloon_pressure)
  const int walk = mp.walk_clock[i] + 1;
  mp.walk_clock[i] = walk;
  g.c0 = 1;
  const double z = philox_normal(g);
  const double target = mp.target[i] + ((double)walk * 180.0) * 0.1666 * z;
  mp.target[i] = target;
  const float p = __fadd_rn(5000.0f, __fmul_rn(mp.obs[i * mp.obs_stride], 9000.0f));
  action[i] = (double)__fsub_rn(p, 100.0f) > target ? 2 : ((double)__fadd_rn(p, 100.0f) < target ? 0 : 1);
}

}  // namespace ble
