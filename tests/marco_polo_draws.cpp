// Host build of the Philox draws of ble_marco_polo_u8 (csrc/ble_explore.h), for tests/test_gpu_marco_polo.py: TEST TOOLING, compiled with
// g++ and tests/emul/ble_intrinsics.h as tests/emul/ble_emul.cpp is.  Stream (seed, env, step): block 0 holds the begin uniforms
// (target, then episode), block 1 on the normal.
#include "../balloon_learning_environment_amd/csrc/ble_step_core.h"
#include "../balloon_learning_environment_amd/csrc/ble_reset.h"

using namespace ble;

extern "C" void marco_polo_draws(uint64_t seed, int64_t n, uint64_t step, double* u_target, double* u_episode, double* normal) {
  for (int64_t i = 0; i < n; ++i) {
    Philox g = philox_init(seed, (uint64_t)i, (uint32_t)step);
    g.key1 ^= (uint32_t)(step >> 32);
    u_target[i] = philox_uniform(g);
    u_episode[i] = philox_uniform(g);
    g.c0 = 1; g.have = 0;
    normal[i] = philox_normal(g);
  }
}
