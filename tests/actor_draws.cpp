// Host build of the Philox words of the sampled actor head (csrc/ble_actor.h ble_ac_head_kernel), for tests/test_gpu_ppo.py and
// tests/test_ppo_host.py: TEST TOOLING, compiled with g++ and tests/emul/ble_intrinsics.h as tests/replay_draws.cpp is.  ble_actor.h
// includes the MFMA headers and does not compile on the host, so the stream of environment e at `step` is restated here:
// philox_init(seed ^ "ACTOR", e, the step's low word), the step's high word xor-ed into key1 -- ble_explore_kernel's keying.
#include "../balloon_learning_environment_amd/csrc/ble_step_core.h"
#include "../balloon_learning_environment_amd/csrc/ble_reset.h"

using namespace ble;

static void first_words(uint64_t seed, int64_t env_offset, int64_t n, uint64_t step, uint32_t* w) {
  for (int64_t i = 0; i < n; ++i) {
    Philox g = philox_init(seed, (uint64_t)(env_offset + i), (uint32_t)step);
    g.key1 ^= (uint32_t)(step >> 32);
    w[i] = philox_u32(g);
  }
}

// w[i] = the first philox_u32 of the actor stream (seed, env_offset + i, step), i < n.
extern "C" void actor_draws(uint64_t seed, int64_t env_offset, int64_t n, uint64_t step, uint32_t* w) {
  first_words(seed ^ 0x4143544F52ull, env_offset, n, step, w);
}

// The same word of the epsilon-greedy stream (ble_explore_kernel) of the same (seed, environment, step).
extern "C" void explore_stream_draws(uint64_t seed, int64_t env_offset, int64_t n, uint64_t step, uint32_t* w) {
  first_words(seed, env_offset, n, step, w);
}
