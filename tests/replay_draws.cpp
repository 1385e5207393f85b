// Host build of the Philox uniforms of the replay samplers (csrc/ble_train.h replay_stream, csrc/ble_replay.h), for
// tests/test_gpu_prio_replay.py and tests/test_prio_replay_host.py: TEST TOOLING, compiled with g++ and tests/emul/ble_intrinsics.h as
// tests/marco_polo_draws.cpp is.  ble_train.h itself holds MFMA builtins and does not compile on the host, so the stream of batch row b
// is restated here: philox_init(seed, b, the counter's low word), the counter's high word in c3.
#include "../balloon_learning_environment_amd/csrc/ble_step_core.h"
#include "../balloon_learning_environment_amd/csrc/ble_reset.h"

using namespace ble;

// u[b * tries + k] = the k-th philox_uniform of the stream (seed, b, counter), b < batch, k < tries.
extern "C" void replay_draws(uint64_t seed, int64_t batch, uint64_t counter, int64_t tries, double* u) {
  for (int64_t b = 0; b < batch; ++b) {
    Philox g = philox_init(seed, (uint64_t)b, (uint32_t)counter);
    g.c3 = (uint32_t)(counter >> 32);
    for (int64_t k = 0; k < tries; ++k) u[b * tries + k] = philox_uniform(g);
  }
}
