// Host build of the evolution strategy's lane functions (csrc/ble_population.h) for tests/test_es_host.py.  TEST TOOLING: never loaded
// by the package.  The noise address and the Philox words are integer arithmetic (the device's bits); the normal deviate goes through
// the host's libm where the device has its own fp64 primitives; everything after eps is IEEE arithmetic without contraction.
#include "../../balloon_learning_environment_amd/csrc/ble_population.h"

using namespace ble;

// the generator of eps_i[q] before its block: key0, key1, c0 .. c3; and the block's four words
extern "C" void emul_es_address(uint64_t seed, uint64_t pair, uint64_t generation, uint64_t q, uint32_t* key_counter, uint32_t* words) {
  Philox g = es_noise_stream(seed, pair, generation, q);
  key_counter[0] = g.key0; key_counter[1] = g.key1;
  key_counter[2] = g.c0; key_counter[3] = g.c1; key_counter[4] = g.c2; key_counter[5] = g.c3;
  philox_refill(g);
  for (int k = 0; k < 4; ++k) words[k] = g.out[k];
}

// eps [streams][d]: stream i, logical parameter q0 + j
extern "C" void emul_es_noise(uint64_t seed, uint64_t generation, int streams, int64_t q0, int64_t d, float* eps) {
  for (int i = 0; i < streams; ++i)
    for (int64_t j = 0; j < d; ++j) eps[i * d + j] = es_noise(seed, (uint64_t)i, generation, (uint64_t)(q0 + j));
}

extern "C" void emul_es_perturb(const float* theta, float sigma, const float* eps, int64_t d, float* plus, float* minus) {
  for (int64_t j = 0; j < d; ++j) es_perturb(theta[j], sigma, eps[j], plus + j, minus + j);
}

// grad [d] from w [streams] and eps [streams][d]
extern "C" void emul_es_gradient(const float* w, const float* eps, int streams, int64_t d, float sigma, float weight_decay,
                                 const float* theta, float* grad) {
  for (int64_t j = 0; j < d; ++j) {
    double acc = 0.0;
    for (int i = 0; i < streams; ++i) acc = es_grad_term(acc, w[i], eps[i * d + j]);
    grad[j] = es_grad_finish(acc, streams, sigma, weight_decay, theta[j]);
  }
}
