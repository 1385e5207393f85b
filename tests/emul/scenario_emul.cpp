// Host build of the scenario winds' lane functions (csrc/ble_scenarios.h: the scenario stream, the risk ranks and score, the prior
// field and the correction) for tests/test_scenario_host.py.  TEST TOOLING: never loaded by the package.  The stream and the ranks are
// integer arithmetic and the score is one fp64 sum in a fixed order, so the host build gives the device's bits there; the prior and the
// correction go through libm's stand-ins (tests/emul/ble_intrinsics.h) and show the algorithm, not the device's last ulp.
#include "../../balloon_learning_environment_amd/csrc/ble_scenarios.h"

using namespace ble;

// the 50 harmonic words of scenario m, drawn in order from one generator (what the lane kernels do)
extern "C" void emul_scenario_draws(uint64_t seed, uint64_t key, uint32_t episode, int m, uint32_t* out50) {
  scenario_draws_fetch(seed, key, episode, m, out50, 1);
}
// harmonic k alone, from its own place in the stream (what the fit's 10 M threads do): (seed, ox, oy, op, ot) as five words
extern "C" void emul_scenario_harmonic(uint64_t seed, uint64_t key, uint32_t episode, int m, int k, uint32_t* out5) {
  const HarmonicDraw d = scenario_harmonic(seed, key, episode, m, k);
  out5[0] = d.hseed; out5[1] = float_bits_u32(d.ox); out5[2] = float_bits_u32(d.oy); out5[3] = float_bits_u32(d.op); out5[4] = float_bits_u32(d.ot);
}
// the 50 words of the environment's TRUE noise (noise_draws_fetch without a cache)
extern "C" void emul_truth_draws(uint64_t seed, uint64_t key, uint32_t episode, uint32_t* out50) {
  noise_draws_fetch(seed, 0, key, episode, nullptr, 1, out50, 1);
}

extern "C" uint64_t emul_risk_ranks(const float* ret, int num) { return risk_ranks(ret, 1, num); }
extern "C" float emul_risk_score(const float* ret, int num, int tail) { return plan_risk_score(ret, 1, num, tail); }

// f_m at q points from 50 given words: both components by wind_noise_from_rows (uv) and one by one (uv_by_component)
extern "C" void emul_scenario_prior(const uint32_t* words50, long long q, const float* x, const float* y, const float* p, const int32_t* t,
                                    float* uv, float* uv_by_component) {
  alignas(16) float lut[kGradLutFloats];
  grad_lut_fill(lut, 0, 1);
  for (long long j = 0; j < q; ++j) {
    wind_noise_from_rows(x[j], y[j], p[j], t[j], words50, 1, lut, &uv[2 * j], &uv[2 * j + 1]);
    for (int c = 0; c < 2; ++c) uv_by_component[2 * j + c] = wind_noise_component_from_rows(c, x[j], y[j], p[j], t[j], words50, 1, lut);
  }
}

// gp_scenario_correction on scenario m of a scenario slab [480 + 240 num] at q points
extern "C" void emul_scenario_correction(const double* slab, int num, int m, int n_obs, long long q, const float* x, const float* y,
                                         const float* p, const int32_t* t, float* uv) {
  alignas(16) double s[kBeliefAlphaAt + kScenarioAlphaDoubles * kScenarioMax];
  for (int k = 0; k < scenario_slab_doubles(num); ++k) s[k] = slab[k];
  double tab[64];
  for (int k = 0; k < 64; ++k) tab[k] = gp_belief_table_entry(k);
  for (long long j = 0; j < q; ++j)
    gp_scenario_correction(s, s + kBeliefAlphaAt + kScenarioAlphaDoubles * m, n_obs, gp_belief_trip(n_obs), x[j], y[j], p[j], t[j], tab,
                           &uv[2 * j], &uv[2 * j + 1]);
}

extern "C" int emul_scenario_slab_doubles(int num) { return scenario_slab_doubles(num); }
