// Host build of the belief's lane function (csrc/ble_gp_belief.h: gp_belief_mean and its table) for tests/test_belief_host.py.
// TEST TOOLING: never loaded by the package.  libm stands in for the hardware seeds (tests/emul/ble_intrinsics.h), so this shows the
// algorithm's error -- the Newton step on the reciprocal square root, the table and the polynomial of the exponential -- not the
// device's last ulp.
#include "../../balloon_learning_environment_amd/csrc/ble_gp_belief.h"

using namespace ble;

// A window of n_obs observations -- loc [n_obs][4] = x m, y m, pressure Pa, t s and alpha [n_obs][2] = K^-1 y -- as a slab, zero beyond
// the window: the layout and the scaling are the header's, the test knows neither.
extern "C" void emul_belief_pack(int n_obs, const double* loc, const double* alpha, double* slab) {
  for (int q = 0; q < kBeliefDoubles; ++q) slab[q] = 0.0;
  for (int i = 0; i < n_obs && i < kBeliefRows; ++i) {
    slab[4 * i] = loc[4 * i] * kBeliefScaleXY; slab[4 * i + 1] = loc[4 * i + 1] * kBeliefScaleXY;
    slab[4 * i + 2] = loc[4 * i + 2] * kBeliefScaleP; slab[4 * i + 3] = loc[4 * i + 3] * kBeliefScaleT;
    slab[kBeliefAlphaAt + 2 * i] = alpha[2 * i]; slab[kBeliefAlphaAt + 2 * i + 1] = alpha[2 * i + 1];
  }
}

// gp_belief_mean at q points; n_trip < 0: the trip count of n_obs itself (gp_belief_trip), else the given one
extern "C" void emul_belief_mean(const double* slab, int n_obs, int n_trip, long long q, const float* x, const float* y, const float* p,
                                 const int32_t* t, float* uv) {
  alignas(16) double s[kBeliefDoubles];
  for (int k = 0; k < kBeliefDoubles; ++k) s[k] = slab[k];
  double tab[64];
  for (int k = 0; k < 64; ++k) tab[k] = gp_belief_table_entry(k);
  const int trip = n_trip < 0 ? gp_belief_trip(n_obs) : n_trip;
  for (long long j = 0; j < q; ++j) gp_belief_mean(s, n_obs, trip, x[j], y[j], p[j], t[j], tab, &uv[2 * j], &uv[2 * j + 1]);
}

extern "C" int emul_belief_doubles() { return kBeliefDoubles; }
