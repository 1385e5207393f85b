// Host build of the step's solar nodes next to the form they replaced (tests/test_solar_nodes_host.py).  TEST TOOLING, built like
// tests/stride_seeds_host.cpp (g++ -O2 -ffp-contract=off -include tests/emul/ble_intrinsics.h): the fp64 seeds are float32-precision, like
// v_rcp_f64 / v_rsq_f64.
//   solar_oms           sun_one_minus_sin_f64 (no reciprocal root) against its former body, kept here as sun_one_minus_sin_f64_seeded
//   solar_time_nodes    solar_nodes_time's declination pair and rate against d_sqrt_fast(1 - sd0^2)
#include "../balloon_learning_environment_amd/csrc/ble_step_core.h"

using namespace ble;

namespace {

// a b + c as the host build rounds it (two roundings) or as the device's contraction does (one)
template <bool kFma> double mad(double a, double b, double c) { return kFma ? d_fma(a, b, c) : a * b + c; }

// The former body of sun_one_minus_sin_f64: BalloonState.latlng (spherical_geometry.py:44-76) folded into the zenith formula
// (solar.py:136-139) step by step --
//   heading = atan2(x, y) -> (cos_h, sin_h) = (y, x) / d, angle a = d / R_earth;
//   sin_lat = cos_a sin_lat0 + sin_a cos_lat0 cos_h,  cos_lat = sqrt(1 - sin_lat^2);
//   d_lng = atan2(yy, xx) with yy = sin_a cos_lat0 sin_h, xx = cos_a - sin_lat0 sin_lat -> cos(B + d_lng) by rotating (cos B, sin B)
//       through (xx, yy) / |(xx, yy)|;
//   sin(el) = sin_lat sin_decl - cos_lat cos_decl cos(B + d_lng)   (the hour angle is B + d_lng -+ 180 deg)
// -- with three reciprocal square roots (1 / d, cos_lat, 1 / |(xx, yy)|) and the d == 0 selects.  kFma: the sums of products contracted
// the way the device build contracted them.
template <bool kFma>
double sun_one_minus_sin_f64_seeded(double sin_lat0, double cos_lat0, double x, double y, double sin_b, double cos_b, double sin_decl,
                                    double cos_decl) {
  const double d2 = mad<kFma>(x, x, y * y);
  const bool moved = d2 > 0.0;
  const double inv_d = moved ? d_rsqrt(moved ? d2 : 1.0) : 0.0;
  const double cos_h = moved ? y * inv_d : 1.0;
  const double sin_h = x * inv_d;
  const double a = (d2 * inv_d) * (1.0 / 6371000.0);
  const double a2 = a * a;
  double sin_a = d_fma(a2, d_fma(a2, d_fma(a2, d_fma(a2, d_fma(a2, d_fma(a2, 1.0 / 6227020800.0, -1.0 / 39916800.0),
                                                         1.0 / 362880.0), -1.0 / 5040.0), 1.0 / 120.0), -1.0 / 6.0), 1.0) * a;
  double cos_a = d_fma(a2, d_fma(a2, d_fma(a2, d_fma(a2, d_fma(a2, d_fma(a2, 1.0 / 479001600.0, -1.0 / 3628800.0),
                                                         1.0 / 40320.0), -1.0 / 720.0), 1.0 / 24.0), -0.5), 1.0);
  const double sin_lat = mad<kFma>(cos_a, sin_lat0, sin_a * cos_lat0 * cos_h);
  const double cos_lat = d_sqrt_fast(d_fma(-sin_lat, sin_lat, 1.0));
  const double yy = sin_a * cos_lat0 * sin_h;
  const double xx = mad<kFma>(-sin_lat0, sin_lat, cos_a);
  const double cos_bl = mad<kFma>(cos_b, xx, -(sin_b * yy)) * d_rsqrt(mad<kFma>(xx, xx, yy * yy));
  const double s = mad<kFma>(sin_lat, sin_decl, -(cos_lat * cos_decl * cos_bl));
  return 1.0 - s;
}

}  // namespace

// in [n][8]: sin_lat0, cos_lat0, x, y, sin_b, cos_b, sin_decl, cos_decl;  out [n][3]: new, seeded, seeded with the device's contractions
extern "C" void solar_oms(int64_t n, const double* in, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    const double* a = in + 8 * i;
    out[3 * i] = sun_one_minus_sin_f64(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
    out[3 * i + 1] = sun_one_minus_sin_f64_seeded<false>(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
    out[3 * i + 2] = sun_one_minus_sin_f64_seeded<true>(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
  }
}
// (sin, cos) of an angle the way hoist_constants and the helper wave form the site's pair
extern "C" void solar_sincos(int64_t n, const double* rad, double* s, double* c) {
  for (int64_t i = 0; i < n; ++i) sincos_f64(rad[i], &s[i], &c[i]);
}
// out [n][4]: cd0, hcd, hsd of solar_nodes_time, and d_sqrt_fast(1 - sd0^2)
extern "C" void solar_time_nodes(int64_t n, const float* sin_decl, const float* sin_decl_rate, float step_s, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    Ephemeris e = {};
    e.sin_decl = sin_decl[i]; e.sin_decl_rate = sin_decl_rate[i];
    const SolarNodes nd = solar_nodes_time(e, 1656633600, 0.0f, step_s);
    const double sd0 = (double)sin_decl[i];
    out[4 * i] = nd.cd0; out[4 * i + 1] = nd.hcd; out[4 * i + 2] = nd.hsd; out[4 * i + 3] = d_sqrt_fast(d_fma(-sd0, sd0, 1.0));
  }
}
