// Host build of the stride's lane functions next to the expressions they replaced (tests/test_stride_seeds_host.py).  TEST TOOLING, built
// like tests/emul (g++ -include tests/emul/ble_intrinsics.h): the fp64 seeds are float32-precision, like v_rcp_f64 / v_rsq_f64.
//   seeds_rate      sqrt(a) / dH of one stride: atm_rate_over_delta_height_f64 against the two-seed form (sqrt(a) through d_sqrt_rs, 1 / dH
//                   through d_rcp), from the window the transition builds around p; the inputs of both go back for the reference
//   seeds_thermal   thermal_increment_f64 against the same function with the twelfth root's argument formed in fp64
//   seeds_acs_*     the ACS table's node positions and acs_down_poly against the form that computed interval and node from (prm1 - 0.05) x 40
#include "../balloon_learning_environment_amd/csrc/ble_step_core.h"

using namespace ble;

namespace {

// the parent's 1 / (H(p + d) - H(p)): one reciprocal, refined, per path
double parent_inv_delta_height(const AtmWindow& w, int j, double lapse, double kl, double cur_hi, double cur_lo, double p, double rp, double d,
                               double t_p, const StrideK& K) {
  const double x = d * rp;
  const double lg = x * d_fma(x, d_fma(x, K.lg3, -0.5), 1.0);
  const bool iso = lapse == 0.0;
  const double y = kl * lg;
  const double em1 = y * d_fma(y, d_fma(y, K.ex3, 0.5), 1.0);
  double inv = lapse * d_rcp(t_p * em1);
  if (iso) inv = d_rcp(t_p * ((-kAirSpecificGasD / 9.80665) * lg));
  const double q = p + d;
  const bool below = q > cur_hi;
  const bool above = !(q > cur_lo);
  if (below || above) {
    const bool at_pb = (j == 0) ? below : (j < 0);
    const double pb = at_pb ? w.pb : w.pt, r_pb = at_pb ? w.r_pb : w.r_pt, tb = at_pb ? w.tb : w.tt;
    const double lapse_q = pick3(below ? j - 1 : j + 1, w.lapse_m1, w.lapse_0, w.lapse_p1);
    const double dh = atm_height_rel_boundary_f64(q, pb, r_pb, tb, lapse_q) - atm_height_rel_boundary_f64(p, pb, r_pb, tb, lapse);
    inv = d_rcp(dh);
  }
  return inv;
}

// the parent's thermal increment: thermal_increment_f64<false> with the twelfth root's argument in fp64
double parent_thermal_increment(double vol, double yc, double t_int, double t_amb, double p, double q_solar_area, double q_earth_area) {
  const StrideK K = stride_k_literal();
  const double v23 = vol * yc;
  const double t2 = t_int * t_int;
  const double q_emit = (t2 * t2) * d_fma(d_fma(kEmitA, t_int, K.emit_b), t_int, K.emit_c);
  const double rt = d_rcp(t_amb), rt2 = rt * rt, rt3 = rt2 * rt;
  const double pw = p * (t_amb + K.t110);
  const double dt = t_amb - t_int;
  double ra = (d_fma(kRayleighT, t_amb, K.ra_t0) * (pw * pw)) * ((vol * (rt3 * rt3)) * __builtin_fabs(dt));
  ra = d_max(ra, 1e-30);
  const double y4 = d_inv_root4(ra, K.five);
  const double ra14 = (ra * y4) * (y4 * y4);
  const double tw_arg = d_fma(2.69e-8, ra, 1.0);
  const double tw = (double)f_pow((float)tw_arg, 1.0f / 12.0f);
  const double nusselt = d_fma(0.457, ra14, 2.0 + tw);
  const double q_conv = ((nusselt * (t_amb * d_inv_root10(t_amb, K.eleven, K.cond_tenth))) * yc) * dt;
  const double q = (q_solar_area + q_earth_area) + (q_conv - q_emit);
  return (q * v23) * VehicleDefault::thermal_scale;
}

}  // namespace

constexpr int kRateOut = 16;
// out [n][16]: parent, new, rp, t_p, lapse_0, lapse_m1, lapse_p1, pb, pt, tb, tt, r_pb, r_pt, flags, kl, -R_d / g
extern "C" void seeds_rate(int64_t n, const double* alpha, const double* p_in, const double* a_in, const double* dir_in, double* out) {
  const StrideK K = stride_k_literal();
  for (int64_t i = 0; i < n; ++i) {
    const double p = p_in[i], a = a_in[i], d = dir_in[i];
    uint32_t flags = 0;
    const AtmWindow win = atm_window(alpha[i], p, &flags);
    double altitude, t_p;
    atm_at_pressure_f64(win, alpha[i], p, &altitude, &t_p);
    const double lapse = win.lapse_0, kl = (-kAirSpecificGasD / 9.80665) * win.lapse_0;
    const double rp = d_rcp(p);
    double* o = out + kRateOut * i;
    o[0] = parent_inv_delta_height(win, 0, lapse, kl, win.pb, win.pt, p, rp, d, t_p, K) * d_sqrt_rs(a);
    o[1] = atm_rate_over_delta_height_f64(win, 0, lapse, kl, win.pb, win.pt, p, rp, d, t_p, a, K);
    o[2] = rp; o[3] = t_p; o[4] = win.lapse_0; o[5] = win.lapse_m1; o[6] = win.lapse_p1; o[7] = win.pb; o[8] = win.pt;
    o[9] = win.tb; o[10] = win.tt; o[11] = win.r_pb; o[12] = win.r_pt; o[13] = (double)flags; o[14] = kl; o[15] = -kAirSpecificGasD / 9.80665;
  }
}
// the argument of the square root as stride_pressure forms it, before the floor, and the direction
extern "C" void seeds_arg(int64_t n, const double* p, const double* vol, const double* n_air, const double* t_amb, double* arg, double* dir) {
  const StrideK K = stride_k_literal();
  for (int64_t i = 0; i < n; ++i) {
    const double yc = inv_cbrt_volume(vol[i]);
    const double mass = d_fma(kAirMolarMassD, n_air[i], K.dry_mass);
    const double num = d_fma(p[i] * vol[i], K.m_over_r, -mass * t_amb[i]);
    dir[i] = __builtin_copysign(1.0, num);
    arg[i] = VehicleDefault::drag_arg * __builtin_fabs(num) * d_rcp(p[i]) * (yc * yc);
  }
}
// the transition pressures of the window around p
extern "C" void seeds_window(double alpha, double p, double* pb, double* pt) {
  uint32_t flags = 0;
  const AtmWindow win = atm_window(alpha, p, &flags);
  *pb = win.pb; *pt = win.pt;
}
// out [n][3]: parent, new, yc
extern "C" void seeds_thermal(int64_t n, const double* vol, const double* t_int, const double* t_amb, const double* p, const double* q_solar,
                              const double* q_earth, double* out) {
  for (int64_t i = 0; i < n; ++i) {
    const double yc = inv_cbrt_volume(vol[i]);
    out[3 * i] = parent_thermal_increment(vol[i], yc, t_int[i], t_amb[i], p[i], q_solar[i], q_earth[i]);
    out[3 * i + 1] = thermal_increment_f64(vol[i], yc, t_int[i], t_amb[i], p[i], q_solar[i], q_earth[i]);
    out[3 * i + 2] = yc;
  }
}
extern "C" double seeds_thermal_scale() { return VehicleDefault::thermal_scale; }
extern "C" double seeds_acs_node(int i) { return kAcsPoly.c[kAcsPolyRow * i + 6]; }
extern "C" double seeds_acs_node_fma(int i) { return d_fma(0.025, (double)i, 0.05); }
// out [n][4]: power and mass flow of acs_down_poly, and of the form with the node position from the index
extern "C" void seeds_acs(int64_t n, const double* prm1, double* out) {
  const StrideK K = stride_k_literal();
  for (int64_t k = 0; k < n; ++k) {
    acs_down_poly(kAcsPoly.c, prm1[k], &out[4 * k], &out[4 * k + 1]);
    int i = (int)((prm1[k] - 0.05) * K.forty);
    i = i < 0 ? 0 : (i > 11 ? 11 : i);
    const double t = d_max(d_min(prm1[k] - d_fma(0.025, (double)i, 0.05), 0.025), 0.0);
    const double* c = kAcsPoly.c + kAcsPolyRow * i;
    out[4 * k + 3] = d_fma(d_fma(d_fma(c[3], t, c[2]), t, c[1]), t, c[0]);
    out[4 * k + 2] = d_fma(c[5], t, c[4]);
  }
}
