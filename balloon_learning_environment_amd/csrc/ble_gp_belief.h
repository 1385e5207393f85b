// ble_gp_belief.h -- the wind an agent believes in: a WindGP fitted ONCE per environment and kept on the device (the belief), its
// posterior mean as a lane function, and the look-ahead flown in forecast + that mean.  DESIGN.md 3j.
//
//   ble_gp_fit_kernel           one workgroup (4 waves) per environment: phases 0-2 of ble_gp_query_kernel -- the window at the anchor
//                               time, K = L L^T, W = L^-1, alpha = K^-1 y -- and then, instead of query points, the compacted window
//                               and alpha stored to the environment's slab in HBM.  The phases are ble_gp_factor.h's functions, the
//                               ones the query kernel calls: one window rule and one factor for both.
//   gp_belief_mean              the lane function: sum_i k(loc_i, (x, y, p, t)) alpha_i for both components, fp64, i ascending, every
//                               product an explicit d_fma, rounded to fp32 once.  No factor, no barrier: 120 kernel evaluations.
//                               One body, gp_scenario_correction: (loc, alpha) as two pointers, to which the scenario winds pass
//                               alpha^m; gp_belief_mean calls it with the alpha of its slab.
//   ble_gp_belief_wind_kernel   one lane per environment at caller-chosen points (the shape of ble_wind_noise_kernel): what ble_step_f32
//                               takes as noise_uv.
//   WindBelief                  the look-ahead's wind policy (ble_lookahead.h): gp_belief_mean in the slot of the noise term.
//   ble_rollout_belief_kernel   ble_rollout_kernel's lanes (rollout_lane) in that wind: the lane map and nothing else.
//
// The slab of an environment (kBeliefDoubles = BLE_GP_BELIEF_DOUBLES doubles, 16-byte aligned):
//   [0, 480)     loc[120][4]: x, y, p, t of the window's observations, chronological, in units of ln2 / 32 length scales
//                (ble_observe.h: twice the square root of the squared distance IS the exponent in units of ln2 / 64)
//   [480, 720)   alpha[120][2]: (K^-1 y)_i of the u and of the v error, interleaved
// Everything beyond the window is zero: a kernel evaluation against a zero row is finite and its alpha is +0.0, so the sum does not
// change -- the trip count of the loop may be any multiple of 4 that covers n_obs, and a wave whose lanes belong to environments with
// different windows runs ONE loop to the largest.
//
// The lane function and its constants build on the host as well (tests/emul/belief_emul.cpp): nothing above the kernels below uses
// more than ble_intrinsics.h and ble_physics.h.
#pragma once
#include "ble_physics.h"

namespace ble {

constexpr int kBeliefRows = 120;                              // kGpMax
constexpr int kBeliefAlphaAt = 4 * kBeliefRows;               // 480
constexpr int kBeliefDoubles = kBeliefAlphaAt + 2 * kBeliefRows;      // 720: BLE_GP_BELIEF_DOUBLES
// 32 / ln 2 over the WindGP's length scales (ble_observe.h's kGpKappa; the same expressions as ble_gp_query_kernel's)
constexpr double kBeliefKappa = 46.16624130844683;
constexpr double kBeliefScaleXY = kBeliefKappa / 357000.0, kBeliefScaleP = kBeliefKappa / 326.0, kBeliefScaleT = kBeliefKappa / 34560.0;

// entry k of gp_exp_neg_scaled's table, s^2 2^(k / 64): 64 doubles the kernels keep in LDS
BLE_FN double gp_belief_table_entry(int k) { return (3.6 * 3.6) * d_exp_fast((double)k * (6.93147180559945286227e-01 / 64.0)); }

#if defined(__HIPCC__)
BLE_FN double belief_fract(double x) { return __builtin_amdgcn_fract(x); }      // v_fract_f64
#else
BLE_FN double belief_fract(double x) { return x - floor(x); }
#endif

// s^2 exp(-|d|) from the scaled coordinate differences: two_sqrt and gp_exp_neg_scaled of ble_observe.h, every product a d_fma
BLE_FN double gp_belief_kernel(double dx, double dy, double dp, double dt, const double* tab) {
  const double X = d_fma(dx, dx, d_fma(dy, dy, d_fma(dp, dp, d_fma(dt, dt, 1e-300))));
  const double y = d_rsq_seed(X);
  const double g = X * y;
  const double rs = g * d_fma(-g, y, 3.0);                    // 2 sqrt(X): one Newton step on the product
  const double f = belief_fract(rs);
  const int nn = (int)(-rs);                                  // -floor(rs)
  const double t = tab[nn & 63];
  const double q = d_fma(f, d_fma(f, d_fma(f, d_fma(f, 5.701900737872891e-10, -2.117286661914034e-07), 5.864904858491492e-05),
                               -0.010830424696128488), 0.9999999999999976);
  return d_ldexp(t * q, nn >> 6);
}

// The posterior mean of the forecast ERROR (u, v) [m/s] at (x, y, p, t_elapsed_s): the forecast is added where the wind is used, as the
// noise term is.  loc: the window (the front of an environment's slab: 16-byte aligned); alpha: K^-1 y of that window, u and v
// interleaved (16-byte aligned); n_obs: the window, 0 -> exactly +0.0f, < 0 -> NaN (a window the ring could not tell:
// ble_gp_fit_kernel); n_trip: a multiple of 4, >= n_obs, <= 120 -- any such value gives the same bits (the note at the top); tab:
// gp_belief_table_entry's 64 entries.  The window and alpha are frozen at the fit's anchor: only the query's time moves.
BLE_FN void gp_scenario_correction(const double* __restrict__ loc_, const double* __restrict__ alpha_, int n_obs, int n_trip, float x,
                                   float y, float p, int32_t t_elapsed_s, const double* tab, float* u, float* v) {
  const double* loc = (const double*)__builtin_assume_aligned(loc_, 16);
  const double* alpha = (const double*)__builtin_assume_aligned(alpha_, 16);
  const double xq = (double)x * kBeliefScaleXY, yq = (double)y * kBeliefScaleXY, pq = (double)p * kBeliefScaleP,
               tq = (double)t_elapsed_s * kBeliefScaleT;
  double su = 0.0, sv = 0.0;
#pragma unroll 1
  for (int i0 = 0; i0 < n_trip; i0 += 4) {
    double k[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double* l = loc + 4 * (i0 + r);
      k[r] = gp_belief_kernel(l[0] - xq, l[1] - yq, l[2] - pq, l[3] - tq, tab);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                             // (i ascending: one fixed order)
      su = d_fma(k[r], alpha[2 * (i0 + r)], su);
      sv = d_fma(k[r], alpha[2 * (i0 + r) + 1], sv);
    }
  }
  const float fnan = __builtin_nanf("");
  *u = n_obs < 0 ? fnan : (n_obs == 0 ? 0.0f : (float)su);
  *v = n_obs < 0 ? fnan : (n_obs == 0 ? 0.0f : (float)sv);
}
// the belief's: the window and alpha of one slab
BLE_FN void gp_belief_mean(const double* __restrict__ slab, int n_obs, int n_trip, float x, float y, float p, int32_t t_elapsed_s,
                           const double* tab, float* u, float* v) {
  gp_scenario_correction(slab, slab + kBeliefAlphaAt, n_obs, n_trip, x, y, p, t_elapsed_s, tab, u, v);
}

// the loop's trip count for a window of n_obs (whatever the word holds: the slab is never overrun)
BLE_FN int gp_belief_trip(int n_obs) {
  const int m = n_obs < 0 ? 0 : (n_obs > kBeliefRows ? kBeliefRows : n_obs);
  return (m + 3) & ~3;
}

}  // namespace ble

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------- the kernels
// Included by ble_kernels.hip after ble_rollout.h (RolloutArgs, rollout_lane): ble_observe.h, ble_gp_query.h (GpQueryShared,
// ble_gp_factor.h), kStepBlock and report_flags are there.
namespace ble {

// struct ble_gp_belief (include/ble_abi.h) as the kernels take it
struct BeliefDev {
  double* slab;          // [n][stride]
  int64_t stride;        // >= kBeliefDoubles, even
  int32_t* n_obs;        // [n]
};
static_assert(kBeliefRows == kGpMax && kBeliefKappa == kGpKappa, "ble_gp_belief.h and ble_observe.h disagree");

// the largest trip count among the lanes of a wave (all 64 lanes call it)
__device__ __forceinline__ int belief_wave_trip(int n_obs) {
  int m = gp_belief_trip(n_obs);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_xor(m, d);
    m = o > m ? o : m;
  }
  return __builtin_amdgcn_readfirstlane(m);
}

// an environment without a posterior: a zero slab and n_obs (0, or -1: NaN)
__device__ inline void gp_fit_empty(const BeliefDev& b, int64_t env, int tid, int n_obs) {
  double* slab = b.slab + env * b.stride;
  for (int q = tid; q < kBeliefDoubles; q += kObsBlock) slab[q] = 0.0;
  if (tid == 0) b.n_obs[env] = n_obs;
}

__global__ __launch_bounds__(kObsBlock, 2) void ble_gp_fit_kernel(GpHistory hist, const uint8_t* __restrict__ reset_mask,
                                                                 const int32_t* __restrict__ time_s, BeliefDev b, uint32_t* err_flags) {
  __shared__ GpQueryShared sh;
  const int64_t env = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t flags = 0;

  // ---- phases 0 - 2 (ble_gp_factor.h) at the anchor time: the window, the exit without a posterior, the window compacted with y in sh.z, the factor, alpha
  const int32_t tq = time_s[env];
  const GpWindow w = gp_window(hist, reset_mask, env, tq, lane);
  const int n_obs = w.n_obs;
  if (w.cut) flags |= kFlagGpWindow;
  const bool untold = gp_window_untold(hist, env, tq, w);
  if (untold || n_obs == 0) {         // no posterior (uniform over the workgroup: no barrier has been reached)
    if (untold && tid == 0 && err_flags != nullptr) atomicOr(err_flags, (uint32_t)kFlagGpWindow);
    gp_fit_empty(b, env, tid, untold ? -1 : 0);
    return;
  }
  gp_clear(sh, tid, lane, wave);
  __syncthreads();
  gp_compact(sh, hist, env, w, tid, lane, wave, [&](int at, float, float, float, int32_t, float err_u, float err_v) {
    sh.z[0][at] = (double)err_u; sh.z[1][at] = (double)err_v;
  });
  __syncthreads();
  gp_factor(sh, n_obs, tid);
  const double alpha_i = gp_solve(sh, n_obs, tid);
  if ((tid & 127) < n_obs) sh.alpha[tid >> 7][tid & 127] = alpha_i;      // (zero beyond the window: gp_clear)
  __syncthreads();

  // ---- the belief: the compacted window and alpha (zero beyond the window: loc and alpha were cleared above)
  double* slab = b.slab + env * b.stride;
  for (int q = tid; q < kBeliefDoubles; q += kObsBlock) {
    const int a = q - kBeliefAlphaAt;
    slab[q] = a < 0 ? sh.loc[q >> 2][q & 3] : sh.alpha[a & 1][a >> 1];
  }
  if (tid == 0) b.n_obs[env] = n_obs;
  if (tid == 0 && err_flags != nullptr && flags != 0) atomicOr(err_flags, flags);
}

constexpr int kBeliefWindBlock = 256;

// the belief's mean error at one caller-chosen point per environment: uv [n][2], ble_step_f32's noise_uv
__global__ __launch_bounds__(kBeliefWindBlock) void ble_gp_belief_wind_kernel(BeliefDev b, const float* __restrict__ x_m,
                                                                             const float* __restrict__ y_m,
                                                                             const float* __restrict__ pressure,
                                                                             const int32_t* __restrict__ elapsed_s, float* __restrict__ uv,
                                                                             int64_t n) {
  __shared__ double tab[64];
  if (threadIdx.x < 64) tab[threadIdx.x] = gp_belief_table_entry((int)threadIdx.x);
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * kBeliefWindBlock + threadIdx.x;
  const bool in_range = e < n;
  const int n_obs = in_range ? b.n_obs[e] : 0;
  const int n_trip = belief_wave_trip(n_obs);
  if (in_range) {
    float u, v;
    gp_belief_mean(b.slab + e * b.stride, n_obs, n_trip, x_m[e], y_m[e], pressure[e], elapsed_s[e], tab, &u, &v);
    uv[2 * e] = u; uv[2 * e + 1] = v;
  }
}

// The look-ahead's wind (ble_lookahead.h) in forecast + the belief's mean: every lane of environment e evaluates gp_belief_mean on e's
// slab at its own pre-step position and time.
struct WindBelief {
  struct Shared {
    __attribute__((aligned(16))) double acs_poly[kAcsPolyDoubles];      // (WindForecast's, and the table)
    float term_save[kTermSaveRows * kStepBlock];
    double tab[64];
  };
  BeliefDev b;
  int n_obs = 0, n_trip = 0;
  const double* slab = nullptr;
  __device__ __forceinline__ void load(int64_t e) { n_obs = b.n_obs[e]; }
  static __device__ __forceinline__ void fill(Shared& shm) {
    if (threadIdx.x < 64) shm.tab[threadIdx.x] = gp_belief_table_entry((int)threadIdx.x);
  }
  __device__ __forceinline__ void fetch(Shared&, int64_t e, bool, int64_t) {
    n_trip = belief_wave_trip(n_obs);          // one loop for the wave, whatever environments its lanes belong to
    slab = b.slab + e * b.stride;
  }
  __device__ __forceinline__ void uv(const Shared& shm, const EnvRegs& s, float& nu, float& nv) const {
    gp_belief_mean(slab, n_obs, n_trip, s.x, s.y, s.p, s.t_elapsed, shm.tab, &nu, &nv);
    // the belief's wind is a VALUE, as the noise is in ble_step_kernel: ble_gp_belief_wind_f32 + ble_step_f32 give the same bits
    asm volatile("" : "+v"(nu), "+v"(nv));
  }
};

// ble_rollout_kernel's lanes (ble_rollout.h: rollout_lane) in that wind.  Reads the belief, writes what ble_rollout_kernel writes.
// kLeaves: the lane's whole end state goes to the leaf arena as well (ble_rollout.h: leaf_store and the trailing pack).
template <class V = VehicleDefault, bool kLeaves = false, class... Leaf>
__global__ __launch_bounds__(kStepBlock) void ble_rollout_belief_kernel(StateDev st, RolloutArgs a, BeliefDev b, uint32_t* err_flags, V veh,
                                                                        Leaf... leaves) {
  static_assert(sizeof...(Leaf) == (kLeaves ? 1 : 0), "with leaves: the leaf arena's StateDev; without: nothing");
  __shared__ WindBelief::Shared shm;
  const int64_t lanes_total = a.n * (int64_t)a.n_plans;          // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  const int64_t e = j < lanes_total ? (int64_t)((uint32_t)j / (uint32_t)a.n_plans) : 0;
  WindBelief wind{b};
  rollout_lane<kLeaves>(st, a, wind, shm, j, lanes_total, e, j, lanes_total, err_flags, veh, leaves...);
}

}  // namespace ble
#endif  // __HIPCC__
