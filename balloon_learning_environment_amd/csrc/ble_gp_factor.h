// ble_gp_factor.h -- the WindGP's window and factor, once: what ble_gp_query_kernel (ble_gp_query.h), ble_gp_fit_kernel (ble_gp_belief.h)
// and ble_gp_fit_scenarios_kernel (ble_scenarios.h) do before their own tails.  One workgroup of kObsBlock threads (4 waves) per
// environment; every function below is called by ALL its threads (the barriers are inside, exactly where the algorithm needs them).
//
//   gp_window    phase 0: the ring's times -> the window |t_i - t_query| < 6 h as two ballots and the cut to the newest 120;
//   gp_window_untold   the rule for evicted entries.  No barrier in either: the caller's early exit (and its atomicOr of the flag)
//                comes right after them.
//   gp_clear     the zeros the later phases rely on and gp_exp_neg_scaled's table; the caller adds its own and places the barrier
//   gp_compact   the window into sh.loc, chronological, in units of the length scales; `keep` stores what else the kernel needs of an entry
//   gp_factor    phases 1a - 1c: K, K = L L^T, W = L^-1 in place
//   gp_solve     phase 2: zeta = W z, then (K^-1 z)_i as the thread's value
//
// All GP algebra is fp64; every product that is fused is an explicit d_fma and every statement is a rounding boundary (the build uses
// -ffp-contract=on), so the three kernels compute the same bits from the same window.  DESIGN.md 3h.
//
// Device-only.  Included by ble_gp_query.h behind GpQueryShared.
#pragma once

namespace ble {

// phase 0's answer, the same in every lane
struct GpWindow {
  int count;                     // the ring's count (0 while a history restart is pending)
  int m;                         // entries the ring holds: min(count, 128); chronological entry e sits in slot (count - m + e) % 128
  unsigned long long b0, b1;     // entries 0 .. 63 and 64 .. 127 inside the window
  int n_obs;                     // the window: at most 120
  int drop;                      // entries inside the 6 h that the cut to the newest 120 leaves out
  bool cut;                      // drop > 0: BLE_FLAG_GP_WINDOW
};

// ---- phase 0: the window at time tq
__device__ __forceinline__ GpWindow gp_window(const GpHistory& hist, const uint8_t* __restrict__ reset_mask, int64_t env, int32_t tq,
                                              int lane) {
  GpWindow w;
  w.count = hist.count[env];
  if (reset_mask != nullptr && reset_mask[env] != 0) w.count = 0;     // a history restart is pending: the next observe() starts afresh
  const int count = w.count;
  const int m = w.m = count < kGpCapacity ? count : kGpCapacity;
  const int32_t* h_t = hist.elapsed_s + env * kGpCapacity;
  // chronological entry e of the ring sits in slot (count - m + e) % 128; every wave reads the times of entries lane and lane + 64
  int32_t ta = tq, tb = tq;
  if (lane < m) ta = h_t[(count - m + lane) % kGpCapacity];
  if (lane + 64 < m) tb = h_t[(count - m + lane + 64) % kGpCapacity];
  const int64_t age_a = (int64_t)ta - (int64_t)tq, age_b = (int64_t)tb - (int64_t)tq;
  w.b0 = __ballot(lane < m && (age_a < 0 ? -age_a : age_a) < kGpHorizonS);       // strict, like the reference
  w.b1 = __ballot(lane + 64 < m && (age_b < 0 ? -age_b : age_b) < kGpHorizonS);
  w.n_obs = __popcll(w.b0) + __popcll(w.b1);
  w.drop = 0;
  w.cut = false;
  if (w.n_obs > kGpMax) { w.drop = w.n_obs - kGpMax; w.n_obs = kGpMax; w.cut = true; }
  return w;
}

// Observations the ring has evicted may belong to the window when its oldest entry does.  They are older than everything in the
// ring: where the window is cut to its newest 120 for a query that is not earlier than the newest observation they would have
// been cut as well (that is ble_observe_kernel's own answer at that time); everywhere else the ring cannot tell -- true:
// BLE_FLAG_GP_WINDOW and NaN.  (Such a window holds the oldest entry: n_obs > 0.)
__device__ __forceinline__ bool gp_window_untold(const GpHistory& hist, int64_t env, int32_t tq, const GpWindow& w) {
  if (w.count > kGpCapacity && (w.b0 & 1ull) != 0) {
    const int32_t t_newest = hist.elapsed_s[env * kGpCapacity + (w.count - 1) % kGpCapacity];
    if (!(w.drop > 0 && tq >= t_newest)) return true;
  }
  return false;
}

// ---- the tables and the zeros: beyond the window loc, z and alpha stay zero, and so do the 128 doubles behind the triangle
__device__ __forceinline__ void gp_clear(GpQueryShared& sh, int tid, int lane, int wave) {
  if (wave == 2) sh.exp2_frac[lane] = kGpSigma2 * d_exp_fast((double)lane * (6.93147180559945286227e-01 / 64.0));
  if (tid < kGpRows) {
    sh.loc[tid][0] = 0.0; sh.loc[tid][1] = 0.0; sh.loc[tid][2] = 0.0; sh.loc[tid][3] = 0.0;
    sh.z[0][tid] = 0.0; sh.z[1][tid] = 0.0; sh.alpha[0][tid] = 0.0; sh.alpha[1][tid] = 0.0;
    sh.inv_diag[tid] = 0.0; sh.part[tid] = 0.0;
  }
  if (tid < 128) sh.W[kCholTri + tid] = 0.0;
}

// ---- compact the window into LDS (chronological), in units of the length scales (ln2 / 32 each: gp_exp_neg_scaled's).  Behind the
// barrier that follows gp_clear.  keep(at, x, y, p, t, err_u, err_v): row `at` of the window and the ring's own values of its entry.
template <class Keep>
__device__ __forceinline__ void gp_compact(GpQueryShared& sh, const GpHistory& hist, int64_t env, const GpWindow& w, int tid, int lane,
                                           int wave, Keep keep) {
  const float* h_xyp = hist.xyp + env * (kGpCapacity * 3);
  const int32_t* h_t = hist.elapsed_s + env * kGpCapacity;
  const float* h_err = hist.err_uv + env * (kGpCapacity * 2);
  if (wave < 2) {
    const unsigned long long b_mine = wave == 0 ? w.b0 : w.b1;
    const int e = tid;                                  // ring entry of this lane (waves 0 and 1: entries 0 .. 127)
    if (((b_mine >> lane) & 1ull) != 0) {
      const int at = __popcll(b_mine & ((1ull << lane) - 1ull)) + (wave == 1 ? __popcll(w.b0) : 0) - w.drop;
      if (at >= 0) {
        const int slot = (w.count - w.m + e) % kGpCapacity;
        const float ox = h_xyp[slot * 3], oy = h_xyp[slot * 3 + 1], op = h_xyp[slot * 3 + 2];
        const int32_t ot = h_t[slot];
        sh.loc[at][0] = (double)ox * (kGpKappa / 357000.0);
        sh.loc[at][1] = (double)oy * (kGpKappa / 357000.0);
        sh.loc[at][2] = (double)op * (kGpKappa / 326.0);
        sh.loc[at][3] = (double)ot * (kGpKappa / 34560.0);
        keep(at, ox, oy, op, ot, h_err[slot * 2], h_err[slot * 2 + 1]);
      }
    }
  }
}

// ---- phase 1: K = s^2 exp(-|d / ls|) + 0.05 I, K = L L^T, W = L^-1 -- all in sh.W, the packed lower triangle (58 KB).  Behind the
// barrier that follows gp_compact; ends on a barrier.  The explicit inverse of the factor is safe in fp64 at cond(K) ~ 3e4.
__device__ __forceinline__ void gp_factor(GpQueryShared& sh, int n_obs, int tid) {
  // ---- phase 1a: K, packed, every entry from the full four-coordinate distance
  const int n_tri = tri(n_obs);            // entries of the packed triangle (tri(i) is the start of row i)
  for (int e = tid; e < n_tri; e += kObsBlock) {
    int i = (int)((__builtin_sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    while (tri(i) > e) --i;
    while (tri(i + 1) <= e) ++i;
    const int j = e - tri(i);
    const double dx = sh.loc[i][0] - sh.loc[j][0], dy = sh.loc[i][1] - sh.loc[j][1], dp = sh.loc[i][2] - sh.loc[j][2],
                 dt = sh.loc[i][3] - sh.loc[j][3];
    const double k = gp_exp_neg_scaled(two_sqrt(dx * dx + dy * dy + dp * dp + dt * dt + 1e-300), sh.exp2_frac);
    sh.W[e] = i == j ? kGpSigma2 + kGpNoise2 : k;
  }
  __syncthreads();

  // ---- phase 1b: K = L L^T, left-looking, column j per step.  Lane pair (i, i + 128) owns row i: the lower lane the first half of
  // the dot product over the columns already done, the upper lane the second.  The running diagonal d_i = K_ii - sum_k L_ik^2 stays
  // in the lower lane's register; the owner of row j + 1 finishes its diagonal inside step j, so no step waits for a square root
  // it has not overlapped with a barrier.
  {
    const int i = tid & 127, h = tid >> 7;
    double* ri = sh.W + tri(i);
    double d_i = (i < n_obs) ? ri[i] : 1.0;
    if (tid == 0) {
      const double sq = __builtin_sqrt(d_i);
      sh.inv_diag[0] = 1.0 / sq; ri[0] = sq;
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j + 1 < n_obs; ++j) {
      const bool row = i > j && i < n_obs;
      const double* rj = sh.W + tri(j);
      const int kmid = j >> 1;
      const int k0 = h ? kmid : 0, k1 = h ? j : kmid;
      double s = 0.0;
      if (row) {
        for (int k = k0; k < k1; ++k) s = d_fma(ri[k], rj[k], s);
        if (h) sh.part[i] = s;
      }
      __syncthreads();
      if (row && !h) {
        const double v = (ri[j] - (s + sh.part[i])) * sh.inv_diag[j];
        ri[j] = v;
        d_i = d_fma(-v, v, d_i);
        if (i == j + 1) {
          const double sq = __builtin_sqrt(d_i);
          sh.inv_diag[i] = 1.0 / sq; ri[i] = sq;
        }
      }
      __syncthreads();
    }
  }

  // ---- phase 1c: W = L^-1 in place, row i per step: W[i][j] = -(1 / L_ii) sum_{k = j}^{i - 1} L[i][k] W[k][j], W[i][i] = 1 / L_ii.
  // Lane pair (j, j + 128) owns column j.  Reads of row i of L come before the step's first barrier, the writes of row i of W after.
  {
    const int j = tid & 127, h = tid >> 7;
#pragma unroll 1
    for (int i = 0; i < n_obs; ++i) {
      const bool act = j < i;
      const double* ri = sh.W + tri(i);
      double s = 0.0;
      if (act) {
        const int kmid = (j + i + 1) >> 1;
        const int k0 = h ? kmid : j, k1 = h ? i : kmid;
        const double* wk = sh.W + tri(k0) + j;          // W[k][j], k = k0 ..: the next row's entry lies k + 1 further
        for (int k = k0; k < k1; ++k) { s = d_fma(ri[k], *wk, s); wk += k + 1; }
        if (h) sh.part[j] = s;
      }
      __syncthreads();
      if (!h) {
        if (act) sh.W[tri(i) + j] = -sh.inv_diag[i] * (s + sh.part[j]);
        else if (j == i) sh.W[tri(i) + i] = sh.inv_diag[i];
      }
      __syncthreads();
    }
  }
}

// ---- phase 2: zeta = W z (left in sh.z), alpha = W^T zeta = K^-1 z -- component c = tid >> 7 on the lanes 128 c .., row i = tid & 127.
// Returns alpha_i of the thread's (i, c), 0.0 beyond the window.  sh.z is read until the last thread has returned: the caller stores
// the value and places the barrier before anything writes z again.
__device__ __forceinline__ double gp_solve(GpQueryShared& sh, int n_obs, int tid) {
  const int i = tid & 127, c = tid >> 7;
  double s = 0.0;
  if (i < n_obs) {
    const double* ri = sh.W + tri(i);
    for (int k = 0; k <= i; ++k) s = d_fma(ri[k], sh.z[c][k], s);
  }
  __syncthreads();
  if (i < n_obs) sh.z[c][i] = s;
  __syncthreads();
  double t = 0.0;
  if (i < n_obs) {
    const double* wk = sh.W + tri(i) + i;              // W[k][i], k = i ..
    for (int k = i; k < n_obs; ++k) { t = d_fma(*wk, sh.z[c][k], t); wk += k + 1; }
  }
  return t;
}

}  // namespace ble
