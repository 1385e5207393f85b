// The WindGP posterior at caller-chosen points (the reference's WindGP.query_batch with ONE query time per environment) for N
// environments on the device -- one workgroup (4 waves) per environment, strictly read-only on the history.
//
//   phase 0    the ring's times -> the window |t_i - t_query| < 6 h (every wave forms the validity ballots itself, as in
//              ble_observe_kernel); more than 120 inside: the newest 120 and BLE_FLAG_GP_WINDOW; the window compacted into LDS in
//              units of the length scales (ln2 / 32 each: gp_exp_neg_scaled's)
//   phase 1    K = s^2 exp(-|d / ls|) + 0.05 I, packed lower triangle in LDS (58 KB), every entry from the full four-coordinate
//              distance; left-looking Cholesky K = L L^T, a column per step, every row's dot product on two lanes;
//              then W = L^-1 IN PLACE, a row per step (row i of W needs row i of L and the rows of W above it)
//   phase 2    zeta = W y, alpha = W^T zeta = K^-1 y (both error components at once, one per half of the workgroup)
//   phase 3    tiles of 16 query points, one per wave and pass: K*^T (120 x 16), lane (g, j) evaluating the entries
//              of observations 4 k + g against query j -- the B operands of v_mfma_f64_16x16x4_f64, made as they are used -- and
//              V = W K*^T = L^-1 K*^T as a triangular x dense product on the matrix pipe, A operands straight from the packed W;
//              mean = K* alpha (accumulated while K* is built), var = s^2 - |V_j|^2 (every lane sums its rows of the D tiles,
//              column_sum the four lanes of a column), deviation = var / s^2; the forecast (wind_forecast_f64: ble_forecast_f32's
//              lane function) is added on request
//
// The explicit inverse of the factor is safe in fp64 at cond(K) ~ 3e4 and turns the part of the work that grows with q into plain
// MFMA products (144 per tile of 16 points at a full window) with no dependency between row blocks.  All GP algebra is fp64.
// LDS 69 KB and <= 256 registers: two workgroups per CU.  DESIGN.md 3h.
//
// Phases 0 - 2 are ble_gp_factor.h's, shared with the two fits (ble_gp_belief.h, ble_scenarios.h); phase 3 is this kernel's own.
#pragma once
#include "ble_observe.h"

namespace ble {

struct GpQueryArgs {
  int64_t n;
  int q;
  int add_forecast;
  const float* xyp;
  const int32_t* time_s;
  const float* wind_grid;
  int64_t grid_env_stride;
  float* mean_uv;
  float* deviation;
};

struct alignas(16) GpQueryShared {
  double exp2_frac[64];          // s^2 2^(k / 64): gp_exp_neg_scaled's table
  double loc[kGpRows][4];        // x, y, p, t of the window's observations in units of ln2 / 32 length scales; zero beyond the window
  double z[2][kGpRows];          // the error components y; then zeta = W y
  double alpha[2][kGpRows];      // K^-1 y; zero beyond the window
  double inv_diag[kGpRows];      // 1 / L[i][i]
  double part[kGpRows];          // the upper lane's half of a row's dot product
  double W[kCholTri + 128];      // K, then L, then W = L^-1: packed lower triangle; then 128 zeros: the "row" of the lanes below the window,
                                 // and the entry of the lanes above the diagonal
};
static_assert(sizeof(GpQueryShared) <= 80 * 1024, "two workgroups per CU need <= 80 KB of LDS each");

}  // namespace ble
#include "ble_gp_factor.h"          // phases 0 - 2 over a GpQueryShared
namespace ble {

// the outputs of an environment without a posterior: the forecast alone (or 0) and `dev`, or NaN
__device__ inline void gp_query_fill(const GpQueryArgs& a, int64_t env, int tid, int32_t tq, bool nan) {
  const float fnan = __builtin_nanf("");
  for (int j = tid; j < a.q; j += kObsBlock) {
    const int64_t o = env * a.q + j;
    double u = 0.0, v = 0.0;
    if (a.add_forecast && !nan)
      wind_forecast_f64(a.wind_grid + env * a.grid_env_stride, a.xyp[o * 3], a.xyp[o * 3 + 1], a.xyp[o * 3 + 2], tq, &u, &v);
    a.mean_uv[o * 2] = nan ? fnan : (float)u;
    a.mean_uv[o * 2 + 1] = nan ? fnan : (float)v;
    a.deviation[o] = nan ? fnan : 0.0f;
  }
}

__global__ __launch_bounds__(kObsBlock, 2) void ble_gp_query_kernel(GpHistory hist, const uint8_t* __restrict__ reset_mask, GpQueryArgs a,
                                                                   uint32_t* err_flags) {
  __shared__ GpQueryShared sh;
  const int64_t env = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t flags = 0;

  // ---- phases 0 - 2 (ble_gp_factor.h): the window, the exit without a posterior, the window compacted with y in sh.z, the factor, alpha
  const int32_t tq = a.time_s[env];
  const GpWindow w = gp_window(hist, reset_mask, env, tq, lane);
  const int n_obs = w.n_obs;
  if (w.cut) flags |= kFlagGpWindow;
  const bool untold = gp_window_untold(hist, env, tq, w);
  if (untold || n_obs == 0) {         // no posterior (uniform over the workgroup: no barrier has been reached)
    if (untold && tid == 0 && err_flags != nullptr) atomicOr(err_flags, (uint32_t)kFlagGpWindow);
    gp_query_fill(a, env, tid, tq, untold);
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

  // ---- phase 3: the query points, 16 per wave and pass.  MFMA register layout (ble_observe.h, measured on gfx950): A lane l holds
  // A[l % 16][l / 16], B lane l holds B[l / 16][l % 16], every register of D lane l an entry of column l % 16.
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int g = lane >> 4, jq = lane & 15;
  const int nb = (n_obs + 15) >> 4;
  const int n_tiles = (a.q + 15) >> 4;
  const float* grid = a.add_forecast ? a.wind_grid + env * a.grid_env_stride : nullptr;
  // the A operands: W[16 I + jq][4 kk + g]; lanes above the diagonal or below the window read the zero behind the triangle.
  // Per row block I the row's start, per K-step an offset of 4: the validity of a K-step is (4 kk + g <= row).
  for (int T = wave; T < n_tiles; T += 4) {
    const int col = 16 * T + jq;
    const bool live = col < a.q;
    const int64_t o = env * a.q + (live ? col : a.q - 1);
    const float xq_f = a.xyp[o * 3], yq_f = a.xyp[o * 3 + 1], pq_f = a.xyp[o * 3 + 2];
    const double xq = (double)xq_f * (kGpKappa / 357000.0), yq = (double)yq_f * (kGpKappa / 357000.0),
                 pq = (double)pq_f * (kGpKappa / 326.0), tqs = (double)tq * (kGpKappa / 34560.0);
    // K-step kk of every row block at once: the entry K*[col][4 kk + g] is evaluated once and multiplied into the accumulators of
    // the row blocks I >= kk / 4 (independent chains: the matrix pipe never waits for its own result), so K*^T needs no registers
    // of its own and the next entry is evaluated under this one's products.
    // A operands W[16 I + jq][4 kk + g]: a per-lane row start and a compile-time offset below the diagonal block (the lanes below
    // the window point at the zeros behind the triangle); a select per K-step inside the diagonal block only.
    int row_at[8], lim[8];
#pragma unroll
    for (int I = 0; I < 8; ++I) {
      const int row = 16 * I + jq;
      row_at[I] = row < n_obs ? tri(row) + g : kCholTri;
      lim[I] = row < n_obs ? row - g : -1;              // K-step kk of the diagonal block reads W[row][4 kk + g] while 4 kk <= lim
    }
    d4 acc[8];
#pragma unroll
    for (int I = 0; I < 8; ++I) acc[I] = d4{0.0, 0.0, 0.0, 0.0};
    double mean_u = 0.0, mean_v = 0.0;
#pragma unroll
    for (int kk = 0; kk < 32; ++kk) {
      if (kk < 4 * nb) {                   // (scalar)
        const int i = 4 * kk + g;
        const double dx = sh.loc[i][0] - xq, dy = sh.loc[i][1] - yq, dp = sh.loc[i][2] - pq, dt = sh.loc[i][3] - tqs;
        const double k = gp_exp_neg_scaled(two_sqrt(dx * dx + dy * dy + dp * dp + dt * dt + 1e-300), sh.exp2_frac);
        mean_u = d_fma(k, sh.alpha[0][i], mean_u);      // (alpha is zero beyond the window)
        mean_v = d_fma(k, sh.alpha[1][i], mean_v);
#pragma unroll
        for (int I = kk >> 2; I < 8; ++I) {
          if (I < nb) {                    // (scalar)
            const double aw = sh.W[(I > (kk >> 2) || 4 * kk <= lim[I]) ? row_at[I] + 4 * kk : kCholTri];
            acc[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(aw, k, acc[I], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);   // (one K-step's operands requested at a time)
    }
    double ssq = 0.0;
#pragma unroll
    for (int I = 0; I < 8; ++I) {
      if (I < nb) {
        ssq = d_fma(acc[I][0], acc[I][0], ssq); ssq = d_fma(acc[I][1], acc[I][1], ssq);
        ssq = d_fma(acc[I][2], acc[I][2], ssq); ssq = d_fma(acc[I][3], acc[I][3], ssq);
      }
    }
    ssq = column_sum(ssq); mean_u = column_sum(mean_u); mean_v = column_sum(mean_v);
    if (g == 0 && live) {
      double fu = 0.0, fv = 0.0;
      if (grid != nullptr) wind_forecast_f64(grid, xq_f, yq_f, pq_f, tq, &fu, &fv);
      double var = kGpSigma2 - ssq;
      var = var < 0.0 ? 0.0 : var;
      a.mean_uv[o * 2] = (float)(mean_u + fu);
      a.mean_uv[o * 2 + 1] = (float)(mean_v + fv);
      a.deviation[o] = (float)(var * (1.0 / kGpSigma2));
    }
  }
  if (tid == 0 && err_flags != nullptr && flags != 0) atomicOr(err_flags, flags);
}

}  // namespace ble
