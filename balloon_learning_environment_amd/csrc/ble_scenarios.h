// ble_scenarios.h -- plan against SAMPLED winds: M scenario winds per environment, each a draw of the noise field the
// WindGP models, corrected so that it passes through the balloon's own measurements (pathwise conditioning, Matheron's rule):
//
//     error_m(x) = f_m(x) + sum_i k(loc_i, x) alpha^m_i,      alpha^m = (K + 0.05 I)^-1 (y - f_m(X))
//
// f_m: wind_noise_from_rows (ble_noise.h, unchanged bits) over harmonics drawn from the scenario stream of (e, m); X, y, K: the window
// frozen at the anchor, as ble_gp_fit_kernel takes it; k: gp_belief_kernel.  The sum of the two terms is ONE fp32 addition of two fp32
// values: the noise value and the correction rounded as gp_belief_mean rounds.
//
//   ble_gp_fit_scenarios_kernel   one workgroup (4 waves) per environment: phases 0-1 of ble_gp_fit_kernel (window, K, L, W = L^-1), then
//                                 for each m: f_m at the window's points, the residual y - f_m, phase 2 -> alpha^m.  The phases are
//                                 ble_gp_factor.h's functions, the ones ble_gp_fit_kernel and the query kernel call.
//   gp_scenario_correction        (ble_gp_belief.h) gp_belief_mean's body with the slab's window and alpha^m as its two pointers.
//   ble_gp_scenario_wind_kernel   one lane per environment at caller-chosen points and a scenario index per environment: what
//                                 ble_step_f32 takes as noise_uv.  prior_only: f_m alone.
//   WindScenario                  the look-ahead's wind policy (ble_lookahead.h): f_m + the correction in the slot of the noise term.
//   ble_rollout_scenarios_kernel  ble_rollout_kernel's lanes (rollout_lane) in that wind, one lane per (e, k, m), j = (e K + k) M + m.
//   ble_plan_risk_kernel          one lane per (e, k): ret [n][K][M] -> score [n][K], the mean of the `tail` smallest scenario returns.
//
// The slab of an environment (stride doubles, 16-byte aligned, stride >= 480 + 240 M and even):
//   [0, 480)                       loc[120][4], exactly ble_gp_fit_kernel's
//   [480 + 240 m, 480 + 240 (m+1)) alpha^m[120][2], u and v interleaved
// Everything beyond the window is zero (the note in ble_gp_belief.h: any trip count that covers n_obs gives the same bits).
//
// The stream, the risk order and the score build on the host as well (tests/emul/scenario_emul.cpp).
#pragma once
#include "ble_noise.h"
#include "ble_gp_belief.h"

namespace ble {

constexpr int kScenarioMax = 16;                                  // BLE_SCENARIO_MAX
constexpr unsigned long long kScenarioKey = 0x5343454E4152ull;    // "SCENAR": no scenario stream is the truth's (seed ^ 0x5EEDF00D)
constexpr int kScenarioBlocks = 32;                               // Philox blocks per scenario: ten harmonics take 90 words = 23 blocks
constexpr int kScenarioAlphaDoubles = 2 * kBeliefRows;            // 240
BLE_FN int scenario_slab_doubles(int num) { return kBeliefAlphaAt + kScenarioAlphaDoubles * num; }

// The generator of scenario m of an environment at its first block: the noise's own construction -- philox_init(seed ^ key constant,
// the environment's key, episode) -- with the key constant kScenarioKey and the block counter started at 32 m.  A function of
// (seed, key, episode, m) alone.
BLE_FN Philox scenario_stream(uint64_t seed, uint64_t key, uint32_t episode, int m) {
  Philox g = philox_init(seed ^ kScenarioKey, key, episode);
  g.c0 = (uint32_t)(m * kScenarioBlocks);
  return g;
}
// Harmonic k = 5 comp + h of that scenario, without drawing the ones before it: harmonic k starts at word 9 k of the stream (one
// seed word and four 53-bit uniforms of two words each), i.e. in block 9 k / 4 with 9 k % 4 of its words already taken.
BLE_FN HarmonicDraw scenario_harmonic(uint64_t seed, uint64_t key, uint32_t episode, int m, int k) {
  Philox g = scenario_stream(seed, key, episode, m);
  g.c0 += (uint32_t)((9 * k) >> 2);
  philox_refill(g);
  g.have = 4 - ((9 * k) & 3);
  return harmonic_draw(g);
}
// The 50 words of scenario m into `dst`, `dst_stride` apart (rows 5 k .. 5 k + 4 = (seed, ox, oy, op, ot) of harmonic k): the layout
// wind_noise_from_rows reads.  Drawn in order from one generator: the same words as scenario_harmonic's.
BLE_FN void scenario_draws_fetch(uint64_t seed, uint64_t key, uint32_t episode, int m, uint32_t* dst, int64_t dst_stride) {
  Philox g = scenario_stream(seed, key, episode, m);
#pragma unroll 1
  for (int k = 0; k < 10; ++k) {
    const HarmonicDraw d = harmonic_draw(g);
    uint32_t* o = dst + (int64_t)(5 * k) * dst_stride;
    o[0] = d.hseed; o[dst_stride] = float_bits_u32(d.ox); o[2 * dst_stride] = float_bits_u32(d.oy);
    o[3 * dst_stride] = float_bits_u32(d.op); o[4 * dst_stride] = float_bits_u32(d.ot);
  }
}

// One component of wind_noise_from_rows: the same calls in the same order, hence the same bits as out[comp] there.
BLE_FN float wind_noise_component_from_rows(int comp, float x_m, float y_m, float pressure, int32_t elapsed_s, const uint32_t* rows,
                                            int64_t stride, const float* lut) {
  BLE_NO_CONTRACT
  float x_km, y_km, t_h;
  noise_coords(x_m, y_m, elapsed_s, &x_km, &y_km, &t_h);
  NoiseAccumulator a;
#pragma unroll 1
  for (int h = 0; h < 5; ++h)
    noise_add_harmonic(a, comp, h, harmonic_draw_from_rows(rows, stride, 5 * comp + h), x_km, y_km, pressure, t_h, lut);
  return noise_finish(a);
}

// ---------------------------------------------------------------------------------------------------------------- the risk score
// The ascending sort key of a FINITE return (-0 counts as +0): key(a) < key(b) <=> a < b.
BLE_FN uint32_t risk_key(float ret) {
  uint32_t u = float_bits_u32(ret);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
BLE_FN bool risk_finite(float ret) { return (float_bits_u32(ret) & 0x7F800000u) != 0x7F800000u; }
// scenario j comes before scenario m: the smaller return, then the smaller index
BLE_FN bool risk_before(uint32_t key_j, int j, uint32_t key_m, int m) { return key_j < key_m || (key_j == key_m && j < m); }
// The ranks of the M <= 16 returns at ret[0], ret[stride], ..., four bits each: nibble m = the number of scenarios in front of m.
// Counted, as plan_rank counts; kept in one 64-bit word, so nothing is indexed at run time but the memory `ret` points to.
BLE_FN uint64_t risk_ranks(const float* ret, int64_t stride, int num) {
  uint64_t ranks = 0;
#pragma unroll 1
  for (int m = 0; m < num; ++m) {
    const uint32_t mine = risk_key(ret[m * stride]);
    uint64_t rank = 0;
#pragma unroll 1
    for (int j = 0; j < num; ++j) rank += risk_before(risk_key(ret[j * stride]), j, mine, m) ? 1u : 0u;
    ranks |= rank << (4 * m);
  }
  return ranks;
}
// The mean of the `tail` smallest of the M returns: summed in fp64 in rank order from 0.0, divided once, rounded to fp32 once.  Any
// non-finite return among the M: NaN (plan_key puts the plan last).  1 <= tail <= num <= 16.
BLE_FN float plan_risk_score(const float* ret, int64_t stride, int num, int tail) {
  bool finite = true;
#pragma unroll 1
  for (int m = 0; m < num; ++m) finite = finite && risk_finite(ret[m * stride]);
  if (!finite) return __builtin_nanf("");
  const uint64_t ranks = risk_ranks(ret, stride, num);
  double sum = 0.0;
#pragma unroll 1
  for (int r = 0; r < tail; ++r) {
#pragma unroll 1
    for (int m = 0; m < num; ++m)
      if ((int)((ranks >> (4 * m)) & 15u) == r) sum += (double)ret[m * stride];     // (ranks are a permutation: exactly one m)
  }
  return (float)(sum / (double)tail);
}

}  // namespace ble

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------- the kernels
// Included by ble_kernels.hip after ble_plan.h: ScalarSeed / EnvSeed, GpQueryShared, RolloutArgs and rollout_lane, belief_wave_trip,
// kStepBlock and report_flags are there.
namespace ble {

// struct ble_gp_scenarios (include/ble_abi.h) as the kernels take it
struct ScenariosDev {
  double* slab;          // [n][stride]
  int64_t stride;        // >= 480 + 240 num, even
  int32_t* n_obs;        // [n]
  int num;               // M: 1 .. kScenarioMax
};
// struct ble_scenario_gen without its seed (S carries it)
struct ScenarioGen {
  const uint32_t* __restrict__ episode;        // [n] or NULL: episode 0
  int64_t env_offset;
};

// an environment without a posterior: a zero slab and n_obs (0: every scenario is its prior; -1: NaN)
__device__ inline void gp_fit_scenarios_empty(const ScenariosDev& b, int64_t env, int tid, int n_obs) {
  double* slab = b.slab + env * b.stride;
  const int doubles = scenario_slab_doubles(b.num);
  for (int q = tid; q < doubles; q += kObsBlock) slab[q] = 0.0;
  if (tid == 0) b.n_obs[env] = n_obs;
}

// what the scenario fit keeps in LDS next to the factor
struct ScenarioFitShared {
  __attribute__((aligned(16))) float grad_lut[kGradLutFloats];
  double y[2][kGpRows];                        // the measurements: sh.z is overwritten by every scenario's phase 2
  float px[kGpRows], py[kGpRows], pp[kGpRows]; // the ring's own float32 x, y, p of the window's points
  int32_t pt[kGpRows];                         // and its int32 t
  uint32_t draws[kScenarioMax][50];            // the harmonic words of every scenario (row m: 50 words, stride 1)
};
static_assert(sizeof(GpQueryShared) + sizeof(ScenarioFitShared) <= 80 * 1024, "two workgroups per CU need <= 80 KB of LDS each");

template <class S>
__global__ __launch_bounds__(kObsBlock, 2) void ble_gp_fit_scenarios_kernel(GpHistory hist, const uint8_t* __restrict__ reset_mask,
                                                                           const int32_t* __restrict__ time_s, ScenariosDev b, S seed,
                                                                           ScenarioGen gen, uint32_t* err_flags) {
  __shared__ GpQueryShared sh;
  __shared__ ScenarioFitShared sc;
  const int64_t env = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t flags = 0;

  // ---- phases 0 - 1 (ble_gp_factor.h) at the anchor time: the window, the exit without a posterior, the window compacted, the factor
  const int32_t tq = time_s[env];
  const GpWindow w = gp_window(hist, reset_mask, env, tq, lane);
  const int n_obs = w.n_obs;
  if (w.cut) flags |= kFlagGpWindow;
  const bool untold = gp_window_untold(hist, env, tq, w);
  if (untold || n_obs == 0) {         // no posterior (uniform over the workgroup: no barrier has been reached)
    if (untold && tid == 0 && err_flags != nullptr) atomicOr(err_flags, (uint32_t)kFlagGpWindow);
    gp_fit_scenarios_empty(b, env, tid, untold ? -1 : 0);
    return;
  }
  // the zeros and tables of the factor and this kernel's own; the harmonics of every scenario
  gp_clear(sh, tid, lane, wave);
  if (tid < kGpRows) {
    sc.y[0][tid] = 0.0; sc.y[1][tid] = 0.0;
    sc.px[tid] = 0.0f; sc.py[tid] = 0.0f; sc.pp[tid] = 0.0f; sc.pt[tid] = 0;
  }
  grad_lut_fill(sc.grad_lut, tid, kObsBlock);
  if (tid < 10 * b.num) {                               // thread (m, k): harmonic k of scenario m, from its own place in the stream
    const int sm = tid / 10, k = tid - 10 * sm;
    const HarmonicDraw d = scenario_harmonic(seed.of(env), seed.key(env, gen.env_offset), gen.episode ? gen.episode[env] : 0u, sm, k);
    uint32_t* o = sc.draws[sm] + 5 * k;
    o[0] = d.hseed; o[1] = float_bits_u32(d.ox); o[2] = float_bits_u32(d.oy); o[3] = float_bits_u32(d.op); o[4] = float_bits_u32(d.ot);
  }
  __syncthreads();
  // y is kept apart from sh.z (every scenario's phase 2 overwrites that), with the ring's own float x, y, p and int t for f_m
  gp_compact(sh, hist, env, w, tid, lane, wave, [&](int at, float ox, float oy, float op, int32_t ot, float err_u, float err_v) {
    sc.y[0][at] = (double)err_u; sc.y[1][at] = (double)err_v;
    sc.px[at] = ox; sc.py[at] = oy; sc.pp[at] = op; sc.pt[at] = ot;
  });
  __syncthreads();
  gp_factor(sh, n_obs, tid);

  // ---- the window, once (zero beyond it: loc was cleared above)
  double* slab = b.slab + env * b.stride;
  for (int q = tid; q < kBeliefAlphaAt; q += kObsBlock) slab[q] = sh.loc[q >> 2][q & 3];

  // ---- per scenario: f_m at the window's points, the residual, phase 2.  Component c on the lanes 128 c .., point i = tid & 127:
  // 2 x 120 evaluations over the 256 threads, one each
  {
    const int i = tid & 127, c = tid >> 7;
#pragma unroll 1
    for (int sm = 0; sm < b.num; ++sm) {
      if (i < n_obs) {
        const float f = wind_noise_component_from_rows(c, sc.px[i], sc.py[i], sc.pp[i], sc.pt[i], sc.draws[sm], 1, sc.grad_lut);
        sh.z[c][i] = sc.y[c][i] - (double)f;
      }
      __syncthreads();
      const double t = gp_solve(sh, n_obs, tid);          // phase 2: alpha^m = K^-1 (y - f_m)
      if (i < kBeliefRows) slab[kBeliefAlphaAt + kScenarioAlphaDoubles * sm + 2 * i + c] = t;      // (0.0 beyond the window)
      __syncthreads();                                     // (the next scenario overwrites z)
    }
  }
  if (tid == 0) b.n_obs[env] = n_obs;
  if (tid == 0 && err_flags != nullptr && flags != 0) atomicOr(err_flags, flags);
}

constexpr int kScenarioWindBlock = 256;
struct ScenarioWindShared {
  __attribute__((aligned(16))) float grad_lut[kGradLutFloats];
  double tab[64];
  uint32_t draws[50 * kScenarioWindBlock];
};

// The scenario wind's ERROR at one caller-chosen point per environment, scenario scenario_index[e]: uv [n][2], ble_step_f32's noise_uv.
// An index outside 0 .. num - 1: NaN, nothing of the slab read.  prior_only: f_m alone (the slab is not read at all).
template <class S>
__global__ __launch_bounds__(kScenarioWindBlock) void ble_gp_scenario_wind_kernel(ScenariosDev b, S seed, ScenarioGen gen,
                                                                                 const int32_t* __restrict__ scenario_index,
                                                                                 const float* __restrict__ x_m, const float* __restrict__ y_m,
                                                                                 const float* __restrict__ pressure,
                                                                                 const int32_t* __restrict__ elapsed_s, int prior_only,
                                                                                 float* __restrict__ uv, int64_t n) {
  __shared__ ScenarioWindShared shm;
  grad_lut_fill(shm.grad_lut, (int)threadIdx.x, kScenarioWindBlock);
  if (threadIdx.x < 64) shm.tab[threadIdx.x] = gp_belief_table_entry((int)threadIdx.x);
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * kScenarioWindBlock + threadIdx.x;
  const bool in_range = e < n;
  const int sm = in_range ? scenario_index[e] : 0;
  const bool valid = in_range && sm >= 0 && sm < b.num;
  const int n_obs = (valid && !prior_only) ? b.n_obs[e] : 0;
  const int n_trip = belief_wave_trip(n_obs);          // (all 64 lanes)
  uint32_t* const rows = shm.draws + threadIdx.x;
  if (valid) scenario_draws_fetch(seed.of(e), seed.key(e, gen.env_offset), gen.episode ? gen.episode[e] : 0u, sm, rows, kScenarioWindBlock);
  if (in_range) {
    float u = __builtin_nanf(""), v = __builtin_nanf("");
    if (valid) {
      float fu, fv;
      wind_noise_from_rows(x_m[e], y_m[e], pressure[e], elapsed_s[e], rows, kScenarioWindBlock, shm.grad_lut, &fu, &fv);
      asm volatile("" : "+v"(fu), "+v"(fv));             // the prior is a VALUE (ble_wind_noise_kernel's bits)
      if (prior_only) {
        u = fu; v = fv;
      } else {
        const double* slab = b.slab + e * b.stride;
        float cu, cv;
        gp_scenario_correction(slab, slab + kBeliefAlphaAt + kScenarioAlphaDoubles * sm, n_obs, n_trip, x_m[e], y_m[e], pressure[e],
                               elapsed_s[e], shm.tab, &cu, &cv);
        asm volatile("" : "+v"(cu), "+v"(cv));           // and so is the correction: ONE fp32 addition of two fp32 values
        u = fu + cu; v = fv + cv;
      }
    }
    uv[2 * e] = u; uv[2 * e + 1] = v;
  }
}

// WindScenario's LDS: WindNoise's (StepNoiseShared, in its order) and the belief's table
struct ScenarioRolloutShared {
  __attribute__((aligned(16))) float grad_lut[kGradLutFloats];
  double acs_poly[kAcsPolyDoubles];
  double tab[64];
  float term_save[kTermSaveRows * kStepBlock];
  uint32_t draws[50 * kStepBlock];
};

// The look-ahead's wind (ble_lookahead.h) in scenario sm of the lane's environment: per agent step f_m and the correction at the
// pre-step state, each a VALUE, their ONE fp32 addition a value again: the bits of ble_gp_scenario_wind_kernel followed by
// ble_step_f32.  Reads the slab; writes nothing but its LDS rows.
template <class S>
struct WindScenario {
  using Shared = ScenarioRolloutShared;
  ScenariosDev b;
  S seed;
  ScenarioGen gen;
  int sm;
  int n_obs = 0, n_trip = 0;
  const double* loc = nullptr;
  const double* alpha = nullptr;
  __device__ __forceinline__ void load(int64_t e) { n_obs = b.n_obs[e]; }
  static __device__ __forceinline__ void fill(Shared& shm) {
    grad_lut_fill(shm.grad_lut, (int)threadIdx.x, kStepBlock);
    if (threadIdx.x < 64) shm.tab[threadIdx.x] = gp_belief_table_entry((int)threadIdx.x);
  }
  __device__ __forceinline__ void fetch(Shared& shm, int64_t e, bool in_range, int64_t) {
    if (in_range)
      scenario_draws_fetch(seed.of(e), seed.key(e, gen.env_offset), gen.episode ? gen.episode[e] : 0u, sm, shm.draws + threadIdx.x, kStepBlock);
    n_trip = belief_wave_trip(n_obs);          // one loop for the wave, whatever environments its lanes belong to
    loc = b.slab + e * b.stride;
    alpha = loc + kBeliefAlphaAt + kScenarioAlphaDoubles * sm;
  }
  __device__ __forceinline__ void uv(const Shared& shm, const EnvRegs& s, float& nu, float& nv) const {
    float fu, fv, cu, cv;
    wind_noise_from_rows(s.x, s.y, s.p, s.t_elapsed, shm.draws + threadIdx.x, kStepBlock, shm.grad_lut, &fu, &fv);
    asm volatile("" : "+v"(fu), "+v"(fv));
    gp_scenario_correction(loc, alpha, n_obs, n_trip, s.x, s.y, s.p, s.t_elapsed, shm.tab, &cu, &cv);
    asm volatile("" : "+v"(cu), "+v"(cv));
    nu = fu + cu; nv = fv + cv;
    // the scenario's wind is a VALUE, as the noise is in ble_step_kernel: ble_gp_scenario_wind_f32 + ble_step_f32 give the same bits
    asm volatile("" : "+v"(nu), "+v"(nv));
  }
};

// ble_rollout_kernel's lanes (ble_rollout.h: rollout_lane) in the scenario winds: one lane per (environment e, plan k, scenario m),
// j = (e K + k) M + m.  Plans are read at [h][e K + k]; ret, steps_flown, reward and final_state are indexed by j (a.n_plans is K;
// lanes_total = n K M).  Reads the state, the caches and the slab; writes none of them.
template <class V, class S>
__global__ __launch_bounds__(kStepBlock) void ble_rollout_scenarios_kernel(StateDev st, RolloutArgs a, ScenariosDev b, S seed, ScenarioGen gen,
                                                                          uint32_t* err_flags, V veh) {
  __shared__ ScenarioRolloutShared shm;
  const int64_t plans_total = a.n * (int64_t)a.n_plans;
  const int64_t lanes_total = plans_total * b.num;               // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  const int64_t ek = j < lanes_total ? (int64_t)((uint32_t)j / (uint32_t)b.num) : 0;
  const int sm = j < lanes_total ? (int)(j - ek * b.num) : 0;
  const int64_t e = (int64_t)((uint32_t)ek / (uint32_t)a.n_plans);
  WindScenario<S> wind{b, seed, gen, sm};
  rollout_lane<false>(st, a, wind, shm, j, lanes_total, e, ek, plans_total, err_flags, veh);
}

// struct ble_plan_risk (include/ble_abi.h) as the kernel takes it
struct PlanRiskArgs {
  int64_t n;
  int n_plans, num, tail;
  const float* __restrict__ ret;               // [n][K][M]
  float* __restrict__ score;                   // [n][K]
};

__global__ __launch_bounds__(256) void ble_plan_risk_kernel(PlanRiskArgs a) {
  const int64_t lanes_total = a.n * (int64_t)a.n_plans;          // n K M < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= lanes_total) return;
  a.score[j] = plan_risk_score(a.ret + j * a.num, 1, a.num, a.tail);
}

}  // namespace ble
#endif  // __HIPCC__
