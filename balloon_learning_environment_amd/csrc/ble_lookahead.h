// ble_lookahead.h -- the ONE lane body of the kernels that fly agent steps from a state without writing it: the rollouts
// (ble_rollout_kernel, ble_rollout_belief_kernel, ble_rollout_scenarios_kernel) and the tree expands (ble_tree_expand_kernel,
// ble_tree_expand_scenarios_kernel, ble_mcts_expand_kernel, ble_mcts_expand_scenarios_kernel).  DESIGN.md 3i, "One look-ahead lane body".
//
// What the seven share is here once, and every bit-for-bit guarantee between them rests on that: the state load, the per-episode
// constants (read from the cache, never stored), the LDS fills, the wind term behind its value barriers, the flown step with its
// non-finite check and the three fp64 return statements.  The loop shell, the stores and `live = live && s.status == kOk`, the freeze
// rule, next to them are shared where that costs nothing: rollout_lane (ble_rollout.h) for the three rollouts, expand_lane (ble_tree.h)
// for the two scenario expands.  ble_tree_expand_kernel and ble_mcts_expand_kernel keep that shell as text: through expand_lane they
// were 0.9 - 2.2 % slower.  A kernel keeps what is its own: its wind object and LDS declaration, its lane map and -- an
// expand -- where the parent lies and the rule by which the lane flies, is carried or is void.
//
// A WIND is a small policy: its LDS object `Shared` (acs_poly and term_save are members of every one, in StepNoiseShared's order: the
// note above that struct), what it loads with the state (`load`), fills before the barrier (`fill`) and fetches after it (`fetch`),
// and the error (nu, nv) it adds to the forecast at a pre-step state (`uv`), a VALUE behind an asm barrier wherever it is computed.
// WindForecast and WindNoise are below; WindBelief sits with gp_belief_mean (ble_gp_belief.h) and WindScenario with
// scenario_draws_fetch (ble_scenarios.h), each after the device structs it holds.
//
// The lane functions are ble_step_kernel's own -- wind_query / wind_gather / agent_step, noise_draws_fetch / wind_noise_from_rows --
// on the same inputs, hence the same bits per step.  The step kernels themselves (ble_step_kernel, ble_step_helper_kernel,
// ble_step_split_kernel) keep their bodies as text: sharing with THEM changed the register allocation of the kernels bench.py times
// (the note above ble_step_helper_kernel).  Sharing among the look-ahead kernels touches none of those: profiles/isa_compare.py
// reports every other kernel identical, profiles/lookahead_resource_usage.txt the 26 look-ahead instantiations before and after
// (profiles/expand_lane_resource_usage.txt: the eight scenario expand instantiations before and after expand_lane; timed in
// profiles/expand_lane_ab.jsonl: the scenario pool expand 0.9 - 1.0 % faster, the scenario beam 0.2 - 0.3 %, the one-wind expands
// instruction-identical and within 0.4 %).
// When the lane body was shared, timed against that parent's library (profiles/lookahead_refactor_ab.jsonl): the forecast rollouts and the expands 0.5 - 1.8 % faster,
// the noise rollout and the scenario kernels within 0.3 %, the belief rollout 0.1 - 0.5 % slower -- more than two runs of one library
// differ (0.1 %), about what instruction-identical kernels of the two libraries differ by (up to 0.3 %).  Three pieces put back as text
// one at a time -- the reward store ahead of the return's statements, the constants block in the kernels, the wind handed to
// rollout_lane by value -- did not find it: the first was 0.7 % slower, the second within 0.3 %, the wind by reference (kept)
// 0.2 - 0.7 % faster.
//
// Device only.  Included by ble_kernels.hip after ble_step_kernel: kStepBlock, StepNoiseShared and report_flags are that file's.
#pragma once
#include <type_traits>
#include "ble_noise.h"
#include "ble_step_core.h"

#if defined(__HIPCC__)
namespace ble {

// What a look-ahead lane holds across its steps, and the per-lane constants of the launch
struct LookaheadLane {
  EnvRegs s;
  EnvConst c;
  EpisodeCacheRow cached = {};
  EnvHoisted hc;
  // the discounted return: fp64, the product and the sum as two statements (two roundings under -ffp-contract=on), rounded to fp32 once
  double acc = 0.0, disc = 1.0;
  int flown = 0;                   // agent steps entered with status OK
  uint32_t flags = 0;
  StrideK K;
  const float* grid;               // the environment's wind grid
  float* park;                     // where agent_step parks the state an episode ended with
};

// Node `at` of `src` (a state at its environment's index, or an arena at a node's), every load issued up front: ble_step_kernel's
// loads.  cache_env: the environment whose per-episode cache row the node's constants belong to.
__device__ __forceinline__ void lookahead_load(LookaheadLane& l, const StateDev& src, int64_t at, const StateDev& st, int64_t n,
                                               int64_t cache_env) {
  EnvRegs& s = l.s;
  EnvConst& c = l.c;
  s.status = src.status[at];
  s.x = src.x[at]; s.y = src.y[at]; s.p = src.pressure[at]; s.t_amb = src.ambient_temperature[at];
  s.t_int = src.internal_temperature[at]; s.vol = src.envelope_volume[at]; s.sp = src.superpressure[at];
  s.n_air = src.mols_air[at]; s.batt = src.battery_charge[at];
  s.acs_power = 0.0f; s.mdot = 0.0f; s.charge = 0.0f; s.load = 0.0f;
  s.t_elapsed = src.time_elapsed_s[at]; s.sunrise_h = src.sunrise_h_rel[at]; s.sunset = src.sunset_rel[at];
  s.alt_fsm = src.alt_fsm[at]; s.env_fsm = src.env_fsm[at]; s.paused = src.power_paused[at];
  c.lat0_deg = src.center_lat_deg[at]; c.lng0_deg = src.center_lng_deg[at];
  c.ir = src.upwelling_infrared[at]; c.alpha = src.alpha[at]; c.start_unix = src.start_unix[at];
  if (st.episode_cache != nullptr) l.cached = episode_cache_load(st.episode_cache, n, cache_env);
}

// ---------------------------------------------------------------------------------------------------------------- the winds
// the forecast alone: no error term
struct WindForecast {
  struct Shared {
    __attribute__((aligned(16))) double acs_poly[kAcsPolyDoubles];      // (16: the cubics are read two doubles at a time)
    float term_save[kTermSaveRows * kStepBlock];
  };
  __device__ __forceinline__ void load(int64_t) {}
  static __device__ __forceinline__ void fill(Shared&) {}
  __device__ __forceinline__ void fetch(Shared&, int64_t, bool, int64_t) {}
  __device__ __forceinline__ void uv(const Shared&, const EnvRegs&, float& nu, float& nv) const { nu = 0.0f; nv = 0.0f; }
};

struct WindBelief;               // ble_gp_belief.h

// forecast + the noise generator's field.  noise_draws_fetch WITHOUT a cache: its fill path is a per-lane write on which the lanes of
// one environment would race; every lane draws its environment's harmonics from the Philox stream keyed by (seed, env_offset + e,
// episode[e]), the key of environment e's own flight, into LDS.
struct WindNoise {
  using Shared = StepNoiseShared;
  StepNoise gen;
  __device__ __forceinline__ void load(int64_t) {}
  static __device__ __forceinline__ void fill(Shared& shm) { grad_lut_fill(shm.grad_lut, (int)threadIdx.x, kStepBlock); }
  __device__ __forceinline__ void fetch(Shared& shm, int64_t e, bool in_range, int64_t n) {
    if (in_range)
      noise_draws_fetch(gen.seed, (uint64_t)e, (uint64_t)(e + gen.env_offset), gen.episode ? gen.episode[e] : 0u, nullptr, n,
                        shm.draws + threadIdx.x, kStepBlock);
  }
  __device__ __forceinline__ void uv(const Shared& shm, const EnvRegs& s, float& nu, float& nv) const {
    wind_noise_from_rows(s.x, s.y, s.p, s.t_elapsed, shm.draws + threadIdx.x, kStepBlock, shm.grad_lut, &nu, &nv);
    // the noise is a VALUE, as in ble_step_kernel: no fusing of the generator's last multiplication into agent_step's sum
    asm volatile("" : "+v"(nu), "+v"(nv));
  }
};

// The wind of a kernel that takes its wind as a tag (the host's with_wind picks it).  The kernel fills the object from its arguments.
constexpr int kTreeWindForecast = 0, kTreeWindNoise = 1, kTreeWindBelief = 2;
template <int kWind>
using LookaheadWind = std::conditional_t<kWind == kTreeWindNoise, WindNoise, std::conditional_t<kWind == kTreeWindBelief, WindBelief, WindForecast>>;

// ---------------------------------------------------------------------------------------------------------------- the lane body
// Before the barrier (the caller's __syncthreads): the ACS table's cubics and the wind's tables into LDS.
template <class W>
__device__ __forceinline__ void lookahead_fill(typename W::Shared& shm) {
  for (int q = (int)threadIdx.x; q < kAcsPolyDoubles; q += kStepBlock) shm.acs_poly[q] = kAcsPoly.c[q];
  W::fill(shm);
}

// After the barrier, all lanes: the per-episode constants of a live lane, the wind's fetch, the stride constants, the lane's grid and
// parking block.  A: RolloutArgs, TreeExpandArgs or MctsExpandArgs.
template <class W, class A, class V>
__device__ __forceinline__ void lookahead_begin(LookaheadLane& l, W& wind, typename W::Shared& shm, const StateDev& st, const A& a, int64_t e,
                                                bool in_range, bool live, const V& veh) {
  if (live) {
    // per-episode constants: from the cache where its entry belongs to these constants; a miss recomputes and does NOT store
    if (st.episode_cache != nullptr && episode_cache_hit(l.cached, l.c)) l.hc = hoisted_from_cache(l.cached, l.c);
    else l.hc = hoist_constants(l.c);
  }
  wind.fetch(shm, e, in_range, a.n);
  l.K = stride_k_vreg(veh.dry_mass, veh.lift, veh.v0);
  l.grid = a.wind_grid + e * a.grid_env_stride;
  l.park = shm.term_save + ((int)threadIdx.x >> 6) * (kTermSaveRows * kTermSaveStride) + ((int)threadIdx.x & 63);
}

// One flown agent step of a live lane under raw action `act`, in the forecast plus the wind's error at the pre-step state; returns
// the reward.  The return's three statements stay three.
template <class W, class A, class V>
__device__ __forceinline__ float lookahead_step(LookaheadLane& l, const W& wind, const typename W::Shared& shm, const A& a, int act,
                                                const V& veh) {
  EnvRegs& s = l.s;
  ++l.flown;
  const WindQuery wq = wind_query(s.x, s.y, s.p, s.t_elapsed);
  WindCorners corners;
  wind_gather(l.grid, wq, &corners);
  float nu, nv;
  wind.uv(shm, s, nu, nv);
  float r;
  agent_step(s, l.c, l.hc, act, corners, wq, nu, nv, a.substeps, shm.acs_poly, l.K, l.park, &r, &l.flags, veh);
  if (!(isfinite(s.p) && isfinite(s.t_int) && isfinite(s.x) && isfinite(s.y) && isfinite(s.batt)))
    l.flags |= kFlagNonFinite;
  const double term = l.disc * (double)r;
  l.acc += term;
  l.disc *= a.gamma;
  return r;
}

}  // namespace ble
#endif  // __HIPCC__
