// ble_rollout.h -- look ahead on the device: K action plans per environment, flown from the state where it lies (ble_rollout_f32).
//
// One lane per (environment e, plan k), lane index j = e K + k < n K: the lane loads environment e's state, flies the plan's
// n_plan_steps x action_repeat agent steps in registers with the look-ahead lane body (ble_lookahead.h: the lane functions
// ble_step_kernel calls, on the same inputs, hence the same bits per step -- tests/test_gpu_rollout.py flies both side by side) and
// stores the discounted return, the number of steps flown and, if asked, every reward and the final (x, y, pressure, battery charge).
//
// The kernel never writes the state: not the state arrays, not last_command, not the per-episode cache (a miss recomputes the
// constants and keeps them in registers) and not the harmonic cache (WindNoise draws into LDS).  Flags go to the call's own word.
//
// Loads: the K lanes of an environment read the same state words (a broadcast inside a wave, L1 / L2 hits across waves); plans, ret,
// steps_flown, reward and final_state are indexed by j and fully coalesced.  rollout_lane below is the loop shell and the stores of
// all three rollout kernels -- this one, ble_rollout_belief_kernel (ble_gp_belief.h) and ble_rollout_scenarios_kernel
// (ble_scenarios.h), which differ in their wind and their lane map alone.
//
// kLeaves (ble_rollout_leaves_f32): the lane also hands back the WHOLE state it ends with -- the EnvRegs after its last
// executed step, the raw action of that step as last_command, the five per-episode constants -- into index j of a second state, the leaf
// arena, after the loop and coalesced in j (leaf_store below).  A lane that flew nothing (a non-OK source) copies the source's words.
// The leaf arena is the kernels' LAST argument, a parameter pack that holds one StateDev with leaves and nothing without: the
// instantiations without leaves keep their argument list, their kernel descriptor and their instructions (profiles/isa_compare.py).
//
// Included by ble_kernels.hip after ble_step_kernel: kStepBlock, StepNoiseShared and report_flags are that file's.
#pragma once
#include <type_traits>
#include "ble_lookahead.h"

namespace ble {

// struct ble_rollout_f32 (include/ble_abi.h) as the kernel takes it
struct RolloutArgs {
  int64_t n;
  int n_plans, n_plan_steps, action_repeat, substeps;
  double gamma;
  const uint8_t* __restrict__ plans;          // [n_plan_steps][n][n_plans]
  const float* __restrict__ wind_grid;
  int64_t grid_env_stride;
  float* __restrict__ ret;                    // [n][n_plans]
  int32_t* __restrict__ steps_flown;          // [n][n_plans]
  float* __restrict__ reward;                 // optional [n_plan_steps * action_repeat][n][n_plans]
  float* __restrict__ final_state;            // optional [4][n][n_plans]
};

template <bool kLeaves> struct LeafLast {};
template <> struct LeafLast<true> { int act = 0; };

// Lane j's leaf: every array ble_step_kernel's write-back stores, and the per-episode constants.  flew: the lane executed a step (its
// source was OK) -- s and last_act are what it holds; otherwise the source's own words at e.  Never the episode cache.
__device__ __forceinline__ void leaf_store(const StateDev& st, const StateDev& lf, int64_t e, int64_t j, bool flew, const EnvRegs& s,
                                           const EnvConst& c, int last_act) {
  if (flew) {
    lf.x[j] = s.x; lf.y[j] = s.y; lf.pressure[j] = s.p; lf.ambient_temperature[j] = s.t_amb;
    lf.internal_temperature[j] = s.t_int; lf.envelope_volume[j] = s.vol; lf.superpressure[j] = s.sp;
    lf.mols_air[j] = s.n_air; lf.battery_charge[j] = s.batt;
    lf.acs_power[j] = s.acs_power; lf.acs_mass_flow[j] = s.mdot; lf.solar_charging[j] = s.charge;
    lf.power_load[j] = s.load;
    lf.time_elapsed_s[j] = s.t_elapsed; lf.sunrise_h_rel[j] = s.sunrise_h; lf.sunset_rel[j] = s.sunset;
    lf.status[j] = s.status; lf.last_command[j] = (uint8_t)last_act;
    lf.alt_fsm[j] = s.alt_fsm; lf.env_fsm[j] = s.env_fsm; lf.power_paused[j] = s.paused;
  } else {
    lf.x[j] = st.x[e]; lf.y[j] = st.y[e]; lf.pressure[j] = st.pressure[e]; lf.ambient_temperature[j] = st.ambient_temperature[e];
    lf.internal_temperature[j] = st.internal_temperature[e]; lf.envelope_volume[j] = st.envelope_volume[e];
    lf.superpressure[j] = st.superpressure[e]; lf.mols_air[j] = st.mols_air[e]; lf.battery_charge[j] = st.battery_charge[e];
    lf.acs_power[j] = st.acs_power[e]; lf.acs_mass_flow[j] = st.acs_mass_flow[e]; lf.solar_charging[j] = st.solar_charging[e];
    lf.power_load[j] = st.power_load[e];
    lf.time_elapsed_s[j] = st.time_elapsed_s[e]; lf.sunrise_h_rel[j] = st.sunrise_h_rel[e]; lf.sunset_rel[j] = st.sunset_rel[e];
    lf.status[j] = st.status[e]; lf.last_command[j] = st.last_command[e];
    lf.alt_fsm[j] = st.alt_fsm[e]; lf.env_fsm[j] = st.env_fsm[e]; lf.power_paused[j] = st.power_paused[e];
  }
  // (the constants' members are pointers to const: a state is read-only there for every other kernel)
  const_cast<float*>(lf.center_lat_deg)[j] = c.lat0_deg; const_cast<float*>(lf.center_lng_deg)[j] = c.lng0_deg;
  const_cast<float*>(lf.upwelling_infrared)[j] = c.ir; const_cast<float*>(lf.alpha)[j] = c.alpha;
  const_cast<int64_t*>(lf.start_unix)[j] = c.start_unix;
}
// the one element of the kernels' trailing pack
__device__ __forceinline__ const StateDev& leaf_arena(const StateDev& lf) { return lf; }

// A rollout lane: index j < lanes_total of ret / steps_flown / reward / final_state (and of the leaf arena), environment e, its plan at
// index jp < plans_total of every row of plans.  The three rollout kernels are their lane maps and this: the loop shell over
// n_plan_steps x action_repeat, the frozen rule, the stores.
template <bool kLeaves, class W, class V, class... Leaf>
__device__ __forceinline__ void rollout_lane(const StateDev& st, const RolloutArgs& a, W& wind, typename W::Shared& shm, int64_t j,
                                             int64_t lanes_total, int64_t e, int64_t jp, int64_t plans_total, uint32_t* err_flags,
                                             const V& veh, const Leaf&... leaves) {
  const bool in_range = j < lanes_total;
  LookaheadLane l;
  bool live = false;
  if (in_range) {
    lookahead_load(l, st, e, st, a.n, e);
    wind.load(e);
    live = l.s.status == kOk;
  }
  lookahead_fill<W>(shm);
  __syncthreads();
  lookahead_begin(l, wind, shm, st, a, e, in_range, live, veh);
  LeafLast<kLeaves> last;                       // (with leaves: the raw action of the last step flown)
  int64_t o = j;                                // (agent step t) * lanes_total + j
#pragma unroll 1
  for (int h = 0; h < a.n_plan_steps; ++h) {
    const int act = in_range ? (int)a.plans[(int64_t)h * plans_total + jp] : 0;
#pragma unroll 1
    for (int rep = 0; rep < a.action_repeat; ++rep, o += lanes_total) {
      if (live) {
        if constexpr (kLeaves) last.act = act;
        const float r = lookahead_step(l, wind, shm, a, act, veh);
        if (a.reward) a.reward[o] = r;
      } else if (in_range) {                    // a non-OK source, or a plan that went terminal: frozen, reward 0
        if (a.reward) a.reward[o] = 0.0f;
      }
      live = live && l.s.status == kOk;
    }
  }
  if (in_range) {
    const EnvRegs& s = l.s;
    a.ret[j] = (float)l.acc;
    a.steps_flown[j] = l.flown;
    if (a.final_state) {
      a.final_state[j] = s.x; a.final_state[lanes_total + j] = s.y; a.final_state[2 * lanes_total + j] = s.p;
      a.final_state[3 * lanes_total + j] = s.batt;
    }
    if constexpr (kLeaves) leaf_store(st, leaf_arena(leaves...), e, j, l.flown > 0, s, l.c, last.act);      // (flown > 0: the source was OK)
  }
  report_flags(l.flags, err_flags);
}

// One lane per (environment e, plan k), j = e K + k, in the forecast or (kNoise) the generator's wind.
template <bool kNoise, class V = VehicleDefault, bool kLeaves = false, class... Leaf>
__global__ __launch_bounds__(kStepBlock) void ble_rollout_kernel(StateDev st, RolloutArgs a, uint32_t* err_flags, StepNoise gen, V veh,
                                                                 Leaf... leaves) {
  static_assert(sizeof...(Leaf) == (kLeaves ? 1 : 0), "with leaves: the leaf arena's StateDev; without: nothing");
  using W = std::conditional_t<kNoise, WindNoise, WindForecast>;
  __shared__ typename W::Shared shm;
  W wind;
  if constexpr (kNoise) wind.gen = gen;
  const int64_t lanes_total = a.n * (int64_t)a.n_plans;          // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  const int64_t e = j < lanes_total ? (int64_t)((uint32_t)j / (uint32_t)a.n_plans) : 0;
  rollout_lane<kLeaves>(st, a, wind, shm, j, lanes_total, e, j, lanes_total, err_flags, veh, leaves...);
}

}  // namespace ble
