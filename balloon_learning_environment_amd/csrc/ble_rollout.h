// ble_rollout.h -- look ahead on the device: K action plans per environment, flown from the state where it lies (ble_rollout_f32).
//
// One lane per (environment e, plan k), lane index j = e K + k < n K: the lane loads environment e's state, flies the plan's
// n_plan_steps x action_repeat agent steps in registers with the lane functions ble_step_kernel calls -- wind_query / wind_gather /
// agent_step and, with a noise generator, noise_draws_fetch / wind_noise_from_rows -- and stores the discounted return, the number of
// steps flown and, if asked, every reward and the final (x, y, pressure, battery charge).  Same lane code on the same inputs as
// ble_step_kernel, hence the same bits per step (tests/test_gpu_rollout.py flies both side by side).
//
// The kernel never writes the state: not the state arrays, not last_command, not the per-episode cache (a miss recomputes the
// constants and keeps them in registers) and not the harmonic cache -- noise_draws_fetch is called WITHOUT a cache, its fill path being
// a per-lane write on which the K lanes of one environment would race; every lane draws its environment's harmonics from the Philox
// stream keyed by (seed, env_offset + e, episode[e]), the key of environment e's own flight, into LDS.  Flags go to the call's own word.
//
// Loads: the K lanes of an environment read the same state words (a broadcast inside a wave, L1 / L2 hits across waves); plans, ret,
// steps_flown, reward and final_state are indexed by j and fully coalesced.  The body below is ble_step_kernel's, a third copy next to
// ble_step_helper_kernel's, on purpose: sharing the load code changes the register allocation of the existing instantiations (the note
// above ble_step_helper_kernel).
//
// kLeaves (ble_rollout_leaves_f32): the lane also hands back the WHOLE state it ends with -- the EnvRegs after its last
// executed step, the raw action of that step as last_command, the five per-episode constants -- into index j of a second state, the leaf
// arena, after the loop and coalesced in j (leaf_store below).  A lane that flew nothing (a non-OK source) copies the source's words.
// The leaf arena is the kernels' LAST argument, a parameter pack that holds one StateDev with leaves and nothing without: the
// instantiations without leaves keep their argument list, their kernel descriptor and their instructions (profiles/isa_compare.py).
//
// Included by ble_kernels.hip after ble_step_kernel: kStepBlock, StepNoiseShared and report_flags are that file's.
#pragma once
#include "ble_noise.h"
#include "ble_step_core.h"

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

template <bool kNoise, class V = VehicleDefault, bool kLeaves = false, class... Leaf>
__global__ __launch_bounds__(kStepBlock) void ble_rollout_kernel(StateDev st, RolloutArgs a, uint32_t* err_flags, StepNoise gen, V veh,
                                                                 Leaf... leaves) {
  static_assert(sizeof...(Leaf) == (kLeaves ? 1 : 0), "with leaves: the leaf arena's StateDev; without: nothing");
  double* acs_poly; float* term_save; float* grad_lut = nullptr; uint32_t* noise_draws = nullptr;
  if constexpr (kNoise) {
    __shared__ StepNoiseShared shm;
    acs_poly = shm.acs_poly; term_save = shm.term_save; grad_lut = shm.grad_lut; noise_draws = shm.draws;
  } else {
    __shared__ double acs_poly_lds[kAcsPolyDoubles];
    __shared__ float term_save_lds[kTermSaveRows * kStepBlock];
    acs_poly = acs_poly_lds; term_save = term_save_lds;
  }
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int64_t lanes_total = a.n * (int64_t)a.n_plans;          // < 2^31 (the entry point checks)
  const int64_t j = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
  const bool in_range = j < lanes_total;
  const int64_t e = in_range ? (int64_t)((uint32_t)j / (uint32_t)a.n_plans) : 0;
  uint32_t flags = 0;
  EnvRegs s;
  EnvConst c;
  EpisodeCacheRow cached = {};
  bool live = false;
  if (in_range) {
    // environment e's state, every load issued up front (ble_step_kernel's loads at index e)
    s.status = st.status[e];
    s.x = st.x[e]; s.y = st.y[e]; s.p = st.pressure[e]; s.t_amb = st.ambient_temperature[e];
    s.t_int = st.internal_temperature[e]; s.vol = st.envelope_volume[e]; s.sp = st.superpressure[e];
    s.n_air = st.mols_air[e]; s.batt = st.battery_charge[e];
    s.acs_power = 0.0f; s.mdot = 0.0f; s.charge = 0.0f; s.load = 0.0f;
    s.t_elapsed = st.time_elapsed_s[e]; s.sunrise_h = st.sunrise_h_rel[e]; s.sunset = st.sunset_rel[e];
    s.alt_fsm = st.alt_fsm[e]; s.env_fsm = st.env_fsm[e]; s.paused = st.power_paused[e];
    c.lat0_deg = st.center_lat_deg[e]; c.lng0_deg = st.center_lng_deg[e];
    c.ir = st.upwelling_infrared[e]; c.alpha = st.alpha[e]; c.start_unix = st.start_unix[e];
    if (st.episode_cache != nullptr) cached = episode_cache_load(st.episode_cache, a.n, e);
    live = s.status == kOk;
  }
  for (int q = (int)threadIdx.x; q < kAcsPolyDoubles; q += kStepBlock) acs_poly[q] = kAcsPoly.c[q];
  if (kNoise) grad_lut_fill(grad_lut, (int)threadIdx.x, kStepBlock);
  __syncthreads();
  EnvHoisted hc;
  if (live) {
    // per-episode constants: from the cache where its entry belongs to these constants; a miss recomputes and does NOT store
    if (st.episode_cache != nullptr && episode_cache_hit(cached, c)) hc = hoisted_from_cache(cached, c);
    else hc = hoist_constants(c);
  }
  if (kNoise && in_range)
    noise_draws_fetch(gen.seed, (uint64_t)e, (uint64_t)(e + gen.env_offset), gen.episode ? gen.episode[e] : 0u, nullptr, a.n,
                      noise_draws + threadIdx.x, kStepBlock);
  const StrideK K = stride_k_vreg(veh.dry_mass, veh.lift, veh.v0);
  const float* const grid = a.wind_grid + e * a.grid_env_stride;
  float* const park = term_save + wave * (kTermSaveRows * kTermSaveStride) + lane;
  // the discounted return: fp64, the product and the sum as two statements (two roundings under -ffp-contract=on), rounded to fp32 once
  double acc = 0.0, disc = 1.0;
  int flown = 0;
  LeafLast<kLeaves> last;                       // (with leaves: the raw action of the last step flown)
  int64_t o = j;                                // (agent step t) * n K + j
#pragma unroll 1
  for (int h = 0; h < a.n_plan_steps; ++h) {
    const int act = in_range ? (int)a.plans[(int64_t)h * lanes_total + j] : 0;
#pragma unroll 1
    for (int rep = 0; rep < a.action_repeat; ++rep, o += lanes_total) {
      if (live) {
        ++flown;
        if constexpr (kLeaves) last.act = act;
        const WindQuery wq = wind_query(s.x, s.y, s.p, s.t_elapsed);
        WindCorners corners;
        wind_gather(grid, wq, &corners);
        float nu = 0.0f, nv = 0.0f;
        if (kNoise) {
          wind_noise_from_rows(s.x, s.y, s.p, s.t_elapsed, noise_draws + threadIdx.x, kStepBlock, grad_lut, &nu, &nv);
          // the noise is a VALUE, as in ble_step_kernel: no fusing of the generator's last multiplication into agent_step's sum
          asm volatile("" : "+v"(nu), "+v"(nv));
        }
        float r;
        agent_step(s, c, hc, act, corners, wq, nu, nv, a.substeps, acs_poly, K, park, &r, &flags, veh);
        if (!(isfinite(s.p) && isfinite(s.t_int) && isfinite(s.x) && isfinite(s.y) && isfinite(s.batt)))
          flags |= kFlagNonFinite;
        if (a.reward) a.reward[o] = r;
        const double term = disc * (double)r;
        acc += term;
        disc *= a.gamma;
      } else if (in_range) {                    // a non-OK source, or a plan that went terminal: frozen, reward 0
        if (a.reward) a.reward[o] = 0.0f;
      }
      live = live && s.status == kOk;
    }
  }
  if (in_range) {
    a.ret[j] = (float)acc;
    a.steps_flown[j] = flown;
    if (a.final_state) {
      a.final_state[j] = s.x; a.final_state[lanes_total + j] = s.y; a.final_state[2 * lanes_total + j] = s.p;
      a.final_state[3 * lanes_total + j] = s.batt;
    }
    if constexpr (kLeaves) leaf_store(st, leaf_arena(leaves...), e, j, flown > 0, s, c, last.act);      // (flown > 0: the source was OK)
  }
  report_flags(flags, err_flags);
}

}  // namespace ble
