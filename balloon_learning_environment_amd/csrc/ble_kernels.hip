// ble_kernels.hip -- gfx950 (MI355X, CDNA4) kernels and the C ABI of libble_hip.so.
//
// Execution model: one wavefront lane per environment, 256-thread workgroups of four independent waves,
// so N = 65 536 environments is 256 workgroups = one per CU, one wave on every SIMD of the 256 CUs.
// The state is struct-of-arrays: every load/store below is a fully coalesced
// 64-lane x 4 B (or 1 B) transaction.  The 317 KB wind grid is shared by all lanes and is
// served from the per-XCD L2 after first touch; each lane gathers its 16 corners as
// 8 x (4 contiguous floats).  Nothing here is a dense contraction: no MFMA.
// Target: gfx950 only (hipcc --offload-arch=gfx950); no other backend, no shims.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <type_traits>

// Instrumentation hooks of ble_step_kernel: empty in the product build.  A profiling build
// (profiles/build_variant.sh ... -DBLE_STEP_BLOCK=64 -DBLE_STEP_INSTR_HEADER='"../../profiles/instr/ble_step_instr.h"') takes per-wave clock
// marks from that header, which is not part of the package.
#ifdef BLE_STEP_INSTR_HEADER
#include BLE_STEP_INSTR_HEADER
#else
#define BLE_STEP_INSTR_BEGIN() do {} while (0)
#define BLE_STEP_MARK(i) do {} while (0)
#define BLE_STEP_INSTR_END() do {} while (0)
#define BLE_STEP_STEP_DONE(k) do {} while (0)
#define BLE_STEP_COUNTS_LIVE 1
#endif

#include "../../include/ble_abi.h"
#include "ble_reset.h"
#include "ble_step_core.h"
#include "ble_noise.h"
#include "ble_step_split.h"
#include "ble_step_helper.h"
#include "ble_observe.h"
#include "ble_gp_query.h"
#include "ble_decode.h"
#include "ble_agent.h"
#include "ble_qnet.h"
#include "ble_train.h"
#include "ble_explore.h"
#include "ble_actor.h"
#include "ble_imitate.h"
#include "ble_replay.h"
#include "ble_population.h"
#include "ble_population_train.h"
#include "ble_population_td.h"
#include "ble_population_prio.h"

using namespace ble;

namespace {

constexpr int kBlock = 64;  // one wavefront per workgroup
// ble_step_kernel's workgroup: BLE_STEP_BLOCK / 64 independent wavefronts (they share the ACS table's LDS copy and one barrier at entry).
// 256 = one workgroup per CU at 65 536 environments, a wave on each of its SIMDs: a quarter of the dispatches of 64-thread workgroups --
// measured 15.5-15.7 against 15.7-15.9 us per fused step and 23.6-23.8 against 24.2 us per one-step launch (profiles/r04_raw/step_block_ab.txt)
#ifndef BLE_STEP_BLOCK
#define BLE_STEP_BLOCK 256
#endif
constexpr int kStepBlock = BLE_STEP_BLOCK;

__device__ __forceinline__ void report_flags(uint32_t flags, uint32_t* err_flags) {
  // wave-level OR, one atomic per wave at most (normally none)
  if (err_flags == nullptr) return;
  if (__any(flags != 0)) {
    for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off, 64);
    if ((threadIdx.x & 63) == 0) atomicOr(err_flags, flags);
  }
}

// `n_steps` consecutive agent steps of the rank's environments in ONE launch: the state is
// loaded once, stays in registers across the steps and is stored once; per step only the
// action byte is read, the 16 wind-grid corners are gathered and reward / terminal are
// written.  n_steps == 1 is the plain BalloonArena.step; n_steps > 1 serves ble_step_n_f32
// (rollouts whose actions are known up front, e.g. the random policy of the headline config).
// action / reward / terminal are [n_steps][n]; active_count is [n_steps][BLE_COUNT_SLOTS].
// kNoise (ble_step_n_f32 with a noise generator, ABI 3): the SimplexWindNoise term of WindField.get_ground_truth
// (wind_field.py:125-145) is evaluated IN the kernel at every step's pre-step position -- the same lane function as
// ble_wind_noise_f32 (wind_noise_cached), hence the same bits as ble_wind_noise_f32 + ble_step_f32 step by step.  A
// separate instantiation: the noise-free rollout keeps its register allocation.
// ble_step_kernel<noise>'s LDS as ONE object in this order: the gradient table (read five times per harmonic at a per-lane index) and the
// arrays the stride loop reads stay within ds_read's 16-bit offset; the 50 KB of harmonic draws, walked by a pointer, come last.  As
// separate objects the compiler put the draws first and the table at the end of 66 KB: every read of it paid an addition of its base.
struct StepNoiseShared {
  __attribute__((aligned(16))) float grad_lut[kGradLutFloats];      // the noise primitive's gradient weights
  double acs_poly[kAcsPolyDoubles];
  float term_save[kTermSaveRows * kStepBlock];
  uint32_t draws[50 * kStepBlock];      // the harmonics' seeds and offsets of the workgroup's environments, fetched once per launch
};
// V: the flight vehicle's constants -- VehicleDefault (compile-time: ble_state_f32.vehicle == NULL) or VehicleRt (a kernel argument, i.e.
// scalar registers: ABI 5) -- as the LAST argument, so that the default instantiation's argument layout is what it was.  VehicleFleet (a
// fleet call, ble_fleet): the palette's field-major image is copied into LDS next to the ACS table, and every lane reads the VehicleRt of
// its own entry from there once, after the barrier; from then on the lane flies what the VehicleRt instantiation flies, in vector
// registers instead of scalar ones (profiles/fleet_resource_usage.txt).
template <bool kNoise, class V = VehicleDefault>
__global__ __launch_bounds__(kStepBlock) void ble_step_kernel(StateDev st, const uint8_t* __restrict__ action,
                                                          const float* __restrict__ wind_grid,
                                                          int64_t grid_env_stride,
                                                          const float* __restrict__ noise_uv,
                                                          float* __restrict__ reward,
                                                          uint8_t* __restrict__ terminal,
                                                          uint8_t* __restrict__ effective_action,
                                                          uint32_t* err_flags, unsigned long long* active_count,
                                                          int64_t n, int substeps, int lanes, int n_steps, StepNoise gen, V veh) {
  // `lanes` (64 or 32) = environments per wavefront.  32 leaves the upper half of the wave
  // idle and doubles the number of waves: an occupancy/latency experiment knob.
  // acs_poly: the ACS table's piecewise cubics; term_save: where a lane parks the state its episode ended with (agent_step), one block
  // per wave
  double* acs_poly; float* term_save; float* grad_lut = nullptr; uint32_t* noise_draws = nullptr;
  if constexpr (kNoise) {
    __shared__ StepNoiseShared shm;
    acs_poly = shm.acs_poly; term_save = shm.term_save; grad_lut = shm.grad_lut; noise_draws = shm.draws;
  } else {
    __shared__ double acs_poly_lds[kAcsPolyDoubles];
    __shared__ float term_save_lds[kTermSaveRows * kStepBlock];
    acs_poly = acs_poly_lds; term_save = term_save_lds;
  }
  constexpr bool kFleet = IsFleet<V>::value;
  double* fleet_lds = nullptr;
  if constexpr (kFleet) {
    __shared__ double fleet_lds_[kFleetRtFields * kFleetMaxVehicles];
    fleet_lds = fleet_lds_;
  }
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int64_t i = ((int64_t)blockIdx.x * (kStepBlock / 64) + wave) * lanes + lane;
  const bool in_range = i < n && lane < lanes;
  uint32_t flags = 0;
  EnvRegs s;
  EnvConst c;
  EpisodeCacheRow cached = {};
  bool live = false;
  BLE_STEP_INSTR_BEGIN();
  if (in_range) {
    // every load is issued up front, unconditionally (one memory round trip)
    s.status = st.status[i];
    s.x = st.x[i]; s.y = st.y[i]; s.p = st.pressure[i]; s.t_amb = st.ambient_temperature[i];
    s.t_int = st.internal_temperature[i]; s.vol = st.envelope_volume[i]; s.sp = st.superpressure[i];
    s.n_air = st.mols_air[i]; s.batt = st.battery_charge[i];
    s.acs_power = 0.0f; s.mdot = 0.0f; s.charge = 0.0f; s.load = 0.0f;
    s.t_elapsed = st.time_elapsed_s[i]; s.sunrise_h = st.sunrise_h_rel[i]; s.sunset = st.sunset_rel[i];
    s.alt_fsm = st.alt_fsm[i]; s.env_fsm = st.env_fsm[i]; s.paused = st.power_paused[i];
    c.lat0_deg = st.center_lat_deg[i]; c.lng0_deg = st.center_lng_deg[i];
    c.ir = st.upwelling_infrared[i]; c.alpha = st.alpha[i]; c.start_unix = st.start_unix[i];
    if (st.episode_cache != nullptr) cached = episode_cache_load(st.episode_cache, n, i);
    live = s.status == kOk;
  }
  int vidx = 0;             // (a fleet) the palette entry of this lane's environment
  if constexpr (kFleet) {
    if (in_range) {
      vidx = veh.index[i];
      if (vidx >= veh.n_vehicles) {          // frozen like a non-OK lane, reads entry 0 (nothing outside the palette)
        flags |= kFlagVehicleIndex;
        live = false;
        vidx = 0;
      }
    }
    for (int j = (int)threadIdx.x; j < kFleetRtFields * kFleetMaxVehicles; j += kStepBlock) fleet_lds[j] = (&veh.f[0][0])[j];
  }
  // the ACS table's piecewise cubics: a compile-time table, constant memory -> LDS (the loop reads it by a per-lane index)
  for (int j = (int)threadIdx.x; j < kAcsPolyDoubles; j += kStepBlock) acs_poly[j] = kAcsPoly.c[j];
  if (kNoise) grad_lut_fill(grad_lut, (int)threadIdx.x, kStepBlock);
  BLE_STEP_MARK(1);
  __syncthreads();
  BLE_STEP_MARK(2);
  const bool was_live = live;
  int last_act = 0;
  const auto& lveh = lane_vehicle(veh, fleet_lds, vidx);      // the vehicle argument itself, or (a fleet) this lane's palette entry
  EnvHoisted hc;
  if (live) {
    // per-episode constants: from the cache unless its entry belongs to other constants (then: recompute, store)
    if (st.episode_cache != nullptr && episode_cache_hit(cached, c)) {
      hc = hoisted_from_cache(cached, c);
    } else {
      hc = hoist_constants(c);
      if (st.episode_cache != nullptr) episode_cache_store(st.episode_cache, n, i, c, hc);
    }
  }
  if (kNoise && in_range)
    noise_draws_fetch(gen.seed, (uint64_t)i, (uint64_t)(i + gen.env_offset), gen.episode ? gen.episode[i] : 0u, gen.harmonic_cache, n,
                      noise_draws + threadIdx.x, kStepBlock);
  const StrideK K = stride_k_vreg(lveh.dry_mass, lveh.lift, lveh.v0);      // the stride loop's fp64 constants as register pairs, once per launch (see d_vreg)
  BLE_STEP_MARK(3);
#pragma unroll 1
  for (int k = 0; k < n_steps; ++k) {
    const int64_t o = (int64_t)k * n + i;
    if (live) {
      const int act = action[o];
      last_act = act;
      // wind at the PRE-step position/time (balloon_arena.py:194,270-275): gather now, blend later
      const WindQuery wq = wind_query(s.x, s.y, s.p, s.t_elapsed);
      WindCorners corners;
      wind_gather(wind_grid + i * grid_env_stride, wq, &corners);
      float nu = 0.0f, nv = 0.0f;
      if (kNoise) {
        wind_noise_from_rows(s.x, s.y, s.p, s.t_elapsed, noise_draws + threadIdx.x, kStepBlock, grad_lut, &nu, &nv);
        // the noise is a VALUE here as it is between ble_wind_noise_f32 and ble_step_f32: without this the compiler is free to
        // fuse the generator's last multiplication into agent_step's `u += noise_u` (one rounding instead of two)
        asm volatile("" : "+v"(nu), "+v"(nv));
      } else if (noise_uv) { nu = noise_uv[2 * i]; nv = noise_uv[2 * i + 1]; }
      float r;
      const int eff = agent_step(s, c, hc, act, corners, wq, nu, nv, substeps, acs_poly, K, term_save + wave * (kTermSaveRows * kTermSaveStride) + lane, &r, &flags, lveh);
      if (!(isfinite(s.p) && isfinite(s.t_int) && isfinite(s.x) && isfinite(s.y) && isfinite(s.batt)))
        flags |= kFlagNonFinite;
      reward[o] = r;
      terminal[o] = s.status != kOk;
      if (effective_action) effective_action[o] = (uint8_t)eff;
    } else if (in_range) {  // balloon.py:288-290 raises; a vectorised env freezes the lane instead
      reward[o] = 0.0f;
      terminal[o] = 1;
      if (effective_action) effective_action[o] = action[o];
    }
    // live-environment count: one atomic per wave, spread over BLE_COUNT_SLOTS addresses and
    // issued after the step so that no load of this wave queues behind it
    if (BLE_STEP_COUNTS_LIVE && active_count) {
      const unsigned long long m = __ballot(live);
      if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(active_count + (int64_t)k * BLE_COUNT_SLOTS + (blockIdx.x & (BLE_COUNT_SLOTS - 1)),
                  (unsigned long long)__popcll(m));
    }
    live = live && s.status == kOk;
    BLE_STEP_STEP_DONE(k);
  }
  BLE_STEP_MARK(4);
  if (was_live) {
    st.x[i] = s.x; st.y[i] = s.y; st.pressure[i] = s.p; st.ambient_temperature[i] = s.t_amb;
    st.internal_temperature[i] = s.t_int; st.envelope_volume[i] = s.vol; st.superpressure[i] = s.sp;
    st.mols_air[i] = s.n_air; st.battery_charge[i] = s.batt;
    st.acs_power[i] = s.acs_power; st.acs_mass_flow[i] = s.mdot; st.solar_charging[i] = s.charge;
    st.power_load[i] = s.load;
    st.time_elapsed_s[i] = s.t_elapsed; st.sunrise_h_rel[i] = s.sunrise_h; st.sunset_rel[i] = s.sunset;
    st.status[i] = s.status; st.last_command[i] = (uint8_t)last_act;
    st.alt_fsm[i] = s.alt_fsm; st.env_fsm[i] = s.env_fsm; st.power_paused[i] = s.paused;
  }
  BLE_STEP_INSTR_END();
  report_flags(flags, err_flags);
}

// The one-lane transition with a helper wave (ble_step_helper.h): 512-thread workgroups, two waves per SIMD -- M, the lane's environment
// minus the solar block, and S, its sun.  One instantiation: no in-kernel noise, the default vehicle.  M below is ble_step_kernel's body
// without its noise, fleet and clock-mark parts (the timing build instruments the one-lane kernel only).  The two bodies are kept as text
// on purpose: moving the state load, the per-episode constants and the state store into functions shared by both changed the register
// allocation and schedule of all six ble_step_kernel instantiations (profiles/isa_compare.py), which needs a timing run of every leg to accept.
__global__ __launch_bounds__(kHelperBlock) void ble_step_helper_kernel(StateDev st, const uint8_t* __restrict__ action,
                                                                     const float* __restrict__ wind_grid, int64_t grid_env_stride,
                                                                     const float* __restrict__ noise_uv, float* __restrict__ reward,
                                                                     uint8_t* __restrict__ terminal, uint8_t* __restrict__ effective_action,
                                                                     uint32_t* err_flags, unsigned long long* active_count, int64_t n,
                                                                     int substeps, int n_steps) {
  __shared__ HelperShared sh;
  __shared__ double acs_poly[kAcsPolyDoubles];
  __shared__ float term_save[kTermSaveRows * kTermSaveStride * kHelperGroups];
  const int hw_wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  for (int j = (int)threadIdx.x; j < kAcsPolyDoubles; j += kHelperBlock) acs_poly[j] = kAcsPoly.c[j];
  const int role = helper_assign_roles(sh, hw_wave, lane);      // (its barriers cover the table)
  const int group = role >> 1;
  HelperGroupShared* const g = &sh.group[group];
  const int64_t i = ((int64_t)blockIdx.x * kHelperGroups + group) * 64 + lane;
  const bool in_range = i < n;
  if (role & 1) {
    helper_wave(st, g, lane, i, in_range, substeps, n_steps);
    return;
  }
  uint32_t flags = 0;
  EnvRegs s;
  EnvConst c;
  EpisodeCacheRow cached = {};
  bool live = false;
  if (in_range) {
    s.status = st.status[i];
    s.x = st.x[i]; s.y = st.y[i]; s.p = st.pressure[i]; s.t_amb = st.ambient_temperature[i];
    s.t_int = st.internal_temperature[i]; s.vol = st.envelope_volume[i]; s.sp = st.superpressure[i];
    s.n_air = st.mols_air[i]; s.batt = st.battery_charge[i];
    s.acs_power = 0.0f; s.mdot = 0.0f; s.charge = 0.0f; s.load = 0.0f;
    s.t_elapsed = st.time_elapsed_s[i]; s.sunrise_h = st.sunrise_h_rel[i]; s.sunset = st.sunset_rel[i];
    s.alt_fsm = st.alt_fsm[i]; s.env_fsm = st.env_fsm[i]; s.paused = st.power_paused[i];
    c.lat0_deg = st.center_lat_deg[i]; c.lng0_deg = st.center_lng_deg[i];
    c.ir = st.upwelling_infrared[i]; c.alpha = st.alpha[i]; c.start_unix = st.start_unix[i];
    if (st.episode_cache != nullptr) cached = episode_cache_load(st.episode_cache, n, i);
    live = s.status == kOk;
  }
  const bool was_live = live;
  int last_act = 0;
  EnvHoisted hc;
  if (live) {
    if (st.episode_cache != nullptr && episode_cache_hit(cached, c)) {
      hc = hoisted_from_cache(cached, c);
    } else {
      hc = hoist_constants(c);
      if (st.episode_cache != nullptr) episode_cache_store(st.episode_cache, n, i, c, hc);
    }
  }
  const StrideK K = stride_k_vreg();
  HelperMain hm{g, lane, 0, 0, 0};
#pragma unroll 1
  for (int k = 0; k < n_steps; ++k) {
    const int64_t o = (int64_t)k * n + i;
    const bool any_live = wave_any(live);
    hm.steps_done = k + 1;                     // (scalar, whole wave: what this step's publication stores, whichever lanes make it)
    if (live) {
      const int act = action[o];
      last_act = act;
      const WindQuery wq = wind_query(s.x, s.y, s.p, s.t_elapsed);
      WindCorners corners;
      wind_gather(wind_grid + i * grid_env_stride, wq, &corners);
      float nu = 0.0f, nv = 0.0f;
      if (noise_uv) { nu = noise_uv[2 * i]; nv = noise_uv[2 * i + 1]; }
      float r;
      const int eff = agent_step(s, c, hc, act, corners, wq, nu, nv, substeps, acs_poly, K, term_save + group * (kTermSaveRows * kTermSaveStride) + lane,
                                 &r, &flags, VehicleDefault(), &hm);
      if (!(isfinite(s.p) && isfinite(s.t_int) && isfinite(s.x) && isfinite(s.y) && isfinite(s.batt)))
        flags |= kFlagNonFinite;
      reward[o] = r;
      terminal[o] = s.status != kOk;
      if (effective_action) effective_action[o] = (uint8_t)eff;
    } else if (in_range) {
      reward[o] = 0.0f;
      terminal[o] = 1;
      if (effective_action) effective_action[o] = action[o];
    }
    if (!any_live) hm.publish_idle();          // S waits for every step's publication
    if (BLE_STEP_COUNTS_LIVE && active_count) {
      const unsigned long long m = __ballot(live);
      if (lane == 0 && m)
        atomicAdd(active_count + (int64_t)k * BLE_COUNT_SLOTS + (blockIdx.x & (BLE_COUNT_SLOTS - 1)), (unsigned long long)__popcll(m));
    }
    live = live && s.status == kOk;
  }
  if (was_live) {
    st.x[i] = s.x; st.y[i] = s.y; st.pressure[i] = s.p; st.ambient_temperature[i] = s.t_amb;
    st.internal_temperature[i] = s.t_int; st.envelope_volume[i] = s.vol; st.superpressure[i] = s.sp;
    st.mols_air[i] = s.n_air; st.battery_charge[i] = s.batt;
    st.acs_power[i] = s.acs_power; st.acs_mass_flow[i] = s.mdot; st.solar_charging[i] = s.charge;
    st.power_load[i] = s.load;
    st.time_elapsed_s[i] = s.t_elapsed; st.sunrise_h_rel[i] = s.sunrise_h; st.sunset_rel[i] = s.sunset;
    st.status[i] = s.status; st.last_command[i] = (uint8_t)last_act;
    st.alt_fsm[i] = s.alt_fsm; st.env_fsm[i] = s.env_fsm; st.power_paused[i] = s.paused;
  }
  report_flags(flags, err_flags);
}

// The same transition for small batches: one environment on the four wavefronts of a 256-thread workgroup (ble_step_split.h).
// Launch bound: two waves per SIMD, what BLE_SPLIT_MAX_ENVS environments put there; three / four spill (profiles/HISTORY.md).
template <bool kNoise>
__global__ __launch_bounds__(kSplitWaves * kSplitLanes, 2) void ble_step_split_kernel(SplitArgs a) {
  __shared__ SplitShared sh;
  __shared__ SplitNoiseShared<kNoise> shn;
  uint32_t flags;
  switch (__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6)) {       // (scalar: one role per wave)
    case 0: flags = split_agent_steps<0, kNoise>(a, sh, shn); break;
    case 1: flags = split_agent_steps<1, kNoise>(a, sh, shn); break;
    case 2: flags = split_agent_steps<2, kNoise>(a, sh, shn); break;
    default: flags = split_agent_steps<3, kNoise>(a, sh, shn); break;
  }
  report_flags(flags, a.err_flags);
}

__global__ __launch_bounds__(256) void ble_forecast_kernel(const float* __restrict__ wind_grid,
                                                           int64_t grid_env_stride, const float* __restrict__ x,
                                                           const float* __restrict__ y,
                                                           const float* __restrict__ pressure,
                                                           const int32_t* __restrict__ elapsed, float* __restrict__ u,
                                                           float* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  // float32 query, fp64 interpolation like scipy's interpn; the float32 result is the correctly rounded reference value
  // (the transition's own, fused lookup blends in fp32: wind_blend_corners)
  double uu, vv;
  wind_forecast_f64(wind_grid + i * grid_env_stride, x[i], y[i], pressure[i], elapsed[i], &uu, &vv);
  u[i] = (float)uu; v[i] = (float)vv;
}

// get_forecast_column (grid_based_wind_field.py:96-132): one wave per column.  The wave
// first collapses the (x, y, t) axes: lanes 0..19 each own one (pressure node, component)
// and blend its 8 (x, y, t) corners -- the "local pressure column" -- into LDS; then every
// lane interpolates its pressure levels from the 10-node column held in LDS.
__global__ __launch_bounds__(kBlock) void ble_forecast_column_kernel(
    const float* __restrict__ wind_grid, int64_t grid_env_stride, const float* __restrict__ x,
    const float* __restrict__ y, const int32_t* __restrict__ elapsed, const float* __restrict__ levels,
    int n_levels, float* __restrict__ out_uv, int64_t n) {
  __shared__ double column[BLE_GRID_NP * 2];
  const int64_t env = blockIdx.x;
  if (env >= n) return;
  const int lane = threadIdx.x;
  const WindQueryD wq = wind_query_xyt_f64(x[env], y[env], elapsed[env]);
  const float* grid = wind_grid + env * grid_env_stride;
  if (lane < BLE_GRID_NP * 2) {
    const int ip = lane >> 1, comp = lane & 1;
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const double w = ((a ? wq.wx : 1.0 - wq.wx) * (b ? wq.wy : 1.0 - wq.wy)) * (d ? wq.wt : 1.0 - wq.wt);
          acc = d_fma((double)grid[((((wq.ix + a) * 21 + (wq.iy + b)) * 10 + ip) * 9 + (wq.it + d)) * 2 + comp], w, acc);
        }
    column[lane] = acc;
  }
  __syncthreads();
  for (int l = lane; l < n_levels; l += kBlock) {
    const float p = f_clamp(levels[l], 5000.0f, 14000.0f);
    int ip = (int)((p - 5000.0f) * (1.0f / 1000.0f));
    ip = ip > 8 ? 8 : ip;
    const double wp = ((double)p - (5000.0 + 1000.0 * (double)ip)) * 1e-3;
    const double u = d_fma(wp, column[(ip + 1) * 2] - column[ip * 2], column[ip * 2]);
    const double v = d_fma(wp, column[(ip + 1) * 2 + 1] - column[ip * 2 + 1], column[ip * 2 + 1]);
    out_uv[(env * n_levels + l) * 2] = (float)u;
    out_uv[(env * n_levels + l) * 2 + 1] = (float)v;
  }
}

// ble_state_rows_f64: struct of arrays -> records of BLE_ROW_DOUBLES doubles, the struct's member order
__global__ __launch_bounds__(64) void ble_state_rows_kernel(StateDev st, int64_t first, int64_t count, double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= count) return;
  const int64_t i = first + r;
  double* o = out + r * BLE_ROW_DOUBLES;
  o[0] = st.x[i]; o[1] = st.y[i]; o[2] = st.pressure[i]; o[3] = st.ambient_temperature[i]; o[4] = st.internal_temperature[i];
  o[5] = st.envelope_volume[i]; o[6] = st.superpressure[i]; o[7] = st.mols_air[i]; o[8] = st.battery_charge[i];
  o[9] = st.acs_power[i]; o[10] = st.acs_mass_flow[i]; o[11] = st.solar_charging[i]; o[12] = st.power_load[i];
  o[13] = st.center_lat_deg[i]; o[14] = st.center_lng_deg[i]; o[15] = st.upwelling_infrared[i]; o[16] = st.alpha[i];
  o[17] = (double)st.start_unix[i]; o[18] = (double)st.time_elapsed_s[i]; o[19] = (double)st.sunrise_h_rel[i]; o[20] = (double)st.sunset_rel[i];
  o[21] = (double)st.status[i]; o[22] = (double)st.last_command[i]; o[23] = (double)st.alt_fsm[i]; o[24] = (double)st.env_fsm[i];
  o[25] = (double)st.power_paused[i];
}

__global__ __launch_bounds__(256) void ble_power_table_kernel(const float* __restrict__ pr,
                                                              const float* __restrict__ soc, float* __restrict__ watts,
                                                              uint32_t* err_flags, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t flags = 0;
  if (i < n) watts[i] = power_table_lookup(pr[i], soc[i], &flags);
  report_flags(flags, err_flags);
}

// ---- probes: the same lane functions, one element per lane ----
__global__ __launch_bounds__(256) void probe_atmosphere_kernel(const float* alpha, const float* pressure, float* height,
                                                               float* temperature, uint32_t* err_flags, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t flags = 0;
  if (i < n) {
    const double p = (double)pressure[i];
    const AtmWindow w = atm_window((double)alpha[i], p, &flags);
    double h, t;
    atm_at_pressure_f64(w, (double)alpha[i], p, &h, &t);
    height[i] = (float)h; temperature[i] = (float)t;
  }
  report_flags(flags, err_flags);
}
__global__ __launch_bounds__(256) void probe_at_height_kernel(const float* alpha, const double* height, double* pressure, double* temperature,
                                                              uint32_t* err_flags, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t flags = 0;
  if (i < n) atm_at_height_f64((double)alpha[i], height[i], &pressure[i], &temperature[i], &flags);
  report_flags(flags, err_flags);
}
__global__ __launch_bounds__(256) void probe_solar_kernel(const float* lat0, const float* lng0, const float* x,
                                                          const float* y, const int64_t* unix_s, float* el_deg,
                                                          float* flux, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Ephemeris e = ephemeris(unix_s[i]);
  int64_t sod = unix_s[i] % 86400;
  if (sod < 0) sod += 86400;
  const double b = (double)sod * (1.0 / 240.0) + 0.25 * e.eot_min + (double)lng0[i];
  double sl, cl;
  sincos_f64((double)lat0[i] * (kPiD / 180.0), &sl, &cl);
  double sb, cb;
  sincos_f64(b * (kPiD / 180.0), &sb, &cb);
  const double oms = sun_one_minus_sin_f64(sl, cl, (double)x[i], (double)y[i], sb, cb, (double)e.sin_decl, (double)e.cos_decl);
  const SunSC sun = sun_refract(sun_from_one_minus_sin((float)oms));
  el_deg[i] = atan2f(sun.sin_el, sun.cos_el) * kRadToDeg;
  flux[i] = e.flux;
}
// BalloonState.latlng (balloon.py:217-220 -> spherical_geometry.py:44-76): the latlng_f64 the observation and the exact solar
// chain evaluate, as degrees
__global__ __launch_bounds__(256) void probe_latlng_kernel(const float* lat0, const float* lng0, const float* x, const float* y,
                                                           double* lat_deg, double* lng_deg, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double sl, cl, lng;
  latlng_f64((double)lat0[i], (double)lng0[i], (double)x[i], (double)y[i], &sl, &cl, &lng);
  lat_deg[i] = asin(sl) * (180.0 / kPiD);          // (libm: the probe reports degrees to 1e-12; the kernels use sin / cos directly)
  lng = lng - 360.0 * floor((lng + 180.0) * (1.0 / 360.0));             // s2 LatLng.normalized(): [-180, 180)
  lng_deg[i] = lng;
}
__global__ __launch_bounds__(256) void probe_solar_power_kernel(const float* el_deg, const float* pressure, float* att,
                                                                float* power, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s, c;
  sincos_f64((double)el_deg[i] * (kPiD / 180.0), &s, &c);
  // thresholds decided on the fp64 input elevation, as the transition's exact path does
  const double el = (double)el_deg[i];
  SunState sun;
  sun.sin_el = (float)s; sun.cos_el = (float)c;
  sun.day = !(el < -4.242); sun.sh33 = el >= 37.738149050524044; sun.sh27 = el >= 34.39486500086289;
  const float a = solar_attenuation(sun.sin_el, pressure[i], sun.day);
  att[i] = a;
  power[i] = solar_power(sun, a);
}
__global__ __launch_bounds__(256) void probe_thermal_kernel(const float* volume, const float* t_int, const float* t_amb,
                                                            const float* pressure, const float* el_deg,
                                                            const float* flux, const float* ir, float* dtdt,
                                                            uint32_t* err_flags, int64_t n, double thermal_scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t flags = 0;
  if (i < n) {
    double s, c;
    sincos_f64((double)el_deg[i] * (kPiD / 180.0), &s, &c);
    const float att = solar_attenuation((float)s, pressure[i], !((double)el_deg[i] < -4.242));
    const double vol = (double)volume[i];
    double yc = (double)f_exp2((-1.0f / 3.0f) * f_log2(volume[i]));
    yc = yc * d_fma(-vol * yc, yc * yc, 4.0) * (1.0 / 3.0);
    flags |= absorptivity_out_of_range((double)t_int[i]) ? kFlagAbsorptivity : 0u;
    dtdt[i] = (float)(0.1 * thermal_increment_f64(vol, yc, (double)t_int[i], (double)t_amb[i], (double)pressure[i],
                                                  (double)((flux[i] * att) * (0.25f * kSolarAbsorptivityTotal)),
                                                  earth_heat_per_area_f64((double)ir[i], &flags), stride_k_literal(), thermal_scale));
  }
  report_flags(flags, err_flags);
}
__global__ __launch_bounds__(256) void probe_sp_volume_kernel(const float* mols_air, const float* t_int,
                                                              const float* pressure, float* volume, float* sp,
                                                              int64_t n, double lift, double v0, double dvdp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double v, s;
  superpressure_volume_f64((double)mols_air[i], (double)t_int[i], (double)pressure[i], d_rcp((double)pressure[i]), &v, &s,
                           stride_k_literal(VehicleDefault::dry_mass, lift, v0), dvdp, 4.0 * dvdp, 1.0 / dvdp);
  volume[i] = (float)v; sp[i] = (float)s;
}
__global__ __launch_bounds__(256) void probe_acs_kernel(const float* pr, float* power, float* eff, float* mdot,
                                                        int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  // power and mass flow through the transition's piecewise-cubic form, the efficiency through the two-table form
  const double prm1 = (double)pr[i] - 1.0;
  double w, md;
  acs_down_poly(kAcsPoly.c, prm1, &w, &md);       // the compile-time table the transition copies into LDS
  power[i] = (float)w; eff[i] = (float)acs_efficiency_f64(kAcsEfficiency, prm1, acs_power_f64(prm1)); mdot[i] = (float)md;
}

// The three safety layers one at a time (ble_probe_safety_f32): the lane functions of agent_step on their own state bytes.
__global__ __launch_bounds__(256) void probe_safety_kernel(int layer, const uint8_t* action, const float* value,
                                                           const float* alpha, int32_t* clocks, double night_load_w,
                                                           double capacity_wh, uint8_t* fsm, uint8_t* effective,
                                                           uint32_t* err_flags, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t flags = 0;
  if (i < n) {
    uint8_t state = fsm[i];
    int eff;
    if (layer == 0) {                               // value = pressure: the altitude the transition compares (fp64)
      const double p = (double)value[i];
      const AtmWindow w = atm_window((double)alpha[i], p, &flags);
      double h, t;
      atm_at_pressure_f64(w, (double)alpha[i], p, &h, &t);
      eff = altitude_safety(action[i], h, &state);
    } else if (layer == 1) {                        // value = superpressure
      eff = envelope_safety(action[i], value[i], &state, alpha != nullptr ? (double)alpha[i] : VehicleDefault::max_sp);     // (ABI 5: `alpha` = the layer's maximum superpressure)
    } else {                                        // value = battery charge; clocks (now, sunrise + 1/2 h, sunset)
      int32_t sr = clocks[3 * i + 1], ss = clocks[3 * i + 2];
      eff = power_safety(action[i], clocks[3 * i], value[i], &sr, &ss, &state, night_load_w, capacity_wh);
      clocks[3 * i + 1] = sr; clocks[3 * i + 2] = ss;
    }
    fsm[i] = state; effective[i] = (uint8_t)eff;
  }
  report_flags(flags, err_flags);
}

// Decoder tail of the wind-field VAE (generative/vae.py:149-186): flow fields psi [n][7][7][90]
// (the last Dense layer's output, flow-field index fastest) -> half-pixel linear resize to
// 23 x 23 (jax.image.resize 'linear': triangle kernel, edge weights renormalised == clamped
// taps) -> central differences u = d psi / dy, v = -d psi / dx on the interior 21 x 21 ->
// the wind grid [n][21][21][10][9][2] the step kernel reads (grid_env_stride = 79 380).
// HBM-write-bound: 317.5 KB written per env against 17.6 KB read.  One workgroup = one environment, 4 groups of 90 threads
// (one per flow field; 24 idle): psi (17.6 KB) is staged in LDS, resized along the second axis once (P[7][23][90], 58 KB: the
// `lo` / `hi` of decode_resized, which depend on the source row alone), and every output row is then produced with the
// first-axis interpolation on the fly, the middle row's lattice points sliding through registers: 6 LDS reads per output and
// no integer division in the loops, against the 16 cached global loads + 4 divisions of the one-thread-per-output form (bound
// by its load issue rate at 1.6 TB/s of writes).  Stores: 720 contiguous bytes per 90 threads.  Same arithmetic, bit for bit.
#ifndef BLE_DECODE_GROUPS
#define BLE_DECODE_GROUPS 6          // (A/B knob of profiles/decode_ab.py: 4 .. 11 groups measured, 6 is the fastest)
#endif
constexpr int kDecodeGroups = BLE_DECODE_GROUPS, kDecodeThreads = (90 * kDecodeGroups + 63) / 64 * 64;
__global__ __launch_bounds__(kDecodeThreads) void ble_decode_flow_kernel(const float* __restrict__ flow, float* __restrict__ grid,
                                                                         int64_t n) {
  __shared__ float psi[7 * 7 * 90];
  __shared__ float part[7 * 23 * 90];        // psi resized along its second axis
  __shared__ int tap0[23];
  __shared__ float w1[23];
  const int64_t env = blockIdx.x;
  if (threadIdx.x < 23) resize_tap((int)threadIdx.x, &tap0[threadIdx.x], &w1[threadIdx.x]);
  for (int t = threadIdx.x; t < 7 * 7 * 90; t += kDecodeThreads) psi[t] = flow[env * (7 * 7 * 90) + t];
  __syncthreads();
  const int f = (int)threadIdx.x % 90, g = (int)threadIdx.x / 90;
  // the threads beyond the last group of 90 (kDecodeThreads rounds up to whole waves) run neither loop but DO reach the
  // barrier: their loops start at the end, there is no early return
  const int g_step = g < kDecodeGroups ? kDecodeGroups : 1;
  for (int rb = g < kDecodeGroups ? g : 7 * 23; rb < 7 * 23; rb += g_step) {
    const int r = rb / 23, b = rb - 23 * r;
    const int b0 = tap0[b], b_lo = b0 < 0 ? 0 : b0, b_hi = b0 + 1 > 6 ? 6 : b0 + 1;
    const float lo = psi[(r * 7 + b_lo) * 90 + f];
    part[rb * 90 + f] = f_fma(w1[b], psi[(r * 7 + b_hi) * 90 + f] - lo, lo);
  }
  __syncthreads();
  float2* out = reinterpret_cast<float2*>(grid + env * (int64_t)(21 * 21 * 90 * 2)) + f;
  for (int i = g < kDecodeGroups ? g : 21; i < 21; i += g_step) {
    // first-axis taps of the lattice rows i, i + 1, i + 2
    int lo_row[3], hi_row[3]; float wa[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int a0 = tap0[i + k];
      lo_row[k] = (a0 < 0 ? 0 : a0) * (23 * 90) + f; hi_row[k] = (a0 + 1 > 6 ? 6 : a0 + 1) * (23 * 90) + f; wa[k] = w1[i + k];
    }
    auto point = [&](int k, int b) {           // decode_resized's last line on the staged lo / hi
      const float lo = part[lo_row[k] + b * 90];
      return f_fma(wa[k], part[hi_row[k] + b * 90] - lo, lo);
    };
    float mid0 = point(1, 0), mid1 = point(1, 1);
    float2* row = out + (int64_t)i * (21 * 90);
#pragma unroll 3
    for (int j = 0; j < 21; ++j) {
      const float mid2 = point(1, j + 2);
      float u, v;
      decode_flow_from_lattice(point(2, j + 1), point(0, j + 1), mid2, mid0, &u, &v);
      row[j * 90] = make_float2(u, v);          // (non-temporal stores measured: 3.8 ms against 3.0 for 32 768 grids)
      mid0 = mid1; mid1 = mid2;
    }
  }
}

// Where a lane's Philox streams come from.  ScalarSeed: one seed for the batch, streams keyed by the GLOBAL environment index
// (env_offset + i).  EnvSeed: a seed per environment, every stream keyed as environment 0 -- environment i draws what environment 0 of
// a one-environment batch with seed env_seed[i] draws (an evaluation's seed flies the same episode in any batch, at any position).
struct ScalarSeed {
  unsigned long long seed;
  static constexpr bool kPerEnv = false;
  __device__ __forceinline__ uint64_t of(int64_t) const { return seed; }
  __device__ __forceinline__ uint64_t key(int64_t i, int64_t env_offset) const { return (uint64_t)(i + env_offset); }
};
struct EnvSeed {
  const unsigned long long* __restrict__ seed;
  static constexpr bool kPerEnv = true;
  __device__ __forceinline__ uint64_t of(int64_t i) const { return seed[i]; }
  __device__ __forceinline__ uint64_t key(int64_t, int64_t) const { return 0; }
};

// mode 0: the wind noise (u, v) of every environment at its (x, y, pressure, elapsed);
// mode 1 (test probe): noise_uv[2 i] = simplex4(x, y, pressure, elapsed as float, seed) -- raw primitive.
// EnvSeed: the harmonic cache is not used (its entries are keyed by (seed, episode), not by the stream's environment index).
template <class S = ScalarSeed>
__global__ __launch_bounds__(256) void ble_wind_noise_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ pressure,
                                                             const int32_t* __restrict__ elapsed, S seed,
                                                             const uint32_t* __restrict__ episode, int mode,
                                                             uint32_t* harmonic_cache, float* __restrict__ noise_uv, int64_t n,
                                                             int64_t env_offset) {
  __shared__ __attribute__((aligned(16))) float grad_lut[kGradLutFloats];
  grad_lut_fill(grad_lut, (int)threadIdx.x, 256);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float u, v;
  if (mode == 0) {
    const uint32_t ep = episode ? episode[i] : 0u;
    if (!S::kPerEnv && harmonic_cache != nullptr)
      wind_noise_cached(x[i], y[i], pressure[i], elapsed[i], seed.of(i), (uint64_t)i, seed.key(i, env_offset), ep, harmonic_cache, n, grad_lut,
                        &u, &v);
    else
      wind_noise(x[i], y[i], pressure[i], elapsed[i], seed.of(i), seed.key(i, env_offset), ep, grad_lut, &u, &v);
  } else {
    u = simplex4(x[i], y[i], pressure[i], (float)elapsed[i] * (1.0f / 3600.0f), (uint32_t)seed.of(i), grad_lut);
    v = 0.0f;
  }
  noise_uv[2 * i] = u; noise_uv[2 * i + 1] = v;
}

// Episode reset for the lanes selected by `mask` (all lanes if mask == nullptr).
// sample != 0: draw the initial conditions (utils/sampling.py, balloon_arena.py:228-268) from
// Philox(seed, env, episode[i]); sample == 0: keep x, y, pressure, centre lat/lng, IR, alpha,
// start_unix as they are.  Then the Newton cold start (stable_init.py:132-157), the sunrise /
// sunset search of PowerSafetyLayer.__init__ and fresh clocks / FSMs / battery (balloon.py:175-215).
// VehicleFleet: every lane cold-starts with its own palette entry (staged in LDS as in ble_step_kernel); with sample_index the entry is
// first drawn for the new episode from Philox(seed ^ kFleetDrawKey, env, episode[i]) -- a stream of its own, so the initial conditions
// are the draws of the other instantiations bit for bit.
constexpr unsigned long long kFleetDrawKey = 0xF1EE7C0DEull;
// S: the seed source (ScalarSeed / EnvSeed above).
template <class V = VehicleDefault, class S = ScalarSeed>
__global__ __launch_bounds__(kBlock) void ble_reset_kernel(StateDev st, const uint8_t* __restrict__ mask,
                                                           S seed, uint32_t* episode, int sample,
                                                           uint32_t* err_flags, int64_t n, int64_t env_offset, V veh) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t flags = 0;
  double* fleet_lds = nullptr;
  int vidx = 0;
  bool frozen = false;          // (a fleet) an index outside the palette
  if constexpr (IsFleet<V>::value) {
    __shared__ double fleet_lds_[kFleetRtFields * kFleetMaxVehicles];
    fleet_lds = fleet_lds_;
    for (int j = (int)threadIdx.x; j < kFleetRtFields * kFleetMaxVehicles; j += kBlock) fleet_lds[j] = (&veh.f[0][0])[j];
    __syncthreads();
    if (i < n && (mask == nullptr || mask[i] != 0)) {
      if (sample && veh.sample_index) {
        Philox g = philox_init(seed.of(i) ^ kFleetDrawKey, seed.key(i, env_offset), episode ? episode[i] : 0u);
        vidx = (int)(((uint64_t)philox_u32(g) * (uint64_t)veh.n_vehicles) >> 32);        // uniform in [0, n_vehicles)
        veh.index[i] = (uint8_t)vidx;
      } else {
        vidx = veh.index[i];
        if (vidx >= veh.n_vehicles) {          // the lane is left as it is (its episode counter included)
          flags |= kFlagVehicleIndex;
          frozen = true;
          vidx = 0;
        }
      }
    }
  }
  const auto& lveh = lane_vehicle(veh, fleet_lds, vidx);
  if (i < n && (mask == nullptr || mask[i] != 0) && (!IsFleet<V>::value || !frozen)) {      // (the other carriers: the condition it always was)
    float alpha, x, y, p, lat0, lng0, ir;
    int64_t start;
    if (sample) {
      const uint32_t ep = episode ? episode[i] : 0u;
      if (episode) episode[i] = ep + 1u;
      Philox g = philox_init(seed.of(i), seed.key(i, env_offset), ep);     // ScalarSeed: keyed by the GLOBAL environment index
      alpha = (float)philox_uniform(g);                                                  // standard_atmosphere.py:82
      start = 1293840000LL + (int64_t)(philox_uniform(g) * (double)(1419984000LL - 1293840000LL));   // sampling.py:65-83
      const double ga = philox_gamma(g, 1.2), gb = philox_gamma(g, 2.0);                // Beta(1.2, 2.0)
      const double radius = 200000.0 * (ga / (ga + gb));                                // balloon_arena.py:153-154,246-247
      double sn, cs;
      sincos_f64(2.0 * kPiD * philox_uniform(g), &sn, &cs);
      x = (float)(cs * radius); y = (float)(sn * radius);
      lat0 = (float)(-10.0 + 20.0 * philox_uniform(g));                                 // sampling.py:37-62
      lng0 = (float)(-175.0 + 350.0 * philox_uniform(g));
      // pressure ~ U[6500, P(50 000 ft)]  (sampling.py:86-117; at_height standard_atmosphere.py:89-120, layer 0)
      const double l0 = atm_lapse_f64(0, (double)alpha);
      const double t_h = 300.0 + l0 * (15240.0 - -610.0);
      const double p_max = 108870.8213 * d_pow_fast(t_h / 300.0, -9.80665 / (kAirSpecificGasD * l0));
      p = (float)(6500.0 + (p_max - 6500.0) * philox_uniform(g));
      // upwelling IR: 315 * sigmoid(N(2, 315)), rejected below 225 (sampling.py:120-152, as written)
      double irs = 315.0;
#pragma unroll 1
      for (int it = 0; it < 64; ++it) {
        const double z = 2.0 + 315.0 * philox_normal(g);
        irs = z > 700.0 ? 315.0 : (z < -700.0 ? 0.0 : 315.0 / (1.0 + d_exp_fast(-z)));
        if (irs >= 225.0) break;
      }
      ir = (float)irs;
      const_cast<float*>(st.alpha)[i] = alpha; st.x[i] = x; st.y[i] = y; st.pressure[i] = p;
      const_cast<float*>(st.center_lat_deg)[i] = lat0; const_cast<float*>(st.center_lng_deg)[i] = lng0;
      const_cast<float*>(st.upwelling_infrared)[i] = ir; const_cast<int64_t*>(st.start_unix)[i] = start;
    } else {
      alpha = st.alpha[i]; x = st.x[i]; y = st.y[i]; p = st.pressure[i]; lat0 = st.center_lat_deg[i];
      lng0 = st.center_lng_deg[i]; ir = st.upwelling_infrared[i]; start = st.start_unix[i];
    }
    SunSite site;
    latlng_f64((double)lat0, (double)lng0, (double)x, (double)y, &site.sin_lat, &site.cos_lat, &site.lng_deg);
    double flux;
    const double el = solar_elevation_f64(site.sin_lat, site.cos_lat, site.lng_deg, start, &flux);
    const StableParams sp = stable_params((double)alpha, (double)p, el, flux, (double)ir, &flags, lveh);
    int64_t sunrise, sunset;
    next_sunrise_sunset(site, start, &sunrise, &sunset);
    st.ambient_temperature[i] = (float)sp.t_amb; st.internal_temperature[i] = (float)sp.t_int;
    st.mols_air[i] = (float)sp.mols_air; st.envelope_volume[i] = (float)sp.volume; st.superpressure[i] = (float)sp.sp;
    st.battery_charge[i] = 2905.6f;                                                      // balloon.py:195
    st.acs_power[i] = 0.0f; st.acs_mass_flow[i] = 0.0f; st.solar_charging[i] = 0.0f; st.power_load[i] = 0.0f;
    st.time_elapsed_s[i] = 0;
    st.sunrise_h_rel[i] = (int32_t)(sunrise + 1800 - start);                             // power_safety.py:43-48
    st.sunset_rel[i] = (int32_t)(sunset - start);
    st.status[i] = kOk; st.last_command[i] = kStay; st.alt_fsm[i] = 0; st.env_fsm[i] = 0; st.power_paused[i] = 0;
    if (st.episode_cache != nullptr) {       // what the transition derives from this episode's constants alone
      EnvConst c;
      c.lat0_deg = lat0; c.lng0_deg = lng0; c.ir = ir; c.alpha = alpha; c.start_unix = start;
      episode_cache_store(st.episode_cache, n, i, c, hoist_constants(c));
    }
  }
  report_flags(flags, err_flags);
}

// StationSeekerAgent.pick_action (csrc/ble_agent.h): one wave per environment, four per workgroup.
constexpr int kSeekerBlock = 256;
__global__ __launch_bounds__(kSeekerBlock) void ble_station_seeker_kernel(const float* __restrict__ obs, int64_t stride,
                                                                          uint8_t* __restrict__ action, int32_t* __restrict__ level,
                                                                          double* __restrict__ scores, uint32_t* err_flags, int64_t n) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t i = (int64_t)blockIdx.x * (kSeekerBlock / 64) + (threadIdx.x >> 6);
  if (i >= n) return;                                       // (a whole wave: no barrier follows)
  bool bad;
  const int lv = seeker_best_level(obs + i * stride, lane, scores != nullptr ? scores + i * kSeekerLevels : nullptr, &bad);
  if (lane == 0) {
    action[i] = seeker_action(lv);
    if (level != nullptr) level[i] = lv;
    if (bad && err_flags != nullptr) atomicOr(err_flags, kFlagAgentNoLevel);
  }
}

// eval_agent's per-step bookkeeping (eval_lib.py:157-190) for the environments that are not yet done: one lane per environment.
__global__ __launch_bounds__(256) void ble_eval_accumulate_kernel(StateDev st, const float* __restrict__ reward, ble_eval_acc acc,
                                                                  double radius_m, int step_index, int max_steps, float* __restrict__ path,
                                                                  double battery_capacity_wh, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || acc.done[i]) return;
  const int t = step_index + 1;
  acc.cumulative_reward[i] += (double)reward[i];
  acc.steps_within_radius[i] += within_radius(st.x[i], st.y[i], radius_m) ? 1 : 0;
  acc.final_timestep[i] = t;
  const uint8_t status = st.status[i];
  if (status != kOk) acc.end_status[i] = status;
  if (status != kOk || t == max_steps) acc.done[i] = 1;
  if (path != nullptr) {                                    // SimpleBalloonState.from_balloon_state (eval_lib.py:68-77)
    float* r = path + i * 6;
    r[0] = st.x[i]; r[1] = st.y[i]; r[2] = st.pressure[i]; r[3] = st.superpressure[i]; r[4] = (float)st.time_elapsed_s[i];
    r[5] = (float)((double)st.battery_charge[i] / battery_capacity_wh);
  }
}

}  // namespace
// the look-ahead kernels' one lane body (ble_lookahead.h, through ble_rollout.h) and ble_rollout_kernel (K action plans per environment,
// read-only on the state): here, after kStepBlock, StepNoiseShared and report_flags
#include "ble_rollout.h"
// the fitted WindGP kept on the device, its mean as a lane function, and the look-ahead flown in it: after ble_rollout.h (RolloutArgs)
#include "ble_gp_belief.h"
#include "ble_plan.h"
// plan by beam search: the expand, select and finish kernels of a shared-prefix tree of plans: after ble_plan.h (the key and rank functions)
#include "ble_tree.h"
// scenario winds (a prior draw of the noise field conditioned on the measurements), the look-ahead flown in them and the risk score: after
// ble_gp_belief.h (belief_wave_trip) and ScalarSeed / EnvSeed
#include "ble_scenarios.h"
// the beam search flown in the scenario winds: after ble_tree.h (the arenas) and ble_scenarios.h (the slab, the rollout's LDS)
#include "ble_tree_scenarios.h"
// guided tree search: PUCT over a node pool; after ble_tree.h (the arenas) and ble_gp_belief.h
#include "ble_mcts.h"
// the guided tree search flown in the scenario winds: a node is a group of M scenario nodes; after ble_mcts.h and ble_tree_scenarios.h
#include "ble_mcts_scenarios.h"
// fp64 primitive probe (test-only entry point): op 0 rcp seed, 1 d_rcp, 2 rsq seed, 3 d_rsqrt,
// 4 d_sqrt_fast, 5 d_log_fast, 6 d_exp_fast, 7 sin (sincos_f64), 8 cos (sincos_f64)
__global__ __launch_bounds__(256) void probe_f64_kernel(const double* x, double* y, int op, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  double r = 0.0, t = 0.0;
  switch (op) {
    case 0: r = d_rcp_seed(v); break;
    case 1: r = d_rcp(v); break;
    case 2: r = d_rsq_seed(v); break;
    case 3: r = d_rsqrt(v); break;
    case 4: r = d_sqrt_fast(v); break;
    case 5: r = d_log_fast(v); break;
    case 6: r = d_exp_fast(v); break;
    case 7: sincos_f64(v, &r, &t); break;
    default: sincos_f64(v, &t, &r); break;
  }
  y[i] = r;
}
namespace {
// what a kernel gets of the caller's ble_state_f32: its device pointers (the struct's prefix)
static_assert(sizeof(StateDev) == offsetof(ble_state_f32, vehicle) && offsetof(StateDev, episode_cache) == offsetof(ble_state_f32, episode_cache) &&
              offsetof(StateDev, start_unix) == offsetof(ble_state_f32, start_unix) && offsetof(StateDev, status) == offsetof(ble_state_f32, status),
              "StateDev is ble_state_f32 without its last member");
inline StateDev state_dev(const ble_state_f32* st) {
  StateDev d;
  __builtin_memcpy(&d, st, sizeof d);
  return d;
}
// Below BLE_SPLIT_MAX_ENVS environments the one-lane kernel leaves most SIMDs idle (n / 64 waves on 1 024 SIMDs) and the
// four-wave kernel still fits one wave per SIMD: it is the faster one (bit-identical results).  ble_set_step_form() forces a
// form (A/B runs and the parity test); BLE_STEP_SPLIT=0 / 1 / 4 in the process environment is read ONCE, when the
// library first needs it, as that switch's initial value (it used to be re-read by getenv on every launch: host work on the
// 3 us launch path and a data race with a concurrent setenv).
// g_step_form: -1 not initialised, 0 automatic, 1 / 4 wavefronts per environment, BLE_STEP_FORM_HELPER (12): one lane per environment plus a
// helper wave per 64 of them (ble_step_helper.h; set by ble_set_step_form only, no environment spelling).
std::atomic<int> g_step_form{-1};
inline int step_form_from_environment() {
  const char* e = getenv("BLE_STEP_SPLIT");
  if (e != nullptr && e[0] != 0 && e[1] == 0) {
    if (e[0] == '0') return 1;
    if (e[0] == '1' || e[0] == '4') return 4;
  }
  return 0;
}
inline int step_form() {
  int f = g_step_form.load(std::memory_order_relaxed);
  if (f < 0) {
    int expected = -1;
    const int init = step_form_from_environment();
    g_step_form.compare_exchange_strong(expected, init, std::memory_order_relaxed);
    f = g_step_form.load(std::memory_order_relaxed);
  }
  return f;
}
// The helper form wants a free second wave slot on the SIMD of every 64 environments: ceil(n / 64) <= 4 x the device's CUs.  The count of
// the calling thread's current device, asked of the runtime once per device; a failure is an error of the launch (BLE_E_NO_DEVICE), never
// a quiet choice of another form.
inline int compute_units() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return BLE_E_NO_DEVICE;
  int cus = cached[dev].load(std::memory_order_relaxed);
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return BLE_E_NO_DEVICE;
    cached[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}
// The form a default-vehicle launch of n environments takes: 1 (ble_step_kernel), 4 (ble_step_split_kernel),
// BLE_STEP_FORM_HELPER (ble_step_helper_kernel), or a negative BLE_E_*.  `noise`: with a wind-noise generator (the helper form has no such
// instantiation: the one-lane form flies).
inline int split_waves(int64_t n, bool noise) {
  int f = step_form();
  if (f == 0) {
    if (n <= BLE_SPLIT_MAX_ENVS) return 4;
    if (noise) return 1;
    const int cus = compute_units();
    if (cus < 0) return cus;
    f = (n + 63) / 64 <= 4 * (int64_t)cus ? BLE_STEP_FORM_HELPER : 1;
  }
  return f == BLE_STEP_FORM_HELPER && noise ? 1 : f;
}
// hipGetLastError is per-thread and sticky: an error left behind by an unrelated runtime call
// of the host application (torch probes pointers / peers at start-up) must not be reported as
// ours, so every launch first drains it, and the launch's own status is kept for
// ble_last_hip_error().
thread_local int g_last_hip_error = 0;
// the form of the calling thread's most recent transition launch (ble_last_step_form): 0 before the first one
thread_local int g_last_step_form = 0;
template <class... P, class... A>
int launch_grid(void (*kernel)(P...), dim3 grid, int threads, void* stream, const A&... args) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, (hipStream_t)stream, args...);
  const hipError_t e = hipGetLastError();
  g_last_hip_error = (int)e;
  return e == hipSuccess ? BLE_OK : BLE_E_LAUNCH;
}
// `kernel` over n environments (or elements), `per_block` of them per workgroup of `threads` threads; n == 0 launches nothing
template <class... P, class... A>
int launch(void (*kernel)(P...), int64_t n, int per_block, int threads, void* stream, const A&... args) {
  if (n == 0) return BLE_OK;
  return launch_grid(kernel, dim3((unsigned)((n + per_block - 1) / per_block)), threads, stream, args...);
}
inline bool state_ok(const ble_state_f32* st) {
  if (!st) return false;
  const void* const* p = reinterpret_cast<const void* const*>(st);
  for (size_t k = 0; k < offsetof(ble_state_f32, episode_cache) / sizeof(void*); ++k)      // (episode_cache is optional)
    if (p[k] == nullptr) return false;
  return true;
}

// ble_vehicle (the reference's dataclass fields) -> the derived constants the lane functions evaluate, in double on the host: the same
// expressions VehicleDefault folds at compile time (a vehicle equal to the defaults yields VehicleDefault's numbers bit for bit:
// tests/test_gpu_vehicle.py flies both instantiations side by side).
inline bool vehicle_ok(const ble_vehicle* v) {
  const double fields[] = {v->envelope_volume_base, v->envelope_volume_dv_pressure, v->envelope_mass, v->envelope_max_superpressure, v->envelope_cod,
                           v->payload_mass, v->nighttime_power_load_w, v->daytime_power_load_w, v->acs_valve_hole_diameter_m, v->battery_capacity_wh,
                           v->mols_lift_gas};
  for (double f : fields)
    if (!(f == f) || f - f != 0.0) return false;                                  // NaN / Inf
  return v->envelope_volume_base > 0.0 && v->envelope_volume_dv_pressure > 0.0 && v->envelope_mass > 0.0 && v->envelope_cod > 0.0 &&
         v->envelope_max_superpressure > 300.0 && v->battery_capacity_wh > 0.0 && v->payload_mass >= 0.0 && v->mols_lift_gas >= 0.0 &&
         v->acs_valve_hole_diameter_m >= 0.0 && v->nighttime_power_load_w >= 0.0 && v->daytime_power_load_w >= 0.0;
}
inline VehicleRt make_vehicle_rt(const ble_vehicle* v) {
  VehicleRt r;
  r.v0 = v->envelope_volume_base; r.dvdp = v->envelope_volume_dv_pressure;
  r.four_dvdp = 4.0 * r.dvdp; r.inv_dvdp = 1.0 / r.dvdp;
  r.inv_cbrt_v0 = 1.0 / cbrt(r.v0);
  r.lift = v->mols_lift_gas;
  r.envelope_mass = v->envelope_mass; r.payload_mass = v->payload_mass; r.he_mass = kHeMolarMassD * r.lift;
  r.dry_mass = r.he_mass + r.envelope_mass + r.payload_mass;                     // balloon.py:417-420 without the air term (kDryMassD's order)
  r.max_sp = v->envelope_max_superpressure;
  r.drag_arg = (2.0 * 9.80665 / v->envelope_cod) * (kGasConstantD / kAirMolarMassD);
  r.thermal_scale = 10.0 * 4.0 * kPiD * 0.38483473658887897 / (1500.0 * r.envelope_mass);
  const double d = v->acs_valve_hole_diameter_m;
  r.valve_k = -0.62 * (kPiD * d * d / 4.0);
  r.night_load_d = v->nighttime_power_load_w; r.capacity_d = v->battery_capacity_wh; r.day_load_d = v->daytime_power_load_w;
  r.day_load = (float)r.day_load_d; r.night_load = (float)r.night_load_d; r.capacity = (float)r.capacity_d;
  r.power_layer = v->power_safety_layer_enabled != 0;
  r.inv_capacity = 1.0 / r.capacity_d;
  r.ceiling_target = (r.payload_mass + r.envelope_mass + r.lift * kHeMolarMassD) * kGasConstantD / (kAirMolarMassD * r.v0);
  r.sp_hi = r.max_sp - 250.0;
  return r;
}

// ble_fleet -> the kernels' VehicleFleet: every entry through make_vehicle_rt (the doubles a single-vehicle call derives), transposed into
// the field-major image; entries beyond n_vehicles stay zero and are never read (an index >= n_vehicles freezes its lane).
static_assert(kFleetMaxVehicles == BLE_FLEET_MAX_VEHICLES, "ble_physics.h and ble_abi.h disagree on the fleet size");
inline bool fleet_ok(const ble_state_f32* st, const ble_fleet* f) {
  if (f == nullptr || f->palette == nullptr || f->vehicle_index == nullptr || f->n_vehicles < 1 || f->n_vehicles > BLE_FLEET_MAX_VEHICLES)
    return false;
  if (st->vehicle != nullptr) return false;                // two sources of the vehicle: refused, not merged
  for (int k = 0; k < f->n_vehicles; ++k)
    if (!vehicle_ok(&f->palette[k])) return false;
  return true;
}
inline VehicleFleet make_fleet(const ble_fleet* f) {
  VehicleFleet v;
  __builtin_memset(&v, 0, sizeof v);
  for (int k = 0; k < f->n_vehicles; ++k) {
    const VehicleRt r = make_vehicle_rt(&f->palette[k]);
#define BLE_FLEET_PUT(j, m) v.f[j][k] = (double)r.m;
    BLE_FLEET_RT_FIELDS(BLE_FLEET_PUT)
#undef BLE_FLEET_PUT
  }
  v.index = f->vehicle_index; v.n_vehicles = f->n_vehicles; v.sample_index = f->sample_index != 0;
  return v;
}
// The palette travels as a kernel argument (3 KB).  HIP bounds a launch's argument block by 4 KB; the largest fleet argument lists --
// the transition's and the observation's -- stay below it (a bound on their sizes: every scalar argument counted as 8 bytes).
constexpr size_t kKernargLimit = 4096;
static_assert(sizeof(StateDev) + 12 * 8 + sizeof(StepNoise) + sizeof(VehicleFleet) <= kKernargLimit, "ble_step_kernel<VehicleFleet>'s arguments");
static_assert(sizeof(StateDev) + 10 * 8 + sizeof(GpHistory) + sizeof(VehicleFleet) <= kKernargLimit, "ble_observe_kernel<VehicleFleet>'s arguments");

// The vehicle a call flies, checked and handed to f as the kernels' carrier: VehicleDefault (st->vehicle == NULL: compile-time constants),
// VehicleRt (st->vehicle) or -- for the fleet entry points, kFleet -- VehicleFleet (`fleet`).  A compile-time choice, so that no kernel
// is instantiated for a carrier its entry point cannot fly.
template <bool kFleet, class F>
int with_vehicle(const ble_state_f32* st, const ble_fleet* fleet, F&& f) {
  if constexpr (kFleet) {
    if (!fleet_ok(st, fleet)) return BLE_E_INVALID_ARG;
    return f(make_fleet(fleet));
  } else {
    if (st->vehicle == nullptr) return f(VehicleDefault{});
    if (!vehicle_ok(st->vehicle)) return BLE_E_INVALID_ARG;
    return f(make_vehicle_rt(st->vehicle));
  }
}
// The wind-noise generator of a fused rollout (NULL: none), handed to f as the kernels' kNoise switch and their StepNoise argument
template <class F>
int with_noise(const ble_noise_gen* g, F&& f) {
  if (g == nullptr) return f(std::false_type{}, StepNoise{0ull, nullptr, nullptr, 0ll});
  return f(std::true_type{}, StepNoise{g->seed, g->episode, g->harmonic_cache, (long long)g->env_offset});
}
// ble_gp_history_f32 -> a GpHistory of the ring alone, for the calls that never read the carried factor (whatever its stride, it is none
// of their business); false for a missing array
inline bool gp_ring(const ble_gp_history_f32* hist, GpHistory* h) {
  if (!hist || !hist->xyp || !hist->elapsed_s || !hist->err_uv || !hist->count) return false;
  *h = GpHistory{hist->xyp, hist->elapsed_s, hist->err_uv, hist->count, nullptr, nullptr, 0};
  return true;
}
// ble_gp_history_f32 -> the observation kernel's GpHistory; false for a missing array or a carried factor whose slab is too short or
// misaligned (a slab shorter than the kernel's layout would be overrun, and overlap the next environment's)
inline bool gp_history(const ble_gp_history_f32* hist, GpHistory* h) {
  if (!gp_ring(hist, h)) return false;
  if (hist->chol != nullptr && (hist->n_chol == nullptr || hist->chol_stride < (int64_t)kCholStride || (hist->chol_stride & 1) != 0))
    return false;
  *h = GpHistory{hist->xyp, hist->elapsed_s, hist->err_uv, hist->count, hist->chol, hist->n_chol, hist->chol_stride};
  return true;
}

// ble_step_f32 / ble_step_n_f32 and their fleet forms.  The default vehicle flies the form split_waves picks (read once per launch: a
// concurrent ble_set_step_form cannot split the decision); a run-time vehicle or a fleet flies the one-lane form at every batch size.
// The one-lane kernel gets kBlock (64) environments per wave.
template <bool kFleet>
int launch_step(const ble_state_f32* st, const ble_fleet* fleet, const uint8_t* action, const float* wind_grid, int64_t grid_env_stride,
                const ble_noise_gen* noise, const float* noise_uv, float* reward, uint8_t* terminal, uint8_t* effective_action,
                uint32_t* err_flags, unsigned long long* active_count, int64_t n, int substeps, int n_steps, void* stream) {
  if (!state_ok(st) || !action || !wind_grid || !reward || !terminal || n < 0 || substeps < 1 || substeps > BLE_MAX_SUBSTEPS || n_steps < 0 ||
      grid_env_stride < 0 || (noise != nullptr && noise->env_offset < 0))      // (a negative offset would key other streams than the reset did)
    return BLE_E_INVALID_ARG;
  return with_vehicle<kFleet>(st, fleet, [&](auto veh) {
    if (n == 0 || n_steps == 0) return BLE_OK;
    return with_noise(noise, [&](auto noise_on, StepNoise gen) {
      constexpr bool kNoise = decltype(noise_on)::value;
      if constexpr (std::is_same_v<decltype(veh), VehicleDefault>) {
        const int waves = split_waves(n, kNoise);
        if (waves < 0) return waves;
        g_last_step_form = waves;
        if (waves == BLE_STEP_FORM_HELPER) {
          if constexpr (!kNoise)                  // (split_waves never answers it with noise)
            return launch(ble_step_helper_kernel, n, 64 * kHelperGroups, kHelperBlock, stream, state_dev(st), action, wind_grid, grid_env_stride,
                          noise_uv, reward, terminal, effective_action, err_flags, active_count, n, substeps, n_steps);
        } else if (waves != 1) {
          const SplitArgs a{state_dev(st), action, wind_grid, grid_env_stride, noise_uv, reward, terminal, effective_action, err_flags,
                            active_count, n, substeps, n_steps, gen};
          return launch(ble_step_split_kernel<kNoise>, n, kSplitLanes, kSplitWaves * kSplitLanes, stream, a);
        }
      }
      g_last_step_form = 1;
      return launch(ble_step_kernel<kNoise, decltype(veh)>, n, kBlock * (kStepBlock / 64), kStepBlock, stream, state_dev(st), action,
                    wind_grid, grid_env_stride, noise_uv, reward, terminal, effective_action, err_flags, active_count, n, substeps, kBlock,
                    n_steps, gen, veh);
    });
  });
}
// ble_reset_at_f32 / ble_reset_seeded_f32 / ble_reset_fleet_at_f32: S is the seed (ScalarSeed or EnvSeed)
template <bool kFleet, class S>
int launch_reset(const ble_state_f32* st, const ble_fleet* fleet, const uint8_t* mask, S seed, uint32_t* episode, int sample,
                 uint32_t* err_flags, int64_t env_offset, int64_t n, void* stream) {
  if (!state_ok(st) || n < 0 || env_offset < 0) return BLE_E_INVALID_ARG;
  return with_vehicle<kFleet>(st, fleet, [&](auto veh) {
    return launch(ble_reset_kernel<decltype(veh), S>, n, kBlock, kBlock, stream, state_dev(st), mask, seed, episode, sample, err_flags, n,
                  env_offset, veh);
  });
}
// ble_observe_f32 / _forecast / _live / _forecast_fleet: one workgroup per environment
template <bool kFleet, bool kLiveOnly>
int launch_observe(const ble_state_f32* st, const ble_fleet* fleet, const float* wind_grid, int64_t grid_env_stride,
                   const float* forecast_levels, const float* noise_uv, const uint8_t* reset_mask, const ble_gp_history_f32* hist, int append,
                   float* obs, uint32_t* err_flags, int64_t n, void* stream) {
  GpHistory h;
  if (!state_ok(st) || !wind_grid || !gp_history(hist, &h) || !obs || n < 0 || grid_env_stride < 0) return BLE_E_INVALID_ARG;
  return with_vehicle<kFleet>(st, fleet, [&](auto veh) {
    return launch(ble_observe_kernel<decltype(veh), kLiveOnly>, n, 1, kObsBlock, stream, state_dev(st), wind_grid, grid_env_stride, noise_uv,
                  reset_mask, h, append, obs, err_flags, n, veh, forecast_levels);
  });
}

// ble_gp_belief -> the kernels' BeliefDev; false for a missing array, a slab that is not 16-byte aligned or a stride that is too short or odd
// (a shorter slab would be overrun, an odd stride would misalign every second environment's)
inline bool gp_belief(const ble_gp_belief* belief, BeliefDev* b) {
  if (!belief || !belief->slab || !belief->n_obs || belief->stride < (int64_t)kBeliefDoubles || (belief->stride & 1) != 0 ||
      (reinterpret_cast<uintptr_t>(belief->slab) & 15u) != 0 || belief->n < 0 || belief->n >= 2147483648LL)
    return false;
  *b = BeliefDev{belief->slab, belief->stride, belief->n_obs};
  return true;
}
static_assert(kBeliefDoubles == BLE_GP_BELIEF_DOUBLES, "ble_gp_belief.h and ble_abi.h disagree on the slab");

// ble_gp_scenarios -> the kernels' ScenariosDev; false for a missing array, a scenario count outside 1 .. BLE_SCENARIO_MAX, a slab that is
// not 16-byte aligned or a stride that is too short for that count or odd
inline bool gp_scenarios(const ble_gp_scenarios* scn, ScenariosDev* b) {
  if (!scn || !scn->slab || !scn->n_obs || scn->num < 1 || scn->num > BLE_SCENARIO_MAX || scn->stride < (int64_t)BLE_GP_SCENARIO_DOUBLES(scn->num) ||
      (scn->stride & 1) != 0 || (reinterpret_cast<uintptr_t>(scn->slab) & 15u) != 0 || scn->n < 0 || scn->n >= 2147483648LL)
    return false;
  *b = ScenariosDev{scn->slab, scn->stride, scn->n_obs, scn->num};
  return true;
}
inline bool scenario_gen_ok(const ble_scenario_gen* gen) { return gen != nullptr && gen->env_offset >= 0; }
// The seed source of a scenario generator, handed to f as the kernels' S: EnvSeed (env_seed given: every stream keyed as environment 0) or
// ScalarSeed (streams keyed by env_offset + e)
template <class F>
int with_scenario_seed(const ble_scenario_gen* gen, F&& f) {
  if (gen->env_seed != nullptr) return f(EnvSeed{gen->env_seed}, ScenarioGen{gen->episode, 0});
  return f(ScalarSeed{gen->seed}, ScenarioGen{gen->episode, gen->env_offset});
}
static_assert(kScenarioMax == BLE_SCENARIO_MAX && BLE_GP_SCENARIO_DOUBLES(3) == kBeliefAlphaAt + 3 * kScenarioAlphaDoubles,
              "ble_scenarios.h and ble_abi.h disagree on the slab");

// what the three rollout calls refuse of st and ro; lanes_per_plan: 1, or the scenarios of a plan
inline bool rollout_ok(const ble_state_f32* st, const struct ble_rollout_f32* ro, int lanes_per_plan) {
  if (!state_ok(st) || !ro || !ro->plans || !ro->wind_grid || !ro->ret || !ro->steps_flown) return false;
  if (ro->n < 0 || ro->n >= 2147483648LL || ro->n_plans < 1 || ro->n * (int64_t)ro->n_plans >= 2147483648LL ||
      ro->n * (int64_t)ro->n_plans * lanes_per_plan >= 2147483648LL || ro->n_plan_steps < 1 || ro->action_repeat < 1 ||
      (int64_t)ro->n_plan_steps * ro->action_repeat > BLE_ROLLOUT_MAX_STEPS)
    return false;
  return ro->substeps >= 1 && ro->substeps <= BLE_MAX_SUBSTEPS && ro->grid_env_stride >= 0 &&
         ro->gamma >= 0.0 && ro->gamma <= 1.0;                        // (a NaN gamma fails both comparisons)
}
// struct ble_rollout_f32 as the rollout kernels take it
inline RolloutArgs rollout_args(const struct ble_rollout_f32* ro) {
  return RolloutArgs{ro->n, ro->n_plans, ro->n_plan_steps, ro->action_repeat, ro->substeps, ro->gamma, ro->plans, ro->wind_grid,
                     ro->grid_env_stride, ro->ret, ro->steps_flown, ro->reward, ro->final_state};
}

// The wind a look-ahead call flies -- a noise generator's, a belief's, or with neither the forecast; never both -- checked and handed to f
// as the kernels' wind tag (kTreeWindForecast / kTreeWindNoise / kTreeWindBelief), their BeliefDev and their StepNoise.  n: the call's batch
template <class F>
int with_wind(const ble_noise_gen* noise, const ble_gp_belief* belief, int64_t n, F&& f) {
  if (noise != nullptr && belief != nullptr) return BLE_E_INVALID_ARG;                  // two winds
  BeliefDev b{nullptr, 0, nullptr};
  const StepNoise none{0ull, nullptr, nullptr, 0ll};
  if (belief != nullptr) {
    if (!gp_belief(belief, &b) || belief->n != n) return BLE_E_INVALID_ARG;             // (a belief of another batch would be read out of bounds)
    return f(std::integral_constant<int, kTreeWindBelief>{}, b, none);
  }
  if (noise == nullptr) return f(std::integral_constant<int, kTreeWindForecast>{}, b, none);
  if (noise->env_offset < 0) return BLE_E_INVALID_ARG;      // (a negative offset would key other streams than the reset did)
  // (the harmonic cache is not handed on: the look-ahead kernels draw into LDS and fill no cache)
  return f(std::integral_constant<int, kTreeWindNoise>{}, b, StepNoise{noise->seed, noise->episode, nullptr, (long long)noise->env_offset});
}

// ble_rollout_f32, ble_rollout_belief_f32 and, with leaves (the leaf arena's StateDev as the one trailing argument), ble_rollout_leaves_f32
template <class... Leaf>
int launch_rollout(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_noise_gen* noise, const ble_gp_belief* belief,
                   uint32_t* err_flags, void* stream, const Leaf&... leaves) {
  if (!rollout_ok(st, ro, 1)) return BLE_E_INVALID_ARG;
  return with_wind(noise, belief, ro->n, [&](auto wind, BeliefDev b, StepNoise gen) {
    return with_vehicle<false>(st, nullptr, [&](auto veh) {
      if (ro->n == 0) return BLE_OK;
      constexpr int kWind = decltype(wind)::value;
      constexpr bool kLeaves = sizeof...(Leaf) > 0;
      const int64_t lanes = ro->n * (int64_t)ro->n_plans;
      if constexpr (kWind == kTreeWindBelief)
        return launch(ble_rollout_belief_kernel<decltype(veh), kLeaves, Leaf...>, lanes, kStepBlock, kStepBlock, stream, state_dev(st),
                      rollout_args(ro), b, err_flags, veh, leaves...);
      else
        return launch(ble_rollout_kernel<kWind == kTreeWindNoise, decltype(veh), kLeaves, Leaf...>, lanes, kStepBlock, kStepBlock, stream,
                      state_dev(st), rollout_args(ro), err_flags, gen, veh, leaves...);
    });
  });
}

// the sizes ble_plan_sample_u8 and ble_plan_select_f32 share
inline bool plan_sizes_ok(int64_t n, int n_plans, int n_plan_steps, int segment, int iteration) {
  return n >= 0 && n < 2147483648LL && n_plans >= 1 && n_plans <= BLE_PLAN_MAX_PLANS && n_plan_steps >= 1 &&
         n_plan_steps <= BLE_ROLLOUT_MAX_STEPS && segment >= 1 && iteration >= 0 && iteration < BLE_PLAN_MAX_ITERATIONS &&
         n * (int64_t)n_plans < 2147483648LL;
}

// ble_plan_sample_u8 and ble_plan_sample_prior_u8: D is the descriptor, which with a prior carries its counts as well
template <class D>
int launch_plan_sample(const D* ps, void* stream) {
  constexpr bool kPrior = std::is_same_v<D, struct ble_plan_sample_prior>;
  if (!ps || !ps->plans || !ps->decision_counter || !ps->best_plan || (ps->iteration > 0 && !ps->elite_counts)) return BLE_E_INVALID_ARG;
  if constexpr (kPrior)
    if (!ps->prior_counts) return BLE_E_INVALID_ARG;
  if (!plan_sizes_ok(ps->n, ps->n_plans, ps->n_plan_steps, ps->segment, ps->iteration) || ps->env_offset < 0) return BLE_E_INVALID_ARG;
  const PlanSampleArgs a{ps->n, ps->env_offset, ps->n_plans, ps->n_plan_steps, ps->segment, ps->iteration, ps->decision_counter,
                         ps->iteration > 0 ? ps->elite_counts : nullptr, ps->best_plan, ps->plans};
  const int64_t lanes = ps->n * (int64_t)ps->n_plans;
  const auto sample = [&](auto seed) {
    if constexpr (kPrior)
      return launch(ble_plan_sample_prior_kernel<decltype(seed)>, lanes, 256, 256, stream, a, ps->prior_counts, seed);
    else
      return launch(ble_plan_sample_kernel<decltype(seed)>, lanes, 256, 256, stream, a, seed);
  };
  if (ps->env_seed != nullptr) return sample(EnvSeed{ps->env_seed});
  return sample(ScalarSeed{ps->seed});
}

}  // namespace

extern "C" {

int ble_abi_version(void) { return BLE_ABI_VERSION; }

int ble_noise_primitive_version(void) { return BLE_NOISE_PRIMITIVE_VERSION; }

int ble_vehicle_default(ble_vehicle* v) {
  if (v == nullptr) return BLE_E_INVALID_ARG;
  v->envelope_volume_base = 1804.0; v->envelope_volume_dv_pressure = 0.0199; v->envelope_mass = 68.5; v->envelope_max_superpressure = 2380.0;
  v->envelope_cod = 0.25; v->payload_mass = 92.5; v->nighttime_power_load_w = 183.7; v->daytime_power_load_w = 120.4;
  v->acs_valve_hole_diameter_m = 0.04; v->battery_capacity_wh = 3058.56; v->mols_lift_gas = 6830.0; v->power_safety_layer_enabled = 1;
  v->reserved_ = 0;
  return BLE_OK;
}

int ble_last_hip_error(void) { return g_last_hip_error; }

int ble_set_step_form(int waves_per_env) {
  if (waves_per_env != 0 && waves_per_env != 1 && waves_per_env != 4 && waves_per_env != BLE_STEP_FORM_HELPER) return BLE_E_INVALID_ARG;
  const int before = step_form();
  g_step_form.store(waves_per_env, std::memory_order_relaxed);
  return before;
}

int ble_last_step_form(void) { return g_last_step_form; }

int ble_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return BLE_E_NO_DEVICE;
  return n;
}

int ble_step_f32(const ble_state_f32* st, const uint8_t* action, const float* wind_grid, int64_t grid_env_stride,
                 const float* noise_uv, float* reward, uint8_t* terminal, uint8_t* effective_action,
                 uint32_t* err_flags, unsigned long long* active_count, int64_t n, int substeps, void* stream) {
  return launch_step<false>(st, nullptr, action, wind_grid, grid_env_stride, nullptr, noise_uv, reward, terminal, effective_action, err_flags,
                            active_count, n, substeps, 1, stream);
}

int ble_step_n_f32(const ble_state_f32* st, const uint8_t* action, const float* wind_grid, int64_t grid_env_stride,
                   const ble_noise_gen* noise, float* reward, uint8_t* terminal, uint32_t* err_flags,
                   unsigned long long* active_count, int64_t n, int substeps, int n_steps, void* stream) {
  return launch_step<false>(st, nullptr, action, wind_grid, grid_env_stride, noise, nullptr, reward, terminal, nullptr, err_flags, active_count,
                            n, substeps, n_steps, stream);
}

int ble_forecast_f32(const float* wind_grid, int64_t grid_env_stride, const float* x_m, const float* y_m,
                     const float* pressure, const int32_t* elapsed_s, float* u, float* v, int64_t n, void* stream) {
  if (!wind_grid || !x_m || !y_m || !pressure || !elapsed_s || !u || !v || n < 0 || grid_env_stride < 0)
    return BLE_E_INVALID_ARG;
  return launch(ble_forecast_kernel, n, 256, 256, stream, wind_grid, grid_env_stride, x_m, y_m, pressure, elapsed_s, u, v, n);
}

int ble_forecast_column_f32(const float* wind_grid, int64_t grid_env_stride, const float* x_m, const float* y_m,
                            const int32_t* elapsed_s, const float* levels_pa, int n_levels, float* out_uv, int64_t n,
                            void* stream) {
  if (!wind_grid || !x_m || !y_m || !elapsed_s || !levels_pa || !out_uv || n < 0 || n_levels < 1 ||
      grid_env_stride < 0)
    return BLE_E_INVALID_ARG;
  return launch(ble_forecast_column_kernel, n, 1, kBlock, stream, wind_grid, grid_env_stride, x_m, y_m, elapsed_s, levels_pa, n_levels, out_uv, n);
}

int ble_observe_forecast_f32(const ble_state_f32* st, const float* wind_grid, int64_t grid_env_stride, const float* forecast_levels,
                             const float* noise_uv, const uint8_t* reset_mask, const ble_gp_history_f32* hist, int append, float* obs,
                             uint32_t* err_flags, int64_t n, void* stream) {
  return launch_observe<false, false>(st, nullptr, wind_grid, grid_env_stride, forecast_levels, noise_uv, reset_mask, hist, append, obs,
                                      err_flags, n, stream);
}

int ble_observe_live_f32(const ble_state_f32* st, const float* wind_grid, int64_t grid_env_stride, const float* noise_uv,
                         const uint8_t* reset_mask, const ble_gp_history_f32* hist, int append, float* obs, uint32_t* err_flags, int64_t n,
                         void* stream) {
  return launch_observe<false, true>(st, nullptr, wind_grid, grid_env_stride, nullptr, noise_uv, reset_mask, hist, append, obs, err_flags, n,
                                     stream);
}

int ble_observe_f32(const ble_state_f32* st, const float* wind_grid, int64_t grid_env_stride, const float* noise_uv,
                    const uint8_t* reset_mask, const ble_gp_history_f32* hist, int append, float* obs,
                    uint32_t* err_flags, int64_t n, void* stream) {
  return ble_observe_forecast_f32(st, wind_grid, grid_env_stride, nullptr, noise_uv, reset_mask, hist, append, obs, err_flags, n, stream);
}

int ble_decode_flow_fields_f32(const float* flow, float* wind_grid, int64_t n, void* stream) {
  if (!flow || !wind_grid || n < 0 || n > 2147483647LL) return BLE_E_INVALID_ARG;
  return launch(ble_decode_flow_kernel, n, 1, kDecodeThreads, stream, flow, wind_grid, n);
}

int ble_wind_noise_at_f32(const float* x_m, const float* y_m, const float* pressure, const int32_t* elapsed_s,
                          unsigned long long seed, const uint32_t* episode, int mode, uint32_t* harmonic_cache,
                          float* noise_uv, int64_t env_offset, int64_t n, void* stream) {
  if (!x_m || !y_m || !pressure || !elapsed_s || !noise_uv || n < 0 || env_offset < 0 || mode < 0 || mode > 1) return BLE_E_INVALID_ARG;
  return launch(ble_wind_noise_kernel<ScalarSeed>, n, 256, 256, stream, x_m, y_m, pressure, elapsed_s, ScalarSeed{seed}, episode, mode,
                harmonic_cache, noise_uv, n, env_offset);
}

int ble_wind_noise_seeded_f32(const float* x_m, const float* y_m, const float* pressure, const int32_t* elapsed_s,
                              const unsigned long long* env_seed, const uint32_t* episode, int mode, float* noise_uv, int64_t n, void* stream) {
  if (!x_m || !y_m || !pressure || !elapsed_s || !env_seed || !noise_uv || n < 0 || mode < 0 || mode > 1) return BLE_E_INVALID_ARG;
  return launch(ble_wind_noise_kernel<EnvSeed>, n, 256, 256, stream, x_m, y_m, pressure, elapsed_s, EnvSeed{env_seed}, episode, mode,
                nullptr, noise_uv, n, 0);
}

int ble_wind_noise_f32(const float* x_m, const float* y_m, const float* pressure, const int32_t* elapsed_s,
                       unsigned long long seed, const uint32_t* episode, int mode, uint32_t* harmonic_cache,
                       float* noise_uv, int64_t n, void* stream) {
  return ble_wind_noise_at_f32(x_m, y_m, pressure, elapsed_s, seed, episode, mode, harmonic_cache, noise_uv, 0, n, stream);
}

int ble_state_rows_f64(const ble_state_f32* st, int64_t first, int64_t count, double* out, int64_t n, void* stream) {
  if (!state_ok(st) || !out || first < 0 || count < 0 || n < 0 || first + count > n) return BLE_E_INVALID_ARG;
  return launch(ble_state_rows_kernel, count, 64, 64, stream, state_dev(st), first, count, out);
}

int ble_power_table_f32(const float* pressure_ratio, const float* state_of_charge, float* watts, uint32_t* err_flags,
                        int64_t n, void* stream) {
  if (!pressure_ratio || !state_of_charge || !watts || n < 0) return BLE_E_INVALID_ARG;
  return launch(ble_power_table_kernel, n, 256, 256, stream, pressure_ratio, state_of_charge, watts, err_flags, n);
}

int ble_probe_atmosphere_f32(const float* alpha, const float* pressure, float* height, float* temperature,
                             uint32_t* err_flags, int64_t n, void* stream) {
  if (!alpha || !pressure || !height || !temperature || n < 0) return BLE_E_INVALID_ARG;
  return launch(probe_atmosphere_kernel, n, 256, 256, stream, alpha, pressure, height, temperature, err_flags, n);
}

int ble_probe_atmosphere_at_height_f64(const float* alpha, const double* height_m, double* pressure, double* temperature, uint32_t* err_flags,
                                       int64_t n, void* stream) {
  if (!alpha || !height_m || !pressure || !temperature || n < 0) return BLE_E_INVALID_ARG;
  return launch(probe_at_height_kernel, n, 256, 256, stream, alpha, height_m, pressure, temperature, err_flags, n);
}

int ble_probe_solar_f32(const float* center_lat_deg, const float* center_lng_deg, const float* x_m, const float* y_m,
                        const int64_t* unix_s, float* el_deg, float* flux, int64_t n, void* stream) {
  if (!center_lat_deg || !center_lng_deg || !x_m || !y_m || !unix_s || !el_deg || !flux || n < 0)
    return BLE_E_INVALID_ARG;
  return launch(probe_solar_kernel, n, 256, 256, stream, center_lat_deg, center_lng_deg, x_m, y_m, unix_s, el_deg, flux, n);
}

int ble_probe_latlng_f64(const float* center_lat_deg, const float* center_lng_deg, const float* x_m, const float* y_m,
                         double* lat_deg, double* lng_deg, int64_t n, void* stream) {
  if (!center_lat_deg || !center_lng_deg || !x_m || !y_m || !lat_deg || !lng_deg || n < 0) return BLE_E_INVALID_ARG;
  return launch(probe_latlng_kernel, n, 256, 256, stream, center_lat_deg, center_lng_deg, x_m, y_m, lat_deg, lng_deg, n);
}

int ble_probe_solar_power_f32(const float* el_deg, const float* pressure, float* attenuation, float* power_w,
                              int64_t n, void* stream) {
  if (!el_deg || !pressure || !attenuation || !power_w || n < 0) return BLE_E_INVALID_ARG;
  return launch(probe_solar_power_kernel, n, 256, 256, stream, el_deg, pressure, attenuation, power_w, n);
}

int ble_probe_thermal_vehicle_f32(const ble_vehicle* vehicle, const float* volume, const float* t_int, const float* t_amb, const float* pressure,
                                  const float* el_deg, const float* flux, const float* upwelling_ir, float* dtdt,
                                  uint32_t* err_flags, int64_t n, void* stream) {
  if (!volume || !t_int || !t_amb || !pressure || !el_deg || !flux || !upwelling_ir || !dtdt || n < 0 || (vehicle != nullptr && !vehicle_ok(vehicle)))
    return BLE_E_INVALID_ARG;
  const double thermal_scale = vehicle != nullptr ? make_vehicle_rt(vehicle).thermal_scale : VehicleDefault::thermal_scale;
  return launch(probe_thermal_kernel, n, 256, 256, stream, volume, t_int, t_amb, pressure, el_deg, flux, upwelling_ir, dtdt, err_flags, n,
                thermal_scale);
}
int ble_probe_thermal_f32(const float* volume, const float* t_int, const float* t_amb, const float* pressure,
                          const float* el_deg, const float* flux, const float* upwelling_ir, float* dtdt,
                          uint32_t* err_flags, int64_t n, void* stream) {
  return ble_probe_thermal_vehicle_f32(nullptr, volume, t_int, t_amb, pressure, el_deg, flux, upwelling_ir, dtdt, err_flags, n, stream);
}

int ble_probe_sp_volume_vehicle_f32(const ble_vehicle* vehicle, const float* mols_air, const float* t_int, const float* pressure, float* volume,
                                    float* superpressure, int64_t n, void* stream) {
  if (!mols_air || !t_int || !pressure || !volume || !superpressure || n < 0 || (vehicle != nullptr && !vehicle_ok(vehicle))) return BLE_E_INVALID_ARG;
  const double lift = vehicle ? vehicle->mols_lift_gas : VehicleDefault::lift, v0 = vehicle ? vehicle->envelope_volume_base : VehicleDefault::v0;
  const double dvdp = vehicle ? vehicle->envelope_volume_dv_pressure : VehicleDefault::dvdp;
  return launch(probe_sp_volume_kernel, n, 256, 256, stream, mols_air, t_int, pressure, volume, superpressure, n, lift, v0, dvdp);
}
int ble_probe_sp_volume_f32(const float* mols_air, const float* t_int, const float* pressure, float* volume,
                            float* superpressure, int64_t n, void* stream) {
  return ble_probe_sp_volume_vehicle_f32(nullptr, mols_air, t_int, pressure, volume, superpressure, n, stream);
}

int ble_reset_at_f32(const ble_state_f32* st, const uint8_t* mask, unsigned long long seed, uint32_t* episode,
                     int sample, uint32_t* err_flags, int64_t env_offset, int64_t n, void* stream) {
  return launch_reset<false>(st, nullptr, mask, ScalarSeed{seed}, episode, sample, err_flags, env_offset, n, stream);
}

int ble_reset_seeded_f32(const ble_state_f32* st, const uint8_t* mask, const unsigned long long* env_seed, uint32_t* episode,
                         int sample, uint32_t* err_flags, int64_t n, void* stream) {
  if (!env_seed) return BLE_E_INVALID_ARG;
  return launch_reset<false>(st, nullptr, mask, EnvSeed{env_seed}, episode, sample, err_flags, 0, n, stream);
}

int ble_station_seeker_f32(const float* obs, int64_t obs_row_stride, uint8_t* action, int32_t* level, double* scores, uint32_t* err_flags,
                           int64_t n, void* stream) {
  if (!obs || !action || n < 0 || obs_row_stride < BLE_OBS_DIM || n > 4LL * 2147483647LL) return BLE_E_INVALID_ARG;
  return launch(ble_station_seeker_kernel, n, kSeekerBlock / 64, kSeekerBlock, stream, obs, obs_row_stride, action, level, scores, err_flags, n);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------- Q-network host code
// The descriptor checks, the sizes and the launchers of ble_qnet_*_f32 and ble_replay_*.
namespace {
bool qnet_ok(const ble_qnet_f32* net) {
  return net != nullptr && net->num_layers >= 1 && net->num_layers <= kQnetMaxLayers && net->input_dim == BLE_OBS_DIM &&
         net->num_actions == 3 && net->num_atoms >= 1 && net->num_atoms <= kQnetMaxAtoms &&
         (net->num_layers == 1 || (net->hidden_units >= 1 && net->hidden_units <= kQnetMaxHidden));
}
// the shape table of a checked descriptor
QnetShape qnet_shape(const ble_qnet_f32* net) {
  return ble::qnet_shape(net->num_layers, net->input_dim, net->hidden_units, net->num_actions, net->num_atoms);
}
// every pointer is a multiple of mask + 1 bytes (NULL is)
template <class... T>
bool aligned(uintptr_t mask, const T*... ptrs) {
  return ((reinterpret_cast<uintptr_t>(ptrs) | ...) & mask) == 0;
}
bool replay_ok(const ble_replay_f32* rp) {
  return rp != nullptr && rp->update_horizon >= 1 && rp->update_horizon <= BLE_REPLAY_MAX_HORIZON && rp->capacity >= rp->update_horizon + 1 &&
         rp->capacity <= (1LL << 40) && rp->num_envs >= 1 && rp->num_envs <= (1LL << 32) && rp->obs_stride >= BLE_OBS_DIM &&
         rp->obs_stride % 4 == 0 && std::isfinite(rp->gamma) && rp->max_tries >= 1 && rp->max_tries <= BLE_REPLAY_MAX_TRIES && rp->obs &&
         aligned(15, rp->obs) && rp->action && rp->reward && rp->terminal && rp->episode_end && rp->count && rp->counter;
}
// transitions: a batch of (state, next_state) pairs; an on-policy batch (PPO, cloning) has no next_state and no discount, and cloning
// without a value term (returns == false) no ret; the soft cloning loss reads no action (actions == false)
bool batch_ok(const ble_train_batch_f32* bt, bool transitions = true, bool returns = true, bool actions = true) {
  return bt != nullptr && bt->batch >= 0 && bt->batch <= BLE_TRAIN_MAX_BATCH && bt->state_stride >= BLE_OBS_DIM && bt->state_stride % 4 == 0 &&
         bt->state_stride <= (1LL << 20) && bt->state && (!transitions || (bt->next_state && bt->discount)) && (!returns || bt->ret) &&
         (!actions || bt->action) &&
         aligned(15, bt->state, bt->next_state);
}
// The workspace of one update on n rows.  branches: how often the online network runs -- 1, or 2 for SARSA (state, then next_state),
// which keeps both branches' activations, dlogits and slabs of partial sums (branch 0's first) and has no target network's logits.
ble_qnet_train_layout train_layout(const QnetShape& s, int branches, int num_atoms, int64_t n) {
  ble_qnet_train_layout y{};
  const int64_t ld = s.ld, L = s.layers;
  y.ld = ld;
  y.slabs = wgrad_slabs(n);
  const int64_t parts = branches * y.slabs;
  int64_t at = 0;
  auto take = [&](int64_t floats) { const int64_t o = at; at += qnet_round_up(floats, 64); return o; };
  y.acts = take(branches * L * n * ld);
  y.target_logits = take(branches == 1 ? n * ld : 0);
  y.targets = take(n * num_atoms);
  y.dlogits = take(branches * n * ld);
  y.scratch = take(4 * n * ld);
  y.partial = take(parts > 1 ? parts * s.max_block : 0);
  y.corrections = take(4);
  y.total = at;
  y.transposed_floats = s.transposed_floats;
  return y;
}
bool tree_ok(const ble_replay_f32* rp, const ble_sum_tree_f64* tr) {
  return tr != nullptr && tr->leaves == rp->capacity * rp->num_envs && tr->leaves <= BLE_SUM_TREE_MAX_LEAVES && tr->padded >= tr->leaves &&
         (tr->padded & (tr->padded - 1)) == 0 && (tr->padded == 1 || tr->padded / 2 < tr->leaves) && tr->nodes && tr->max_priority &&
         aligned(7, tr->nodes, tr->max_priority);
}
// the per-layer host arrays of ble_qnet_pack_f32 / ble_qnet_unpack_f32
bool layers_ok(const ble_qnet_f32* net, const float* const* kernel, const float* const* bias) {
  if (!kernel || !bias) return false;
  for (int l = 0; l < net->num_layers; ++l)
    if (!kernel[l] || !bias[l]) return false;
  return true;
}

// A sampler kernel, one workgroup per batch row, then the update counter the draws are keyed by advances; B == 0 launches nothing.
template <class... P, class... A>
int launch_sample_then_advance(void (*kernel)(P...), const ble_replay_f32* rp, const ble_train_batch_f32* bt, void* stream, const A&... args) {
  if (bt->batch == 0) return BLE_OK;
  const int status = launch_grid(kernel, dim3((unsigned)bt->batch), kReplayBlock, stream, args...);
  if (status != BLE_OK) return status;
  return launch_grid(ble_train_advance_kernel, dim3(1), 1, stream, rp->counter);
}

// Where layer l of a Dense stack writes its n rows of ld floats: base + (keep ? l : l & 1) n ld -- every layer kept, or two buffers
// in turn -- and the last layer to `last` instead when that is set.  layer_stride, when set, replaces n ld (kept layers that lie further
// apart: the two branches of SARSA).
struct DenseOut {
  float* base;
  bool keep;
  float* last;
  int64_t layer_stride = 0;
};
// The Dense stack of shape s over the weight image w, on n rows of x (row stride ldx).  The first layer reads the caller's rows, the
// others the previous layer's activations; ReLU after every layer but the last.  Returns the first failing status.
int launch_dense_stack(const QnetShape& s, const float* w, const float* x, int64_t ldx, int64_t n, DenseOut out, void* stream) {
  const unsigned row_tiles = (unsigned)((n + kQnetRows - 1) / kQnetRows);
  for (int l = 0; l < s.layers; ++l) {
    const int groups = s.mp[l] / kQnetCols;
    const bool first = l == 0, last = l == s.layers - 1;
    const auto dense = first ? (last ? ble_qnet_dense_kernel<true, false> : ble_qnet_dense_kernel<true, true>)
                             : (last ? ble_qnet_dense_kernel<false, false> : ble_qnet_dense_kernel<false, true>);
    float* y = last && out.last ? out.last : out.base + (out.keep ? l : l & 1) * (out.layer_stride ? out.layer_stride : n * s.ld);
    const int status = launch_grid(dense, dim3((unsigned)groups * row_tiles), kQnetBlock, stream, x, ldx, s.k[l], s.kp[l], w + s.offset[l], y,
                                   s.ld, groups, n);
    if (status != BLE_OK) return status;
    x = y;
    ldx = s.ld;
  }
  return BLE_OK;
}

// The descriptor of ble_qnet_td_*: td_kind_ok is all the workspace query reads; nothing else knows the kind and optimiser ranges.
bool td_kind_ok(const ble_td_f32* td) { return td != nullptr && td->kind >= BLE_TD_DQN_MSE && td->kind <= BLE_TD_SARSA_MSE; }
bool td_ok(const ble_td_f32* td) {
  return td_kind_ok(td) && (td->optimizer == BLE_TD_OPT_ADAM || td->optimizer == BLE_TD_OPT_SGD) &&
         (td->kind != BLE_TD_SARSA_MSE || (td->next_action != nullptr && std::isfinite(td->gamma)));
}
// The descriptor of ble_qnet_ppo_step_f32.
bool ppo_ok(const ble_ppo_f32* ppo) {
  return ppo != nullptr && std::isfinite(ppo->clip) && ppo->clip > 0.0f && std::isfinite(ppo->value_coef) && std::isfinite(ppo->entropy_coef) &&
         ppo->old_logp != nullptr && ppo->advantage != nullptr;
}
// The descriptor of ble_qnet_bc_step_f32.
bool bc_ok(const ble_bc_f32* bc) {
  return bc != nullptr && std::isfinite(bc->label_smoothing) && bc->label_smoothing >= 0.0f && bc->label_smoothing < 1.0f &&
         std::isfinite(bc->value_coef);
}
// The descriptor of ble_qnet_soft_bc_step_f32.
bool soft_ok(const ble_soft_bc_f32* soft) {
  return soft != nullptr && std::isfinite(soft->inv_temperature) && soft->inv_temperature > 0.0f && std::isfinite(soft->label_smoothing) &&
         soft->label_smoothing >= 0.0f && soft->label_smoothing < 1.0f && std::isfinite(soft->value_coef) && soft->target_q != nullptr;
}
// The loss of an update: a kind of ble_td_f32, PPO's (ble_qnet_ppo_step_f32: ppo != nullptr), cloning's (ble_qnet_bc_step_f32:
// bc != nullptr), soft cloning's (ble_qnet_soft_bc_step_f32: soft != nullptr), or QR-DQN's (ble_qnet_train_step_f32, which has no
// descriptor).
constexpr int kKindQr = -1, kKindPpo = -2, kKindBc = -3, kKindSoftBc = -4;
int update_kind(const ble_td_f32* td, const ble_ppo_f32* ppo = nullptr, const ble_bc_f32* bc = nullptr, const ble_soft_bc_f32* soft = nullptr) {
  return soft != nullptr ? kKindSoftBc : bc != nullptr ? kKindBc : ppo != nullptr ? kKindPpo : td != nullptr ? td->kind : kKindQr;
}
int update_branches(int kind) { return kind == BLE_TD_SARSA_MSE ? 2 : 1; }

// The arguments of one update, td == nullptr for ble_qnet_train_step_f32.  Where the two entry points differ, each keeps the answer
// it was published with (a caller may rely on either):
//  * kappa is the QR loss's alone, and a ble_td_f32 needs a one-atom network: each form checks what its loss kernel reads;
//  * SARSA has no target network, so it alone accepts target == NULL;
//  * lr: the QR form's only reader is Adam, so it checks lr under apply_update; the TD form, which has SGD too, checks it always;
//  * Adam's state and hyperparameters are wanted when Adam runs: under apply_update, and not with BLE_TD_OPT_SGD.
// PPO (ppo != nullptr, td == nullptr) needs a two-atom network and its own descriptor; it has no target network, no next_state and no
// kappa, and is the QR form in what it asks of lr and Adam.  Cloning (bc != nullptr, td == ppo == nullptr) is PPO in all of that, and
// reads batch->ret only under a value coefficient other than 0.  Soft cloning (soft != nullptr, the others NULL) is cloning in all of
// that, and reads no batch->action.
bool update_ok(const ble_qnet_train_f32* tr, const ble_td_f32* td, const ble_ppo_f32* ppo, const ble_bc_f32* bc, const ble_train_batch_f32* bt,
               const float* loss, const ble_soft_bc_f32* soft = nullptr) {
  const bool on_policy = ppo != nullptr || bc != nullptr || soft != nullptr;
  const bool returns = soft != nullptr ? !(soft->value_coef == 0.0f)
                                       : (bc == nullptr || !(bc->value_coef == 0.0f));      // (a NaN coefficient is refused below, whatever ret is)
  if (!tr || !qnet_ok(&tr->net) || !batch_ok(bt, !on_policy, returns, soft == nullptr) || !loss || !tr->net.weights || !tr->grad || !tr->workspace)
    return false;
  if (soft != nullptr) {
    if (tr->net.num_atoms != 2 || !soft_ok(soft)) return false;
  } else if (bc != nullptr) {
    if (tr->net.num_atoms != 2 || !bc_ok(bc)) return false;
  } else if (ppo != nullptr) {
    if (tr->net.num_atoms != 2 || !ppo_ok(ppo)) return false;
  } else {
    if (td == nullptr ? (!(tr->kappa > 0.0f) || !std::isfinite(tr->kappa)) : (tr->net.num_atoms != 1 || !td_ok(td))) return false;
    if (update_branches(update_kind(td)) == 1 && !tr->target) return false;
  }
  if (tr->net.num_layers > 1 && !tr->weights_t) return false;
  if ((td != nullptr || tr->apply_update) && !std::isfinite(tr->lr)) return false;
  if (tr->apply_update && (td == nullptr || td->optimizer == BLE_TD_OPT_ADAM) &&
      (!tr->adam_m || !tr->adam_v || !tr->adam_step || !std::isfinite(tr->adam_b1) || !std::isfinite(tr->adam_b2) || !std::isfinite(tr->adam_eps)))
    return false;
  return aligned(15, tr->net.weights, tr->target, tr->grad, tr->workspace, tr->adam_m, tr->adam_v, tr->weights_t);
}

// One update on a checked, non-empty batch: the shape, the workspace's parts and the stages in launch order.  Every stage returns the
// first failing status.  branches: 1, or 2 for SARSA, whose online network runs on state (branch 0) and on next_state (branch 1) --
// layer l's kept output is then 2 n stacked rows, branch 0 first.
struct TrainStep {
  const ble_qnet_train_f32* tr;
  const ble_td_f32* td;
  const ble_ppo_f32* ppo;
  const ble_bc_f32* bc;
  const ble_soft_bc_f32* soft;
  const ble_train_batch_f32* bt;
  void* stream;
  const QnetShape s;
  const int kind, branches;
  const ble_qnet_train_layout lay;
  const int64_t n, ld;
  float* const ws;

  TrainStep(const ble_qnet_train_f32* tr_, const ble_td_f32* td_, const ble_ppo_f32* ppo_, const ble_bc_f32* bc_,
            const ble_train_batch_f32* bt_, void* stream_, const ble_soft_bc_f32* soft_ = nullptr)
      : tr(tr_), td(td_), ppo(ppo_), bc(bc_), soft(soft_), bt(bt_), stream(stream_), s(qnet_shape(&tr_->net)),
        kind(update_kind(td_, ppo_, bc_, soft_)),
        branches(update_branches(kind)),
        lay(train_layout(s, branches, tr_->net.num_atoms, bt_->batch)), n(bt_->batch), ld(lay.ld), ws(tr_->workspace) {}
  float* acts(int l, int br = 0) const { return ws + lay.acts + (branches * l + br) * n * ld; }      // the online network's kept output of layer l

  // a kind with a target network: the target's pass on next_state (ping-pong, its logits end in target_logits); then the online
  // network once per branch, on state and (SARSA) on next_state, every layer kept.  PPO and cloning (hard or soft) have no target pass.
  int forward() const {
    if (branches == 1 && kind != kKindPpo && kind != kKindBc && kind != kKindSoftBc) {
      const int status = launch_dense_stack(s, tr->target, bt->next_state, bt->state_stride, n,
                                            DenseOut{ws + lay.scratch, false, ws + lay.target_logits}, stream);
      if (status != BLE_OK) return status;
    }
    for (int br = 0; br < branches; ++br) {
      const int status = launch_dense_stack(s, tr->net.weights, br == 0 ? bt->state : bt->next_state, bt->state_stride, n,
                                            DenseOut{acts(0, br), true, nullptr, branches * n * ld}, stream);
      if (status != BLE_OK) return status;
    }
    return BLE_OK;
  }
  // the loss kernel of the kind, one wave per row; `other`: the target network's logits, or (SARSA) the next_state branch's
  int loss(float* row_loss, uint32_t* err_flags) const {
    const float* logits = acts(s.layers - 1);
    const float* other = branches == 2 ? acts(s.layers - 1, 1) : ws + lay.target_logits;
    if (kind == kKindPpo)      // (aux where the other kinds write targets)
      return launch_grid(ble_ppo_loss_kernel, dim3((unsigned)n), kTrainLossBlock, stream, logits, ld, (const float*)bt->ret,
                         (const uint8_t*)bt->action, ppo->old_logp, ppo->advantage, ppo->clip, ppo->value_coef, ppo->entropy_coef, n,
                         ws + lay.targets, ws + lay.dlogits, row_loss, err_flags);
    if (kind == kKindBc)       // (aux where PPO writes its own)
      return launch_grid(ble_bc_loss_kernel, dim3((unsigned)n), kTrainLossBlock, stream, logits, ld, (const float*)bt->ret,
                         (const uint8_t*)bt->action, bc->label_smoothing, bc->value_coef, n, ws + lay.targets, ws + lay.dlogits, row_loss,
                         err_flags);
    if (kind == kKindSoftBc)   // (aux where cloning writes its own; no flag to set)
      return launch_grid(ble_soft_bc_loss_kernel, dim3((unsigned)n), kTrainLossBlock, stream, logits, ld, (const float*)bt->ret,
                         soft->target_q, soft->inv_temperature, soft->label_smoothing, soft->value_coef, n, ws + lay.targets,
                         ws + lay.dlogits, row_loss);
    if (kind == kKindQr)
      return launch_grid(ble_qr_loss_kernel, dim3((unsigned)n), kTrainLossBlock, stream, logits, other, ld, tr->net.num_actions,
                         tr->net.num_atoms, (const float*)bt->ret, (const float*)bt->discount, (const uint8_t*)bt->action, tr->kappa, n,
                         ws + lay.targets, ws + lay.dlogits, row_loss, err_flags);
    const auto kernel = kind == BLE_TD_DQN_MSE ? ble_td_loss_kernel<kTdDqnMse>
                        : kind == BLE_TD_DQN_HUBER ? ble_td_loss_kernel<kTdDqnHuber> : ble_td_loss_kernel<kTdSarsaMse>;
    return launch_grid(kernel, dim3((unsigned)n), kTrainLossBlock, stream, logits, other, ld, tr->net.num_actions, (const float*)bt->ret,
                       (const float*)bt->discount, (const uint8_t*)bt->action, td->next_action, td->mask, td->gamma, n, ws + lay.targets,
                       ws + lay.dlogits, row_loss, err_flags);
  }
  // from the last layer: dW (+ db) over the batch slabs of each branch (branch 0's slabs first), their reduction in that order, then dX
  // for the layer below over every row of every branch
  int backward() const {
    const int64_t rows = branches * n;
    float* dyb[2] = {ws + lay.scratch + (branches == 1 ? 2 : 0) * n * ld, ws + lay.scratch + (branches == 1 ? 3 : 2) * n * ld};
    const unsigned row_tiles = (unsigned)((rows + kQnetRows - 1) / kQnetRows);
    const int slabs = (int)lay.slabs, parts = branches * slabs;
    const int64_t slab_rows = slabs == 1 ? n : (n + slabs - 1) / slabs;
    const float* dy = ws + lay.dlogits;
    for (int l = s.layers - 1; l >= 0; --l) {
      const int64_t blk = s.block(l);
      float* dst = parts == 1 ? tr->grad + s.offset[l] : ws + lay.partial;
      int status;
      for (int br = 0; br < branches; ++br) {
        const float* x = l == 0 ? (br == 0 ? bt->state : bt->next_state) : acts(l - 1, br);
        status = launch_grid(ble_qnet_wgrad_kernel, dim3((unsigned)((s.kp[l] + 31) / 32), (unsigned)(s.mp[l] / kQnetCols), (unsigned)slabs),
                             64, stream, x, l == 0 ? bt->state_stride : ld, s.k[l], s.kp[l], dy + br * n * ld, ld, s.m[l], s.mp[l], n,
                             slab_rows, dst + br * slabs * blk, blk);
        if (status != BLE_OK) return status;
      }
      if (parts > 1) {
        status = launch(ble_wgrad_reduce_kernel, blk, 256, 256, stream, (const float*)(ws + lay.partial), parts, blk, blk,
                        tr->grad + s.offset[l]);
        if (status != BLE_OK) return status;
      }
      if (l == 0) break;
      const int groups = s.mpt(l) / kQnetCols;
      float* dx = dyb[l & 1];
      status = launch_grid(ble_qnet_dgrad_kernel, dim3((unsigned)groups * row_tiles), kQnetBlock, stream, dy, ld, s.kpt(l),
                           (const float*)(tr->weights_t + s.toffset[l]), (const float*)acts(l - 1), dx, groups, rows);
      if (status != BLE_OK) return status;
      dy = dx;
    }
    return BLE_OK;
  }
  // Adam (its prologue first), or plain SGD for BLE_TD_OPT_SGD
  int optimise() const {
    if (td != nullptr && td->optimizer == BLE_TD_OPT_SGD)
      return launch(ble_sgd_kernel, s.offset[s.layers], kAdamBlock, kAdamBlock, stream, const_cast<float*>(tr->net.weights), tr->weights_t,
                    (const float*)tr->grad, tr->lr, s);
    float* corr = ws + lay.corrections;
    const int status = launch_grid(ble_adam_prologue_kernel, dim3(1), 1, stream, tr->adam_step, tr->adam_b1, tr->adam_b2, corr);
    if (status != BLE_OK) return status;
    return launch(ble_adam_kernel, s.offset[s.layers], kAdamBlock, kAdamBlock, stream, const_cast<float*>(tr->net.weights), tr->weights_t,
                  (const float*)tr->grad, tr->adam_m, tr->adam_v, (const float*)corr, tr->lr, (float)tr->adam_b1,
                  (float)(1.0 - tr->adam_b1), (float)tr->adam_b2, (float)(1.0 - tr->adam_b2), tr->adam_eps, s);
  }
};

// ble_qnet_train_step_f32 (td == nullptr), ble_qnet_td_step_f32, ble_qnet_ppo_step_f32 (ppo != nullptr), ble_qnet_bc_step_f32
// (bc != nullptr) and ble_qnet_soft_bc_step_f32 (soft != nullptr): forward, loss, backward, optimiser.
int launch_update(const ble_qnet_train_f32* tr, const ble_td_f32* td, const ble_train_batch_f32* bt, float* loss, uint32_t* err_flags,
                  void* stream, const ble_ppo_f32* ppo = nullptr, const ble_bc_f32* bc = nullptr, const ble_soft_bc_f32* soft = nullptr) {
  if (!update_ok(tr, td, ppo, bc, bt, loss, soft)) return BLE_E_INVALID_ARG;
  if (bt->batch == 0) return BLE_OK;
  const TrainStep t(tr, td, ppo, bc, bt, stream, soft);
  if (const int status = t.forward(); status != BLE_OK) return status;
  if (const int status = t.loss(loss, err_flags); status != BLE_OK) return status;
  if (const int status = t.backward(); status != BLE_OK) return status;
  return tr->apply_update ? t.optimise() : BLE_OK;
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------------------------- Q-network agents
int ble_qnet_workspace_f32(const ble_qnet_f32* net, int64_t n, int64_t* packed_floats, int64_t* scratch_floats) {
  if (!qnet_ok(net) || n < 0) return BLE_E_INVALID_ARG;
  const QnetShape s = qnet_shape(net);
  if (packed_floats != nullptr) *packed_floats = s.offset[s.layers];
  if (scratch_floats != nullptr) *scratch_floats = 2 * n * s.ld;
  return BLE_OK;
}

int ble_qnet_pack_f32(const ble_qnet_f32* net, const float* const* kernel, const float* const* bias, float* packed) {
  if (!qnet_ok(net) || !layers_ok(net, kernel, bias) || !packed) return BLE_E_INVALID_ARG;
  qnet_pack(qnet_shape(net), kernel, bias, packed);
  return BLE_OK;
}

int ble_qnet_forward_f32(const ble_qnet_f32* net, const float* obs, int64_t obs_row_stride, float* scratch, uint8_t* action,
                         float* q_values, int64_t n, void* stream) {
  if (!qnet_ok(net) || !net->weights || !obs || !scratch || !action || n < 0 || obs_row_stride < BLE_OBS_DIM) return BLE_E_INVALID_ARG;
  if (!aligned(15, net->weights, scratch)) return BLE_E_INVALID_ARG;
  const QnetShape s = qnet_shape(net);
  const int64_t ld = s.ld;
  if ((ld / kQnetCols) * ((n + kQnetRows - 1) / kQnetRows) > 2147483647LL) return BLE_E_INVALID_ARG;
  if (n == 0) return BLE_OK;
  const int status = launch_dense_stack(s, net->weights, obs, obs_row_stride, n, DenseOut{scratch, false, nullptr}, stream);
  if (status != BLE_OK) return status;
  return launch(ble_qnet_head_kernel, n, kQnetHeadBlock, kQnetHeadBlock, stream, scratch + ((s.layers - 1) & 1) * n * ld, ld, net->num_actions,
                net->num_atoms, action, q_values, n);
}

// ---------------------------------------------------------------------------------------------------------------- Q-network training
int ble_qnet_unpack_f32(const ble_qnet_f32* net, const float* packed, float* const* kernel, float* const* bias) {
  if (!qnet_ok(net) || !packed || !layers_ok(net, kernel, bias)) return BLE_E_INVALID_ARG;
  qnet_unpack(qnet_shape(net), packed, kernel, bias);
  return BLE_OK;
}

int ble_replay_sample_f32(const ble_replay_f32* rp, const ble_train_batch_f32* bt, unsigned long long seed, uint32_t* err_flags,
                          void* stream) {
  if (!replay_ok(rp) || !batch_ok(bt)) return BLE_E_INVALID_ARG;
  return launch_sample_then_advance(ble_replay_sample_kernel, rp, bt, stream, *rp, *bt, (uint64_t)seed, err_flags);
}

int ble_qnet_train_workspace_f32(const ble_qnet_train_f32* tr, const ble_train_batch_f32* bt, ble_qnet_train_layout* out) {
  if (!tr || !qnet_ok(&tr->net) || !bt || bt->batch < 0 || bt->batch > BLE_TRAIN_MAX_BATCH || !out) return BLE_E_INVALID_ARG;
  *out = train_layout(qnet_shape(&tr->net), 1, tr->net.num_atoms, bt->batch);
  return BLE_OK;
}

int ble_qnet_transpose_f32(const ble_qnet_f32* net, const float* packed, float* packed_t) {
  if (!qnet_ok(net) || !packed || !packed_t) return BLE_E_INVALID_ARG;
  qnet_transpose(qnet_shape(net), packed, packed_t);
  return BLE_OK;
}

int ble_qnet_train_step_f32(const ble_qnet_train_f32* tr, const ble_train_batch_f32* bt, float* loss, uint32_t* err_flags, void* stream) {
  return launch_update(tr, nullptr, bt, loss, err_flags, stream);
}

int ble_qnet_td_workspace_f32(const ble_qnet_train_f32* tr, const ble_td_f32* td, const ble_train_batch_f32* bt, ble_qnet_train_layout* out) {
  if (!tr || !qnet_ok(&tr->net) || tr->net.num_atoms != 1 || !td_kind_ok(td) || !bt || bt->batch < 0 || bt->batch > BLE_TRAIN_MAX_BATCH || !out)
    return BLE_E_INVALID_ARG;
  *out = train_layout(qnet_shape(&tr->net), update_branches(td->kind), 1, bt->batch);
  return BLE_OK;
}

int ble_qnet_td_step_f32(const ble_qnet_train_f32* tr, const ble_td_f32* td, const ble_train_batch_f32* bt, float* loss, uint32_t* err_flags,
                         void* stream) {
  return td != nullptr ? launch_update(tr, td, bt, loss, err_flags, stream) : BLE_E_INVALID_ARG;
}

int ble_qnet_explore_u8(const ble_explore_f32* ex, uint8_t* action, void* stream) {
  if (!ex || !action || ex->n < 0 || ex->n > 4LL * 2147483647LL * 256 || !(ex->epsilon >= 0.0f && ex->epsilon <= 1.0f)) return BLE_E_INVALID_ARG;
  return launch(ble_explore_kernel, ex->n, 256, 256, stream, action, (int64_t)ex->n, ex->epsilon, (uint64_t)ex->seed, (uint64_t)ex->step);
}

// ---------------------------------------------------------------------------------------------------------------- on-policy training
int ble_ac_act_f32(const ble_qnet_f32* net, const ble_ac_rows_f32* rows, float* scratch, const ble_ac_sample* sample, void* stream) {
  if (!qnet_ok(net) || net->num_atoms != 2 || !net->weights || !rows || !rows->obs || !scratch || !rows->action || !rows->logp || !rows->value ||
      rows->n < 0 || rows->obs_row_stride < BLE_OBS_DIM)
    return BLE_E_INVALID_ARG;
  if (sample != nullptr && (!sample->step || sample->env_offset < 0)) return BLE_E_INVALID_ARG;
  if (!aligned(15, net->weights, scratch)) return BLE_E_INVALID_ARG;
  const QnetShape s = qnet_shape(net);
  const int64_t ld = s.ld, n = rows->n;
  if ((ld / kQnetCols) * ((n + kQnetRows - 1) / kQnetRows) > 2147483647LL) return BLE_E_INVALID_ARG;
  if (n == 0) return BLE_OK;
  const int status = launch_dense_stack(s, net->weights, rows->obs, rows->obs_row_stride, n, DenseOut{scratch, false, nullptr}, stream);
  if (status != BLE_OK) return status;
  return launch(ble_ac_head_kernel, n, kQnetHeadBlock, kQnetHeadBlock, stream, (const float*)(scratch + ((s.layers - 1) & 1) * n * ld), ld,
                (uint64_t)(sample ? sample->seed : 0), (int64_t)(sample ? sample->env_offset : 0),
                (const unsigned long long*)(sample ? sample->step : nullptr), rows->action, rows->logp, rows->value, rows->probs, n);
}

// ---------------------------------------------------------------------------------------------------------------- populations
namespace {
// the stride between the images of a population: room for one image, every image 256-byte aligned when image 0 is
bool member_stride_ok(const QnetShape& s, int64_t member_stride) { return member_stride >= s.offset[s.layers] && member_stride % 64 == 0; }

// launch_dense_stack for a population: P members of R rows each, member p on the image w + p member_stride; two buffers in turn, or
// (keep) every layer kept: layer l of all P R rows at base + l P R ld; the last layer to `last_out` instead when that is set.
int launch_dense_stack_grouped(const QnetShape& s, const float* w, int64_t member_stride, const float* x, int64_t ldx, int64_t members,
                               int64_t rows_per_member, float* base, void* stream, bool keep = false, float* last_out = nullptr) {
  const int64_t n = members * rows_per_member;
  const int64_t tiles_per_member = (rows_per_member + kQnetRows - 1) / kQnetRows;
  for (int l = 0; l < s.layers; ++l) {
    const int groups = s.mp[l] / kQnetCols;
    const bool first = l == 0, last = l == s.layers - 1;
    const auto dense = first ? (last ? ble_qnet_dense_grouped_kernel<true, false> : ble_qnet_dense_grouped_kernel<true, true>)
                             : (last ? ble_qnet_dense_grouped_kernel<false, false> : ble_qnet_dense_grouped_kernel<false, true>);
    float* y = last && last_out ? last_out : base + (keep ? l : l & 1) * n * s.ld;
    const int status = launch_grid(dense, dim3((unsigned)(groups * tiles_per_member * members)), kQnetBlock, stream, x, ldx, s.k[l], s.kp[l],
                                   w + s.offset[l], member_stride, y, s.ld, groups, rows_per_member, tiles_per_member);
    if (status != BLE_OK) return status;
    x = y;
    ldx = s.ld;
  }
  return BLE_OK;
}

// the shape table the evolution kernels take by value: the layers' packed blocks and the first logical parameter of each
EsDims es_dims(const QnetShape& s) {
  EsDims d{};
  d.d = s;
  for (int l = 0; l < s.layers; ++l) d.logical[l + 1] = d.logical[l] + (int64_t)s.k[l] * s.m[l] + s.m[l];
  return d;
}
bool es_ok(const ble_es_f32* es) {
  return es != nullptr && qnet_ok(&es->net) && es->generation != nullptr && es->members >= 1 && (!es->antithetic || es->members % 2 == 0) &&
         std::isfinite(es->sigma) && es->sigma > 0.0f && std::isfinite(es->weight_decay);
}
bool same_shape(const ble_qnet_f32& a, const ble_qnet_f32& b) {
  return a.num_layers == b.num_layers && a.input_dim == b.input_dim && a.hidden_units == b.hidden_units && a.num_actions == b.num_actions &&
         a.num_atoms == b.num_atoms;
}
const ble_train_batch_f32 kNoBatch{};      // batch 0: the layout ble_qnet_apply_grad_f32's workspace has
}  // namespace

namespace {
// what ble_qnet_forward_grouped_f32 refuses
bool grouped_ok(const ble_qnet_grouped_f32* pop) {
  if (!pop || !qnet_ok(&pop->net) || !pop->net.weights || !pop->obs || !pop->scratch || !pop->action || pop->obs_row_stride < BLE_OBS_DIM)
    return false;
  if (!aligned(15, pop->net.weights, pop->scratch)) return false;
  if (pop->members < 1 || pop->rows_per_member < 1 || pop->rows_per_member > 2147483647LL) return false;
  if (pop->head != BLE_POP_HEAD_Q && pop->head != BLE_POP_HEAD_ACTOR_GREEDY) return false;
  if (pop->head == BLE_POP_HEAD_Q ? (pop->value != nullptr || pop->probs != nullptr) : (pop->net.num_atoms != 2 || pop->q_values != nullptr))
    return false;
  const QnetShape s = qnet_shape(&pop->net);
  if (!member_stride_ok(s, pop->member_stride)) return false;
  const int64_t groups = s.ld / kQnetCols;
  return pop->members * pop->rows_per_member < 2147483648LL / groups;      // (P R < 2^62; so groups * P * ceil(R / 128) < 2^31 as well)
}

// The grouped Dense stack of a checked population, then its head.  An actor head (greedy: sample == nullptr) writes a log-probability
// and a value per row: without the caller's arrays, into the activation buffer the last layer did not write (n * ld >= 64 n floats).
int launch_grouped_forward(const ble_qnet_grouped_f32* pop, const ble_ac_sample* sample, float* logp, void* stream) {
  const QnetShape s = qnet_shape(&pop->net);
  const int64_t ld = s.ld, P = pop->members, R = pop->rows_per_member, n = P * R;
  int status = launch_dense_stack_grouped(s, pop->net.weights, pop->member_stride, pop->obs, pop->obs_row_stride, P, R, pop->scratch, stream);
  if (status != BLE_OK) return status;
  const float* logits = pop->scratch + ((s.layers - 1) & 1) * n * ld;
  if (pop->head == BLE_POP_HEAD_Q)
    return launch(ble_qnet_head_kernel, n, kQnetHeadBlock, kQnetHeadBlock, stream, logits, ld, pop->net.num_actions, pop->net.num_atoms,
                  pop->action, pop->q_values, n);
  float* spare = pop->scratch + (s.layers & 1) * n * ld;
  return launch(ble_ac_head_kernel, n, kQnetHeadBlock, kQnetHeadBlock, stream, logits, ld, (uint64_t)(sample ? sample->seed : 0),
                (int64_t)(sample ? sample->env_offset : 0), (const unsigned long long*)(sample ? sample->step : nullptr), pop->action,
                logp ? logp : spare, pop->value ? pop->value : spare + n, pop->probs, n);
}
}  // namespace

int ble_qnet_forward_grouped_f32(const ble_qnet_grouped_f32* pop, void* stream) {
  if (!grouped_ok(pop)) return BLE_E_INVALID_ARG;
  return launch_grouped_forward(pop, nullptr, nullptr, stream);
}

// The sampled (or, sample == NULL, greedy) actor head over a population: row p R + r is keyed by (seed, env_offset + p R + r, *step),
// what member p alone draws at env_offset + p R.
int ble_ac_act_grouped_f32(const ble_qnet_grouped_f32* pop, const ble_ac_sample* sample, float* logp, void* stream) {
  if (!grouped_ok(pop) || pop->head != BLE_POP_HEAD_ACTOR_GREEDY || !logp) return BLE_E_INVALID_ARG;
  if (sample != nullptr && (!sample->step || sample->env_offset < 0)) return BLE_E_INVALID_ARG;
  return launch_grouped_forward(pop, sample, logp, stream);
}

int ble_es_perturb_f32(const ble_es_f32* es, void* stream) {
  if (!es_ok(es) || !es->net.weights || !es->population || !aligned(15, es->net.weights, es->population)) return BLE_E_INVALID_ARG;
  const QnetShape s = qnet_shape(&es->net);
  if (!member_stride_ok(s, es->member_stride)) return BLE_E_INVALID_ARG;
  return launch(ble_es_perturb_kernel, s.offset[s.layers], kEsBlock, kEsBlock, stream, es->net.weights, es->population, es->member_stride,
                (int)es->members, (int)(es->antithetic != 0), es->sigma, (uint64_t)es->seed, (const unsigned long long*)es->generation,
                es_dims(s));
}

int ble_es_gradient_f32(const ble_es_f32* es, const ble_qnet_train_f32* tr, const float* w, void* stream) {
  if (!es_ok(es) || !tr || !qnet_ok(&tr->net) || !same_shape(es->net, tr->net) || !tr->net.weights || !tr->grad || !w ||
      !aligned(15, tr->net.weights, tr->grad))
    return BLE_E_INVALID_ARG;
  const QnetShape s = qnet_shape(&tr->net);
  const int streams = es->antithetic ? es->members / 2 : es->members;
  const int status = launch(ble_es_gradient_kernel, s.offset[s.layers], kEsBlock, kEsBlock, stream, tr->net.weights, tr->grad, w, streams,
                            es->sigma, es->weight_decay, (uint64_t)es->seed, (const unsigned long long*)es->generation, es_dims(s));
  if (status != BLE_OK) return status;
  return launch_grid(ble_train_advance_kernel, dim3(1), 1, stream, es->generation);
}

int ble_qnet_apply_grad_f32(const ble_qnet_train_f32* tr, void* stream) {
  if (!tr || !qnet_ok(&tr->net) || !tr->net.weights || !tr->grad || !tr->workspace) return BLE_E_INVALID_ARG;
  if (tr->net.num_layers > 1 && !tr->weights_t) return BLE_E_INVALID_ARG;
  if (tr->apply_update && (!std::isfinite(tr->lr) || !tr->adam_m || !tr->adam_v || !tr->adam_step || !std::isfinite(tr->adam_b1) ||
                           !std::isfinite(tr->adam_b2) || !std::isfinite(tr->adam_eps)))
    return BLE_E_INVALID_ARG;
  if (!aligned(15, tr->net.weights, tr->grad, tr->workspace, tr->adam_m, tr->adam_v, tr->weights_t)) return BLE_E_INVALID_ARG;
  if (!tr->apply_update) return BLE_OK;
  return TrainStep(tr, nullptr, nullptr, nullptr, &kNoBatch, stream).optimise();
}

namespace {
bool gae_sizes_ok(const ble_gae_block_f32* g) {
  return g != nullptr && g->steps >= 0 && g->num_envs >= 0 && g->num_envs <= (1LL << 32) && g->steps <= (1LL << 40) &&
         (g->num_envs == 0 || g->steps <= (1LL << 40) / g->num_envs);
}
}  // namespace

int ble_gae_f32(const ble_gae_block_f32* g, void* stream) {
  if (!gae_sizes_ok(g) || !std::isfinite(g->gamma) || !std::isfinite(g->lambda) || !g->reward || !g->value || !g->boot_value || !g->terminal ||
      !g->episode_end || !g->advantage || !g->ret)
    return BLE_E_INVALID_ARG;
  if (g->steps == 0) return BLE_OK;
  return launch(ble_gae_kernel, g->num_envs, 256, 256, stream, g->reward, g->value, g->boot_value, g->terminal, g->episode_end, g->gamma,
                g->lambda, g->advantage, g->ret, (int64_t)g->steps, (int64_t)g->num_envs);
}

int ble_adv_normalize_f32(const ble_gae_block_f32* g, void* stream) {
  if (!gae_sizes_ok(g) || !g->advantage) return BLE_E_INVALID_ARG;
  const int64_t m = g->steps * g->num_envs;
  if (m == 0) return BLE_OK;
  return launch_grid(ble_adv_normalize_kernel, dim3(1), kAdvNormBlock, stream, g->advantage, m);
}

int ble_qnet_ppo_step_f32(const ble_qnet_train_f32* tr, const ble_ppo_f32* ppo, const ble_train_batch_f32* bt, float* loss, uint32_t* err_flags,
                          void* stream) {
  return ppo != nullptr ? launch_update(tr, nullptr, bt, loss, err_flags, stream, ppo) : BLE_E_INVALID_ARG;
}

// ---------------------------------------------------------------------------------------------------------------- populations, by gradient
extern "C++" {      // (templates: this block sits inside the file's extern "C")
namespace {
// The loss of a grouped TD update from its descriptor's kind: kKindQr, BLE_TD_DQN_MSE or BLE_TD_DQN_HUBER; anything else is refused.
bool td_grouped_kind_ok(int32_t kind) { return kind == BLE_TD_GROUPED_QUANTILE || kind == BLE_TD_DQN_MSE + 1 || kind == BLE_TD_DQN_HUBER + 1; }
int td_grouped_kind(int32_t kind) { return kind == BLE_TD_GROUPED_QUANTILE ? kKindQr : kind - 1; }
// what each grouped descriptor asks of the network's atoms: PPO an actor-critic's two, a DQN kind one, the quantile loss any
bool grouped_atoms_ok(const ble_ppo_grouped_f32* g) { return g->tr.net.num_atoms == 2; }
bool grouped_atoms_ok(const ble_td_grouped_f32* g) {
  return g->reserved2_ == 0 && td_grouped_kind_ok(g->kind) && (g->kind == BLE_TD_GROUPED_QUANTILE || g->tr.net.num_atoms == 1);
}
// The sizes of a grouped update (G: ble_ppo_grouped_f32 or ble_td_grouped_f32): what the workspace query reads.
template <class G>
bool grouped_sizes_ok(const G* g) {
  if (!g || !qnet_ok(&g->tr.net) || !grouped_atoms_ok(g) || g->reserved_ != 0) return false;
  const int64_t P = g->members, B = g->rows_per_member;
  if (P < 1 || B < 1 || P > 65535 || B > BLE_TRAIN_MAX_BATCH || P * B > BLE_TRAIN_MAX_BATCH) return false;
  if (P * wgrad_slabs(B) > 65535) return false;                                          // (grid z of dW)
  const int64_t groups = qnet_shape(&g->tr.net).ld / kQnetCols;
  return groups * P * ((B + kQnetRows - 1) / kQnetRows) < 2147483648LL;
}
// train_layout at n = P B, but the slabs are the member's (a function of B) and every member has its own partial sums.  num_atoms:
// the floats per row of `targets` (PPO's aux: 2).
ble_qnet_train_layout grouped_train_layout(const QnetShape& s, int64_t P, int64_t B, int num_atoms) {
  ble_qnet_train_layout y{};
  const int64_t ld = s.ld, L = s.layers, n = P * B;
  y.ld = ld;
  y.slabs = wgrad_slabs(B);
  int64_t at = 0;
  auto take = [&](int64_t floats) { const int64_t o = at; at += qnet_round_up(floats, 64); return o; };
  y.acts = take(L * n * ld);
  y.target_logits = take(n * ld);
  y.targets = take(n * num_atoms);
  y.dlogits = take(n * ld);
  y.scratch = take(4 * n * ld);
  y.partial = take(y.slabs > 1 ? P * y.slabs * s.max_block : 0);
  y.corrections = take(4);
  y.total = at;
  y.transposed_floats = s.transposed_floats;
  return y;
}
// the per-member arrays and per-row inputs of each descriptor beyond lr: all there, 4-byte aligned (lr: grouped_update_ok)
bool grouped_arrays_ok(const ble_ppo_grouped_f32* g) {
  return g->clip && g->value_coef && g->entropy_coef && g->old_logp && g->advantage &&
         aligned(3, g->clip, g->value_coef, g->entropy_coef, g->old_logp, g->advantage);
}
// (kappa is the quantile loss's alone, as in the plain entry points; a target network is what every grouped TD kind has)
bool grouped_arrays_ok(const ble_td_grouped_f32* g) {
  return (g->kind != BLE_TD_GROUPED_QUANTILE || g->kappa) && aligned(3, g->kappa) && g->tr.target && aligned(15, g->tr.target);
}
template <class G>
bool grouped_update_ok(const G* g, const ble_train_batch_f32* bt, const float* loss) {
  constexpr bool kTd = std::is_same<G, ble_td_grouped_f32>::value;
  if (!grouped_sizes_ok(g) || !batch_ok(bt, kTd, true, true) || !loss) return false;
  const ble_qnet_train_f32& tr = g->tr;
  if (!tr.net.weights || !tr.grad || !tr.workspace) return false;
  if (bt->batch != (int64_t)g->members * g->rows_per_member) return false;
  const QnetShape s = qnet_shape(&tr.net);
  if (!member_stride_ok(s, g->member_stride)) return false;
  if (tr.net.num_layers > 1 && (!tr.weights_t || g->transposed_stride < s.transposed_floats || g->transposed_stride % 64 != 0)) return false;
  if (!g->lr || !aligned(3, g->lr) || !grouped_arrays_ok(g)) return false;
  if (tr.apply_update &&
      (!tr.adam_m || !tr.adam_v || !tr.adam_step || !std::isfinite(tr.adam_b1) || !std::isfinite(tr.adam_b2) || !std::isfinite(tr.adam_eps)))
    return false;
  return aligned(15, tr.net.weights, tr.grad, tr.workspace, tr.adam_m, tr.adam_v, tr.weights_t);
}

// One grouped update on a checked batch, beside TrainStep: the shape, the workspace's parts and the stages in launch order.  It serves
// both grouped descriptors: PPO's (ppo != nullptr) and the TD one (td != nullptr), which differ in the loss stage and in the TD kinds'
// target pass; the online forward, the backward and the optimiser read the fields the two descriptors share.
struct GroupedTrainStep {
  // what the stages after the loss read of either descriptor
  struct Members {
    int64_t member_stride, transposed_stride;
    const float* lr;
  };
  const ble_ppo_grouped_f32* ppo;
  const ble_td_grouped_f32* td;
  const Members g;
  const ble_qnet_train_f32* tr;
  const ble_train_batch_f32* bt;
  void* stream;
  const QnetShape s;
  const int64_t P, B, n;
  const ble_qnet_train_layout lay;
  const int64_t ld, tstride;
  float* const ws;

  template <class G>
  GroupedTrainStep(const G* g_, const ble_train_batch_f32* bt_, void* stream_)
      : ppo(pick<ble_ppo_grouped_f32>(g_)), td(pick<ble_td_grouped_f32>(g_)), g{g_->member_stride, g_->transposed_stride, g_->lr}, tr(&g_->tr),
        bt(bt_), stream(stream_), s(qnet_shape(&g_->tr.net)), P(g_->members), B(g_->rows_per_member), n(P * B),
        lay(grouped_train_layout(s, P, B, ppo != nullptr ? 2 : g_->tr.net.num_atoms)), ld(lay.ld),
        tstride(s.layers > 1 ? g_->transposed_stride : 0), ws(g_->tr.workspace) {}
  template <class W, class G>
  static const W* pick(const G* g_) {
    if constexpr (std::is_same<W, G>::value) return g_;
    else return nullptr;
  }
  float* acts(int l) const { return ws + lay.acts + l * n * ld; }

  // a TD kind: the target images' pass on next_state first (ping-pong in scratch, its logits end in target_logits); then the online
  // images on state, every layer kept
  int forward() const {
    if (td != nullptr) {
      const int status = launch_dense_stack_grouped(s, tr->target, g.member_stride, bt->next_state, bt->state_stride, P, B, ws + lay.scratch,
                                                    stream, false, ws + lay.target_logits);
      if (status != BLE_OK) return status;
    }
    return launch_dense_stack_grouped(s, tr->net.weights, g.member_stride, bt->state, bt->state_stride, P, B, acts(0), stream, true);
  }
  int loss(float* row_loss, uint32_t* err_flags) const {
    const float* logits = acts(s.layers - 1);
    if (ppo != nullptr)
      return launch_grid(ble_ppo_loss_grouped_kernel, dim3((unsigned)n), kTrainLossBlock, stream, logits, ld, (const float*)bt->ret,
                         (const uint8_t*)bt->action, ppo->old_logp, ppo->advantage, ppo->clip, ppo->value_coef, ppo->entropy_coef, B,
                         ws + lay.targets, ws + lay.dlogits, row_loss, err_flags);
    const float* other = ws + lay.target_logits;
    const int kind = td_grouped_kind(td->kind);
    if (kind == kKindQr)
      return launch_grid(ble_qr_loss_grouped_kernel, dim3((unsigned)n), kTrainLossBlock, stream, logits, other, ld, tr->net.num_actions,
                         tr->net.num_atoms, (const float*)bt->ret, (const float*)bt->discount, (const uint8_t*)bt->action, td->kappa, B,
                         ws + lay.targets, ws + lay.dlogits, row_loss, err_flags);
    const auto kernel = kind == BLE_TD_DQN_MSE ? ble_td_loss_grouped_kernel<kTdDqnMse> : ble_td_loss_grouped_kernel<kTdDqnHuber>;
    return launch_grid(kernel, dim3((unsigned)n), kTrainLossBlock, stream, logits, other, ld, tr->net.num_actions, (const float*)bt->ret,
                       (const float*)bt->discount, (const uint8_t*)bt->action, B, ws + lay.targets, ws + lay.dlogits, row_loss, err_flags);
  }
  // TrainStep::backward with the member coordinate: the slabs and their rows come from B
  int backward() const {
    float* dyb[2] = {ws + lay.scratch + 2 * n * ld, ws + lay.scratch + 3 * n * ld};
    const int64_t tiles_per_member = (B + kQnetRows - 1) / kQnetRows;
    const int slabs = (int)lay.slabs;
    const int64_t slab_rows = slabs == 1 ? B : (B + slabs - 1) / slabs;
    const float* dy = ws + lay.dlogits;
    for (int l = s.layers - 1; l >= 0; --l) {
      const int64_t blk = s.block(l);
      float* grad = tr->grad + s.offset[l];
      const float* x = l == 0 ? bt->state : acts(l - 1);
      int status = launch_grid(ble_qnet_wgrad_grouped_kernel,
                               dim3((unsigned)((s.kp[l] + 31) / 32), (unsigned)(s.mp[l] / kQnetCols), (unsigned)(P * slabs)), 64, stream, x,
                               l == 0 ? bt->state_stride : ld, s.k[l], s.kp[l], dy, ld, s.m[l], s.mp[l], B, slab_rows, slabs,
                               slabs == 1 ? grad : ws + lay.partial, slabs == 1 ? g.member_stride : slabs * blk,
                               slabs == 1 ? (int64_t)0 : blk);
      if (status != BLE_OK) return status;
      if (slabs > 1) {
        status = launch_grid(ble_wgrad_reduce_grouped_kernel, dim3((unsigned)((blk + 255) / 256), (unsigned)P), 256, stream,
                             (const float*)(ws + lay.partial), slabs, blk, blk, grad, g.member_stride);
        if (status != BLE_OK) return status;
      }
      if (l == 0) break;
      const int groups = s.mpt(l) / kQnetCols;
      float* dx = dyb[l & 1];
      status = launch_grid(ble_qnet_dgrad_grouped_kernel, dim3((unsigned)(groups * tiles_per_member * P)), kQnetBlock, stream, dy, ld,
                           s.kpt(l), (const float*)(tr->weights_t + s.toffset[l]), tstride, (const float*)acts(l - 1), dx, groups, B,
                           tiles_per_member);
      if (status != BLE_OK) return status;
      dy = dx;
    }
    return BLE_OK;
  }
  int optimise() const {
    float* corr = ws + lay.corrections;
    const int status = launch_grid(ble_adam_prologue_kernel, dim3(1), 1, stream, tr->adam_step, tr->adam_b1, tr->adam_b2, corr);
    if (status != BLE_OK) return status;
    const int64_t image = s.offset[s.layers];
    return launch_grid(ble_adam_grouped_kernel, dim3((unsigned)((image + kAdamBlock - 1) / kAdamBlock), (unsigned)P), kAdamBlock, stream,
                       const_cast<float*>(tr->net.weights), tr->weights_t, (const float*)tr->grad, tr->adam_m, tr->adam_v, (const float*)corr,
                       g.lr, g.member_stride, tstride, (float)tr->adam_b1, (float)(1.0 - tr->adam_b1), (float)tr->adam_b2,
                       (float)(1.0 - tr->adam_b2), tr->adam_eps, s);
  }
};

// ble_qnet_ppo_step_grouped_f32 and ble_qnet_td_step_grouped_f32: forward, loss, backward, optimiser.
template <class G>
int launch_grouped_update(const G* g, const ble_train_batch_f32* bt, float* loss, uint32_t* err_flags, void* stream) {
  if (!grouped_update_ok(g, bt, loss)) return BLE_E_INVALID_ARG;
  const GroupedTrainStep t(g, bt, stream);
  if (const int status = t.forward(); status != BLE_OK) return status;
  if (const int status = t.loss(loss, err_flags); status != BLE_OK) return status;
  if (const int status = t.backward(); status != BLE_OK) return status;
  return g->tr.apply_update ? t.optimise() : BLE_OK;
}
}  // namespace
}  // extern "C++"

int ble_qnet_ppo_grouped_workspace_f32(const ble_ppo_grouped_f32* g, ble_qnet_train_layout* layout) {
  if (!grouped_sizes_ok(g) || !layout) return BLE_E_INVALID_ARG;
  *layout = grouped_train_layout(qnet_shape(&g->tr.net), g->members, g->rows_per_member, 2);
  return BLE_OK;
}

int ble_qnet_ppo_step_grouped_f32(const ble_ppo_grouped_f32* g, const ble_train_batch_f32* bt, float* loss, uint32_t* err_flags, void* stream) {
  return launch_grouped_update(g, bt, loss, err_flags, stream);
}

// ---------------------------------------------------------------------------------------------------------------- populations of replay learners
int ble_qnet_td_grouped_workspace_f32(const ble_td_grouped_f32* g, ble_qnet_train_layout* layout) {
  if (!grouped_sizes_ok(g) || !layout) return BLE_E_INVALID_ARG;
  *layout = grouped_train_layout(qnet_shape(&g->tr.net), g->members, g->rows_per_member, g->tr.net.num_atoms);
  return BLE_OK;
}

int ble_qnet_td_step_grouped_f32(const ble_td_grouped_f32* g, const ble_train_batch_f32* bt, float* loss, uint32_t* err_flags, void* stream) {
  return launch_grouped_update(g, bt, loss, err_flags, stream);
}

int ble_replay_sample_grouped_f32(const ble_replay_f32* rp, int32_t members, const unsigned long long* seeds, const ble_train_batch_f32* bt,
                                  uint32_t* err_flags, void* stream) {
  if (!replay_ok(rp) || !batch_ok(bt) || members < 1 || rp->num_envs % members != 0 || bt->batch % members != 0 || !seeds || !aligned(7, seeds))
    return BLE_E_INVALID_ARG;
  return launch_sample_then_advance(ble_replay_sample_grouped_kernel, rp, bt, stream, *rp, *bt, seeds, (int64_t)(bt->batch / members),
                                    (int64_t)(rp->num_envs / members), err_flags);
}

int ble_qnet_explore_grouped_u8(const ble_explore_grouped_f32* ex, uint8_t* action, void* stream) {
  if (!ex || !action || ex->n < 0 || ex->n > 4LL * 2147483647LL * 256 || ex->members < 1 || ex->n % ex->members != 0 || ex->reserved_ != 0 ||
      !ex->epsilon || !ex->seed || !aligned(3, ex->epsilon) || !aligned(7, ex->seed))
    return BLE_E_INVALID_ARG;
  return launch(ble_explore_grouped_kernel, ex->n, 256, 256, stream, action, (int64_t)ex->n, (int64_t)(ex->n / ex->members), ex->epsilon,
                ex->seed, (uint64_t)ex->step);
}

// ---------------------------------------------------------------------------------------------------------------- imitation
int ble_qnet_bc_step_f32(const ble_qnet_train_f32* tr, const ble_bc_f32* bc, const ble_train_batch_f32* bt, float* loss, uint32_t* err_flags,
                         void* stream) {
  return bc != nullptr ? launch_update(tr, nullptr, bt, loss, err_flags, stream, nullptr, bc) : BLE_E_INVALID_ARG;
}

int ble_qnet_soft_bc_step_f32(const ble_qnet_train_f32* tr, const ble_soft_bc_f32* soft, const ble_train_batch_f32* bt, float* loss,
                              uint32_t* err_flags, void* stream) {
  return soft != nullptr ? launch_update(tr, nullptr, bt, loss, err_flags, stream, nullptr, nullptr, soft) : BLE_E_INVALID_ARG;
}

int ble_dagger_mix_u8(const ble_dagger_mix_f32* mix, void* stream) {
  if (!mix || mix->n < 0 || mix->n > 2147483647LL * kDaggerMixBlock || mix->env_offset < 0 || !(mix->beta >= 0.0f && mix->beta <= 1.0f))
    return BLE_E_INVALID_ARG;
  if (mix->n > 0 && (!mix->step || !mix->learner || !mix->expert || !mix->action)) return BLE_E_INVALID_ARG;
  return launch(ble_dagger_mix_kernel, mix->n, kDaggerMixBlock, kDaggerMixBlock, stream, mix->learner, mix->expert, mix->beta,
                (uint64_t)mix->seed, (int64_t)mix->env_offset, mix->step, mix->action, mix->took_expert, (int64_t)mix->n);
}

// ---------------------------------------------------------------------------------------------------------------- prioritized replay
int ble_replay_tree_add_f64(const ble_replay_f32* rp, const ble_sum_tree_f64* tr, void* stream) {
  if (!replay_ok(rp) || !tree_ok(rp, tr)) return BLE_E_INVALID_ARG;
  return launch_grid(ble_tree_add_kernel, dim3(1), kTreeBlock, stream, *rp, *tr);
}

int ble_replay_sample_prioritized_f32(const ble_replay_f32* rp, const ble_sum_tree_f64* tr, const ble_train_batch_f32* bt, float* priority,
                                      unsigned long long seed, uint32_t* err_flags, void* stream) {
  if (!replay_ok(rp) || !tree_ok(rp, tr) || !batch_ok(bt) || !bt->index || !priority) return BLE_E_INVALID_ARG;
  return launch_sample_then_advance(ble_replay_sample_prio_kernel, rp, bt, stream, *rp, *tr, *bt, priority, (uint64_t)seed, err_flags);
}

int ble_replay_set_priority_f32(const ble_replay_f32* rp, const ble_sum_tree_f64* tr, const ble_train_batch_f32* bt, const float* priority,
                                const float* loss, float* weighted_loss, uint32_t* err_flags, void* stream) {
  if (!replay_ok(rp) || !tree_ok(rp, tr) || !batch_ok(bt) || !bt->index || !priority || !loss || !weighted_loss) return BLE_E_INVALID_ARG;
  if (bt->batch == 0) return BLE_OK;
  return launch_grid(ble_set_priority_kernel, dim3(1), kTreeBlock, stream, (int64_t)rp->capacity, (int64_t)rp->num_envs, *tr,
                     (const int64_t*)bt->index, (int64_t)bt->batch, priority, loss, weighted_loss, err_flags);
}

int ble_marco_polo_u8(const ble_marco_polo_f32* mp, uint8_t* action, void* stream) {
  if (!mp || !action || mp->n < 0 || mp->n > 4LL * 2147483647LL * 256 || mp->obs_stride < 1 ||
      !(mp->exploratory_episode_probability >= 0.0 && mp->exploratory_episode_probability <= 1.0) || !mp->obs || !mp->begin || !mp->step ||
      !mp->phase_clock || !mp->walk_clock || !mp->exploratory_episode || !mp->exploratory_phase || !mp->target || !aligned(7, mp->target))
    return BLE_E_INVALID_ARG;
  if (mp->n == 0) return BLE_OK;
  const int status = launch(ble_marco_polo_kernel, mp->n, 256, 256, stream, *mp, action);
  if (status != BLE_OK) return status;
  return launch_grid(ble_train_advance_kernel, dim3(1), 1, stream, mp->step);
}

// ---------------------------------------------------------------------------------------------------------------- a population's prioritized replay
extern "C++" {
namespace {
// P solo tree images over the one ring of a population: per-member sizes, as tree_ok's
bool tree_grouped_ok(const ble_replay_f32* rp, const ble_sum_tree_grouped_f64* tr) {
  return tr != nullptr && tr->members >= 1 && tr->members <= 2147483647LL && rp->num_envs % tr->members == 0 &&
         tr->leaves == rp->capacity * (rp->num_envs / tr->members) && tr->leaves <= BLE_SUM_TREE_MAX_LEAVES && tr->padded >= tr->leaves &&
         (tr->padded & (tr->padded - 1)) == 0 && (tr->padded == 1 || tr->padded / 2 < tr->leaves) && tr->member_stride >= 2 * tr->padded &&
         tr->nodes && tr->max_priority && aligned(7, tr->nodes, tr->max_priority);
}
}  // namespace
}  // extern "C++"

int ble_replay_tree_add_grouped_f64(const ble_replay_f32* rp, const ble_sum_tree_grouped_f64* tr, void* stream) {
  if (!replay_ok(rp) || !tree_grouped_ok(rp, tr)) return BLE_E_INVALID_ARG;
  return launch_grid(ble_tree_add_grouped_kernel, dim3((unsigned)tr->members), kTreeBlock, stream, *rp, *tr,
                     (int64_t)(rp->num_envs / tr->members));
}

int ble_replay_sample_prioritized_grouped_f32(const ble_replay_f32* rp, const ble_sum_tree_grouped_f64* tr, const unsigned long long* seeds,
                                              const ble_train_batch_f32* bt, float* priority, uint32_t* err_flags, void* stream) {
  if (!replay_ok(rp) || !tree_grouped_ok(rp, tr) || !batch_ok(bt) || bt->batch % tr->members != 0 || !bt->index || !priority || !seeds ||
      !aligned(7, seeds))
    return BLE_E_INVALID_ARG;
  return launch_sample_then_advance(ble_replay_sample_prio_grouped_kernel, rp, bt, stream, *rp, *tr, *bt, priority, seeds,
                                    (int64_t)(bt->batch / tr->members), (int64_t)(rp->num_envs / tr->members), err_flags);
}

int ble_replay_set_priority_grouped_f32(const ble_replay_f32* rp, const ble_sum_tree_grouped_f64* tr, const ble_train_batch_f32* bt,
                                        const float* priority, const float* loss, float* weighted_loss, uint32_t* err_flags, void* stream) {
  if (!replay_ok(rp) || !tree_grouped_ok(rp, tr) || !batch_ok(bt) || bt->batch % tr->members != 0 || !bt->index || !priority || !loss ||
      !weighted_loss)
    return BLE_E_INVALID_ARG;
  if (bt->batch == 0) return BLE_OK;
  return launch_grid(ble_set_priority_grouped_kernel, dim3((unsigned)tr->members), kTreeBlock, stream, (int64_t)rp->capacity,
                     (int64_t)(rp->num_envs / tr->members), *tr, (const int64_t*)bt->index, (int64_t)(bt->batch / tr->members), priority, loss,
                     weighted_loss, err_flags);
}

int ble_marco_polo_grouped_u8(const ble_marco_polo_grouped_f32* mp, uint8_t* action, void* stream) {
  if (!mp || !action || mp->n < 0 || mp->n > 4LL * 2147483647LL * 256 || mp->obs_stride < 1 || mp->reserved_ != 0 || mp->members < 1 ||
      mp->n % mp->members != 0 || !mp->probability || !mp->seed || !aligned(7, mp->probability, mp->seed) || !mp->obs || !mp->begin ||
      !mp->step || !mp->phase_clock || !mp->walk_clock || !mp->exploratory_episode || !mp->exploratory_phase || !mp->target ||
      !aligned(7, mp->target))
    return BLE_E_INVALID_ARG;
  if (mp->n == 0) return BLE_OK;
  const int status = launch(ble_marco_polo_grouped_kernel, mp->n, 256, 256, stream, *mp, (int64_t)(mp->n / mp->members), action);
  if (status != BLE_OK) return status;
  return launch_grid(ble_train_advance_kernel, dim3(1), 1, stream, mp->step);
}

int ble_eval_accumulate_f32(const ble_state_f32* st, const float* reward, const ble_eval_acc* acc, double radius_m, int step_index,
                            int max_steps, float* flight_path, int64_t n, void* stream) {
  if (!state_ok(st) || !reward || !acc || !acc->cumulative_reward || !acc->steps_within_radius || !acc->final_timestep || !acc->done ||
      !acc->end_status || n < 0 || step_index < 0 || max_steps <= step_index)
    return BLE_E_INVALID_ARG;
  if (st->vehicle != nullptr && !vehicle_ok(st->vehicle)) return BLE_E_INVALID_ARG;
  const double capacity = st->vehicle != nullptr ? st->vehicle->battery_capacity_wh : VehicleDefault::capacity_d;     // balloon.py:173
  return launch(ble_eval_accumulate_kernel, n, 256, 256, stream, state_dev(st), reward, *acc, radius_m, step_index, max_steps, flight_path,
                capacity, n);
}

int ble_reset_f32(const ble_state_f32* st, const uint8_t* mask, unsigned long long seed, uint32_t* episode,
                  int sample, uint32_t* err_flags, int64_t n, void* stream) {
  return ble_reset_at_f32(st, mask, seed, episode, sample, err_flags, 0, n, stream);
}

int ble_probe_f64_prims(const double* x, double* y, int op, int64_t n, void* stream) {
  if (!x || !y || n < 0 || op < 0 || op > 8) return BLE_E_INVALID_ARG;
  return launch(probe_f64_kernel, n, 256, 256, stream, x, y, op, n);
}

int ble_probe_acs_f32(const float* pressure_ratio, float* power_w, float* efficiency, float* mass_flow, int64_t n,
                      void* stream) {
  if (!pressure_ratio || !power_w || !efficiency || !mass_flow || n < 0) return BLE_E_INVALID_ARG;
  return launch(probe_acs_kernel, n, 256, 256, stream, pressure_ratio, power_w, efficiency, mass_flow, n);
}

int ble_probe_safety_f32(int layer, const uint8_t* action, const float* value, const float* alpha, int32_t* clocks,
                         double night_load_w, double capacity_wh, uint8_t* fsm, uint8_t* effective_action,
                         uint32_t* err_flags, int64_t n, void* stream) {
  if (layer < 0 || layer > 2 || !action || !value || !fsm || !effective_action || n < 0) return BLE_E_INVALID_ARG;
  if ((layer == 0 && !alpha) || (layer == 2 && (!clocks || !(capacity_wh > 0.0)))) return BLE_E_INVALID_ARG;
  return launch(probe_safety_kernel, n, 256, 256, stream, layer, action, value, alpha, clocks, night_load_w, capacity_wh, fsm, effective_action,
                err_flags, n);
}

// ---- fleets (include/ble_abi.h::ble_fleet): the one-lane transition, the reset and the observation with a palette
int ble_step_fleet_f32(const ble_state_f32* st, const ble_fleet* fleet, const uint8_t* action, const float* wind_grid, int64_t grid_env_stride,
                       const float* noise_uv, float* reward, uint8_t* terminal, uint8_t* effective_action, uint32_t* err_flags,
                       unsigned long long* active_count, int64_t n, int substeps, void* stream) {
  return launch_step<true>(st, fleet, action, wind_grid, grid_env_stride, nullptr, noise_uv, reward, terminal, effective_action, err_flags,
                           active_count, n, substeps, 1, stream);
}

int ble_step_n_fleet_f32(const ble_state_f32* st, const ble_fleet* fleet, const uint8_t* action, const float* wind_grid, int64_t grid_env_stride,
                         const ble_noise_gen* noise, float* reward, uint8_t* terminal, uint32_t* err_flags, unsigned long long* active_count,
                         int64_t n, int substeps, int n_steps, void* stream) {
  return launch_step<true>(st, fleet, action, wind_grid, grid_env_stride, noise, nullptr, reward, terminal, nullptr, err_flags, active_count, n,
                           substeps, n_steps, stream);
}

int ble_reset_fleet_at_f32(const ble_state_f32* st, const ble_fleet* fleet, const uint8_t* mask, unsigned long long seed, uint32_t* episode,
                           int sample, uint32_t* err_flags, int64_t env_offset, int64_t n, void* stream) {
  return launch_reset<true>(st, fleet, mask, ScalarSeed{seed}, episode, sample, err_flags, env_offset, n, stream);
}

int ble_observe_forecast_fleet_f32(const ble_state_f32* st, const ble_fleet* fleet, const float* wind_grid, int64_t grid_env_stride,
                                   const float* forecast_levels, const float* noise_uv, const uint8_t* reset_mask, const ble_gp_history_f32* hist,
                                   int append, float* obs, uint32_t* err_flags, int64_t n, void* stream) {
  return launch_observe<true, false>(st, fleet, wind_grid, grid_env_stride, forecast_levels, noise_uv, reset_mask, hist, append, obs, err_flags,
                                     n, stream);
}

int ble_gp_query_f32(const ble_gp_history_f32* hist, const uint8_t* reset_mask, const struct ble_gp_query_f32* query, uint32_t* err_flags,
                     void* stream) {
  GpHistory h;
  if (!gp_ring(hist, &h) || !query) return BLE_E_INVALID_ARG;
  if (!query->xyp || !query->time_s || !query->mean_uv || !query->deviation || query->n < 0 || query->q < 1 ||
      query->n * (int64_t)query->q >= 2147483648LL || query->n >= 2147483648LL)
    return BLE_E_INVALID_ARG;
  if (query->add_forecast != 0 && (!query->wind_grid || query->grid_env_stride < 0)) return BLE_E_INVALID_ARG;
  const GpQueryArgs a{query->n, query->q, query->add_forecast != 0 ? 1 : 0, query->xyp, query->time_s, query->wind_grid,
                      query->grid_env_stride, query->mean_uv, query->deviation};
  return launch(ble_gp_query_kernel, query->n, 1, kObsBlock, stream, h, reset_mask, a, err_flags);
}

int ble_rollout_f32(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_noise_gen* noise, uint32_t* err_flags, void* stream) {
  return launch_rollout(st, ro, noise, nullptr, err_flags, stream);
}

int ble_gp_fit_f32(const ble_gp_history_f32* hist, const uint8_t* reset_mask, const int32_t* time_s, const ble_gp_belief* belief,
                   uint32_t* err_flags, void* stream) {
  // (the number of environments is the belief's)
  GpHistory h;
  BeliefDev b;
  if (!gp_ring(hist, &h) || !time_s || !gp_belief(belief, &b)) return BLE_E_INVALID_ARG;
  const int64_t n = belief->n;
  return launch(ble_gp_fit_kernel, n, 1, kObsBlock, stream, h, reset_mask, time_s, b, err_flags);
}

int ble_gp_belief_wind_f32(const ble_gp_belief* belief, const float* x_m, const float* y_m, const float* pressure, const int32_t* elapsed_s,
                           float* uv, void* stream) {
  BeliefDev b;
  if (!gp_belief(belief, &b) || !x_m || !y_m || !pressure || !elapsed_s || !uv) return BLE_E_INVALID_ARG;
  const int64_t n = belief->n;
  return launch(ble_gp_belief_wind_kernel, n, kBeliefWindBlock, kBeliefWindBlock, stream, b, x_m, y_m, pressure, elapsed_s, uv, n);
}

int ble_rollout_belief_f32(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_gp_belief* belief, uint32_t* err_flags,
                           void* stream) {
  if (belief == nullptr) return BLE_E_INVALID_ARG;                                      // (no belief is no forecast here: ble_rollout_f32's)
  return launch_rollout(st, ro, nullptr, belief, err_flags, stream);
}

namespace {
// an array of `a` that is the same array of `b`
inline bool state_arrays_shared(const ble_state_f32* a, const ble_state_f32* b) {
  const void* const* pa = reinterpret_cast<const void* const*>(a);
  const void* const* pb = reinterpret_cast<const void* const*>(b);
  for (size_t k = 0; k < offsetof(ble_state_f32, episode_cache) / sizeof(void*); ++k)
    if (pa[k] == pb[k]) return true;
  return false;
}
}  // namespace

// The look-ahead with its leaves handed back as full states: ble_rollout_f32 (noise, or neither wind) or
// ble_rollout_belief_f32 (belief) with the leaf arena as the kernels' last argument.
int ble_rollout_leaves_f32(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_noise_gen* noise, const ble_gp_belief* belief,
                           const ble_state_f32* leaves, uint32_t* err_flags, void* stream) {
  if (!state_ok(st) || !state_ok(leaves)) return BLE_E_INVALID_ARG;                     // (the leaves' vehicle and episode cache are not read)
  if (state_arrays_shared(leaves, st)) return BLE_E_INVALID_ARG;                        // a leaf array that IS the source's: st is never written
  return launch_rollout(st, ro, noise, belief, err_flags, stream, state_dev(leaves));
}

int ble_plan_sample_u8(const struct ble_plan_sample* ps, void* stream) { return launch_plan_sample(ps, stream); }

int ble_plan_select_f32(const struct ble_plan_select* sel, void* stream) {
  if (!sel || !sel->ret || !sel->plans || !sel->best_return || !sel->best_k || !sel->best_plan || !sel->action) return BLE_E_INVALID_ARG;
  if (!plan_sizes_ok(sel->n, sel->n_plans, sel->n_plan_steps, sel->segment, sel->iteration) || sel->elite < 0 || sel->elite > sel->n_plans ||
      (sel->elite >= 1 && !sel->elite_counts))
    return BLE_E_INVALID_ARG;
  const PlanSelectArgs a{sel->n, sel->n_plans, sel->n_plan_steps, sel->segment, sel->iteration, sel->elite, sel->ret, sel->plans,
                         sel->best_return, sel->best_k, sel->best_plan, sel->action, sel->elite_counts, sel->advance_counter};
  return launch(ble_plan_select_kernel, sel->n, 1, kPlanSelectBlock, stream, a);
}

// ---- expert iteration
int ble_plan_prior_u16(const struct ble_plan_prior* pr, void* stream) {
  if (!pr || !pr->probs || !pr->prior_counts || pr->n < 0 || pr->segments < 1 || pr->segments > BLE_ROLLOUT_MAX_STEPS || pr->strength < 0 ||
      pr->strength > 65535 || pr->n * (int64_t)pr->segments >= 2147483648LL)
    return BLE_E_INVALID_ARG;
  const int64_t total = pr->n * (int64_t)pr->segments;
  return launch(ble_plan_prior_kernel, total, 256, 256, stream, pr->probs, (int)pr->strength, (int)pr->segments, pr->prior_counts, total);
}

int ble_plan_sample_prior_u8(const struct ble_plan_sample_prior* ps, void* stream) { return launch_plan_sample(ps, stream); }

int ble_plan_action_values_f32(const struct ble_plan_action_values* av, void* stream) {
  if (!av || !av->ret || !av->first_action || !av->q || !av->q_k || !av->visits || av->n < 0 || av->n >= 2147483648LL || av->n_plans < 1 ||
      av->n_plans > BLE_PLAN_MAX_PLANS || av->n * (int64_t)av->n_plans >= 2147483648LL)
    return BLE_E_INVALID_ARG;
  const PlanActionValuesArgs a{av->n, av->n_plans, av->accumulate, av->ret, av->first_action, av->q, av->q_k, av->visits};
  return launch(ble_plan_action_values_kernel, av->n, 1, kPlanSelectBlock, stream, a);
}

// ---- a learned terminal value
int ble_plan_bootstrap_f32(const struct ble_plan_bootstrap* b, void* stream) {
  if (!b || !b->ret || !b->steps_flown || !b->leaf_status || !b->value || !b->score || b->n < 0 || b->n >= 2147483648LL || b->n_plans < 1 ||
      b->n_plans > BLE_PLAN_MAX_PLANS || b->n * (int64_t)b->n_plans >= 2147483648LL || !(b->gamma >= 0.0 && b->gamma <= 1.0))
    return BLE_E_INVALID_ARG;                                         // (a NaN gamma fails both comparisons)
  const int64_t total = b->n * (int64_t)b->n_plans;
  const PlanBootstrapArgs a{total, b->gamma, b->ret, b->steps_flown, b->leaf_status, b->value, b->score};
  return launch(ble_plan_bootstrap_kernel, total, 256, 256, stream, a);
}

// The observation of imagined states: one workgroup per leaf, the leaf form of ble_observe_kernel -- `append` carries
// leaves_per_env and `n` the row stride (the note above the kernel).  The ring alone is handed on: the carried factor is never read.
int ble_observe_leaves_f32(const ble_state_f32* leaves, int32_t leaves_per_env, const float* wind_grid, int64_t grid_env_stride,
                           const uint8_t* reset_mask, const ble_gp_history_f32* hist, float* obs, int64_t obs_row_stride, uint32_t* err_flags,
                           int64_t n_leaves, void* stream) {
  GpHistory h;
  if (!state_ok(leaves) || !wind_grid || !obs || !gp_ring(hist, &h)) return BLE_E_INVALID_ARG;
  if (leaves_per_env < 1 || n_leaves < 0 || n_leaves >= 2147483648LL || n_leaves % leaves_per_env != 0 || obs_row_stride < BLE_OBS_DIM ||
      grid_env_stride < 0)
    return BLE_E_INVALID_ARG;
  return with_vehicle<false>(leaves, nullptr, [&](auto veh) {
    return launch(ble_observe_kernel<decltype(veh), false, true>, n_leaves, 1, kObsBlock, stream, state_dev(leaves), wind_grid, grid_env_stride,
                  (const float*)nullptr, reset_mask, h, (int)leaves_per_env, obs, err_flags, obs_row_stride, veh, (const float*)nullptr);
  });
}

// ---- plan by beam search
namespace {
// an arena's pointers as the kernels take them; `state` has been checked by the caller
inline TreeArenaDev tree_arena_dev(const struct ble_tree_arena& a) { return TreeArenaDev{state_dev(a.state), a.acc, a.disc, a.flown, a.ret}; }
// the sizes the three calls share: n, the beam, and a level's number of children
inline bool tree_sizes_ok(int64_t n, int beam) {
  return n >= 0 && n < 2147483648LL && beam >= 1 && beam <= BLE_TREE_MAX_BEAM && n * (int64_t)(3 * beam) < 2147483648LL;
}
inline bool tree_children_ok(int n_children, int beam) { return n_children >= 3 && n_children <= 3 * beam && n_children % 3 == 0; }
static_assert(kTreeMaxBeam == BLE_TREE_MAX_BEAM && kTreeMaxDepth == BLE_ROLLOUT_MAX_STEPS, "ble_tree.h and ble_abi.h disagree");

// what both expand calls refuse of st and ex; nodes_per_child: 1, or the scenarios of a group
inline bool tree_expand_ok(const ble_state_f32* st, const struct ble_tree_expand* ex, int nodes_per_child) {
  if (!state_ok(st) || !ex || !ex->wind_grid || !state_ok(ex->dst.state) || !ex->dst.acc || !ex->dst.disc || !ex->dst.flown || !ex->dst.ret)
    return false;
  if (!tree_sizes_ok(ex->n, ex->beam) || ex->n * (int64_t)(3 * ex->beam) * nodes_per_child >= 2147483648LL || ex->segment < 1 ||
      ex->action_repeat < 1 || ex->depth < 1 || (int64_t)ex->depth * ex->segment * ex->action_repeat > BLE_ROLLOUT_MAX_STEPS ||
      ex->reserved_ != 0)
    return false;
  if (ex->substeps < 1 || ex->substeps > BLE_MAX_SUBSTEPS || ex->grid_env_stride < 0 ||
      !(ex->gamma >= 0.0 && ex->gamma <= 1.0))                       // (a NaN gamma fails both comparisons)
    return false;
  if (state_arrays_shared(ex->dst.state, st)) return false;                             // st is never written
  if (ex->parent_children == 0) return ex->n_parents == 1;                              // level 1
  if (!ex->parent || !state_ok(ex->src.state) || !ex->src.acc || !ex->src.disc || !ex->src.flown) return false;
  if (!tree_children_ok(ex->parent_children, ex->beam) || ex->n_parents < 1 || ex->n_parents > ex->parent_children || ex->n_parents > ex->beam)
    return false;
  return !(state_arrays_shared(ex->dst.state, ex->src.state) || ex->dst.acc == ex->src.acc || ex->dst.disc == ex->src.disc ||
           ex->dst.flown == ex->src.flown);                                             // a level is not expanded in place
}
// the arena an expand reads its parents from: ex->src, or on level 1 st's own environments (src.acc == NULL tells the kernel)
inline TreeArenaDev tree_source_dev(const ble_state_f32* st, const struct ble_tree_expand* ex) {
  if (ex->parent_children == 0) return TreeArenaDev{state_dev(st), nullptr, nullptr, nullptr, nullptr};
  return tree_arena_dev(ex->src);
}
// struct ble_tree_expand as the expand kernels take it
inline TreeExpandArgs tree_expand_args(const struct ble_tree_expand* ex) {
  return TreeExpandArgs{ex->n, ex->n_parents, ex->parent_children, ex->beam, ex->segment * ex->action_repeat, ex->substeps, ex->gamma,
                        ex->wind_grid, ex->grid_env_stride, ex->parent};
}
}  // namespace

int ble_tree_expand_f32(const ble_state_f32* st, const struct ble_tree_expand* ex, const ble_noise_gen* noise, const ble_gp_belief* belief,
                        uint32_t* err_flags, void* stream) {
  if (!tree_expand_ok(st, ex, 1)) return BLE_E_INVALID_ARG;
  return with_wind(noise, belief, ex->n, [&](auto wind, BeliefDev b, StepNoise gen) {
    return with_vehicle<false>(st, nullptr, [&](auto veh) {
      if (ex->n == 0) return BLE_OK;
      return launch(ble_tree_expand_kernel<decltype(wind)::value, decltype(veh)>, ex->n * (int64_t)(3 * ex->n_parents), kStepBlock, kStepBlock,
                    stream, state_dev(st), tree_expand_args(ex), tree_source_dev(st, ex), tree_arena_dev(ex->dst), b, gen, err_flags, veh);
    });
  });
}

int ble_tree_expand_scenarios_f32(const ble_state_f32* st, const struct ble_tree_expand* ex, const ble_gp_scenarios* scn,
                                  const ble_scenario_gen* gen, uint32_t* err_flags, void* stream) {
  ScenariosDev b;
  if (!gp_scenarios(scn, &b) || !scenario_gen_ok(gen) || !tree_expand_ok(st, ex, scn->num) || scn->n != ex->n)
    return BLE_E_INVALID_ARG;                                         // (scenarios of another batch would be read out of bounds)
  return with_vehicle<false>(st, nullptr, [&](auto veh) {
    if (ex->n == 0) return BLE_OK;
    return with_scenario_seed(gen, [&](auto seed, ScenarioGen g) {
      return launch(ble_tree_expand_scenarios_kernel<decltype(veh), decltype(seed)>, ex->n * (int64_t)(3 * ex->n_parents) * scn->num, kStepBlock,
                    kStepBlock, stream, state_dev(st), tree_expand_args(ex), tree_source_dev(st, ex), tree_arena_dev(ex->dst), b, seed, g,
                    err_flags, veh);
    });
  });
}

int ble_tree_select_f32(const struct ble_tree_select* sel, void* stream) {
  if (!sel || !sel->ret || !sel->parent || !sel->choice || !tree_sizes_ok(sel->n, sel->beam) || !tree_children_ok(sel->n_children, sel->beam))
    return BLE_E_INVALID_ARG;
  const TreeSelectArgs a{sel->n, sel->n_children, sel->beam, sel->ret, sel->parent, sel->choice};
  return launch(ble_tree_select_kernel, sel->n, 1, kPlanSelectBlock, stream, a);
}

int ble_tree_finish_f32(const struct ble_tree_finish* fin, void* stream) {
  if (!fin || !fin->ret || !fin->source_status || !fin->choice || !fin->best_plan || !fin->action || !fin->best_return ||
      (fin->q == nullptr) != (fin->visits == nullptr))
    return BLE_E_INVALID_ARG;
  if (!tree_sizes_ok(fin->n, fin->beam) || !tree_children_ok(fin->n_children, fin->beam) || fin->depth < 1 || fin->segment < 1 ||
      (int64_t)fin->depth * fin->segment > BLE_ROLLOUT_MAX_STEPS || (fin->depth == 1 && fin->n_children != 3))
    return BLE_E_INVALID_ARG;
  const TreeFinishArgs a{fin->n, fin->n_children, fin->beam, fin->depth, fin->segment, fin->ret, fin->score ? fin->score : fin->ret,
                         fin->source_status, fin->choice, fin->best_plan, fin->action, fin->best_return, fin->q, fin->visits};
  return launch(ble_tree_finish_kernel, fin->n, 1, kPlanSelectBlock, stream, a);
}

// ---- guided tree search
namespace {
static_assert(kMctsMaxLeaves == BLE_MCTS_MAX_LEAVES && kMctsEmpty == BLE_MCTS_EMPTY && kMctsExpand == BLE_MCTS_EXPAND &&
              kMctsRevisit == BLE_MCTS_REVISIT, "ble_mcts.h and ble_abi.h disagree");
// what all four calls refuse of the pool
inline bool mcts_pool_ok(const struct ble_mcts_pool* p) {
  if (!p || !state_ok(p->nodes.state) || !p->nodes.acc || !p->nodes.disc || !p->nodes.flown || !p->nodes.ret || !p->parent ||
      !p->first_child || !p->depth || !p->visits || !p->pending || !p->value_sum || !p->g || !p->prior || !p->g_range || !p->leaf || !p->kind)
    return false;
  if (p->n < 0 || p->n >= 2147483648LL || p->num_rounds < 1 || p->leaves_per_round < 1 ||
      (int64_t)p->num_rounds * p->leaves_per_round > BLE_MCTS_MAX_LEAVES || p->max_depth < 1 || p->segment < 1 ||
      (int64_t)p->max_depth * p->segment > BLE_ROLLOUT_MAX_STEPS || p->reserved_ != 0)
    return false;
  return p->n * (int64_t)(1 + 3 * p->num_rounds * p->leaves_per_round) < 2147483648LL;
}
inline bool mcts_round_ok(const struct ble_mcts_pool* p, int32_t round) { return round >= 0 && round < p->num_rounds; }
inline MctsPoolDev mcts_pool_dev(const struct ble_mcts_pool* p) {
  return MctsPoolDev{p->n, p->num_rounds, p->leaves_per_round, p->max_depth, p->segment, tree_arena_dev(p->nodes),
                     MctsStats{p->parent, p->first_child, p->depth, p->visits, p->pending, p->value_sum, p->g, p->prior, p->g_range},
                     p->leaf, p->kind};
}
constexpr int kMctsEnvsPerBlock = kMctsBlock;    // select, backup, finish: one lane per environment
// what both expand calls refuse of st and ex, the pool having passed its own checks
inline bool mcts_expand_ok(const ble_state_f32* st, const struct ble_mcts_pool* pool, const struct ble_mcts_expand* ex) {
  return state_ok(st) && ex && ex->wind_grid && mcts_round_ok(pool, ex->round) && ex->action_repeat >= 1 &&
         (int64_t)pool->max_depth * pool->segment * ex->action_repeat <= BLE_ROLLOUT_MAX_STEPS && ex->substeps >= 1 &&
         ex->substeps <= BLE_MAX_SUBSTEPS && ex->reserved_ == 0 && ex->grid_env_stride >= 0 && ex->gamma >= 0.0 && ex->gamma <= 1.0 &&
         !state_arrays_shared(pool->nodes.state, st);                 // (a NaN gamma fails both comparisons)
}
// struct ble_mcts_expand as the expand kernels take it
inline MctsExpandArgs mcts_expand_args(const struct ble_mcts_pool* pool, const struct ble_mcts_expand* ex) {
  return MctsExpandArgs{pool->n, ex->round, pool->segment * ex->action_repeat, ex->substeps, ex->gamma, ex->wind_grid, ex->grid_env_stride};
}
}  // namespace

int ble_mcts_select_f32(const struct ble_mcts_pool* pool, int32_t round, double c_puct, const uint8_t* source_status, const float* root_prior,
                        void* stream) {
  if (!mcts_pool_ok(pool) || !mcts_round_ok(pool, round) || !source_status || !(c_puct >= 0.0 && c_puct <= 1.7976931348623157e308))
    return BLE_E_INVALID_ARG;                                         // (a NaN c_puct fails both comparisons)
  return launch(ble_mcts_select_kernel, pool->n, kMctsEnvsPerBlock, kMctsBlock, stream, mcts_pool_dev(pool), (int)round, c_puct, source_status,
                root_prior);
}

int ble_mcts_expand_f32(const ble_state_f32* st, const struct ble_mcts_pool* pool, const struct ble_mcts_expand* ex, const ble_noise_gen* noise,
                        const ble_gp_belief* belief, uint32_t* err_flags, void* stream) {
  if (!mcts_pool_ok(pool) || !mcts_expand_ok(st, pool, ex)) return BLE_E_INVALID_ARG;
  return with_wind(noise, belief, pool->n, [&](auto wind, BeliefDev b, StepNoise gen) {
    return with_vehicle<false>(st, nullptr, [&](auto veh) {
      if (pool->n == 0) return BLE_OK;
      return launch(ble_mcts_expand_kernel<decltype(wind)::value, decltype(veh)>, pool->n * (int64_t)(3 * pool->leaves_per_round), kStepBlock,
                    kStepBlock, stream, state_dev(st), mcts_expand_args(pool, ex), mcts_pool_dev(pool), b, gen, err_flags, veh);
    });
  });
}

int ble_mcts_backup_f32(const struct ble_mcts_pool* pool, int32_t round, const float* value, const float* probs, void* stream) {
  if (!mcts_pool_ok(pool) || !mcts_round_ok(pool, round) || (value == nullptr) != (probs == nullptr)) return BLE_E_INVALID_ARG;
  return launch(ble_mcts_backup_kernel, pool->n, kMctsEnvsPerBlock, kMctsBlock, stream, mcts_pool_dev(pool), (int)round, value, probs);
}

int ble_mcts_finish_f32(const struct ble_mcts_pool* pool, const struct ble_mcts_finish* fin, void* stream) {
  if (!mcts_pool_ok(pool) || !fin || !fin->source_status || !fin->best_plan || !fin->action || !fin->best_return || !fin->q || !fin->visits ||
      !fin->pv_length)
    return BLE_E_INVALID_ARG;
  const MctsFinishArgs a{fin->source_status, fin->best_plan, fin->action, fin->best_return, fin->q, fin->visits, fin->pv_length};
  return launch(ble_mcts_finish_kernel, pool->n, kMctsEnvsPerBlock, kMctsBlock, stream, mcts_pool_dev(pool), a);
}

// ---- guided tree search in scenario winds
namespace {
// what both scenario calls refuse of the pool and M: the pool's own checks, M, and the node count of a round's slice
inline bool mcts_groups_ok(const struct ble_mcts_pool* p, int64_t num) {
  return mcts_pool_ok(p) && num >= 1 && num <= BLE_SCENARIO_MAX && p->n * (int64_t)(3 * p->leaves_per_round) * num < 2147483648LL;
}
}  // namespace

int ble_mcts_expand_scenarios_f32(const ble_state_f32* st, const struct ble_mcts_pool* pool, const struct ble_mcts_expand* ex,
                                  const ble_gp_scenarios* scn, const ble_scenario_gen* gen, uint32_t* err_flags, void* stream) {
  ScenariosDev b;
  if (!gp_scenarios(scn, &b) || !scenario_gen_ok(gen) || !mcts_groups_ok(pool, scn->num) || scn->n != pool->n || !mcts_expand_ok(st, pool, ex))
    return BLE_E_INVALID_ARG;                                         // (scenarios of another batch would be read out of bounds)
  return with_vehicle<false>(st, nullptr, [&](auto veh) {
    if (pool->n == 0) return BLE_OK;
    return with_scenario_seed(gen, [&](auto seed, ScenarioGen g) {
      return launch(ble_mcts_expand_scenarios_kernel<decltype(veh), decltype(seed)>, pool->n * (int64_t)(3 * pool->leaves_per_round) * scn->num,
                    kStepBlock, kStepBlock, stream, state_dev(st), mcts_expand_args(pool, ex), mcts_pool_dev(pool), b, seed, g, err_flags, veh);
    });
  });
}

int ble_mcts_backup_scenarios_f32(const struct ble_mcts_pool* pool, int32_t round, int32_t num, int32_t tail, const float* value,
                                  const float* probs, uint8_t* group_status, double* group_g, void* stream) {
  if (!mcts_groups_ok(pool, num) || !mcts_round_ok(pool, round) || tail < 1 || tail > num || (value == nullptr) != (probs == nullptr) ||
      !group_status || !group_g)
    return BLE_E_INVALID_ARG;
  return launch(ble_mcts_backup_scenarios_kernel, pool->n, kMctsEnvsPerBlock, kMctsBlock, stream, mcts_pool_dev(pool), (int)round, (int)num,
                (int)tail, value, probs, group_status, group_g);
}

int ble_gp_fit_scenarios_f32(const ble_gp_history_f32* hist, const uint8_t* reset_mask, const int32_t* time_s, const ble_gp_scenarios* scn,
                             const ble_scenario_gen* gen, uint32_t* err_flags, void* stream) {
  GpHistory h;
  ScenariosDev b;
  if (!gp_ring(hist, &h) || !time_s || !gp_scenarios(scn, &b) || !scenario_gen_ok(gen)) return BLE_E_INVALID_ARG;
  return with_scenario_seed(gen, [&](auto seed, ScenarioGen g) {
    return launch(ble_gp_fit_scenarios_kernel<decltype(seed)>, scn->n, 1, kObsBlock, stream, h, reset_mask, time_s, b, seed, g, err_flags);
  });
}

int ble_gp_scenario_wind_f32(const ble_gp_scenarios* scn, const ble_scenario_gen* gen, const int32_t* scenario_index, const float* x_m,
                             const float* y_m, const float* pressure, const int32_t* elapsed_s, int prior_only, float* uv, void* stream) {
  ScenariosDev b;
  if (!gp_scenarios(scn, &b) || !scenario_gen_ok(gen) || !scenario_index || !x_m || !y_m || !pressure || !elapsed_s || !uv ||
      (prior_only != 0 && prior_only != 1))
    return BLE_E_INVALID_ARG;
  const int64_t n = scn->n;
  return with_scenario_seed(gen, [&](auto seed, ScenarioGen g) {
    return launch(ble_gp_scenario_wind_kernel<decltype(seed)>, n, kScenarioWindBlock, kScenarioWindBlock, stream, b, seed, g, scenario_index, x_m,
                  y_m, pressure, elapsed_s, prior_only, uv, n);
  });
}

int ble_rollout_scenarios_f32(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_gp_scenarios* scn,
                              const ble_scenario_gen* gen, uint32_t* err_flags, void* stream) {
  ScenariosDev b;
  if (!gp_scenarios(scn, &b) || !scenario_gen_ok(gen) || !rollout_ok(st, ro, scn->num) || scn->n != ro->n)
    return BLE_E_INVALID_ARG;                                         // (scenarios of another batch would be read out of bounds)
  return with_vehicle<false>(st, nullptr, [&](auto veh) {
    if (ro->n == 0) return BLE_OK;
    return with_scenario_seed(gen, [&](auto seed, ScenarioGen g) {
      return launch(ble_rollout_scenarios_kernel<decltype(veh), decltype(seed)>, ro->n * (int64_t)ro->n_plans * scn->num, kStepBlock, kStepBlock,
                    stream, state_dev(st), rollout_args(ro), b, seed, g, err_flags, veh);
    });
  });
}

int ble_plan_risk_f32(const struct ble_plan_risk* risk, void* stream) {
  if (!risk || !risk->ret || !risk->score || risk->n < 0 || risk->n >= 2147483648LL || risk->n_plans < 1 || risk->n_plans > BLE_PLAN_MAX_PLANS ||
      risk->num < 1 || risk->num > BLE_SCENARIO_MAX || risk->tail < 1 || risk->tail > risk->num ||
      risk->n * (int64_t)risk->n_plans * risk->num >= 2147483648LL)
    return BLE_E_INVALID_ARG;
  const PlanRiskArgs a{risk->n, risk->n_plans, risk->num, risk->tail, risk->ret, risk->score};
  return launch(ble_plan_risk_kernel, risk->n * (int64_t)risk->n_plans, 256, 256, stream, a);
}

}  // extern "C"
