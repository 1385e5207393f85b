// ble_step_helper.h -- the one-lane transition with the sun on a co-resident helper wave.
//
// At 65 536 environments ble_step_kernel runs one wave per SIMD and is bound by instruction issue: a lone wave pays a full issue slot for
// every 32-bit instruction the SIMD could retire in half of it (profiles/r02_microbench.md, valu_op_cost).  Here every group of 64
// environments has two full waves on one SIMD, lane = environment in both:
//   M  agent_step without the solar block: the whole fp64 carried chain, the atmosphere window, the safety layers, the wind, the
//      attenuation's pressure half, power, battery, parking, reward;
//   S  what does not depend on the state: the ephemeris (a step AHEAD of M), the three solar nodes, sun_at_stride for every stride and
//      for the reward, the panel factor, the flux ramp and the attenuation's pressure-independent half -- one 16-byte SunRecord per stride.
// S never reads anything M computes inside a step and M never waits for S inside a stride unless S is behind (stride 0 of a step at most):
// no barrier after the prologue.  The hand-over is LDS: M publishes (x, y, u, v, t_elapsed, live lanes) once per step -- the first thing it
// does in a step, as soon as the wind gather has landed: S computes the three site nodes while M runs its own per-step part --, S fills a ring of
// kHelperRing records per lane; three monotonic counters per group (steps published, records ready, records taken) order it.  A write
// is followed by s_waitcnt lgkmcnt(0) and then the counter's store; a wave's LDS operations execute in order.
// Both loops are driven by the scalar n_steps and substeps alone; M publishes every step, also when none of its lanes is live (then S
// produces nothing and M reads nothing: both see the same ballot), so neither can wait for something that does not come.
// S and M call the lane functions of ble_step_core.h; a value crosses in the type it has there: bit-identical to ble_step_kernel.
#pragma once
#include "ble_step_core.h"

namespace ble {

constexpr int kHelperGroups = 4;                       // groups of 64 environments per workgroup: one per SIMD of a CU
constexpr int kHelperBlock = 2 * 64 * kHelperGroups;   // M and S of every group
constexpr int kHelperRing = 32;                        // records per lane S may be ahead of M (a power of two): more than the 19 of a default step

struct alignas(16) HelperGroupShared {
  SunRecord ring[kHelperRing][64];
  SunRecord reward_park[64];          // the reward's record of a lane whose episode ended inside the step
  float x[64], y[64], u[64], v[64];   // M's publication of a step
  int32_t t_elapsed[64];
  unsigned long long live;            // ballot of M's live lanes in that step
  int steps_published;                // M
  int records_taken;                  // M: every record below this index has been read
  int records_ready;                  // S: every record below this index is written
  int pad_;
};
struct HelperShared {
  HelperGroupShared group[kHelperGroups];
  int ticket[4];                      // waves that have arrived on each SIMD
  int placed[kHelperBlock / 64];      // the role each wave drew (-1: its SIMD was full)
};

BLE_FN int helper_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
BLE_FN int helper_counter_load(const int* p) { return helper_uniform(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)); }
// data first, then the counter (see the header)
BLE_FN void helper_counter_store(int* p, int v) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
BLE_FN void helper_wait_above(const int* p, int need, int* seen) {       // until *p > need
  int r = helper_counter_load(p);
  while (r <= need) { __builtin_amdgcn_s_sleep(1); r = helper_counter_load(p); }
  *seen = r;
  asm volatile("" ::: "memory");
}

// Roles of the workgroup's eight waves: 2 g = M of group g, 2 g + 1 = its S.  The first wave to arrive on SIMD q is M of group q, the
// second its S (HW_REG_HW_ID; a ticket per SIMD in LDS); a wave that finds its SIMD full takes the lowest free role -- every wave derives
// the same map from `placed`, so the roles are a permutation whatever the placement was.  Two barriers (the prologue's); zeroes the counters.
BLE_FN int helper_assign_roles(HelperShared& sh, int hw_wave, int lane) {
  // HW_REG_HW_ID (register 4): bits 5:4 = SIMD id  ->  s_getreg_b32 hwreg(4, 4, 2): simm16 = (size - 1) << 11 | offset << 6 | id
  const int simd = (int)__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4) & 3;
  const int tid = hw_wave * 64 + lane;
  if (tid < 4) sh.ticket[tid] = 0;
  if (tid < kHelperGroups) {
    sh.group[tid].live = 0ull; sh.group[tid].steps_published = 0; sh.group[tid].records_taken = 0; sh.group[tid].records_ready = 0;
  }
  __syncthreads();
  if (lane == 0) {
    const int t = atomicAdd(&sh.ticket[simd], 1);
    sh.placed[hw_wave] = t < 2 ? 2 * simd + t : -1;
  }
  __syncthreads();
  constexpr int kWaves = kHelperBlock / 64;
  int taken = 0, unplaced_before = 0;
#pragma unroll
  for (int q = 0; q < kWaves; ++q) {
    const int p = helper_uniform(sh.placed[q]);
    if (p >= 0) taken |= 1 << p;
    else if (q < hw_wave) ++unplaced_before;
  }
  int role = helper_uniform(sh.placed[hw_wave]);
  if (role < 0) {
    role = 0;
#pragma unroll
    for (int r = 0, free_seen = 0; r < kWaves; ++r)
      if (!((taken >> r) & 1)) { if (free_seen == unplaced_before) role = r; ++free_seen; }
  }
  return role;
}

// M's side of the hand-over: agent_step's `helper`.  base: the index of the step's first record; ready_seen: the last value read of the
// group's records_ready (the counter is read again only when it does not cover the record wanted: S is up to kHelperRing ahead).
// steps_done: the kernel's own scalar loop index + 1, set by the kernel on the whole wave before every step -- what both publications
// store; never a count carried here.  base and ready_seen ARE carried, and agent_step updates them under the mask of the live lanes only:
// they are read under that mask alone, and a lane that is live now was live in every earlier step of the launch, so its copy is current.
struct HelperMain {
  static constexpr bool kOn = true;
  HelperGroupShared* g;
  int lane;
  int base, ready_seen, steps_done;
  BLE_FN void publish(float x, float y, float u, float v, int32_t t_elapsed) {
    g->x[lane] = x; g->y[lane] = y; g->u[lane] = u; g->v[lane] = v; g->t_elapsed[lane] = t_elapsed;
    g->live = __builtin_amdgcn_ballot_w64(true);          // (every lane that runs this step writes the same ballot)
    helper_counter_store(&g->steps_published, steps_done);
  }
  BLE_FN SunRecord read(int index) const { return g->ring[index & (kHelperRing - 1)][lane]; }
  // the record of stride k.  On even strides: tells S that every earlier record of the ring has been read (the reads were issued before this store).
  BLE_FN SunRecord record(int k) {
    const int index = helper_uniform(base) + k;
    if ((k & 1) == 0) {
      asm volatile("" ::: "memory");
      __hip_atomic_store(&g->records_taken, index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (__builtin_expect(helper_uniform(ready_seen) <= index, 0)) helper_wait_above(&g->records_ready, index, &ready_seen);
    return read(index);
  }
  // the reward's record of a lane that has not ended: the sun after the last stride; then the step's records are done with
  BLE_FN SunRecord record_end(int substeps) {
    const int index = helper_uniform(base) + substeps;
    if (__builtin_expect(helper_uniform(ready_seen) <= index, 0)) helper_wait_above(&g->records_ready, index, &ready_seen);
    const SunRecord r = read(index);
    base = index + 1;
    return r;
  }
  // rare (inside the end-of-episode block, some lanes only): the record of stride k is the reward's sun of a lane that ran k strides.  It
  // is at most one ahead of the stride being run; kept aside because the ring may wrap before the reward is formed.
  BLE_FN void park_reward_record(int k) {
    const int index = helper_uniform(base) + k;
    int seen;
    helper_wait_above(&g->records_ready, index, &seen);
    g->reward_park[lane] = read(index);
  }
  BLE_FN SunRecord parked_reward_record() const { return g->reward_park[lane]; }
  // a step in which no lane is live: nothing is read, S is told so
  BLE_FN void publish_idle() {
    g->live = 0ull;
    helper_counter_store(&g->steps_published, steps_done);
  }
};

// S: the whole life of a helper wave.  `i`: the environment of this lane (that of M's lane of the same number); `in_range`: it exists.
BLE_FN void helper_wave(const StateDev& st, HelperGroupShared* g, int lane, int64_t i, bool in_range, int substeps, int n_steps) {
  EnvConst c = {0.0f, 0.0f, 0.0f, 0.0f, 0};
  int32_t t_s = 0;                     // the step's start time as S predicts it: a lane that stays live advances by a whole step
  bool ok = false;
  if (in_range) {
    c.lat0_deg = st.center_lat_deg[i]; c.lng0_deg = st.center_lng_deg[i];
    c.ir = st.upwelling_infrared[i]; c.alpha = st.alpha[i]; c.start_unix = st.start_unix[i];
    t_s = st.time_elapsed_s[i];
    ok = st.status[i] == kOk;
  }
  // hoist_constants' sincos, once per launch, always: the episode cache's row of this environment is M's to read and to rewrite (a key
  // read here next to M's store of a missed entry could pair new keys with old values); the cached pair came from this very expression
  double sin_lat0 = 0.0, cos_lat0 = 1.0;
  if (ok) sincos_f64((double)c.lat0_deg * (kPiD / 180.0), &sin_lat0, &cos_lat0);
  const float step_s = (float)(10 * substeps);
  int next = 0;                        // index of the next record
  int taken_seen = 0, published_seen = 0;
  bool all_frozen = false;             // (scalar) M has published a step without a live lane: the waits below are all that is left
#pragma unroll 1
  for (int step = 0; step < n_steps; ++step) {
    // ---- ahead of M: what needs the time alone
    int64_t t0 = c.start_unix + (int64_t)t_s;
    Ephemeris e0 = {};
    SolarNodes nodes = {};
    if (!all_frozen) {
      e0 = ephemeris(t0);
      nodes = solar_nodes_time(e0, t0, c.lng0_deg, step_s);
    }
    // ---- M's publication of this step
    if (published_seen <= step) helper_wait_above(&g->steps_published, step, &published_seen);
    const unsigned long long live_mask = g->live;
    const uint32_t live_lo = (uint32_t)helper_uniform((int)(uint32_t)live_mask), live_hi = (uint32_t)helper_uniform((int)(uint32_t)(live_mask >> 32));
    if (live_lo == 0u && live_hi == 0u) { all_frozen = true; continue; }          // no live lane: M reads no record of this step (and of no later one)
    const bool live = (((lane < 32 ? live_lo : live_hi) >> (lane & 31)) & 1u) != 0u;
    float x = g->x[lane], y = g->y[lane], u = g->u[lane], v = g->v[lane];
    int32_t t_pub = g->t_elapsed[lane];
    if (!live) { x = 0.0f; y = 0.0f; u = 0.0f; v = 0.0f; t_pub = t_s; }
    const bool moved = t_pub != t_s;             // never for a lane that was live in every earlier step of the launch; the prediction is a convenience, not a premise
    if (__builtin_expect(wave_any(moved), 0)) if (moved) {
      t_s = t_pub;
      t0 = c.start_unix + (int64_t)t_s;
      e0 = ephemeris(t0);
      nodes = solar_nodes_time(e0, t0, c.lng0_deg, step_s);
    }
    const float fl0 = e0.flux, dfl = e0.flux_rate * 10.0f;
    const SunQuadratic sq = solar_nodes_site(nodes, sin_lat0, cos_lat0, x, y, u, v, substeps);
    // ---- one record per stride, and the reward's (kk == substeps)
#pragma unroll 1
    for (int kk = 0; kk <= substeps; ++kk) {
      const SunState sun = sun_at_stride(kk, sq, c, u, v, x, y, t_s);
      SunRecord rec;
      rec.diff = solar_airmass_diff(sun.sin_el);
      rec.panel_factor = solar_panel_factor(sun);
      rec.flux = f_fma((float)kk, dfl, fl0);
      rec.bits = sun.day ? 1u : 0u;
      // room in the ring: record `next` replaces record next - kHelperRing
      if (__builtin_expect(next - taken_seen >= kHelperRing, 0)) helper_wait_above(&g->records_taken, next - kHelperRing, &taken_seen);
      g->ring[next & (kHelperRing - 1)][lane] = rec;
      ++next;
      helper_counter_store(&g->records_ready, next);
    }
    t_s += 10 * substeps;
  }
}

}  // namespace ble
