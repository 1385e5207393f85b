/*
 * ble_abi.h -- C ABI of libble_hip.so, the MI355X (gfx950) vectorised Balloon Learning
 * Environment transition.
 *
 * The reference (google/balloon-learning-environment, pure Python) has no FFI for this
 * path; the seams it does have are Python classes.  Each entry point below replaces the
 * arithmetic behind one of those seams, for N environments at once, and is what a
 * ctypes binding inside the reference would call (INTEGRATION.md shows the stub).
 * Paths are relative to /root/reference/balloon_learning_environment/.
 *
 * Conventions
 *  - All array pointers are DEVICE pointers (HIP), caller-owned, struct-of-arrays,
 *    length n unless stated.  No torch types, no C++ types.
 *  - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream).  The caller keeps the buffers alive until the stream has passed
 *    the call, and synchronises before reading results on the host.
 *  - Return value: BLE_OK (0) or a negative BLE_E_* code for host-side argument / launch
 *    errors.  The library never throws, aborts or asserts on the device.  Conditions on
 *    which the reference raises *inside* the arithmetic (range checks) are OR-ed into
 *    the device word `err_flags` (BLE_FLAG_*), which the host mirror turns back into the
 *    reference's exceptions.
 *  - Arguments are checked before anything else: an invalid one answers BLE_E_INVALID_ARG
 *    whatever n is, n == 0 included; valid arguments with n == 0 answer BLE_OK and launch
 *    nothing.
 *  - Thread-safe.  The library's global state is the step form (ble_set_step_form:
 *    process-global, atomic) and the status of each thread's last launch (ble_last_hip_error:
 *    per thread).  Different streams may run concurrently on disjoint buffers.
 *  - Units and encodings follow the reference: metres, Pa, K, mol, Wh, W, kg/s, seconds;
 *    actions 0=DOWN 1=STAY 2=UP (env/balloon/control.py:21-25); status 0=OK
 *    1=OUT_OF_POWER 2=BURST 3=ZEROPRESSURE (env/balloon/balloon.py:66-70).
 */
#ifndef BLE_ABI_H_
#define BLE_ABI_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ble_state_f32 gained the optional episode_cache; ble_wind_noise_f32 the optional harmonic_cache; ble_gp_history_f32 gained chol_stride and the carried slab grew to 7620 doubles (packed Cholesky L -> Lt D Lt^T +
 *    drop vector + zeta / d): a caller built against version 1 allocates 7260 doubles per environment. */
/* 3: ble_step_n_f32 gained `noise` (ble_noise_gen: the wind-noise generator evaluated inside the fused rollout). */
/* 4: ble_set_step_form, ble_probe_latlng_f64, the shard forms ble_reset_at_f32 / ble_wind_noise_at_f32 / ble_noise_gen.env_offset. */
/* 5: ble_state_f32 gained the optional `vehicle` (ble_vehicle: BalloonState's flight-vehicle constants and
 *    power_safety_layer_enabled as run-time inputs); ble_noise_primitive_version(); ble_set_step_form(2) is refused (the two-wavefront
 *    form left the library); ble_step_n_f32 rejects a negative ble_noise_gen.env_offset. */
#define BLE_ABI_VERSION 5

/* Version of the wind-noise PRIMITIVE's bit pattern (csrc/ble_noise.h::simplex4 and the hash / draw streams under it).  The primitive
 * is this library's own (the reference's opensimplex==0.3 noise4d is absent and unpinned), so its values are defined by this
 * repository -- and whenever they change, for whatever reason, this number is bumped: a noise seed recorded against version k flies
 * the same wind only on a library that reports k.  The host mirror refuses a library whose version differs from the one its oracle
 * (oracle/noise_oracle.py::PRIMITIVE_VERSION) and the committed fixture (tests/golden/f14_wind_noise.npz::noise_primitive_version)
 * were made with; checkpoints carry it.  1: rounds 2-4.  2: round 5 (explicit FMAs in a corner's sums, offsets by select). */
#define BLE_NOISE_PRIMITIVE_VERSION 2

/* return codes */
#define BLE_OK 0
#define BLE_E_INVALID_ARG (-1) /* NULL required pointer, n < 0, substeps outside 1 .. BLE_MAX_SUBSTEPS ... */
#define BLE_E_LAUNCH (-2)      /* hipLaunchKernel / hipGetLastError failed */
#define BLE_E_NO_DEVICE (-3)   /* no HIP device visible */

/* bits OR-ed into *err_flags by the kernels (where the reference raises) */
#define BLE_FLAG_PRESSURE_RANGE 1u /* standard_atmosphere.py:126-127 assert */
#define BLE_FLAG_ABSORPTIVITY 2u   /* thermal.py:142-145 ValueError */
#define BLE_FLAG_SOLAR_RANGE 4u    /* solar.py:190-197 ValueError */
#define BLE_FLAG_POWER_TABLE 16u   /* power_table.py:24 assert */
#define BLE_FLAG_NONFINITE 32u     /* a state value became NaN/Inf (no reference analogue) */
#define BLE_FLAG_GP_WINDOW 64u     /* > 120 observations inside the WindGP's 6 h window (steps < 180 s): oldest dropped */
#define BLE_FLAG_PRESSURE_SEARCH 128u /* pressure_range_builder.py:104-108,180-182 ValueError */
#define BLE_FLAG_DAY_CYCLE 256u    /* features.py:432-437 ZeroDivisionError: the next sunrise exactly one day after the next sunset
                                      (polar night); the two day-cycle features of that environment are NaN */
#define BLE_FLAG_VEHICLE_INDEX 512u /* a fleet call (ble_fleet): an environment's vehicle_index >= n_vehicles -- the lane is frozen
                                       (state, history and observation untouched), nothing is read outside the palette */
#define BLE_FLAG_AGENT_NO_LEVEL 1024u /* ble_station_seeker_f32: no valid pressure level (station_seeker_agent.py:113-115 assert), or a
                                         feature the score reads is not finite -- action STAY (1), level -1 */

/* wind grid geometry: generative/vae.py:30-38,77-93 (FieldShape defaults) */
#define BLE_GRID_NX 21 /* x (lat axis of the grid), -500..500 km step 50 */
#define BLE_GRID_NY 21 /* y, -500..500 km step 50 */
#define BLE_GRID_NP 10 /* pressure, 5000..14000 Pa step 1000 */
#define BLE_GRID_NT 9  /* time, 0..48 h step 6 */
#define BLE_GRID_FLOATS (BLE_GRID_NX * BLE_GRID_NY * BLE_GRID_NP * BLE_GRID_NT * 2) /* 79380 */
#define BLE_COUNT_SLOTS 64 /* width of the live-environment counter, see ble_step_f32 */

/*
 * BalloonState's flight-vehicle constants (balloon.py:156-172: dataclass FIELDS with defaults), mols_lift_gas (:183, a state
 * field no transition changes) and power_safety_layer_enabled (:200, read by simulate_step :305).  A HOST struct of doubles --
 * the reference's are Python floats and several defaults (0.0199, 183.7, 3058.56) are not float32 numbers.  One vehicle per
 * call: every environment of a batch flies the same one (the reference builds one BalloonState per balloon; batches of
 * different vehicles are different calls).  ble_vehicle_default() fills in the reference's defaults.
 */
typedef struct ble_vehicle {
  double envelope_volume_base;         /* [m^3]   1804      balloon.py:157 */
  double envelope_volume_dv_pressure;  /* [m^3/Pa] 0.0199   :158 */
  double envelope_mass;                /* [kg]    68.5      :159 */
  double envelope_max_superpressure;   /* [Pa]    2380      :160 (burst threshold and EnvelopeSafetyLayer's argument, :204-205) */
  double envelope_cod;                 /* [.]     0.25      :163 */
  double payload_mass;                 /* [kg]    92.5      :166 */
  double nighttime_power_load_w;       /* [W]     183.7     :168 */
  double daytime_power_load_w;         /* [W]     120.4     :169 */
  double acs_valve_hole_diameter_m;    /* [m]     0.04      :171 */
  double battery_capacity_wh;          /* [Wh]    3058.56   :173 */
  double mols_lift_gas;                /* [mol]   6830      :183 */
  int32_t power_safety_layer_enabled;  /* bool    1         :200 */
  int32_t reserved_;                   /* 0 */
} ble_vehicle;

/*
 * Per-environment simulator state, struct of device arrays.
 * Replaces: BalloonState (env/balloon/balloon.py:73-250), the three safety-layer
 * objects it owns (altitude_safety.py:63-111, envelope_safety.py:93-157,
 * power_safety.py:26-126) and Atmosphere's per-episode alpha
 * (standard_atmosphere.py:76-87).
 * The flight-vehicle constants: `vehicle` below (ABI 5).  NULL -- every BASELINE configuration -- selects kernels in which the
 * reference's defaults are compile-time constants (csrc/ble_physics.h::VehicleDefault); a non-NULL vehicle selects a second
 * instantiation of the same lane functions that reads them from scalar registers (csrc/ble_physics.h::VehicleRt).
 */
typedef struct ble_state_f32 {
  /* mutable, read+written by ble_step_f32 (balloon.py:175-195) */
  float* x;                    /* [m]  units.Distance x, W->E offset from the station */
  float* y;                    /* [m] */
  float* pressure;             /* [Pa] */
  float* ambient_temperature;  /* [K] */
  float* internal_temperature; /* [K] */
  float* envelope_volume;      /* [m^3] */
  float* superpressure;        /* [Pa] */
  float* mols_air;             /* [mol] */
  float* battery_charge;       /* [Wh] */
  /* derived, written by ble_step_f32 (balloon.py:189-193) */
  float* acs_power;      /* [W] */
  float* acs_mass_flow;  /* [kg/s] */
  float* solar_charging; /* [W] */
  float* power_load;     /* [W] */
  /* per-episode constants, read only */
  const float* center_lat_deg;     /* BalloonState.center_latlng */
  const float* center_lng_deg;
  const float* upwelling_infrared; /* [W/m^2] balloon.py:208 */
  const float* alpha;              /* Atmosphere lapse-rate mix, standard_atmosphere.py:82-84 */
  const int64_t* start_unix;       /* date_time when time_elapsed == 0, UTC seconds */
  /* clocks: date_time = start_unix + time_elapsed_s (balloon.py:546-547) */
  int32_t* time_elapsed_s;
  /* PowerSafetyLayer._sunrise_with_hysteresis / ._sunset, seconds relative to start_unix */
  int32_t* sunrise_h_rel;
  int32_t* sunset_rel;
  /* discrete state */
  uint8_t* status;       /* BalloonStatus */
  uint8_t* last_command; /* raw action of the last step, balloon.py:286 */
  uint8_t* alt_fsm;      /* 0 NOMINAL 1 LOW 2 VERY_LOW         (altitude_safety.py:40-44) */
  uint8_t* env_fsm;      /* 0 NOMINAL 1 LOW_CRITICAL 2 LOW 3 HIGH 4 HIGH_CRITICAL (envelope_safety.py:45-50) */
  uint8_t* power_paused; /* PowerSafetyLayer.navigation_is_paused */
  /* OPTIONAL (may be NULL), opaque: [BLE_EPISODE_CACHE_ROWS][n] doubles, zero-initialised by the caller.  What the
   * transition derives from the per-episode constants alone (the atmosphere's two transition pressures -- two pows --,
   * sin / cos of the centre latitude, the earth-IR heat per unit area), keyed by the bit patterns of (alpha,
   * center_lat_deg, upwelling_infrared).  ble_reset_f32 fills it; ble_step_f32 / ble_step_n_f32 read it and, where an
   * entry does not match the constants in `st` (edited by hand, or never reset on the device), recompute and store it --
   * so it can never go stale.  NULL: recomputed by every launch (0.8 us per launch).  Entries are functions of the episode's
   * constants alone, not of the vehicle. */
  double* episode_cache;
  /* OPTIONAL (may be NULL), ABI 5: HOST pointer to the vehicle every environment of this call flies, read on the host when the
   * call is made (not retained).  NULL = the reference's defaults.  Honoured by ble_step_f32 / ble_step_n_f32 (one lane per
   * environment whatever the batch size), ble_reset_f32 / ble_reset_at_f32 (the cold start) and ble_observe_f32 (battery state of
   * charge, excess energy, the reachable pressure range).  A vehicle with a non-positive volume base, dV/dp, capacity, drag
   * coefficient or maximum superpressure <= 300 Pa (envelope_safety.py's bands would overlap) is rejected with BLE_E_INVALID_ARG. */
  const ble_vehicle* vehicle;
} ble_state_f32;
#define BLE_EPISODE_CACHE_ROWS 7
#define BLE_MAX_SUBSTEPS 60
/* Up to this many environments ble_step_f32 / ble_step_n_f32 -- with or without a wind-noise generator -- run the
 * four-wavefronts-per-environment form of the transition (csrc/ble_step_split.h: 4 x n / 64 waves -- one per SIMD up to
 * 16 384 environments, two up to 32 768), above it the one-lane-per-environment kernel (one wave per SIMD at 65 536).
 * Above it, without a wind-noise generator and while ceil(n / 64) <= 4 x the device's compute units (every SIMD has a free
 * second wave slot: n <= 65 536 on 256 CUs), the one-lane kernel flies with a helper wave per 64 environments that evaluates the
 * strides' sun (csrc/ble_step_helper.h, BLE_STEP_FORM_HELPER).
 * The forms are bit-identical; ble_set_step_form() forces one.  A run-time vehicle (st->vehicle) or a fleet always flies the
 * one-lane form, whatever ble_set_step_form or the automatic choice says. */
#define BLE_SPLIT_MAX_ENVS 32768
/* ble_set_step_form's value for the one-lane form with a helper wave (not a number of wavefronts per environment; additive, ABI
 * version unchanged).  A launch with a wind-noise generator flies the plain one-lane form when this is forced. */
#define BLE_STEP_FORM_HELPER 12

int ble_abi_version(void);

/* BLE_NOISE_PRIMITIVE_VERSION of the loaded library (above). */
int ble_noise_primitive_version(void);

/* Fills *v with the reference's defaults (balloon.py:156-173,183,200); returns BLE_OK or BLE_E_INVALID_ARG (v == NULL). */
int ble_vehicle_default(ble_vehicle* v);

/* hipError_t (as int) of the calling thread's most recent launch through this library; 0 = success.
 * Diagnostic companion of BLE_E_LAUNCH. */
int ble_last_hip_error(void);

/* Which form of the transition kernel ble_step_f32 / ble_step_n_f32 launch: 0 = automatic (by batch size, above), 1 = one
 * lane per environment, 4 = four wavefronts per environment, BLE_STEP_FORM_HELPER (12) = one lane per environment plus a helper
 * wave per 64 environments.  2 is refused with BLE_E_INVALID_ARG since ABI 5, like every other
 * value: the two-wavefront form was never selected and measured slower at every batch size.
 * Process-global, thread-safe; takes effect with the next launch.  Returns the previous setting (>= 0) or
 * BLE_E_INVALID_ARG.  The initial value comes from BLE_STEP_SPLIT in the process environment when the library first looks at
 * it -- once, not per launch: 0 -> one lane, 1 or 4 -> four wavefronts, anything else (2 included) or
 * unset -> automatic.  (ABI 4; ABI 3 re-read the variable on every launch.)  Honoured for the default vehicle only: a run-time
 * vehicle or a fleet always flies the one-lane form. */
int ble_set_step_form(int waves_per_env);

/* The form of the calling thread's most recent ble_step_f32 / ble_step_n_f32 launch (or of their fleet forms): 1, 4 or
 * BLE_STEP_FORM_HELPER -- what was forced, or what the automatic choice took (above); 0 before the first launch.  A launch the
 * automatic choice could not decide (the device would not tell its compute units) fails with BLE_E_NO_DEVICE and leaves this
 * alone.  Diagnostic, like ble_last_hip_error.  Additive, ABI version unchanged. */
int ble_last_step_form(void);

/* Number of visible HIP devices (>= 0) or BLE_E_NO_DEVICE. */
int ble_device_count(void);

/*
 * One agent step (180 s = `substeps` x 10 s) for n environments.  `substeps` = time_delta / stride of
 * Balloon.simulate_step, 1 .. BLE_MAX_SUBSTEPS: the reference's 18, and up to 10 minutes per step, are held to
 * the parity bar (tests/test_gpu_parity.py); beyond that the per-step solar interpolation and the float32
 * accumulators of the state drift past 1e-5 (measured at 120), so longer steps are refused, not approximated.
 * Replaces BalloonArena.step (env/balloon_arena.py:184-202) up to, not including, the
 * feature constructor:
 *     wind = WindField.get_ground_truth(x, y, pressure, time_elapsed)   wind_field.py:125-145
 *          = GridBasedWindField.get_forecast(...) + noise               grid_based_wind_field.py:70-94
 *     Balloon.simulate_step(wind, atmosphere, action, 3 min, 10 s)     balloon.py:263-328
 * and BalloonEnv.step's reward / terminal (env/balloon_env.py:172-186,
 * perciatelli_reward_function :44-102).
 *
 *   st            state, mutated in place
 *   action        n bytes, 0 DOWN / 1 STAY / 2 UP (control.py:22-26).  Not range-checked on the device (the reference's
 *                 AltitudeControlCommand(3) raises on the host, and so does this package's single-environment facade):
 *                 any other value flies like STAY and is stored in last_command as given
 *   wind_grid     BLE_GRID_FLOATS floats, row-major (x, y, pressure, time, uv) = the
 *                 reference's `field` ndarray (21,21,10,9,2)
 *   grid_env_stride  0: one grid shared by all envs; otherwise env i reads
 *                 wind_grid + i * grid_env_stride (floats) -- per-env forecasts
 *   noise_uv      optional n x 2 additive wind noise [m/s] (the SimplexWindNoise term,
 *                 simplex_wind_noise.py; NULL = 0)
 *   reward        n floats out;  terminal  n bytes out (status != OK after the step)
 *   effective_action  optional n bytes out: the action after the three safety layers
 *   err_flags     optional device uint32, BLE_FLAG_* OR-ed in
 *   active_count  optional device uint64[BLE_COUNT_SLOTS]: the number of envs that were
 *                 actually stepped (status == OK on entry) is ADDED, spread over the slots
 *                 (one same-address atomic per wave would serialise 1 024 waves for ~11 us);
 *                 the caller sums the slots
 * Envs whose status != OK on entry are skipped: state untouched, reward 0, terminal 1
 * (the reference raises AssertionError, balloon.py:288-290; the host mirror does too).
 * The form of the kernel: BLE_SPLIT_MAX_ENVS and ble_set_step_form above; a run-time vehicle flies the one-lane form
 * whatever they say.
 */
int ble_step_f32(const ble_state_f32* st, const uint8_t* action, const float* wind_grid,
                 int64_t grid_env_stride, const float* noise_uv, float* reward, uint8_t* terminal,
                 uint8_t* effective_action, uint32_t* err_flags, unsigned long long* active_count,
                 int64_t n, int substeps, void* stream);

/*
 * The wind-noise generator of a fused rollout: the arguments of ble_wind_noise_f32 (below) that do not change from
 * step to step.  One noise field per (seed, environment index, episode[i]).
 */
typedef struct ble_noise_gen {
  unsigned long long seed;
  const uint32_t* episode;  /* optional device uint32[n]: the per-environment episode counters ble_reset_f32 maintains (NULL = 0) */
  uint32_t* harmonic_cache; /* optional, as for ble_wind_noise_f32: [BLE_NOISE_CACHE_ROWS][n] words */
  int64_t env_offset;       /* ABI 4: index of this call's environment 0 in the GLOBAL batch (0 on one GPU; the shard's first
                               environment on a rank of a sharded run).  The noise field of environment i is keyed by
                               (seed, env_offset + i, episode[i]): a sharded batch flies the fields the unsharded one does */
} ble_noise_gen;

/*
 * `n_steps` consecutive agent steps in ONE kernel launch: the state stays in registers
 * between the steps (loaded once, stored once); per step only the action is read and
 * reward / terminal are written.  action / reward / terminal are [n_steps][n] row-major;
 * active_count, if given, is [n_steps][BLE_COUNT_SLOTS].  Same semantics per step as
 * ble_step_f32.
 *   noise   NULL: every step flies in the forecast (WindField.get_forecast; noise term 0, SURVEY 8(d)'s bench
 *           definition).  Otherwise the reference's WindField.get_ground_truth (wind_field.py:125-145): at every
 *           step the SimplexWindNoise term is evaluated inside the kernel at the pre-step (x, y, pressure, elapsed)
 *           with the generator `noise` describes -- bit for bit what n_steps rounds of ble_wind_noise_f32(mode 0)
 *           followed by ble_step_f32(noise_uv) produce (tests/test_gpu_parity.py).
 */
int ble_step_n_f32(const ble_state_f32* st, const uint8_t* action, const float* wind_grid,
                   int64_t grid_env_stride, const ble_noise_gen* noise, float* reward, uint8_t* terminal,
                   uint32_t* err_flags, unsigned long long* active_count, int64_t n, int substeps, int n_steps,
                   void* stream);

/*
 * Episode reset on the device for the environments with mask[i] != 0 (mask NULL = all).
 * Replaces BalloonArena.reset's balloon part (env/balloon_arena.py:161-182,228-268):
 *   sample != 0  draw alpha, start time, position, centre lat/lng, pressure, upwelling IR with the
 *                reference's distributions (utils/sampling.py:37-152) from a Philox4x32-10 stream
 *                keyed by (seed, env index, episode[i]); episode[i] (optional device uint32[n]) is
 *                then incremented.  (The reference's JAX threefry streams are not reproduced.)
 *   sample == 0  keep x, y, pressure, center_lat/lng_deg, upwelling_infrared, alpha, start_unix.
 * then stable_init.cold_start_to_stable_params (env/balloon/stable_init.py:132-157),
 * PowerSafetyLayer.__init__'s sunrise/sunset search (env/balloon/power_safety.py:40-48 ->
 * env/balloon/solar.py:432-483), battery 2905.6 Wh, clocks 0, FSMs NOMINAL, status OK.
 * Writes the per-episode "constants" of `st` too when sample != 0 (they are const only to
 * ble_step_f32).  The wind field is reset by the caller (new grid pointer / contents).
 */
int ble_reset_f32(const ble_state_f32* st, const uint8_t* mask, unsigned long long seed,
                  uint32_t* episode, int sample, uint32_t* err_flags, int64_t n, void* stream);
/* The same for a SHARD of a larger batch (ABI 4): environment i of this call is environment env_offset + i of the global
 * batch and draws from the Philox stream (seed, env_offset + i, episode[i]) -- the union of the shards' resets is the reset
 * of the unsharded batch, whatever the sharding.  ble_reset_f32 is this with env_offset = 0. */
int ble_reset_at_f32(const ble_state_f32* st, const uint8_t* mask, unsigned long long seed,
                     uint32_t* episode, int sample, uint32_t* err_flags, int64_t env_offset, int64_t n, void* stream);

/*
 * GridBasedWindField.get_forecast (grid_based_wind_field.py:70-94,145-187) for n query
 * points: clamp, time boomerang, float32 query packing, 16-corner interpolation.
 */
int ble_forecast_f32(const float* wind_grid, int64_t grid_env_stride, const float* x_m,
                     const float* y_m, const float* pressure, const int32_t* elapsed_s, float* u,
                     float* v, int64_t n, void* stream);

/*
 * GridBasedWindField.get_forecast_column (grid_based_wind_field.py:96-132): for each of
 * n (x, y, elapsed) columns, the forecast at `n_levels` shared pressure levels.
 * out_uv is [n][n_levels][2].
 */
int ble_forecast_column_f32(const float* wind_grid, int64_t grid_env_stride, const float* x_m,
                            const float* y_m, const int32_t* elapsed_s, const float* levels_pa,
                            int n_levels, float* out_uv, int64_t n, void* stream);

/*
 * Observation for n environments: PerciatelliFeatureConstructor.observe + get_features
 * (env/features.py:301-330,400-581) with its WindGP (env/wind_gp.py:90-241: Matern nu = 0.5,
 * refit on the observations of the last 6 h) and get_pressure_range
 * (env/balloon/pressure_range_builder.py:203-275).  One workgroup per environment.
 *
 *   noise_uv     optional [n][2]: measured wind minus forecast at the balloon (the reference's
 *                WindGP.observe error term, wind_gp.py:118-123); NULL = 0
 *   reset_mask   optional [n]: != 0 starts a new episode's history (the reference builds a new
 *                feature constructor in BalloonArena.reset, balloon_arena.py:171-177)
 *   hist         per-env ring of the last BLE_GP_CAPACITY observations, caller-allocated device
 *                memory, zero-initialised `count`
 *   append       1: observe() then get_features(); 0: get_features() on the existing history
 *   obs          [n][BLE_OBS_DIM] float32 out
 */
#define BLE_OBS_DIM 1099
#define BLE_GP_CAPACITY 128
#define BLE_GP_CHOL_STRIDE 7620 /* 120 * 121 / 2 doubles (packed factor) + 120 (the drop vector of the next slide) + 2 * 120 (zeta_u / d, zeta_v / d) */
typedef struct ble_gp_history_f32 {
  float* xyp;         /* [n][BLE_GP_CAPACITY][3]  x m, y m, pressure Pa */
  int32_t* elapsed_s; /* [n][BLE_GP_CAPACITY]     time_elapsed of the observation */
  float* err_uv;      /* [n][BLE_GP_CAPACITY][2]  measured - forecast, m/s */
  int32_t* count;     /* [n] observations appended this episode; ring slot = count % BLE_GP_CAPACITY */
  double* chol;       /* optional [n][BLE_GP_CHOL_STRIDE]: the current window's K + noise = Lt D Lt^T (unit-lower Lt,
                         d on the diagonal, packed lower triangle, 7260 doubles) followed by the drop vector
                         p = L22^-1 l21 of the next slide (120 doubles) and zeta / d for the two error components
                         (zeta = Lt^-1 y, 2 x 120 doubles), carried from call to call so that the
                         per-step refit of the reference (wind_gp.py:186-188) becomes an O(n^2) slide;
                         opaque to the caller; NULL = refit in LDS every call */
  int32_t* n_chol;    /* [n] rows of `chol` in use (required when chol != NULL), zero-initialised */
  int64_t chol_stride; /* doubles between the slabs of consecutive environments in `chol`: >= BLE_GP_CHOL_STRIDE AND EVEN
                          when chol != NULL (the kernel moves the slab as 16-byte double2 pairs, so every slab must start
                          16-byte aligned: `chol` itself 16-byte aligned, the stride a multiple of two doubles).  A smaller
                          or odd value is rejected with BLE_E_INVALID_ARG -- the kernel would write past the caller's
                          allocation or fault on a misaligned pair; ignored when chol == NULL */
} ble_gp_history_f32;
int ble_observe_f32(const ble_state_f32* st, const float* wind_grid, int64_t grid_env_stride,
                    const float* noise_uv, const uint8_t* reset_mask, const ble_gp_history_f32* hist,
                    int append, float* obs, uint32_t* err_flags, int64_t n, void* stream);
/* ... for a forecast that is NOT a grid (ABI 5).  The reference's feature constructor takes any wind_field.WindField
 * (features.py:290-299) and asks it for the column above the balloon, forecast.get_forecast_column(x, y, 181 levels, elapsed)
 * (features.py:499-503 -> wind_gp.py:218-222) -- e.g. the SimpleStaticWindField of its unit tests (wind_field.py:149-184), a step
 * function of pressure that no (21, 21, 10, 9) grid reproduces.
 *   forecast_levels  optional [n][181][2] float32: the caller's forecast (u, v) [m/s] at the levels 5 000 + 50 k Pa, k = 0 .. 180, at each
 *                    environment's position and time.  NULL: the column comes from wind_grid, as in ble_observe_f32 (which is this
 *                    call with NULL).  wind_grid must be a valid grid either way (its column is then computed and not used). */
int ble_observe_forecast_f32(const ble_state_f32* st, const float* wind_grid, int64_t grid_env_stride, const float* forecast_levels,
                             const float* noise_uv, const uint8_t* reset_mask, const ble_gp_history_f32* hist,
                             int append, float* obs, uint32_t* err_flags, int64_t n, void* stream);

/*
 * Tail of the wind-field VAE decoder (generative/vae.py:149-186, Decoder.__call__ after the
 * last Dense layer): n sets of 7 x 7 x 90 flow fields -> half-pixel linear resize to 23 x 23
 * -> central differences -> n wind grids [21][21][10][9][2] (grid_env_stride = 79 380 floats).
 * The four Dense layers before it are plain GEMMs (rocBLAS/hipBLASLt through torch.matmul).
 * n < 2^31 per call (one workgroup per grid).
 */
int ble_decode_flow_fields_f32(const float* flow, float* wind_grid, int64_t n, void* stream);

/*
 * SimplexWindNoise.get_wind_noise (env/simplex_wind_noise.py:214-259) for n environments at their
 * positions: noise_uv [n][2] in m/s, to be passed as `noise_uv` to ble_step_f32 / ble_observe_f32.
 * Five harmonics per component with the reference's weights and spacings; generator seeds and
 * offsets per (seed, env, episode[i]).  The 4-D noise primitive is NOT opensimplex 0.3's (absent,
 * unpinned): see csrc/ble_noise.h.  mode 1 is a test probe of the raw primitive.
 *   harmonic_cache  optional (may be NULL), opaque: [BLE_NOISE_CACHE_ROWS][n] 32-bit words, zero-initialised by the caller.
 *                   The reference draws a harmonic's generator seed and offsets once per reset and keeps them in its
 *                   NoisyWindHarmonic objects (simplex_wind_noise.py:97-114); this is where they are kept here, keyed by
 *                   (seed, episode[i]) -- an entry drawn for another key is redrawn (50 Philox draws) and stored.
 *                   NULL: redrawn by every call.  Same values either way.
 */
#define BLE_NOISE_CACHE_ROWS 53
int ble_wind_noise_f32(const float* x_m, const float* y_m, const float* pressure, const int32_t* elapsed_s,
                       unsigned long long seed, const uint32_t* episode, int mode, uint32_t* harmonic_cache,
                       float* noise_uv, int64_t n, void* stream);
/* ... for a shard whose environment 0 is environment env_offset of the global batch (ABI 4; see ble_reset_at_f32). */
int ble_wind_noise_at_f32(const float* x_m, const float* y_m, const float* pressure, const int32_t* elapsed_s,
                          unsigned long long seed, const uint32_t* episode, int mode, uint32_t* harmonic_cache,
                          float* noise_uv, int64_t env_offset, int64_t n, void* stream);

/*
 * Rows of the struct-of-arrays state as records (ABI 5): out[count][BLE_ROW_DOUBLES] doubles, row r = environment first + r, the 26
 * per-environment members of ble_state_f32 in the struct's order (x ... power_paused), every value converted exactly (float32, int32,
 * int64 seconds < 2^53 and bytes are all doubles).  What a host consumer that wants ONE balloon as an object -- BalloonArena.
 * get_balloon_state / get_simulator_state (env/balloon_arena.py:204-226), the evaluation loop's per-step read (eval/eval_lib.py:163) --
 * copies back in one transfer instead of 26.
 */
#define BLE_ROW_DOUBLES 26
int ble_state_rows_f64(const ble_state_f32* st, int64_t first, int64_t count, double* out, int64_t n, void* stream);

/* power_table.lookup (env/balloon/power_table.py:21-38). watts out as float. */
int ble_power_table_f32(const float* pressure_ratio, const float* state_of_charge, float* watts,
                        uint32_t* err_flags, int64_t n, void* stream);

/*
 * Function-level probes: run exactly the device functions ble_step_f32 uses, one lane
 * per element, so that each reference function can be parity-tested on its own.
 */
/* Atmosphere.at_pressure (standard_atmosphere.py:122-154): height [m], temperature [K] */
int ble_probe_atmosphere_f32(const float* alpha, const float* pressure, float* height,
                             float* temperature, uint32_t* err_flags, int64_t n, void* stream);
/* Atmosphere.at_height (standard_atmosphere.py:89-120): pressure [Pa] and temperature [K] at heights [m], float64 (ABI 5; until then the
 * host mirror inverted ble_probe_atmosphere_f32 by bracketing its float32 outputs: 1e-7).  Heights outside [-610 m, 85 000 m) set
 * BLE_FLAG_PRESSURE_RANGE (the reference asserts, :94-95). */
int ble_probe_atmosphere_at_height_f64(const float* alpha, const double* height_m, double* pressure, double* temperature,
                                       uint32_t* err_flags, int64_t n, void* stream);
/* solar_calculator at BalloonState.latlng (solar.py:43-174, spherical_geometry.py:44-76):
 * sin/cos of the refraction-corrected elevation, elevation [deg] and flux [W/m^2] */
int ble_probe_solar_f32(const float* center_lat_deg, const float* center_lng_deg, const float* x_m,
                        const float* y_m, const int64_t* unix_s, float* el_deg, float* flux,
                        int64_t n, void* stream);
/* BalloonState.latlng (balloon.py:217-220, spherical_geometry.py:44-76): latitude / longitude [deg, float64] of the point
 * (x, y) metres east / north of the centre -- the function the observation and the exact solar chain evaluate (ABI 4) */
int ble_probe_latlng_f64(const float* center_lat_deg, const float* center_lng_deg, const float* x_m, const float* y_m,
                         double* lat_deg, double* lng_deg, int64_t n, void* stream);
/* solar_atmospheric_attenuation + solar_power (solar.py:177-209,515-536) from el [deg] */
int ble_probe_solar_power_f32(const float* el_deg, const float* pressure, float* attenuation,
                              float* power_w, int64_t n, void* stream);
/* thermal.d_balloon_temperature_dt (thermal.py:175-230) */
int ble_probe_thermal_f32(const float* volume, const float* t_int, const float* t_amb,
                          const float* pressure, const float* el_deg, const float* flux,
                          const float* upwelling_ir, float* dtdt, uint32_t* err_flags, int64_t n,
                          void* stream);
/* calculate_superpressure_and_volume (balloon.py:552-609) */
int ble_probe_sp_volume_f32(const float* mols_air, const float* t_int, const float* pressure,
                            float* volume, float* superpressure, int64_t n, void* stream);
/* ... with the function's own vehicle arguments (mols_lift_gas, envelope_volume_base, envelope_volume_dv_pressure: balloon.py:552-558)
 * taken from `vehicle` (ABI 5; NULL = the defaults), and d_balloon_temperature_dt with its balloon_mass argument (thermal.py:175-181) =
 * vehicle->envelope_mass */
int ble_probe_sp_volume_vehicle_f32(const ble_vehicle* vehicle, const float* mols_air, const float* t_int, const float* pressure,
                                    float* volume, float* superpressure, int64_t n, void* stream);
int ble_probe_thermal_vehicle_f32(const ble_vehicle* vehicle, const float* volume, const float* t_int, const float* t_amb,
                                  const float* pressure, const float* el_deg, const float* flux,
                                  const float* upwelling_ir, float* dtdt, uint32_t* err_flags, int64_t n,
                                  void* stream);
/* acs.get_most_efficient_power / get_fan_efficiency / get_mass_flow (acs.py:44-68) */
int ble_probe_acs_f32(const float* pressure_ratio, float* power_w, float* efficiency,
                      float* mass_flow, int64_t n, void* stream);

/* The three safety layers of the transition one at a time, stateful across calls through `fsm` (in/out, one byte per
 * element; a fresh layer = 0):
 *   layer 0  AltitudeSafetyLayer.get_action (altitude_safety.py:63-111): value = pressure [Pa], alpha = the
 *            atmosphere's lapse-rate blend; fsm 0 NOMINAL 1 LOW 2 VERY_LOW;
 *   layer 1  EnvelopeSafetyLayer.get_action (envelope_safety.py:109-157, max superpressure 2380 Pa): value =
 *            superpressure [Pa]; fsm 0 NOMINAL 1 LOW_CRITICAL 2 LOW 3 HIGH 4 HIGH_CRITICAL;
 *   layer 2  PowerSafetyLayer.get_action (power_safety.py:52-126): value = battery charge [Wh]; clocks [n][3] =
 *            (now, sunrise + 30 min, sunset) in seconds from a common epoch -- the layer moves the two events on
 *            by whole days, in place; fsm = navigation_is_paused; night_load_w / capacity_wh as the reference's
 *            arguments (the transition passes 183.7 W and 3058.56 Wh).
 * effective_action [n] = the layer's answer to action [n] (0 DOWN 1 STAY 2 UP). */
int ble_probe_safety_f32(int layer, const uint8_t* action, const float* value, const float* alpha,
                         int32_t* clocks, double night_load_w, double capacity_wh, uint8_t* fsm,
                         uint8_t* effective_action, uint32_t* err_flags, int64_t n, void* stream);
/* ABI 5: for layer 1 `alpha`, if not NULL, holds each element's maximum superpressure [Pa] (EnvelopeSafetyLayer.__init__'s argument,
 * envelope_safety.py:100-107); NULL = the reference vehicle's 2 380 Pa. */

/* The kernel's own fp64 primitives (reciprocal / rsqrt seeds and refinements, log, exp,
 * sincos), element-wise on device doubles.  op: 0 rcp seed, 1 rcp, 2 rsq seed, 3 rsqrt,
 * 4 sqrt, 5 log, 6 exp, 7 sin, 8 cos.  Test-only. */
int ble_probe_f64_prims(const double* x, double* y, int op, int64_t n, void* stream);

/*
 * Fleets: a batch whose environments fly DIFFERENT vehicles, in one call (additive to ABI 5; the single-vehicle entry points and
 * ble_state_f32 are unchanged).  The reference builds one BalloonState per balloon, each with its own vehicle constants
 * (balloon.py:156-173,183,200); a fleet is a palette of up to BLE_FLEET_MAX_VEHICLES such vehicles and, per environment, the index of
 * the entry it flies.  Every palette entry is derived on the host exactly as ble_state_f32.vehicle is, so an environment flies bit
 * for bit what a single-vehicle call with its entry as st->vehicle flies.
 *   palette        HOST array [n_vehicles], read when the call is made, not retained (like ble_state_f32.vehicle): a captured graph
 *                  keeps the palette it was recorded with
 *   n_vehicles     1 .. BLE_FLEET_MAX_VEHICLES
 *   sample_index   honoured by ble_reset_fleet_at_f32 only: != 0 together with sample != 0 draws vehicle_index[i] uniformly in
 *                  [0, n_vehicles) for the new episode, from a Philox stream keyed by (seed, env_offset + i, episode[i]) that is
 *                  disjoint from the initial conditions' (those stay bit for bit ble_reset_at_f32's), and writes it back
 *   vehicle_index  DEVICE uint8[n]: the palette entry each environment flies.  An entry >= n_vehicles sets BLE_FLAG_VEHICLE_INDEX and
 *                  freezes that environment for the call (reward 0, terminal 1, effective action = action; state untouched)
 * The fleet entry points take the arguments of their single-vehicle counterparts plus `fleet` after `st`, and answer
 * BLE_E_INVALID_ARG (before any HIP call) for a NULL fleet, palette or vehicle_index, n_vehicles outside 1 .. 16, a palette entry
 * that ble_state_f32.vehicle would refuse, or st->vehicle != NULL (two sources of the vehicle are refused, not merged).
 * The transition flies the one-lane-per-environment form at every batch size, whatever ble_set_step_form says (as a run-time
 * vehicle does).
 */
#define BLE_FLEET_MAX_VEHICLES 16
typedef struct ble_fleet {
  const ble_vehicle* palette;
  int32_t n_vehicles;
  int32_t sample_index;
  uint8_t* vehicle_index;
} ble_fleet;
int ble_step_fleet_f32(const ble_state_f32* st, const ble_fleet* fleet, const uint8_t* action, const float* wind_grid,
                       int64_t grid_env_stride, const float* noise_uv, float* reward, uint8_t* terminal,
                       uint8_t* effective_action, uint32_t* err_flags, unsigned long long* active_count,
                       int64_t n, int substeps, void* stream);
int ble_step_n_fleet_f32(const ble_state_f32* st, const ble_fleet* fleet, const uint8_t* action, const float* wind_grid,
                         int64_t grid_env_stride, const ble_noise_gen* noise, float* reward, uint8_t* terminal,
                         uint32_t* err_flags, unsigned long long* active_count, int64_t n, int substeps, int n_steps,
                         void* stream);
int ble_reset_fleet_at_f32(const ble_state_f32* st, const ble_fleet* fleet, const uint8_t* mask, unsigned long long seed,
                           uint32_t* episode, int sample, uint32_t* err_flags, int64_t env_offset, int64_t n, void* stream);
int ble_observe_forecast_fleet_f32(const ble_state_f32* st, const ble_fleet* fleet, const float* wind_grid, int64_t grid_env_stride,
                                   const float* forecast_levels, const float* noise_uv, const uint8_t* reset_mask,
                                   const ble_gp_history_f32* hist, int append, float* obs, uint32_t* err_flags, int64_t n,
                                   void* stream);

/*
 * Evaluation (additive to ABI 5): the StationSeeker controller, eval_agent's per-step bookkeeping and per-environment seeds.
 *
 * ble_station_seeker_f32: StationSeekerAgent.pick_action / find_best_pressure_level / altitude_score / wind_score
 * (agents/station_seeker_agent.py:72-186) on the feature decoding of env/features.py:146-266, in float64 on the float32 features.
 *   obs             device float32 [n] rows of BLE_OBS_DIM features, obs_row_stride (>= BLE_OBS_DIM) floats apart
 *   action          device uint8 [n]: UP (2) below the centre level 180, DOWN (0) above it, STAY (1) at it
 *   level           optional device int32 [n]: the chosen relative level 0 .. 360 (the reference's first strict maximum)
 *   scores          optional device double [n][361]: every level's altitude_score, 0 where the level is not valid
 *   err_flags       optional device uint32: BLE_FLAG_AGENT_NO_LEVEL (action 1, level -1 for that environment)
 */
int ble_station_seeker_f32(const float* obs, int64_t obs_row_stride, uint8_t* action, int32_t* level, double* scores,
                           uint32_t* err_flags, int64_t n, void* stream);

/*
 * ble_eval_accumulate_f32: the body of eval_agent's step loop (eval/eval_lib.py:157-190) after a transition, for every environment
 * with done[i] == 0: cumulative_reward += reward (float64), steps_within_radius += (sqrt(x^2 + y^2) <= radius_m, float64 on the
 * float32 state, not contracted), final_timestep = step_index + 1; a status other than OK is stored in end_status and sets done, and so
 * does step_index + 1 == max_steps.  Nothing of an environment that is done is touched.  All five arrays are device [n] and required.
 *   flight_path     optional device float32 [n][6]: this step's SimpleBalloonState row of every environment not done before the call --
 *                   x [m], y [m], pressure [Pa], superpressure [Pa], elapsed [s], battery state of charge (st->vehicle's capacity)
 */
typedef struct ble_eval_acc {
  double* cumulative_reward;
  int32_t* steps_within_radius;
  int32_t* final_timestep;
  uint8_t* done;
  uint8_t* end_status;
} ble_eval_acc;
int ble_eval_accumulate_f32(const ble_state_f32* st, const float* reward, const ble_eval_acc* acc, double radius_m, int step_index,
                            int max_steps, float* flight_path, int64_t n, void* stream);

/*
 * ble_observe_live_f32: ble_observe_f32 for the environments whose status is OK only.  An environment that has terminated (status
 * OUT_OF_POWER, BURST or ZEROPRESSURE) is not observed: its WindGP history, its observation row and err_flags are left as they are --
 * the reference's eval_agent stops observing a balloon once its episode is done (eval/eval_lib.py:185-190), and the step kernels
 * freeze such a lane's clock, so observing it again would add entries at one frozen time.
 */
int ble_observe_live_f32(const ble_state_f32* st, const float* wind_grid, int64_t grid_env_stride, const float* noise_uv,
                         const uint8_t* reset_mask, const ble_gp_history_f32* hist, int append, float* obs, uint32_t* err_flags, int64_t n,
                         void* stream);

/*
 * Per-environment seeds: ble_reset_f32 and ble_wind_noise_f32 with a device seed per environment (env_seed, uint64 [n]) in place of the
 * batch's scalar seed.  Environment i draws from the Philox streams that environment 0 of a one-environment batch with scalar seed
 * env_seed[i] draws from: key (env_seed[i], 0, episode[i]) -- a seed flies the same episode in any batch and at any position.
 * st->vehicle is honoured as by ble_reset_f32 (fleets are not).  The noise form keeps no harmonic cache: it draws the harmonics from
 * the Philox stream on every call (same values).
 */
int ble_reset_seeded_f32(const ble_state_f32* st, const uint8_t* mask, const unsigned long long* env_seed, uint32_t* episode,
                         int sample, uint32_t* err_flags, int64_t n, void* stream);
int ble_wind_noise_seeded_f32(const float* x_m, const float* y_m, const float* pressure, const int32_t* elapsed_s,
                              const unsigned long long* env_seed, const uint32_t* episode, int mode, float* noise_uv, int64_t n,
                              void* stream);

/*
 * Q-network agents (additive to ABI 5): the eval-mode forward pass of the reference's QuantileNetwork and MLPNetwork
 * (agents/networks.py) -- the policy of its QR-DQN (quantile, perciatelli44, finetune_perciatelli), DQN and MLP agents.
 *
 * ble_qnet_f32 describes a network: num_layers Dense layers (>= 1), input_dim -> hidden_units -> ... -> num_actions * num_atoms, ReLU
 * after every layer but the last.  Supported: input_dim == BLE_OBS_DIM, num_actions == 3, num_layers 1 .. 64, hidden_units 1 .. 8192
 * (ignored when num_layers == 1), num_atoms 1 .. 4096 (1: MLPNetwork, q equals the logits); anything else is BLE_E_INVALID_ARG.
 * weights is the DEVICE image ble_qnet_pack_f32 made (zero-padded, fragment-ordered; its layout is private to the library).
 */
typedef struct ble_qnet_f32 {
  int32_t num_layers;
  int32_t input_dim;
  int32_t hidden_units;
  int32_t num_actions;
  int32_t num_atoms;
  int32_t reserved_;         /* 0 */
  const float* weights;
} ble_qnet_f32;

/* Sizes, in floats, of the packed weights and of the scratch a forward pass over n rows needs (either pointer may be NULL). */
int ble_qnet_workspace_f32(const ble_qnet_f32* net, int64_t n, int64_t* packed_floats, int64_t* scratch_floats);

/* HOST: packs the reference's parameters -- kernel[l] row-major [in][out] float32, bias[l] [out] float32, host pointers -- into
 * packed (host, ble_qnet_workspace_f32's packed_floats); net->weights is not read.  Copy the image to the device once. */
int ble_qnet_pack_f32(const ble_qnet_f32* net, const float* const* kernel, const float* const* bias, float* packed);

/*
 * ble_qnet_forward_f32: the network on n observation rows, then q[a] = the mean of action a's num_atoms logits (summed in ascending
 * atom order, divided by num_atoms, float32) and action = argmax q with jnp.argmax's rule (the lowest index among equal maxima; the
 * first NaN if a q is NaN; no error flag).  float32 in, float32 accumulation on v_mfma_f32_32x32x2_f32.  Batch invariant: every
 * output's reduction order depends on the network's shape only, so a row's q and action are the same bits at any n, at any position
 * and at any row stride.
 *   obs             device float32 [n] rows of BLE_OBS_DIM features, obs_row_stride (>= BLE_OBS_DIM) floats apart; nothing past a
 *                   row's BLE_OBS_DIM features is read
 *   scratch         device float32, ble_qnet_workspace_f32(net, n)'s scratch_floats, 256-byte aligned (the activations)
 *   action          device uint8 [n]
 *   q_values        optional device float32 [n][num_actions]
 */
int ble_qnet_forward_f32(const ble_qnet_f32* net, const float* obs, int64_t obs_row_stride, float* scratch, uint8_t* action,
                         float* q_values, int64_t n, void* stream);

/*
 * Q-network training (additive to ABI 5): Dopamine 4.0.0's JaxQuantileAgent update -- uniform n-step replay, the QR-DQN target and
 * quantile Huber loss, backprop through the Dense stack, optax 0.0.9 Adam -- on the device.  fp32 data, fp32 accumulation, no
 * floating-point atomics: every reduction has one order fixed by the shapes, so an update is a pure function of (parameters, replay,
 * seeds, counters).  Sizes and counts travel inside the descriptors below (no int64_t argument).
 */
#define BLE_FLAG_REPLAY_EMPTY 2048u  /* ble_replay_sample_f32: no valid n-step window in max_tries draws -- the row is all zeros,
                                        discount 0, index (-1, -1) */
#define BLE_FLAG_TRAIN_ACTION 4096u  /* ble_qnet_train_step_f32: a batch action >= num_actions -- the row's loss and gradient are 0 */
#define BLE_REPLAY_MAX_HORIZON 64
#define BLE_REPLAY_MAX_TRIES 1024
#define BLE_TRAIN_MAX_BATCH 1048576

/* HOST: the inverse of ble_qnet_pack_f32 -- kernel[l] row-major [in][out] and bias[l] [out] (host) from the host image packed. */
int ble_qnet_unpack_f32(const ble_qnet_f32* net, const float* packed, float* const* kernel, float* const* bias);

/*
 * The replay ring of N environments stepped in lockstep: row s % capacity holds step s of every environment.  Steps
 * max(0, count - capacity) .. count - 1 are held.  obs[s] is the observation action[s] was taken on; reward[s], terminal[s] and
 * episode_end[s] (!= 0: the episode ended at this step, by a terminal or by the time limit) describe the transition.  With auto
 * reset obs[s + 1] after an episode end is the first observation of the next episode.
 */
typedef struct ble_replay_f32 {
  int64_t capacity;          /* T >= update_horizon + 1 */
  int64_t num_envs;          /* N >= 1 */
  int32_t update_horizon;    /* n, 1 .. BLE_REPLAY_MAX_HORIZON */
  int32_t obs_stride;        /* floats per stored observation, >= BLE_OBS_DIM, a multiple of 4; columns past BLE_OBS_DIM not read */
  double gamma;              /* finite; gamma^k is the float32 rounding of the float64 power, as Dopamine's table */
  int32_t max_tries;         /* draws per batch row before BLE_FLAG_REPLAY_EMPTY, 1 .. BLE_REPLAY_MAX_TRIES */
  int32_t reserved_;         /* 0 */
  const float* obs;          /* device [T][N][obs_stride], 16-byte aligned */
  const uint8_t* action;     /* device [T][N] */
  const float* reward;       /* device [T][N] */
  const uint8_t* terminal;   /* device [T][N] */
  const uint8_t* episode_end;/* device [T][N] */
  const int64_t* count;      /* device: steps written */
  unsigned long long* counter; /* device: the update counter; each sample call draws with it, then advances it by one */
} ble_replay_f32;

/* One batch of B transitions (what ble_replay_sample_f32 writes and ble_qnet_train_step_f32 reads). */
typedef struct ble_train_batch_f32 {
  int64_t batch;             /* B, 0 .. BLE_TRAIN_MAX_BATCH */
  int64_t state_stride;      /* floats per state row, >= BLE_OBS_DIM, a multiple of 4; the sampler zero-fills columns >= BLE_OBS_DIM */
  float* state;              /* device [B][state_stride], 16-byte aligned */
  float* next_state;         /* device [B][state_stride], 16-byte aligned */
  float* ret;                /* device [B]: sum_{k<m} gamma^k r_{t+k} */
  float* discount;           /* device [B]: gamma^n, 0 if a terminal ends the window */
  uint8_t* action;           /* device [B] */
  int64_t* index;            /* optional device [B][2]: the sampled (t, env) */
} ble_train_batch_f32;

/*
 * ble_replay_sample_f32: B uniform draws of (t, env) from the Philox stream keyed by (seed, batch row, *counter), each redrawn until
 * its window is valid (at most max_tries draws).  A window is valid when steps t .. t + n are held and, among t .. t + n - 1, no
 * episode end comes before the first terminal (a time-limit end without a terminal invalidates it).  m = n, or 1 + the position of the
 * first terminal.  state = obs[t], next_state = obs[t + m] (Dopamine's next_state_index), ret and discount as above.  Two launches
 * (the draw and gather, then the counter's advance).
 */
int ble_replay_sample_f32(const ble_replay_f32* replay, const ble_train_batch_f32* batch, unsigned long long seed, uint32_t* err_flags,
                          void* stream);

/*
 * The trainer: the online image net.weights (updated in place), the target image, the gradient, Adam's m and v (all of
 * ble_qnet_workspace_f32's packed_floats, device, 16-byte aligned, the padding of every one zero), weights_t (the transposed image of
 * layers 1 .. L-1 that dX = dY W^T reads: ble_qnet_transpose_f32 makes it, the update rewrites it), adam_step (device: the step count,
 * advanced before each update) and the workspace (ble_qnet_train_workspace_f32's layout).
 */
typedef struct ble_qnet_train_f32 {
  ble_qnet_f32 net;
  const float* target;
  float* weights_t;
  float* grad;
  float* adam_m;
  float* adam_v;
  unsigned long long* adam_step;
  float* workspace;
  double adam_b1, adam_b2;                 /* optax.adam(lr, b1, b2, eps, eps_root=0): 1 - b and 1 - b^t are float64, rounded to float32 */
  float lr, adam_eps;
  float kappa;                             /* Huber threshold, > 0 */
  int32_t apply_update;                    /* 0: the gradient only (weights, weights_t, m, v and adam_step untouched) */
} ble_qnet_train_f32;

/* Offsets (floats from tr->workspace) of the workspace of a batch of B rows. */
typedef struct ble_qnet_train_layout {
  int64_t ld;                /* floats per activation row (the widest padded layer) */
  int64_t acts;              /* [L][B][ld]: every online layer's output (ReLU applied but on the last: the logits) */
  int64_t target_logits;     /* [B][ld]: the target network's logits on next_state */
  int64_t targets;           /* [B][num_atoms]: T_j = ret + discount * z_target(s')[a*, j] */
  int64_t dlogits;           /* [B][ld]: dL/dlogits of the objective mean_b L_b (zero off the batch action's atoms) */
  int64_t scratch;           /* the target ping-pong and the backward dY ping-pong */
  int64_t partial;           /* [slabs][largest layer block]: dW / db partial sums of batch slabs, combined in slab order */
  int64_t slabs;             /* batch slabs of the dW reduction (a function of B alone) */
  int64_t corrections;       /* [4]: 1 - b1^t, 1 - b2^t of the current Adam step */
  int64_t total;             /* floats of the whole workspace */
  int64_t transposed_floats; /* floats of weights_t */
} ble_qnet_train_layout;

int ble_qnet_train_workspace_f32(const ble_qnet_train_f32* tr, const ble_train_batch_f32* batch, ble_qnet_train_layout* layout);

/* HOST: weights_t from a host image packed (ble_qnet_train_workspace_f32's transposed_floats floats). */
int ble_qnet_transpose_f32(const ble_qnet_f32* net, const float* packed, float* packed_t);

/*
 * ble_qnet_train_step_f32: one QR-DQN update on batch: the target forward on next_state, the online forward on state
 * (the eval forward's instructions: the same logits' bits), the loss and dL/dlogits, dW / db into grad (the packed layout) and dX
 * layer by layer, then Adam on every packed element (apply_update != 0).  loss: device float32 [B], the per-row loss L_b.
 */
int ble_qnet_train_step_f32(const ble_qnet_train_f32* tr, const ble_train_batch_f32* batch, float* loss, uint32_t* err_flags, void* stream);

/*
 * TD learners of one-atom networks (additive to ABI 5; DESIGN §3g "DQN and SARSA"): the logits [B][3] are the Q-values.
 *   BLE_TD_DQN_MSE    Dopamine 4.0.0 JaxDQNAgent with loss_type = 'mse' (configs/dqn.gin): T = ret + discount max_a q_target(s')[a],
 *                     L_b = (T - q(s)[action])^2
 *   BLE_TD_DQN_HUBER  the same target, L_b = Huber_1(T - q(s)[action]) (JaxDQNAgent's default loss_type)
 *   BLE_TD_SARSA_MSE  the reference's agents/mlp_agent.py train(): L_b = (q(s)[action] - (ret + gamma q(s')[next_action]))^2 with the
 *                     online parameters on both sides and the gradient through both; batch->ret is the reward, batch->discount is
 *                     not read, tr->target is not read
 * The objective is mean_b L_b (masked rows counted in B).  The optimiser is the trainer's Adam (adam_* of ble_qnet_train_f32) or
 * optax.sgd(tr->lr): w -= lr g, which needs no Adam state.
 */
#define BLE_TD_DQN_MSE 0
#define BLE_TD_DQN_HUBER 1
#define BLE_TD_SARSA_MSE 2
#define BLE_TD_OPT_ADAM 0
#define BLE_TD_OPT_SGD 1

typedef struct ble_td_f32 {
  int32_t kind;               /* BLE_TD_* */
  int32_t optimizer;          /* BLE_TD_OPT_* */
  float gamma;                /* SARSA's discount, finite (not read by the DQN kinds) */
  int32_t reserved_;          /* 0 */
  const uint8_t* next_action; /* SARSA: device [B], the action taken at next_state */
  const uint8_t* mask;        /* SARSA, optional: device [B]; mask[b] != 0: row b's loss and both of its dlogits rows are exactly 0 */
} ble_td_f32;

/*
 * HOST: the workspace of ble_qnet_td_step_f32 for a batch of B rows.  The DQN kinds answer ble_qnet_train_workspace_f32's layout.
 * SARSA keeps both branches: acts is [L][2][B][ld] (layer l: the B rows of state, then the B rows of next_state), dlogits [2 B][ld] in
 * that order, targets [B], scratch the backward dY ping-pong of 2 B rows, partial [2 slabs][largest layer block] with slabs the batch
 * slabs of ONE branch (state's slabs first), target_logits empty.
 */
int ble_qnet_td_workspace_f32(const ble_qnet_train_f32* tr, const ble_td_f32* td, const ble_train_batch_f32* batch,
                              ble_qnet_train_layout* layout);

/*
 * ble_qnet_td_step_f32: one update of a one-atom network (net.num_atoms == 1) on batch.  DQN kinds: ble_qnet_train_step_f32's
 * stages with the TD loss in place of the quantile loss.  SARSA: the online forward on state and on next_state (every layer kept), the
 * loss and dL/dlogits of both branches, dW / db of each layer as the sum of the state branch's batch slabs then the next_state
 * branch's, in that order, dX over the 2 B rows.  Then the optimiser (apply_update != 0).  No floating-point atomics; every sum in an
 * order fixed by the shapes and B.  loss: device float32 [B].  An action >= num_actions (either action, for SARSA) sets
 * BLE_FLAG_TRAIN_ACTION and zeroes the row.  tr->kappa is not read.
 */
int ble_qnet_td_step_f32(const ble_qnet_train_f32* tr, const ble_td_f32* td, const ble_train_batch_f32* batch, float* loss,
                         uint32_t* err_flags, void* stream);

/* epsilon-greedy: action[i] (the greedy action in, the taken action out) becomes uniform in {0, 1, 2} when a uniform u < epsilon; u and
 * the random action come from the Philox stream keyed by (seed, i, step). */
typedef struct ble_explore_f32 {
  int64_t n;
  float epsilon;             /* 0 .. 1 */
  int32_t reserved_;         /* 0 */
  unsigned long long seed;
  unsigned long long step;
} ble_explore_f32;

int ble_qnet_explore_u8(const ble_explore_f32* ex, uint8_t* action, void* stream);

/*
 * On-policy training (additive to ABI 5): an actor-critic is a network with num_atoms == 2 whose six outputs z[a * 2 + j]
 * are read as: policy logit of action a = z[2a], state value V = z[1]; z[3] and z[5] are not read and receive a zero gradient.
 * fp32, one rounding per operation, every branch a select, no floating-point atomics.  As with the other training entry points every
 * size travels in a descriptor (no int64_t argument).
 *
 * log-softmax of the three policy logits (both heads): m = max z, e_a = expf(z_a - m), S = (e0 + e1) + e2, lp_a = (z_a - m) - logf(S),
 * p_a = e_a / S.  Finite logits give finite lp_a.
 */
typedef struct ble_ac_rows_f32 {
  int64_t n;                   /* rows, >= 0 */
  int64_t obs_row_stride;      /* floats between rows, >= BLE_OBS_DIM */
  const float* obs;            /* device [n] rows of BLE_OBS_DIM features */
  uint8_t* action;             /* device [n] */
  float* logp;                 /* device [n]: lp of the action */
  float* value;                /* device [n]: z[1] */
  float* probs;                /* optional device [n][3] */
} ble_ac_rows_f32;

/* The sampled head: row i draws u = (w >> 8) 2^-24, w the first 32-bit word of the Philox stream keyed by (seed ^ 0x4143544F52,
 * env_offset + i, *step) (ble_qnet_explore_u8's keying under another constant), and takes action = u < p0 ? 0 : (u < p0 + p1 ? 1 : 2).
 * The draw of environment env_offset + i at *step does not depend on n or on the row's position.  *step is read, not advanced. */
typedef struct ble_ac_sample {
  unsigned long long seed;
  int64_t env_offset;          /* >= 0 */
  const unsigned long long* step; /* device */
  int64_t reserved_;           /* 0 */
} ble_ac_sample;

/*
 * ble_ac_act_f32: ble_qnet_forward_f32's Dense stack on rows->obs (the same instructions: the same logits' bits), then one lane per
 * row.  sample == NULL: greedy, argmax over z[0], z[2], z[4] with ble_qnet_forward_f32's rule (the lowest index among equal maxima;
 * the first NaN).  scratch: ble_qnet_workspace_f32(net, n)'s scratch_floats, 16-byte aligned.  net->num_atoms must be 2.
 */
int ble_ac_act_f32(const ble_qnet_f32* net, const ble_ac_rows_f32* rows, float* scratch, const ble_ac_sample* sample, void* stream);

/*
 * A rollout block of T steps of N environments, every array [T][N] (boot_value [N]): generalised advantage estimation, t descending
 * from T - 1 with A_next = 0:
 *   nv = t == T - 1 ? boot_value[e] : value[t + 1][e];  boot = terminal ? 0 : (episode_end ? value[t][e] : nv);
 *   delta = (reward + gamma boot) - value[t][e];  A = delta + (gamma lambda) (episode_end ? 0 : A_next);
 *   advantage[t][e] = A;  ret[t][e] = A + value[t][e].
 * episode_end is terminal | time limit.  A terminal step bootstraps nothing; a step cut by the time limit, whose next observation
 * already belongs to the new episode, bootstraps from its own value; both cut the trace.
 */
typedef struct ble_gae_block_f32 {
  int64_t steps;               /* T, >= 0 */
  int64_t num_envs;            /* N, >= 0; T N <= 2^40 */
  float gamma, lambda;         /* finite */
  const float* reward;
  const float* value;
  const float* boot_value;
  const uint8_t* terminal;
  const uint8_t* episode_end;
  float* advantage;
  float* ret;
} ble_gae_block_f32;

/* Writes advantage and ret, nothing else.  T N == 0 launches nothing. */
int ble_gae_f32(const ble_gae_block_f32* gae, void* stream);

/* In place over the M = T N advantages of the block, float64, one 256-thread workgroup in a fixed order (thread k sums elements k,
 * k + 256, ... ascending, thread 0 adds the 256 partials ascending): mean = S / M, var = sum (A - mean)^2 / M by a second pass of the
 * same shape, A <- (float)((A - mean) / (sqrt(var) + 1e-8)).  Reads only gae->steps, num_envs and advantage. */
int ble_adv_normalize_f32(const ble_gae_block_f32* gae, void* stream);

typedef struct ble_ppo_f32 {
  float clip;                  /* epsilon: finite, > 0 */
  float value_coef;            /* c_v, finite */
  float entropy_coef;          /* c_e, finite */
  int32_t reserved_;           /* 0 */
  const float* old_logp;       /* device [B]: lp of the batch action when it was taken */
  const float* advantage;      /* device [B] */
} ble_ppo_f32;

/*
 * ble_qnet_ppo_step_f32: one clipped-PPO update of a two-atom network on batch: ble_qnet_train_step_f32's stages without the target
 * pass -- the online forward on batch->state with every layer kept, the loss below and its dL/dlogits, the same backward, then Adam
 * under apply_update.  tr->target, batch->next_state, batch->discount and tr->kappa are not read and may be NULL; batch->ret is R.
 * The workspace is ble_qnet_train_workspace_f32's; where the other kinds write targets ([B][2] floats) it writes aux[b] = (lp_act, H).
 * Per row, with A = advantage[b], (lp, p) the log-softmax of z[0], z[2], z[4]:
 *   H = -((p0 lp0 + p1 lp1) + p2 lp2);  rho = expf(lp_act - old_logp[b]);  s1 = rho A;  s2 = clamp(rho, 1 - clip, 1 + clip) A;
 *   active = s1 <= s2;  L_b = (-(active ? s1 : s2) + c_v (z[1] - R)^2) - c_e H;
 *   dL/dz[2a] = ((active ? -((A rho) ((a == act) - p_a)) : 0) + c_e (p_a (lp_a + H))) / B;  dL/dz[1] = (2 c_v (z[1] - R)) / B.
 * An action >= 3 sets BLE_FLAG_TRAIN_ACTION and zeroes the row.  B == 0 launches nothing.
 */
int ble_qnet_ppo_step_f32(const ble_qnet_train_f32* tr, const ble_ppo_f32* ppo, const ble_train_batch_f32* batch, float* loss,
                          uint32_t* err_flags, void* stream);

/*
 * Imitation (additive to ABI 5): behaviour cloning of the actor-critic above on labelled rows, and the DAgger mixture of
 * the learner's and the expert's actions.  §3m's arithmetic rules; both heads share the log-softmax above.
 */
typedef struct ble_bc_f32 {
  float label_smoothing;       /* s: finite, in [0, 1) */
  float value_coef;            /* c_v, finite; 0: no value term, batch->ret is not read and may be NULL */
  int64_t reserved_;           /* 0 */
} ble_bc_f32;

/*
 * ble_qnet_bc_step_f32: one cloning update of a two-atom network on batch, batch->action holding the expert's labels:
 * ble_qnet_ppo_step_f32's stages with another loss -- no target pass; tr->target, batch->next_state, batch->discount and tr->kappa
 * are not read and may be NULL; lr and Adam as ble_qnet_ppo_step_f32 asks.  The workspace is ble_qnet_train_workspace_f32's; where
 * the other kinds write targets ([B][2] floats) it writes aux[b] = (lp_act, agree).
 * Per row, with act = action[b], R = ret[b], (lp, p) the log-softmax of z[0], z[2], z[4]:
 *   s3 = s / 3;  hi = (1 - s) + s3;  q_a = (a == act) ? hi : s3;  CE = -((q0 lp0 + q1 lp1) + q2 lp2);
 *   L_b = CE + c_v (z[1] - R)^2;  dL/dz[2a] = (p_a - q_a) / B;  dL/dz[1] = (2 c_v (z[1] - R)) / B;
 *   agree = 1.0f when the greedy action of these logits (ble_ac_act_f32's rule) equals act, else 0.0f.
 * c_v == 0: L_b = CE and dL/dz[1] is exactly 0.  z[3], z[5] and the padded columns receive zero.
 * An action >= 3 sets BLE_FLAG_TRAIN_ACTION and zeroes the row's loss, aux and gradient.  B == 0 launches nothing.
 */
int ble_qnet_bc_step_f32(const ble_qnet_train_f32* tr, const ble_bc_f32* bc, const ble_train_batch_f32* batch, float* loss,
                         uint32_t* err_flags, void* stream);

/* Row i draws u = (w >> 8) 2^-24, w the first 32-bit word of the Philox stream keyed by (seed ^ 0x444147474552, env_offset + i, *step)
 * (ble_ac_act_f32's keying under another constant), and takes action[i] = u < beta ? expert[i] : learner[i]; took_expert[i] = u < beta.
 * beta = 0 copies the learner, beta = 1 the expert.  The draw of environment env_offset + i at *step does not depend on n or on the
 * row's position.  *step is read, not advanced.  action may alias learner. */
typedef struct ble_dagger_mix_f32 {
  int64_t n;                   /* rows, >= 0 */
  float beta;                  /* finite, in [0, 1] */
  int32_t reserved_;           /* 0 */
  unsigned long long seed;
  int64_t env_offset;          /* >= 0 */
  const unsigned long long* step; /* device */
  const uint8_t* learner;      /* device [n] */
  const uint8_t* expert;       /* device [n] */
  uint8_t* action;             /* device [n] */
  uint8_t* took_expert;        /* optional device [n] */
} ble_dagger_mix_f32;

/* n == 0 launches nothing and needs no pointer. */
int ble_dagger_mix_u8(const ble_dagger_mix_f32* mix, void* stream);

/*
 * Soft targets (additive to ABI 5): cloning against a distribution over the three actions made from per-action values
 * target_q [B][3] -- a planner's per-action plan returns (ble_plan_action_values_f32), Q-values -- where ble_qnet_bc_step_f32 takes one
 * label.  §3m's arithmetic rules; the log-softmax is the heads' own.
 */
typedef struct ble_soft_bc_f32 {
  float inv_temperature;       /* beta: finite, > 0 */
  float label_smoothing;       /* s: finite, in [0, 1) */
  float value_coef;            /* c_v, finite; 0: no value term, batch->ret is not read and may be NULL */
  int32_t reserved_;           /* 0 */
  const float* target_q;       /* device [B][3]; a non-finite entry marks an action without a value */
} ble_soft_bc_f32;

/*
 * ble_qnet_soft_bc_step_f32: ble_qnet_bc_step_f32's stages with the soft loss; batch->action is not read and may be NULL.
 * Per row, with q = target_q[b], R = ret[b], (lp, p) the log-softmax of z[0], z[2], z[4]:
 *   valid_a = isfinite(q_a);  y_a = valid_a ? q_a beta : -Inf;  (lt, t) = the log-softmax of y (an invalid action: t_a = 0 exactly);
 *   u_a = (1 - s) t_a;  t'_a = u_a + s / 3;  CE = -((t'0 lp0 + t'1 lp1) + t'2 lp2);  L_b = CE + c_v (z[1] - R)^2;
 *   dL/dz[2a] = (p_a - t'_a) / B;  dL/dz[1] = (2 c_v (z[1] - R)) / B;
 *   aux[b] = (lp[a*], agree), a* the valid action whose q comes first in ble_plan_select_f32's order (the value descending, -0 == +0,
 *   then a ascending), agree = 1.0f when the greedy action of these logits equals a*.
 * No valid action: the row's loss, aux and gradient are exactly 0 and no flag is set.  Exactly one valid action a: the row's loss, aux
 * and gradient are ble_qnet_bc_step_f32's with the label a, bit for bit.  B == 0 launches nothing.
 * BLE_E_INVALID_ARG before any HIP call: what ble_qnet_bc_step_f32 refuses (but a NULL batch->action); a NULL soft or target_q; beta not
 * finite or <= 0.
 */
int ble_qnet_soft_bc_step_f32(const ble_qnet_train_f32* tr, const ble_soft_bc_f32* soft, const ble_train_batch_f32* batch, float* loss,
                              uint32_t* err_flags, void* stream);

/*
 * Prioritized n-step replay (additive to ABI 5): Dopamine 4.0.0's OutOfGraphPrioritizedReplayBuffer over the ring above.
 * An fp64 sum tree over capacity x num_envs leaves: leaf (t % capacity) num_envs + env is the n-step window that starts at ring row t
 * of that environment.  A heap padded to a power of two: nodes[1] is the root, nodes[padded + i] leaf i, nodes[0] unused, the padded
 * leaves 0.  Every parent is recomputed as left + right, never updated by a delta.  Initial state: all nodes 0, *max_priority = 1.
 */
#define BLE_FLAG_REPLAY_PRIORITY 8192u  /* ble_replay_set_priority_f32: a non-finite or negative loss -- its leaf is left unchanged */
#define BLE_SUM_TREE_MAX_LEAVES (1LL << 31)

typedef struct ble_sum_tree_f64 {
  int64_t leaves;            /* capacity x num_envs of the replay it indexes */
  int64_t padded;            /* the smallest power of two >= leaves */
  double* nodes;             /* device [2 padded], 8-byte aligned */
  double* max_priority;      /* device [1]: max_recorded_priority, never falls */
} ble_sum_tree_f64;

/*
 * ble_replay_tree_add_f64, after each vector step is added (*count = s + 1): zeroes row s % capacity (its windows are overwritten) and
 * gives row (s - n) % capacity, whose windows have just become complete, *max_priority -- 0 for a window that is not valid (one that
 * crosses a time-limit end without a terminal).  Every nonzero leaf is a valid window.  One workgroup: the two leaf rows, then their
 * ancestors level by level.
 */
int ble_replay_tree_add_f64(const ble_replay_f32* replay, const ble_sum_tree_f64* tree, void* stream);

/*
 * ble_replay_sample_prioritized_f32: stratified draws.  Row b draws q = total (b + u) / B from the Philox stream keyed by (seed, b,
 * *counter) and walks the tree down in fp64 (left if q < left sum, else q -= left sum and right; a child whose sum is 0 is never
 * entered); a draw on an invalid window is redrawn from the whole tree (q = total u), at most max_tries draws (BLE_FLAG_REPLAY_EMPTY as
 * the uniform sampler).  Writes the batch as ble_replay_sample_f32 does (batch->index is required) and priority[b] (device float32 [B]):
 * the sampled leaf, 0 for a failed row.  Advances *counter by one.
 */
int ble_replay_sample_prioritized_f32(const ble_replay_f32* replay, const ble_sum_tree_f64* tree, const ble_train_batch_f32* batch,
                                      float* priority, unsigned long long seed, uint32_t* err_flags, void* stream);

/*
 * ble_replay_set_priority_f32, after an update on that batch: leaf = sqrt(loss[b] + 1e-10) (float32, then stored as fp64), in batch
 * order (the later row wins on a duplicate index); rows with index -1 are skipped; a non-finite or negative loss leaves its leaf and
 * sets BLE_FLAG_REPLAY_PRIORITY; *max_priority rises to the largest new leaf; ancestors recomputed.  weighted_loss[b] (device float32
 * [B]) = (w_b / max w) loss[b], w_b = 1 / sqrt(priority[b] + 1e-10): the loss Dopamine reports -- the gradient is NOT weighted.
 * Failed rows: 0, and out of the max.  One workgroup, no atomics.
 */
int ble_replay_set_priority_f32(const ble_replay_f32* replay, const ble_sum_tree_f64* tree, const ble_train_batch_f32* batch,
                                const float* priority, const float* loss, float* weighted_loss, uint32_t* err_flags, void* stream);

/*
 * Marco Polo exploration (the reference's MarcoPoloExploration with a RandomWalkAgent; one call = one 3-minute agent step), one lane
 * per environment.  begin[i] != 0: begin_episode -- walk clock 0, target U[6500, 11400) Pa (float32), phase clock 0, exploratory episode
 * when u <= exploratory_episode_probability, RL phase; action[i] is kept.  Otherwise step -- phase clock + 1; in an exploratory episode
 * the phase toggles when it has run out (RL >= 80 steps, exploratory >= 40) and the clock restarts; in the exploratory phase walk clock
 * + 1, target += (180 walk) 0.1666 z (fp64), action[i] = UP (2) if p - 100 > target, DOWN (0) if p + 100 < target, else STAY (1), with
 * p = 5000 + 9000 obs[i][0] in float32.  Draws: Philox keyed by (seed, i, *step); block 0 holds the two begin uniforms (target, then
 * episode; 24 bits), block 1 on the normal.  Advances *step by one.
 */
typedef struct ble_marco_polo_f32 {
  int64_t n;
  int32_t obs_stride;                      /* floats between observation rows, >= 1 (feature 0 is read) */
  int32_t reserved_;                       /* 0 */
  double exploratory_episode_probability;  /* 0 .. 1 */
  unsigned long long seed;
  const float* obs;                        /* device [n][obs_stride] */
  const uint8_t* begin;                    /* device [n] */
  unsigned long long* step;                /* device: the draw key's step */
  int32_t* phase_clock;                    /* device [n]: agent steps in the current phase */
  int32_t* walk_clock;                     /* device [n]: the random walk's steps this episode */
  uint8_t* exploratory_episode;            /* device [n] */
  uint8_t* exploratory_phase;              /* device [n] */
  double* target;                          /* device [n]: the random walk's target pressure, Pa */
} ble_marco_polo_f32;

int ble_marco_polo_u8(const ble_marco_polo_f32* mp, uint8_t* action, void* stream);

/*
 * The WindGP posterior at caller-chosen points (the reference's WindGP.query_batch, env/wind_gp.py:126-241, with ONE query time per
 * environment): q points per environment against the observation ring that ble_observe_f32 keeps.  Added without a new ABI version.
 *
 * Per environment e: the window holds every ring entry i < min(count, BLE_GP_CAPACITY) with |t_i - time_s[e]| < 21 600 s (strict);
 *   K = 3.6^2 exp(-|(a - b) / (357 000 m, 357 000 m, 326 Pa, 34 560 s)|) + 0.05 I over the window, mean = K* K^-1 y (+ the grid
 *   forecast at (x, y, p, time_s[e]) when add_forecast), deviation = max(3.6^2 - |L^-1 k*|^2, 0) / 3.6^2, all in fp64.
 *   - an empty window, count == 0 or reset_mask[e] != 0 (a history restart is pending until the next observe): mean 0 (+ forecast),
 *     deviation 0
 *   - more than 120 entries in the window: the newest 120, and BLE_FLAG_GP_WINDOW (what ble_observe_f32 does)
 *   - count > BLE_GP_CAPACITY and the oldest ring entry inside the window: observations the ring no longer holds may belong to the
 *     window.  BLE_FLAG_GP_WINDOW, and NaN in that environment's mean_uv and deviation -- unless the window was cut to its newest 120
 *     for a time_s[e] not earlier than the newest observation: the evicted ones, older still, would have been cut as well.
 * The call reads `hist` (the ring and count; never chol / n_chol) and writes nothing but its outputs and err_flags.
 * BLE_E_INVALID_ARG before any HIP call: NULL hist, query, ring pointer, xyp, time_s, mean_uv or deviation; n < 0, q < 1,
 * n * q >= 2^31; add_forecast with a NULL grid.  n == 0: BLE_OK without a launch.  reset_mask and err_flags may be NULL.
 */
/* (a struct TAG only, no typedef: the entry point carries the same name, and tags live in a name space of their own) */
struct ble_gp_query_f32 {
  int64_t n;                 /* environments */
  int32_t q;                 /* query points per environment, >= 1, n * q < 2^31 */
  int32_t add_forecast;      /* 1: add the grid forecast at every point to the mean */
  const float* xyp;          /* [n][q][3]  x m, y m, pressure Pa */
  const int32_t* time_s;     /* [n] the ONE query time of each environment, seconds elapsed (past, now or future) */
  const float* wind_grid;    /* required when add_forecast; else may be NULL */
  int64_t grid_env_stride;   /* floats between the grids of consecutive environments; 0: one grid for all */
  float* mean_uv;            /* [n][q][2] out, m/s */
  float* deviation;          /* [n][q]    out, variance / sigma^2 as in the reference */
};
int ble_gp_query_f32(const ble_gp_history_f32* hist, const uint8_t* reset_mask, const struct ble_gp_query_f32* query, uint32_t* err_flags,
                     void* stream);

/*
 * Look ahead: K = n_plans action plans per environment, each flown for H = n_plan_steps entries x action_repeat agent steps from the
 * state where it lies -- "from where each balloon is now, what happens under these K action sequences?".  One lane per
 * (environment e, plan k); per agent step the semantics of ble_step_n_f32: the same lane functions on the same inputs, hence the same
 * bits as a copy of environment e stepped with plan k's actions (tests/test_gpu_rollout.py).  A lane whose source status is not OK, or
 * whose plan went terminal, is frozen: reward 0 from then on.  Actions are not range-checked (ble_step_f32).  Added without a new ABI
 * version.
 *   noise   NULL: every plan flies in the forecast.  Otherwise the ground-truth wind of ble_step_n_f32 with the same generator: the
 *           noise field of environment e is keyed by (seed, env_offset + e, episode[e]) whatever k, so a plan flies exactly the noise
 *           environment e itself will fly.  harmonic_cache is ignored: the call reads and fills no cache.
 *   ret     the discounted return sum_t gamma^t r_t over the agent steps the plan flew, accumulated in fp64 in the order of t (the
 *           product and the sum rounded separately), rounded to float once.
 *   steps_flown  the number of agent steps entered with status OK: 0 for a non-OK source, t + 1 when step t went terminal,
 *           H * action_repeat for a plan that survives.
 * Window of validity: the call reads `st`, `plans` and the grid when the kernel runs (stream order) and NEVER writes the state: not the
 * state arrays, not last_command, not episode_cache (a miss is recomputed, not stored).  It writes ret, steps_flown, the optional
 * outputs and err_flags -- give it a flag word of its own: a hypothetical plan that leaves the valid range sets the BLE_FLAG_* of a
 * flight that never happened (a non-finite state: BLE_FLAG_NONFINITE).  The WindGP history is not advanced.
 * BLE_E_INVALID_ARG before any HIP call: NULL st, state array, ro, plans, wind_grid, ret or steps_flown; n < 0, n_plans < 1,
 * n_plan_steps < 1, action_repeat < 1, n_plan_steps * action_repeat > BLE_ROLLOUT_MAX_STEPS, n * n_plans >= 2^31; substeps outside
 * 1 .. BLE_MAX_SUBSTEPS; a negative grid_env_stride or noise->env_offset; gamma NaN or outside [0, 1]; an invalid st->vehicle.
 * n == 0: BLE_OK without a launch.  A fleet has no form of this call.
 */
#define BLE_ROLLOUT_MAX_STEPS 960      /* agent steps per plan: two days of 180 s steps */
/* (a struct TAG only, as for ble_gp_query_f32) */
struct ble_rollout_f32 {
  int64_t n;                 /* source environments */
  int32_t n_plans;           /* K >= 1, n * K < 2^31 */
  int32_t n_plan_steps;      /* H >= 1 */
  int32_t action_repeat;     /* >= 1: every plan entry is flown this many agent steps; H * action_repeat <= BLE_ROLLOUT_MAX_STEPS */
  int32_t substeps;          /* 1 .. BLE_MAX_SUBSTEPS */
  double gamma;              /* finite, 0 <= gamma <= 1 */
  const uint8_t* plans;      /* [H][n][K] */
  const float* wind_grid;    /* as for ble_step_f32 */
  int64_t grid_env_stride;
  float* ret;                /* [n][K] out */
  int32_t* steps_flown;      /* [n][K] out */
  float* reward;             /* optional [H * action_repeat][n][K] out */
  float* final_state;        /* optional [4][n][K] out: x, y, pressure, battery_charge after the last executed step */
};
int ble_rollout_f32(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_noise_gen* noise, uint32_t* err_flags,
                    void* stream);

/*
 * The belief: a WindGP fitted ONCE per environment and kept on the device, so that its posterior mean can be evaluated again and again
 * without a refit -- at caller-chosen points (ble_gp_belief_wind_f32) and inside a look-ahead (ble_rollout_belief_f32).  Added without a
 * new ABI version.
 *
 * slab: BLE_GP_BELIEF_DOUBLES doubles per environment -- the window's 120 x 4 coordinates, then 2 x 120 of K^-1 y; the layout is the
 * library's own.  Entries beyond the window are zero.  n_obs[e]: the observations in environment e's window; 0: no posterior (the mean
 * is exactly 0); -1: the window reaches observations the ring no longer holds (the mean is NaN).
 */
#define BLE_GP_BELIEF_DOUBLES 720
typedef struct ble_gp_belief {
  double* slab;              /* device [n][stride], 16-byte aligned */
  int64_t stride;            /* doubles between the slabs of consecutive environments: >= BLE_GP_BELIEF_DOUBLES and even */
  int32_t* n_obs;            /* device [n] */
  int64_t n;                 /* environments the belief holds (the sizes of these calls travel in the struct: no int64_t argument) */
} ble_gp_belief;

/*
 * Fits the WindGP of every environment at the anchor time time_s[e] (seconds elapsed) and stores it in `belief`: the window rules of
 * ble_gp_query_f32 -- |t_i - time_s[e]| < 21 600 s strict; more than 120 inside: the newest 120 and BLE_FLAG_GP_WINDOW; count == 0, a
 * pending reset_mask[e] or an empty window: n_obs 0 and a zero slab; count > BLE_GP_CAPACITY with the oldest ring entry inside an uncut
 * window: n_obs -1, a zero slab and BLE_FLAG_GP_WINDOW.  All algebra in fp64.  Reads the ring and count of `hist` (never chol / n_chol);
 * writes the belief and err_flags, nothing else.
 * BLE_E_INVALID_ARG before any HIP call: NULL hist, ring pointer, time_s, belief, slab or n_obs; a slab that is not 16-byte aligned, a
 * stride below BLE_GP_BELIEF_DOUBLES or odd; belief->n < 0 or >= 2^31.  belief->n == 0: BLE_OK without a launch.  reset_mask and err_flags
 * may be NULL.  hist, reset_mask and time_s hold belief->n environments.
 */
int ble_gp_fit_f32(const ble_gp_history_f32* hist, const uint8_t* reset_mask, const int32_t* time_s, const ble_gp_belief* belief,
                   uint32_t* err_flags, void* stream);

/*
 * The belief's posterior mean of the forecast ERROR at one point per environment: uv [n][2] m/s = sum_i k(loc_i, (x, y, p, t)) alpha_i
 * in fp64, rounded to float once -- the shape and role of ble_wind_noise_f32: what ble_step_f32 takes as noise_uv.  The forecast is NOT
 * added.  The window and K^-1 y are those of the fit's anchor time; only the query's time moves: the mean equals the reference's
 * WindGP.query at (x, y, p, t) whenever the reference's window at t is the anchor's window, and is the posterior of the anchor's
 * window otherwise (its correction decays with |t - t_i| / 34 560 s: far from the measurements the belief relaxes to the forecast).
 * n_obs 0: exactly +0.0f.  n_obs < 0: NaN.
 * BLE_E_INVALID_ARG: NULL belief, slab, n_obs or array; a misaligned slab, a stride below BLE_GP_BELIEF_DOUBLES or odd; belief->n < 0
 * or >= 2^31.  belief->n == 0: BLE_OK without a launch.  The arrays hold belief->n environments.
 */
int ble_gp_belief_wind_f32(const ble_gp_belief* belief, const float* x_m, const float* y_m, const float* pressure, const int32_t* elapsed_s,
                           float* uv, void* stream);

/*
 * ble_rollout_f32 flown in the wind the agent believes: forecast + the belief's mean, evaluated by every lane at its own pre-step
 * position and time (where ble_rollout_f32 with a generator evaluates the noise).  Per agent step the same bits as
 * ble_gp_belief_wind_f32 at the lane's state followed by ble_step_f32 with that noise_uv.  `ro`, the outputs, the window of validity
 * and the no-write rule are ble_rollout_f32's; the belief is read, never written.  An environment whose n_obs is -1 flies NaN: its
 * returns are non-finite and BLE_FLAG_NONFINITE goes to err_flags (the call's own word).
 * BLE_E_INVALID_ARG: everything ble_rollout_f32 refuses, and a NULL belief, slab or n_obs, a misaligned slab, a stride below
 * BLE_GP_BELIEF_DOUBLES or odd, a belief->n other than ro->n.  n == 0: BLE_OK without a launch.  A fleet has no form of this call.
 */
int ble_rollout_belief_f32(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_gp_belief* belief, uint32_t* err_flags,
                           void* stream);

/*
 * Plan on the device: sample K action plans per environment, fly them (ble_rollout_f32 / ble_rollout_belief_f32) and pick the best --
 * the two ends of a model-predictive decision, optionally iterated as a cross-entropy search.  Added without a new ABI version; every
 * size travels in a struct (no int64_t argument).
 *
 * ble_plan_sample_u8 writes plans [H][n][K], the layout ble_rollout_f32 reads.  A plan is piecewise constant: entry h belongs to
 * segment h / segment, each segment takes ONE 32-bit Philox word and draws
 *     r = (word * (E + 3)) >> 32;   action = 0 if r < c0 + 1, 1 if r < c0 + c1 + 2, else 2
 * where c0, c1, c2 are the segment's elite counts (iteration > 0; E their sum) or zero (iteration 0: uniform thirds).  Integers only.
 * The stream of plan k of environment e: Philox4x32-10 with the key (seed_e ^ 0x504C414E53) -- its high word xor the high word of the
 * decision counter -- and the counter (block, low word of the decision counter, low and high word of key_e); seed_e, key_e =
 * seed, env_offset + e, or with env_seed: env_seed[e], 0.  Block = (iteration * 1024 + k) * 256 + s / 4 for segment s, which takes
 * output word s % 4.  So a plan depends on (seed, the environment's key, decision counter, iteration, k, H, segment, its counts) and
 * never on n, K or the other environments of the batch.
 * Iteration 0 fixes the first slots, as far as K reaches: k = 0 all STAY (1), k = 1 all DOWN (0), k = 2 all UP (2), k = 3 the warm
 * start: entry h = best_plan[min(h + 1, H - 1)][e].
 * BLE_E_INVALID_ARG before any HIP call: NULL ps, plans, decision_counter or best_plan; iteration > 0 with NULL elite_counts; n < 0 or
 * >= 2^31, n_plans outside 1 .. BLE_PLAN_MAX_PLANS, n_plan_steps outside 1 .. BLE_ROLLOUT_MAX_STEPS, segment < 1, iteration outside
 * 0 .. BLE_PLAN_MAX_ITERATIONS - 1, n * n_plans >= 2^31, env_offset < 0.  n == 0: BLE_OK without a launch.
 */
#define BLE_PLAN_MAX_PLANS 1024
#define BLE_PLAN_MAX_ITERATIONS 16
/* (struct TAGS only, as for ble_rollout_f32) */
struct ble_plan_sample {
  int64_t n;                                 /* environments */
  int32_t n_plans;                           /* K */
  int32_t n_plan_steps;                      /* H entries per plan */
  int32_t segment;                           /* entries per segment, >= 1 */
  int32_t iteration;                         /* 0 .. BLE_PLAN_MAX_ITERATIONS - 1 */
  unsigned long long seed;                   /* the batch's seed (env_seed == NULL) */
  const unsigned long long* env_seed;        /* optional device [n]: a seed per environment, every stream keyed as environment 0 */
  int64_t env_offset;                        /* index of environment 0 in the global batch (env_seed == NULL) */
  const unsigned long long* decision_counter;/* device, one word: read, not written */
  const uint16_t* elite_counts;              /* device [n][ceil(H / segment)][3]: read when iteration > 0 */
  const uint8_t* best_plan;                  /* device [H][n]: read by the warm start */
  uint8_t* plans;                            /* device [H][n][K] out */
};
int ble_plan_sample_u8(const struct ble_plan_sample* ps, void* stream);

/*
 * ble_plan_select_f32: one wavefront per environment over ret [n][K], the returns of the plans ble_plan_sample_u8 wrote.
 * The order: a finite return before a non-finite one (Inf or NaN: all equal), then the return descending (-0 == +0), then k ascending.
 * The first plan in that order is compared with the incumbent -- best_return[e] as the earlier iterations of this decision left it;
 * none in iteration 0 -- and replaces it when it is finite and strictly greater, or the incumbent is not finite; a tie keeps the
 * incumbent.  Written: best_return [n]; best_k [n], the plan's index or -1 when the incumbent stayed; best_plan [H][n] (only when
 * replaced); action [n] = best_plan[0][e].  Iteration 0 without a finite plan: best_plan all STAY, best_return -Inf, best_k -1.
 * elite = E >= 1: also elite_counts [n][ceil(H / segment)][3], per segment and action the number of the first E plans in the order
 * that take it, for the next iteration's sampler.  advance_counter, when given, is incremented by one (the decision counter, after
 * the decision's last sampler: stream order).
 * BLE_E_INVALID_ARG before any HIP call: NULL sel, ret, plans, best_return, best_k, best_plan or action; the sampler's limits on n,
 * n_plans, n_plan_steps, segment and iteration; elite < 0 or > n_plans; elite >= 1 with NULL elite_counts.  n == 0: BLE_OK without a
 * launch (and without advancing the counter).
 */
struct ble_plan_select {
  int64_t n;
  int32_t n_plans;
  int32_t n_plan_steps;
  int32_t segment;
  int32_t iteration;
  int32_t elite;                             /* E: 0 .. n_plans */
  int32_t reserved_;
  const float* ret;                          /* device [n][K] */
  const uint8_t* plans;                      /* device [H][n][K] */
  float* best_return;                        /* device [n]: read when iteration > 0, written */
  int32_t* best_k;                           /* device [n] out */
  uint8_t* best_plan;                        /* device [H][n]: written where a plan replaces the incumbent */
  uint8_t* action;                           /* device [n] out */
  uint16_t* elite_counts;                    /* device [n][ceil(H / segment)][3] out, required when elite >= 1 */
  unsigned long long* advance_counter;       /* optional device word */
};
int ble_plan_select_f32(const struct ble_plan_select* sel, void* stream);

/*
 * Scenario winds: M = num sampled winds per environment instead of the belief's one mean.  Scenario m of environment e
 * is a draw f_m of the wind-noise field (the generator of ble_wind_noise_f32 with harmonics from the scenario stream below) corrected
 * so that it passes through the balloon's measurements (pathwise conditioning):
 *     error_m(x) = f_m(x) + sum_i k(loc_i, x) alpha^m_i,      alpha^m = (K + 0.05 I)^-1 (y - f_m(X))
 * with X, y, K the window of ble_gp_fit_f32 frozen at the anchor.  f_m(x) and the correction are each rounded to float (the
 * correction as ble_gp_belief_wind_f32 rounds) and added in ONE float addition.  The forecast is NOT added.  n_obs 0: the correction is
 * exactly +0.0f, a scenario is its prior draw; n_obs -1: NaN.  Added without a new ABI version; every size travels in a struct.
 *
 * The stream of (e, m): Philox4x32-10 with the key (seed_e ^ 0x5343454E4152) and the counter (block, episode[e], low and high word of
 * key_e), block = 32 m + b for the stream's b-th block; seed_e, key_e = seed, env_offset + e, or with env_seed: env_seed[e], 0.  Words
 * are taken from a block in the order 3, 2, 1, 0; harmonic k = 5 comp + h takes nine words from word 9 k on: the generator seed, then
 * four uniforms (hi, lo) -> ((hi << 32 | lo) >> 11) * 2^-53, offset = (float)(2 u - 1) for x, y, pressure, time -- the draws of the
 * true noise, whose key constant is 0x5EEDF00D: no scenario is the truth.  A function of (seed_e, key_e, episode[e], m) alone.
 *
 * slab: BLE_GP_SCENARIO_DOUBLES(num) doubles per environment -- the window's 120 x 4 coordinates once (bit for bit ble_gp_fit_f32's),
 * then per scenario 120 x 2 of alpha^m.  Entries beyond the window are zero.  n_obs[e]: as in ble_gp_belief.
 */
#define BLE_SCENARIO_MAX 16
#define BLE_GP_SCENARIO_DOUBLES(num) (480 + 240 * (num))
typedef struct ble_gp_scenarios {
  double* slab;              /* device [n][stride], 16-byte aligned */
  int64_t stride;            /* doubles between the slabs of consecutive environments: >= BLE_GP_SCENARIO_DOUBLES(num) and even */
  int32_t* n_obs;            /* device [n] */
  int64_t n;                 /* environments */
  int32_t num;               /* M: 1 .. BLE_SCENARIO_MAX */
  int32_t reserved_;
} ble_gp_scenarios;
typedef struct ble_scenario_gen {
  unsigned long long seed;                   /* the batch's seed (env_seed == NULL) */
  const unsigned long long* env_seed;        /* optional device [n]: a seed per environment, every stream keyed as environment 0 */
  const uint32_t* episode;                   /* optional device [n]: the episode counters (NULL: 0) */
  int64_t env_offset;                        /* index of environment 0 in the global batch (env_seed == NULL), >= 0 */
} ble_scenario_gen;

/*
 * ble_gp_fit_scenarios_f32: the window, K and its factor once per environment (the rules of ble_gp_fit_f32, BLE_FLAG_GP_WINDOW
 * included), then alpha^m for m = 0 .. num - 1; f_m(X) is evaluated from the ring's own float32 x, y, p and int32 t, bit for bit what
 * ble_gp_scenario_wind_f32(prior_only = 1) returns there.  Reads the ring and count of `hist`; writes scn and err_flags.
 * BLE_E_INVALID_ARG before any HIP call: NULL hist, ring pointer, time_s, scn, slab, n_obs or gen; num outside 1 .. BLE_SCENARIO_MAX; a
 * slab that is not 16-byte aligned, a stride below BLE_GP_SCENARIO_DOUBLES(num) or odd; scn->n < 0 or >= 2^31; gen->env_offset < 0.
 * scn->n == 0: BLE_OK without a launch.  reset_mask and err_flags may be NULL.
 */
int ble_gp_fit_scenarios_f32(const ble_gp_history_f32* hist, const uint8_t* reset_mask, const int32_t* time_s, const ble_gp_scenarios* scn,
                             const ble_scenario_gen* gen, uint32_t* err_flags, void* stream);

/*
 * The scenario wind's forecast ERROR at one point per environment, scenario scenario_index[e] (device int32 [n]): uv [n][2] m/s, what
 * ble_step_f32 takes as noise_uv -- the shape and role of ble_gp_belief_wind_f32.  prior_only = 1: f_m alone (the slab is not read).  An
 * index outside 0 .. num - 1: NaN.
 * BLE_E_INVALID_ARG: what ble_gp_fit_scenarios_f32 refuses of scn and gen; a NULL array; prior_only other than 0 or 1.
 */
int ble_gp_scenario_wind_f32(const ble_gp_scenarios* scn, const ble_scenario_gen* gen, const int32_t* scenario_index, const float* x_m,
                             const float* y_m, const float* pressure, const int32_t* elapsed_s, int prior_only, float* uv, void* stream);

/*
 * ble_rollout_belief_f32 flown in the scenario winds: one lane per (environment e, plan k, scenario m), lane index
 * j = (e * K + k) * M + m.  `ro` is ble_rollout_f32's with plans [H][n][K] as there and the outputs one axis longer: ret [n][K][M],
 * steps_flown [n][K][M], optional reward [H * action_repeat][n][K][M] and final_state [4][n][K][M].  Per agent step the same bits as
 * ble_gp_scenario_wind_f32 at the lane's pre-step state followed by ble_step_f32 with that noise_uv.  The state, its caches and scn are
 * read, never written.  An environment whose n_obs is -1 flies NaN (BLE_FLAG_NONFINITE in err_flags, the call's own word).
 * BLE_E_INVALID_ARG: everything ble_rollout_f32 refuses; what ble_gp_fit_scenarios_f32 refuses of scn and gen; scn->n other than
 * ro->n; n * K * M >= 2^31.  n == 0: BLE_OK without a launch.  A fleet has no form of this call.
 */
int ble_rollout_scenarios_f32(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_gp_scenarios* scn,
                              const ble_scenario_gen* gen, uint32_t* err_flags, void* stream);

/*
 * ble_plan_risk_f32: ret [n][K][M] -> score [n][K], the mean of the `tail` smallest scenario returns of every plan: tail = M the
 * expectation, tail = 1 the worst case, between them a CVaR.  The order: the return ascending (-0 == +0), then m ascending; the sum is
 * taken in that order in double from 0.0, divided by tail once and rounded to float once.  Any non-finite scenario return: NaN (which
 * ble_plan_select_f32 puts last).  ble_plan_select_f32 then runs on score as on any ret [n][K].
 * BLE_E_INVALID_ARG before any HIP call: NULL risk, ret or score; n < 0 or >= 2^31; n_plans outside 1 .. BLE_PLAN_MAX_PLANS; num outside
 * 1 .. BLE_SCENARIO_MAX; tail outside 1 .. num; n * n_plans * num >= 2^31.  n == 0: BLE_OK without a launch.
 */
struct ble_plan_risk {
  int64_t n;
  int32_t n_plans;                           /* K */
  int32_t num;                               /* M */
  int32_t tail;                              /* 1 .. M */
  int32_t reserved_;
  const float* ret;                          /* device [n][K][M] */
  float* score;                              /* device [n][K] out */
};
int ble_plan_risk_f32(const struct ble_plan_risk* risk, void* stream);

/*
 * Expert iteration: a policy prior for the sampler and per-action values of the plans flown.  Added without a new ABI
 * version; every size travels in a struct.
 *
 * ble_plan_prior_u16: probabilities probs [n][3] -> counts [n][segments][3], the layout of elite_counts, one lane per (e, s):
 *     w_s = s < 16 ? strength >> s : 0;   v = p_a * (float)w_s (one fp32 product);   c = p_a > 0 ? min(65535, trunc(v)) : 0
 * (a NaN or negative p_a, and a v that is NaN, give 0).  The sampler's P(a) = (c_a + 1) / (c_0 + c_1 + c_2 + 3) then leans towards the
 * prior with a weight that halves per segment.
 * BLE_E_INVALID_ARG before any HIP call: NULL pr, probs or prior_counts; n < 0; segments outside 1 .. BLE_ROLLOUT_MAX_STEPS; strength
 * outside 0 .. 65 535; n * segments >= 2^31.  n == 0: BLE_OK without a launch.
 */
struct ble_plan_prior {
  int64_t n;                                 /* environments */
  int32_t segments;                          /* ceil(H / segment) of the sampler */
  int32_t strength;                          /* 0 .. 65 535 */
  const float* probs;                        /* device [n][3] */
  uint16_t* prior_counts;                    /* device [n][segments][3] out */
};
int ble_plan_prior_u16(const struct ble_plan_prior* pr, void* stream);

/*
 * ble_plan_sample_prior_u8: ble_plan_sample_u8, except that iteration 0 draws its free plans (k >= 4) from prior_counts where
 * ble_plan_sample_u8 draws from zeros; the fixed slots, the streams, the keying and the warm start are the same, iterations >= 1 read
 * elite_counts, and all-zero prior_counts give ble_plan_sample_u8's plans bit for bit.  The fields before prior_counts are struct
 * ble_plan_sample's, in its order.
 * BLE_E_INVALID_ARG before any HIP call: what ble_plan_sample_u8 refuses, and a NULL prior_counts.
 */
struct ble_plan_sample_prior {
  int64_t n;
  int32_t n_plans;
  int32_t n_plan_steps;
  int32_t segment;
  int32_t iteration;
  unsigned long long seed;
  const unsigned long long* env_seed;
  int64_t env_offset;
  const unsigned long long* decision_counter;
  const uint16_t* elite_counts;
  const uint8_t* best_plan;
  uint8_t* plans;
  const uint16_t* prior_counts;              /* device [n][ceil(H / segment)][3]: read in iteration 0 */
};
int ble_plan_sample_prior_u8(const struct ble_plan_sample_prior* ps, void* stream);

/*
 * ble_plan_action_values_f32: one wavefront per environment over ret [n][K] (the returns, or the risk scores) and the plans' first
 * entries first_action [n][K] (plans[0]; an entry >= 2 counts as 2).  Per action a, the plan that comes first in ble_plan_select_f32's
 * order among those whose first action is a:
 *   q [n][3]       its return, bits unchanged; -Inf when no plan with a finite return takes a
 *   q_k [n][3]     its index; -1 when q is -Inf
 *   visits [n][3]  how many of the K plans take a
 * accumulate != 0 (the later iterations of a decision): q[e][a] is replaced only by ble_plan_select_f32's incumbent rule -- the new
 * value is finite and strictly better, or the stored one is not finite -- and q_k then names the new plan; otherwise q stays and q_k
 * is -1.  visits adds up.  Integer compares of (key, k) pairs only.  After a decision, an environment with a finite best_return has
 * q[e][action[e]] == best_return[e] bit for bit, and no other entry of q[e] before it in the order.
 * BLE_E_INVALID_ARG before any HIP call: NULL av, ret, first_action, q, q_k or visits; n < 0 or >= 2^31; n_plans outside
 * 1 .. BLE_PLAN_MAX_PLANS; n * n_plans >= 2^31.  n == 0: BLE_OK without a launch.
 */
struct ble_plan_action_values {
  int64_t n;
  int32_t n_plans;                           /* K */
  int32_t accumulate;                        /* 0: write; else: merge into q, q_k, visits */
  const float* ret;                          /* device [n][K] */
  const uint8_t* first_action;               /* device [n][K] */
  float* q;                                  /* device [n][3] */
  int32_t* q_k;                              /* device [n][3] */
  int32_t* visits;                           /* device [n][3] */
};
int ble_plan_action_values_f32(const struct ble_plan_action_values* av, void* stream);

/*
 * A learned terminal value: the look-ahead hands its leaves back as full states, the observation kernel observes them
 * against the parent's history, and a critic's value of every leaf is added to the plan's return.  Added without a new ABI version.
 *
 * ble_rollout_leaves_f32: ble_rollout_f32 (noise, or neither wind: the forecast) or ble_rollout_belief_f32 (belief) -- never both winds
 * -- writing ret, steps_flown, reward and final_state exactly as those calls do, bit for bit, and in addition every lane's end state
 * into `leaves`, an ordinary ble_state_f32 whose arrays hold n * n_plans environments.  Lane j = e * n_plans + k stores into index j
 * the state it holds after its last executed step: every array ble_step_f32 writes back (x .. power_load, time_elapsed_s,
 * sunrise_h_rel, sunset_rel, status, last_command, alt_fsm, env_fsm, power_paused), last_command being the RAW action of the last step
 * flown and status the lane's own (terminal if the plan went terminal), and the five per-episode constants center_lat_deg,
 * center_lng_deg, upwelling_infrared, alpha and start_unix.  A lane that flew nothing (a source that is not OK) stores the source's own
 * values, last_command included.  A leaf arena is therefore a valid state for every entry point.  leaves->vehicle is not read;
 * leaves->episode_cache is neither read nor written and may be NULL.  st is never written.  Scenarios and fleets have no such form.
 * BLE_E_INVALID_ARG before any HIP call: everything the underlying call refuses; both noise and belief given; a NULL leaves or leaf
 * array; a leaf array that is the same array of st.  n == 0: BLE_OK without a launch.
 */
int ble_rollout_leaves_f32(const ble_state_f32* st, const struct ble_rollout_f32* ro, const ble_noise_gen* noise,
                           const ble_gp_belief* belief, const ble_state_f32* leaves, uint32_t* err_flags, void* stream);

/*
 * ble_observe_leaves_f32: the 1099 features of n_leaves imagined states, one workgroup per leaf j.  The state words are read at index
 * j of `leaves`; the history ring, reset_mask and the grid (wind_grid + e * grid_env_stride) belong to the parent e = j /
 * leaves_per_env.  The semantics are get_features() of a balloon that arrived at the leaf's state at the leaf's time having measured
 * nothing on the way: the window is |t_i - t_leaf| < 6 h over the parent's ring, a pending reset_mask[e] gives an empty history, nothing
 * is appended and the window is refitted -- hist->chol and hist->n_chol are never read, and NOTHING of hist is written.  On a live
 * leaf the row equals ble_observe_f32(append = 0) without a carried factor on the same state and ring, bit for bit.  A leaf whose
 * status is not OK gets +0.0f in all 1099 entries and sets no flag.  Row j of obs starts at obs + j * obs_row_stride.  The vehicle is
 * leaves->vehicle (NULL: the default); there is no fleet form and no forecast_levels.
 * BLE_E_INVALID_ARG before any HIP call: NULL leaves, leaf array, hist, ring pointer (xyp, elapsed_s, err_uv, count), wind_grid or obs;
 * leaves_per_env < 1; n_leaves < 0, >= 2^31 or not a multiple of leaves_per_env; obs_row_stride < BLE_OBS_DIM; grid_env_stride < 0.
 * n_leaves == 0: BLE_OK without a launch.
 */
int ble_observe_leaves_f32(const ble_state_f32* leaves, int32_t leaves_per_env, const float* wind_grid, int64_t grid_env_stride,
                           const uint8_t* reset_mask, const ble_gp_history_f32* hist, float* obs, int64_t obs_row_stride,
                           uint32_t* err_flags, int64_t n_leaves, void* stream);

/*
 * ble_plan_bootstrap_f32: one lane per (e, k):
 *     d = 1.0; repeat steps_flown times: d *= gamma     (the rollout's own sequence: its discount after steps_flown steps, bit for bit)
 *     t = d * (double)value;   s = (double)ret + t      (two roundings)
 *     score = leaf_status == 0 ? (float)s : ret         (a select: a dead leaf's value is never looked at)
 * A non-finite value on a live leaf gives a non-finite score, which ble_plan_select_f32 orders last.  score may alias ret.
 * BLE_E_INVALID_ARG before any HIP call: NULL b or array; n < 0 or >= 2^31; n_plans outside 1 .. BLE_PLAN_MAX_PLANS; n * n_plans >=
 * 2^31; gamma not in [0, 1] (NaN included).  n == 0: BLE_OK without a launch.
 */
struct ble_plan_bootstrap {
  int64_t n;
  int32_t n_plans;                           /* K */
  int32_t reserved_;
  double gamma;
  const float* ret;                          /* device [n][K] */
  const int32_t* steps_flown;                /* device [n][K] */
  const uint8_t* leaf_status;                /* device [n * K]: the leaf arena's status */
  const float* value;                        /* device [n * K]: V(leaf) */
  float* score;                              /* device [n][K] out; may be ret */
};
int ble_plan_bootstrap_f32(const struct ble_plan_bootstrap* b, void* stream);

/* ------------------------------------------------------------------------------------------------ a population of policies
 * ble_qnet_forward_grouped_f32: P = members networks of ONE shape in one batch of P * R rows: rows [p R, (p + 1) R) go through weight
 * image p, which starts at net.weights + p * member_stride floats.  Row p R + r gets the bits ble_qnet_forward_f32 (head = BLE_POP_HEAD_Q)
 * or greedy ble_ac_act_f32 (head = BLE_POP_HEAD_ACTOR_GREEDY) of member p alone gives row r: the forward's batch-invariance contract, so
 * there is no tolerance.  scratch: the floats ble_qnet_workspace_f32 reports for n = P * R; the last layer's output (the logits) is
 * rows of ld floats at scratch + ((num_layers - 1) & 1) * P * R * ld.  Nothing outside rows [0, P R) of an output is written.
 * BLE_E_INVALID_ARG before any HIP call: what ble_qnet_forward_f32 refuses (descriptor, NULL net.weights / obs / scratch / action,
 * obs_row_stride < BLE_OBS_DIM, net.weights or scratch not 16-byte aligned); members < 1 or rows_per_member < 1; P * R >= 2^31 / groups
 * (groups = the widest padded layer / 64); member_stride < the image's size or not a multiple of 64; a head outside the two below;
 * BLE_POP_HEAD_ACTOR_GREEDY on a network whose num_atoms != 2, or with q_values; value or probs with BLE_POP_HEAD_Q.  The sampling
 * head of a population is ble_ac_act_grouped_f32 (below).
 */
#define BLE_POP_HEAD_Q 0
#define BLE_POP_HEAD_ACTOR_GREEDY 1
typedef struct ble_qnet_grouped_f32 {
  ble_qnet_f32 net;                          /* the members' shape, and weights = image 0 (device) */
  int32_t members;                           /* P >= 1 */
  int32_t head;                              /* BLE_POP_HEAD_* */
  int64_t member_stride;                     /* floats between images: >= packed_floats, a multiple of 64 */
  int64_t rows_per_member;                   /* R >= 1 */
  int64_t obs_row_stride;                    /* floats between observation rows, >= BLE_OBS_DIM */
  const float* obs;                          /* device [P * R] rows */
  float* scratch;                            /* device, 2 * P * R * ld floats */
  uint8_t* action;                           /* device [P * R] out */
  float* q_values;                           /* device [P * R][3] out, or NULL (BLE_POP_HEAD_Q) */
  float* value;                              /* device [P * R] out, or NULL (BLE_POP_HEAD_ACTOR_GREEDY) */
  float* probs;                              /* device [P * R][3] out, or NULL (BLE_POP_HEAD_ACTOR_GREEDY) */
} ble_qnet_grouped_f32;
int ble_qnet_forward_grouped_f32(const ble_qnet_grouped_f32* pop, void* stream);

/*
 * An evolution strategy over a packed image.  eps_i[q], the noise of stream i on LOGICAL parameter q (layer by layer, the kernel
 * row-major [in][out], then the bias: ble_qnet_unpack_f32's order), is (float) of the normal deviate (Box-Muller, cosine branch, of two
 * 53-bit uniforms) made from the four words of ONE Philox4x32-10 block: key = (seed ^ 0x45564F4C5645) with bits 32..63 of *generation
 * XORed into its high word, counter = (q & 0xFFFFFFFF, *generation & 0xFFFFFFFF, i, q >> 32).  It depends on nothing else: not on the
 * population's size, the launch, or sigma.
 * ble_es_perturb_f32: antithetic: image 2i = theta + fl(sigma * eps_i), image 2i + 1 = theta - fl(sigma * eps_i), i < members / 2
 * (members even); otherwise image i = theta + fl(sigma * eps_i), i < members.  theta: net.weights (packed).  Padding slots of every
 * image get +0.0f; the floats between images are not written.
 * ble_es_gradient_f32: tr->grad[q] = (float)(-(1 / (streams * sigma)) * sum_i (double)w[i] * (double)eps_i[q]), i ascending in float64
 * (each product rounded, then each sum), rounded once; with weight_decay != 0, then + fl(weight_decay * theta[q]) (theta:
 * tr->net.weights).  streams = members / 2 (antithetic; w[i] = (u_2i - u_2i+1) / 2) or members.  Padding slots of tr->grad get +0.0f.
 * Then *generation += 1 in stream order (device memory: a captured graph advances it on replay).
 * BLE_E_INVALID_ARG before any HIP call: NULL es, net.weights (perturb), population (perturb), generation, tr / tr->grad /
 * tr->net.weights / w (gradient); a bad network descriptor, or (gradient) one that differs from tr->net in shape; members < 1, or odd
 * with antithetic; member_stride < the image's size or not a multiple of 64 (perturb); sigma not finite or <= 0; weight_decay not finite.
 */
typedef struct ble_es_f32 {
  ble_qnet_f32 net;                          /* the shape, and weights = the centre image theta (device) */
  int32_t members;                           /* P */
  int32_t antithetic;                        /* != 0: pairs (P even) */
  int64_t member_stride;                     /* floats between images of `population` */
  float* population;                         /* device: image 0 (ble_es_perturb_f32 writes P images) */
  float sigma;
  float weight_decay;
  uint64_t seed;
  unsigned long long* generation;            /* device [1] */
} ble_es_f32;
int ble_es_perturb_f32(const ble_es_f32* es, void* stream);
int ble_es_gradient_f32(const ble_es_f32* es, const ble_qnet_train_f32* tr, const float* w, void* stream);

/*
 * ble_qnet_apply_grad_f32: the optimiser stage of ble_qnet_train_step_f32 alone, on whatever tr->grad holds: Adam's prologue
 * (*adam_step += 1, the bias corrections), Adam, the weights_t mirror -- the same kernels with the same arguments.  tr->workspace: at
 * least 64 floats (the layout of batch 0; the first 4 hold the corrections).  tr->apply_update == 0: BLE_OK, nothing launched.
 * BLE_E_INVALID_ARG before any HIP call: NULL tr, net.weights, grad or workspace; a bad network descriptor; weights_t NULL with more than
 * one layer; under apply_update: lr or an Adam hyperparameter not finite, NULL adam_m / adam_v / adam_step; a pointer not 16-byte aligned.
 */
int ble_qnet_apply_grad_f32(const ble_qnet_train_f32* tr, void* stream);

/* ------------------------------------------------------------------------------------- a population trained by gradient
 * ble_qnet_ppo_step_grouped_f32: one clipped-PPO update of P = members two-atom networks of ONE shape on a batch of P * B rows, rows
 * [p B, (p + 1) B) member p's.  Member p's part of every result -- rows [p B, (p + 1) B) of loss and of the workspace's acts, aux
 * (`targets`) and dlogits; the image-sized blocks at + p * member_stride of grad, net.weights, adam_m, adam_v and at
 * + p * transposed_stride of weights_t -- holds the bytes ble_qnet_ppo_step_f32 gives member p's own trainer on those B rows with
 * lr[p], clip[p], value_coef[p], entropy_coef[p]: the objective of member p is the mean over ITS B rows, the dW slabs are
 * wgrad_slabs(B)'s, and every sum runs in the plain update's order.  No tolerance.  The floats between images are neither read nor
 * written; the padding inside a gradient image is written as 0.  One Adam step counter serves the population (*adam_step += 1 per
 * update; the members update in lockstep).  An action >= 3 sets BLE_FLAG_TRAIN_ACTION and zeroes that row only.
 *
 * The workspace (ble_qnet_ppo_grouped_workspace_f32) is ble_qnet_train_workspace_f32's layout at a batch of P * B rows with two
 * differences: slabs = the dW slabs of B rows (not of P * B), and partial holds P * slabs blocks when slabs > 1.
 *
 * BLE_E_INVALID_ARG before any HIP call: what ble_qnet_ppo_step_f32 refuses for the corresponding fields (descriptor, batch, NULL
 * net.weights / grad / workspace / loss, weights_t NULL with more than one layer, under apply_update NULL adam_m / adam_v / adam_step
 * or a non-finite Adam hyperparameter, a pointer not 16-byte aligned); num_atoms != 2; members < 1 or rows_per_member < 1;
 * batch->batch != P * B; P * B > BLE_TRAIN_MAX_BATCH; P > 65 535 or P * slabs > 65 535; groups * P * ceil(B / 128) >= 2^31 (groups =
 * the widest padded layer / 64); member_stride < the image or not a multiple of 64; with more than one layer transposed_stride <
 * transposed_floats or not a multiple of 64; a NULL among lr, clip, value_coef, entropy_coef, old_logp, advantage, or one that is not
 * 4-byte aligned; reserved_ != 0.  The per-member arrays are DEVICE memory: the entry cannot see their values (a clip <= 0, a NaN
 * learning rate); the caller validates what it uploads (agents/population.py does).
 */
typedef struct ble_ppo_grouped_f32 {
  ble_qnet_train_f32 tr;        /* the members' shape; net.weights, weights_t, grad, adam_m, adam_v = member 0's; adam_step, workspace,
                                   adam_b1/b2/eps, apply_update shared; tr.lr, tr.target, tr.kappa not read */
  int32_t members;              /* P >= 1 */
  int32_t reserved_;            /* 0 */
  int64_t member_stride;        /* floats between members in weights, grad, adam_m, adam_v: >= the image, a multiple of 64 */
  int64_t transposed_stride;    /* floats between members' weights_t: >= transposed_floats, a multiple of 64 (any value with one layer) */
  int64_t rows_per_member;      /* B >= 1; batch->batch must equal P * B; rows [p B, (p + 1) B) are member p's */
  const float* lr;              /* device [P] */
  const float* clip;            /* device [P] */
  const float* value_coef;      /* device [P] */
  const float* entropy_coef;    /* device [P] */
  const float* old_logp;        /* device [P * B] */
  const float* advantage;       /* device [P * B] */
} ble_ppo_grouped_f32;
/* Reads the network descriptor, members, rows_per_member and reserved_ only; refuses what the update refuses of them. */
int ble_qnet_ppo_grouped_workspace_f32(const ble_ppo_grouped_f32* g, ble_qnet_train_layout* layout);
int ble_qnet_ppo_step_grouped_f32(const ble_ppo_grouped_f32* g, const ble_train_batch_f32* batch, float* loss, uint32_t* err_flags, void* stream);

/*
 * ble_ac_act_grouped_f32: ble_qnet_forward_grouped_f32's Dense stack, then ble_ac_act_f32's head over all P * R rows.  pop->head must
 * be BLE_POP_HEAD_ACTOR_GREEDY (a two-atom network read as an actor).  sample == NULL: the greedy result of
 * ble_qnet_forward_grouped_f32.  Otherwise row p R + r draws with the key (seed, env_offset + p R + r, *step): what member p's own
 * ble_ac_act_f32 on its R rows draws with env_offset + p R.  logp: device [P * R], required; pop->value and pop->probs are optional.
 * BLE_E_INVALID_ARG before any HIP call: what ble_qnet_forward_grouped_f32 refuses; another head; NULL logp; a sample with a NULL step
 * or env_offset < 0.
 */
int ble_ac_act_grouped_f32(const ble_qnet_grouped_f32* pop, const ble_ac_sample* sample, float* logp, void* stream);

/* --------------------------------------------------------------------------------- a population of replay learners
 * ble_qnet_td_step_grouped_f32: one QR-DQN or DQN update of P = members networks of ONE shape on a batch of P * B rows, rows
 * [p B, (p + 1) B) member p's.  The contract is §3q's and §3r's: member p's part of every result -- rows [p B, (p + 1) B) of loss and of
 * the workspace's acts, target_logits, targets and dlogits; the image-sized blocks at + p * member_stride of grad, net.weights, adam_m,
 * adam_v and at + p * transposed_stride of weights_t -- holds the bytes ble_qnet_train_step_f32 (kind BLE_TD_GROUPED_QUANTILE) or
 * ble_qnet_td_step_f32 with BLE_TD_DQN_MSE / BLE_TD_DQN_HUBER and BLE_TD_OPT_ADAM (kind = that BLE_TD_* + 1) gives member p's own
 * trainer -- its online image, its target image tr.target + p * member_stride, lr[p], kappa[p] -- on those B rows: the objective of
 * member p is the mean over ITS B rows, the dW slabs are wgrad_slabs(B)'s, every sum runs in the plain update's order.  No tolerance,
 * no floating-point atomics.  The floats between images are neither read nor written; the padding inside a gradient image is written as
 * 0.  One Adam step counter serves the population.  An action >= 3 sets BLE_FLAG_TRAIN_ACTION and zeroes that row only.  SARSA and
 * BLE_TD_OPT_SGD have no grouped form.
 *
 * The workspace (ble_qnet_td_grouped_workspace_f32) is ble_qnet_train_workspace_f32's layout at a batch of P * B rows with
 * ble_qnet_ppo_grouped_workspace_f32's two differences: slabs = the dW slabs of B rows, and partial holds P * slabs blocks when
 * slabs > 1.  The query reads the network descriptor, members, rows_per_member, kind and both reserved fields only.
 *
 * BLE_E_INVALID_ARG before any HIP call: what ble_qnet_ppo_step_grouped_f32 refuses of the fields the two descriptors share and what
 * ble_qnet_train_step_f32 / ble_qnet_td_step_f32 refuse of the batch (NULL next_state or discount among it); a kind outside the three;
 * a DQN kind on a network whose num_atoms != 1; NULL tr.target, or one not 16-byte aligned; NULL lr; NULL kappa with the quantile kind
 * (the DQN kinds do not read it); lr or kappa not 4-byte aligned; reserved_ or reserved2_ != 0.  The per-member arrays are DEVICE
 * memory: the entry cannot see their values (a NaN learning rate, a kappa <= 0); the caller validates what it uploads
 * (agents/population.py does: finite lr, kappa > 0).
 */
#define BLE_TD_GROUPED_QUANTILE 0            /* ble_td_grouped_f32.kind: this, BLE_TD_DQN_MSE + 1 or BLE_TD_DQN_HUBER + 1 */
typedef struct ble_td_grouped_f32 {
  ble_qnet_train_f32 tr;        /* the members' shape; net.weights, target, weights_t, grad, adam_m, adam_v = member 0's (target at the
                                   images' member_stride); adam_step, workspace, adam_b1/b2/eps, apply_update shared; tr.lr and
                                   tr.kappa not read */
  int32_t members;              /* P >= 1 */
  int32_t reserved_;            /* 0 */
  int64_t member_stride;        /* floats between members in weights, target, grad, adam_m, adam_v: >= the image, a multiple of 64 */
  int64_t transposed_stride;    /* floats between members' weights_t: >= transposed_floats, a multiple of 64 (any value with one layer) */
  int64_t rows_per_member;      /* B >= 1; batch->batch must equal P * B; rows [p B, (p + 1) B) are member p's */
  int32_t kind;                 /* BLE_TD_GROUPED_QUANTILE, BLE_TD_DQN_MSE + 1, BLE_TD_DQN_HUBER + 1 */
  int32_t reserved2_;           /* 0 */
  const float* lr;              /* device [P] */
  const float* kappa;           /* device [P], > 0: the quantile kind's Huber thresholds (not read by the DQN kinds; may be NULL there) */
} ble_td_grouped_f32;
int ble_qnet_td_grouped_workspace_f32(const ble_td_grouped_f32* g, ble_qnet_train_layout* layout);
int ble_qnet_td_step_grouped_f32(const ble_td_grouped_f32* g, const ble_train_batch_f32* batch, float* loss, uint32_t* err_flags, void* stream);

/*
 * ble_replay_sample_grouped_f32: ble_replay_sample_f32 for a population over ONE ring of N = replay->num_envs = P * R columns, columns
 * [p R, (p + 1) R) member p's, into a batch of batch->batch = P * B rows.  Row p B + b draws from the Philox stream keyed by
 * (seeds[p], b, *counter) exactly as the plain sampler does on a ring of R columns -- t over the same span, the column
 * e = (e32 * R) >> 32, the window tested, emitted and gathered at column p R + e -- so rows [p B, (p + 1) B) are what
 * ble_replay_sample_f32 writes from a ring holding only member p's R columns with seed seeds[p] and the same counter, with the index's
 * column + p R.  A failed draw gives zeros, index (-1, -1) and BLE_FLAG_REPLAY_EMPTY for that row only.  The counter advances once per
 * call (two launches; batch 0: none, as the plain call).
 * BLE_E_INVALID_ARG before any HIP call: what ble_replay_sample_f32 refuses; members < 1; num_envs % members != 0;
 * batch->batch % members != 0; NULL seeds or seeds not 8-byte aligned.  seeds: device uint64 [P].
 */
int ble_replay_sample_grouped_f32(const ble_replay_f32* replay, int32_t members, const unsigned long long* seeds,
                                  const ble_train_batch_f32* batch, uint32_t* err_flags, void* stream);

/*
 * ble_qnet_explore_grouped_u8: ble_qnet_explore_u8 for a population of P members of R = n / P rows: row p R + r draws from the stream
 * keyed by (seed[p], r, step) and becomes uniform in {0, 1, 2} when u < epsilon[p] -- member p's own ble_qnet_explore_u8 on its R
 * rows, each member at its own exploration rate.
 * BLE_E_INVALID_ARG before any HIP call: NULL ex or action; n < 0 or past ble_qnet_explore_u8's limit; members < 1; n % members != 0;
 * NULL epsilon or seed; epsilon not 4-byte or seed not 8-byte aligned; reserved_ != 0.  epsilon and seed are DEVICE memory: the caller
 * validates 0 <= epsilon <= 1 (agents/qnet_train.py's explore_grouped does, of what it uploads).
 */
typedef struct ble_explore_grouped_f32 {
  int64_t n;                           /* P * R actions */
  int32_t members;                     /* P >= 1 */
  int32_t reserved_;                   /* 0 */
  const float* epsilon;                /* device [P], each 0 .. 1 */
  const unsigned long long* seed;      /* device [P] */
  unsigned long long step;
} ble_explore_grouped_f32;
int ble_qnet_explore_grouped_u8(const ble_explore_grouped_f32* ex, uint8_t* action, void* stream);

/* ------------------------------------------------- prioritized replay and Marco Polo for a population
 * P = members sum trees over the ONE ring of ble_replay_sample_grouped_f32 (N = replay->num_envs = P * R columns, columns
 * [p R, (p + 1) R) member p's).  Member p's tree is a solo tree image in the sense of ble_sum_tree_f64 over leaves = capacity * R
 * leaves, leaf (t % capacity) R + r the window of column p R + r, at nodes + p * member_stride, with its own max_priority[p].  The
 * contract is §3t's: member p's block of nodes, max_priority[p] and rows [p B, (p + 1) B) of every batch array hold the bytes the plain
 * entry point gives a ring of member p's R columns with that tree, seeds[p] and the same counter (the index's column + p R).  The
 * doubles between the trees (member_stride > 2 padded) are neither read nor written.  No floating-point atomics; err_flags is set with
 * an integer atomic OR.  Added without a new ABI version.
 */
typedef struct ble_sum_tree_grouped_f64 {
  int64_t members;           /* P >= 1, dividing replay->num_envs (and batch->batch where a batch is given) */
  int64_t leaves;            /* PER MEMBER: capacity x num_envs / members */
  int64_t padded;            /* PER MEMBER: the smallest power of two >= leaves */
  int64_t member_stride;     /* doubles between members' trees, >= 2 padded */
  double* nodes;             /* device [P][member_stride], 8-byte aligned: member p's heap in its first 2 padded doubles */
  double* max_priority;      /* device [P], 8-byte aligned: each member's max_recorded_priority, never falls */
} ble_sum_tree_grouped_f64;

/*
 * ble_replay_tree_add_grouped_f64: ble_replay_tree_add_f64 for every member after one vector step was added, one workgroup per member.
 * ble_replay_sample_prioritized_grouped_f32: batch->batch = P * B rows, one workgroup per row; row p B + b draws from the Philox stream
 *   keyed by (seeds[p], b, *counter), q = total_p (b + u) / B over member p's tree, redrawn from that tree on an invalid window;
 *   priority [P * B] (device float32): the sampled leaf, 0 for a failed row, which fails alone (zeros, index (-1, -1),
 *   BLE_FLAG_REPLAY_EMPTY).  Advances *counter once.  seeds: device uint64 [P].
 * ble_replay_set_priority_grouped_f32: ble_replay_set_priority_f32 per member, one workgroup per member over rows [p B, (p + 1) B): the
 *   weights are normalised by the largest over member p's valid rows; leaves in batch order; a row whose index is -1 or whose column
 *   lies outside [p R, (p + 1) R) is skipped; a non-finite or negative loss leaves its leaf and sets BLE_FLAG_REPLAY_PRIORITY;
 *   max_priority[p] rises to member p's largest new leaf.
 * BLE_E_INVALID_ARG before any HIP call: what the plain entry points and ble_replay_sample_grouped_f32 refuse of the corresponding
 * fields; members < 1; num_envs % members != 0; batch->batch % members != 0; leaves != capacity * num_envs / members; padded not the
 * smallest power of two >= leaves; leaves > BLE_SUM_TREE_MAX_LEAVES; member_stride < 2 padded; NULL or misaligned nodes, max_priority
 * or seeds; a missing batch->index.  A batch of 0 rows: BLE_OK, nothing launched.
 */
int ble_replay_tree_add_grouped_f64(const ble_replay_f32* replay, const ble_sum_tree_grouped_f64* tree, void* stream);
int ble_replay_sample_prioritized_grouped_f32(const ble_replay_f32* replay, const ble_sum_tree_grouped_f64* tree,
                                              const unsigned long long* seeds, const ble_train_batch_f32* batch, float* priority,
                                              uint32_t* err_flags, void* stream);
int ble_replay_set_priority_grouped_f32(const ble_replay_f32* replay, const ble_sum_tree_grouped_f64* tree,
                                        const ble_train_batch_f32* batch, const float* priority, const float* loss, float* weighted_loss,
                                        uint32_t* err_flags, void* stream);

/*
 * ble_marco_polo_grouped_u8: ble_marco_polo_u8 for P members of R = n / P lanes: lane p R + r draws from the stream keyed by
 * (seed[p], r, *step) and its episode is exploratory when u <= probability[p] -- member p's own explorer on its R rows.  The state
 * arrays hold n = P * R lanes; one step counter, advanced once per call.
 * BLE_E_INVALID_ARG before any HIP call: what ble_marco_polo_u8 refuses of the shared fields; members < 1; n % members != 0; NULL
 * probability or seed, or either not 8-byte aligned; reserved_ != 0.  probability and seed are DEVICE memory: the caller validates
 * 0 <= probability <= 1 (agents/marco_polo.py does, of what it uploads).
 */
typedef struct ble_marco_polo_grouped_f32 {
  int64_t n;                               /* P * R lanes */
  int32_t obs_stride;                      /* floats between observation rows, >= 1 (feature 0 is read) */
  int32_t reserved_;                       /* 0 */
  int64_t members;                         /* P >= 1 */
  const double* probability;               /* device [P], each 0 .. 1: exploratory_episode_probability per member */
  const unsigned long long* seed;          /* device [P] */
  const float* obs;                        /* device [n][obs_stride] */
  const uint8_t* begin;                    /* device [n] */
  unsigned long long* step;                /* device: the draw key's step */
  int32_t* phase_clock;                    /* device [n] */
  int32_t* walk_clock;                     /* device [n] */
  uint8_t* exploratory_episode;            /* device [n] */
  uint8_t* exploratory_phase;              /* device [n] */
  double* target;                          /* device [n] */
} ble_marco_polo_grouped_f32;
int ble_marco_polo_grouped_u8(const ble_marco_polo_grouped_f32* mp, uint8_t* action, void* stream);

/* ----------------------------------------------------------------------------------------------- plan by beam search
 * A shared-prefix tree of action plans, searched level by level: D levels, one EDGE = one action flown segment * action_repeat agent
 * steps.  Per environment P_0 = 1 (the environment itself), C_d = 3 P_{d-1} children at level d, P_d = min(C_d, B) parents for the next;
 * child index c = 3 r + a, r the parent's rank in the previous selection, a in {0 DOWN, 1 STAY, 2 UP}.  A level is ble_tree_expand_f32
 * followed by ble_tree_select_f32; ble_tree_finish_f32 closes the search.  Added without a new ABI version.
 *
 * A node arena (ble_tree_arena) holds the nodes of one level, node (e, c) at index e * C_d + c: `state`, a leaf arena in the sense of
 * ble_rollout_leaves_f32 (every array that call writes), and what the rollout lane keeps in registers across steps: acc (the discounted
 * return so far, fp64), disc (gamma^flown as the rollout multiplies it up, fp64), flown (int32), and ret = (float)acc.  Two arenas of
 * n * 3 B nodes serve a whole search, alternating as source and destination.
 *
 * ble_tree_expand_f32: one lane per (e, r, a).  The lane loads node parent[e][r] of `src` -- at level 1 (parent_children == 0)
 * environment e of `st`, with acc 0, disc 1, flown 0 --, flies the edge with ble_rollout_f32's / ble_rollout_belief_f32's loop body and
 * stores the child into index e * 3 n_parents + c of `dst`.  The grid, the noise key (seed, env_offset + e, episode[e]), the belief slab
 * and the per-episode cache are environment e's, whatever the node.  A non-void node reached by (a_1 .. a_d) holds, bit for bit, the
 * state, (float)acc and flown ble_rollout_leaves_f32 gives the plan a_1 x segment, .., a_d x segment flown from environment e in the same
 * wind.  A parent whose status is not OK flies nothing: its a = 0 child is the parent carried on unchanged (state, acc, disc, flown), its
 * a = 1 and a = 2 children are VOID: the same copy with acc = NaN.  A node whose acc is NaN is void: it flies nothing and all its
 * children are void.  st, the history and every cache are never written; flags go to err_flags -- give it a word of its own, as for
 * ble_rollout_f32.  noise / belief: ble_rollout_leaves_f32's two winds (neither: the forecast).
 * BLE_E_INVALID_ARG before any HIP call: NULL st, state array, ex, wind_grid, dst.state or an array of it, dst.acc / disc / flown / ret;
 * n < 0; beam outside 1 .. BLE_TREE_MAX_BEAM; n * 3 * beam >= 2^31; segment < 1, action_repeat < 1, depth < 1 or
 * depth * segment * action_repeat > BLE_ROLLOUT_MAX_STEPS; substeps outside 1 .. BLE_MAX_SUBSTEPS; gamma NaN or outside [0, 1]; a
 * negative grid_env_stride or noise->env_offset; both noise and belief; what ble_rollout_belief_f32 refuses of a belief, a belief whose n
 * is not ex->n included; an invalid st->vehicle; reserved_ != 0; level 1 (parent_children == 0) with n_parents != 1; a later level with a
 * NULL parent, src.state (or an array of it), src.acc / disc / flown, parent_children not a multiple of 3 in 3 .. 3 * beam, or n_parents
 * outside 1 .. min(parent_children, beam); an array of dst.state that is the same array of st or of src.state (st is never written, and
 * a level is not expanded in place).  n == 0: BLE_OK without a launch.  A fleet has no form of this call.
 */
#define BLE_TREE_MAX_BEAM 256
struct ble_tree_arena {
  const ble_state_f32* state;                /* a leaf arena of n * 3 * beam environments (its vehicle and episode cache are not read) */
  double* acc;                               /* device [n * 3 * beam] */
  double* disc;                              /* device [n * 3 * beam] */
  int32_t* flown;                            /* device [n * 3 * beam] */
  float* ret;                                /* device [n * 3 * beam]: (float)acc; of a level, [n][C_d] */
};
struct ble_tree_expand {
  int64_t n;                                 /* source environments */
  int32_t beam;                              /* B, 1 .. BLE_TREE_MAX_BEAM: the row length of parent */
  int32_t depth;                             /* D >= 1: the levels of the whole search (bounds the plan: D * segment * action_repeat) */
  int32_t n_parents;                         /* P_{d-1}: 1 at level 1 */
  int32_t parent_children;                   /* C_{d-1}: 0 at level 1 (the parents are st's environments) */
  int32_t segment;                           /* >= 1 plan entries per edge */
  int32_t action_repeat;                     /* >= 1 agent steps per plan entry */
  int32_t substeps;                          /* 1 .. BLE_MAX_SUBSTEPS */
  int32_t reserved_;                         /* 0 */
  double gamma;                              /* finite, 0 <= gamma <= 1 */
  const float* wind_grid;                    /* as for ble_step_f32 */
  int64_t grid_env_stride;
  const int32_t* parent;                     /* device [n][beam]: ble_tree_select_f32's list of the level above; level 1: not read */
  struct ble_tree_arena src;                 /* the level above; level 1: not read */
  struct ble_tree_arena dst;                 /* this level, written */
};
int ble_tree_expand_f32(const ble_state_f32* st, const struct ble_tree_expand* ex, const ble_noise_gen* noise, const ble_gp_belief* belief,
                        uint32_t* err_flags, void* stream);

/*
 * ble_tree_select_f32: one wavefront per environment over ret [n][C], the returns of a level's children, in ble_plan_select_f32's order
 * with k := c: a finite return before a non-finite one, then the return descending (-0 == +0), then c ascending.  The first
 * min(C, beam) children in that order become parent[e][0 ..] and, the same numbers, choice[e][0 ..] -- the caller keeps one choice list
 * per level, [D][n][beam], for the walk back.  Entries from min(C, beam) on are not written.  Integer compares only, no atomics.
 * BLE_E_INVALID_ARG before any HIP call: NULL sel, ret, parent or choice; n < 0; beam outside 1 .. BLE_TREE_MAX_BEAM; n_children not a
 * multiple of 3 in 3 .. 3 * beam; n * 3 * beam >= 2^31.  n == 0: BLE_OK without a launch.
 */
struct ble_tree_select {
  int64_t n;
  int32_t n_children;                        /* C_d */
  int32_t beam;                              /* B */
  const float* ret;                          /* device [n][C_d] */
  int32_t* parent;                           /* device [n][beam] out */
  int32_t* choice;                           /* device [n][beam] out: this level's list */
};
int ble_tree_select_f32(const struct ble_tree_select* sel, void* stream);

/*
 * ble_tree_finish_f32: one wavefront per environment over the C_D children of the last level.  The key of a child is score[e][c]
 * (NULL: ret[e][c]; with a leaf value, ble_plan_bootstrap_f32's score of the last arena) in the order above.  The child of rank 0 is
 * walked back through choice -- the action of level d is c_d % 3 and c_{d-1} = choice[d - 1][e][c_d / 3] -- giving
 *   best_plan [D * segment][n]   each level's action repeated over its segment
 *   action [n]                   the first of them
 *   best_return [n]              the key of that child, bits unchanged
 * An environment whose source is not OK (source_status[e] != 0) gets best_plan all STAY, action STAY and best_return +0.0f; one with no
 * finite key gets all STAY and best_return -Inf (ble_plan_select_f32's answer).  On request (q and visits both given), with the meaning
 * and encoding of ble_plan_action_values_f32: q[e][a] the best key among the children whose level-1 action is a, -Inf when none of them
 * has a finite key; visits[e][a] the number of non-void children (ret not NaN) whose level-1 action is a.
 * BLE_E_INVALID_ARG before any HIP call: NULL fin, ret, source_status, choice, best_plan, action or best_return; exactly one of q and
 * visits; n < 0; beam outside 1 .. BLE_TREE_MAX_BEAM; n_children not a multiple of 3 in 3 .. 3 * beam; depth < 1, segment < 1 or
 * depth * segment > BLE_ROLLOUT_MAX_STEPS; depth == 1 with n_children != 3; n * 3 * beam >= 2^31.  n == 0: BLE_OK without a launch.
 */
struct ble_tree_finish {
  int64_t n;
  int32_t n_children;                        /* C_D */
  int32_t beam;                              /* B */
  int32_t depth;                             /* D */
  int32_t segment;
  const float* ret;                          /* device [n][C_D]: the last arena's ret */
  const float* score;                        /* device [n][C_D], or NULL: ret */
  const uint8_t* source_status;              /* device [n]: st->status */
  const int32_t* choice;                     /* device [D][n][beam]: levels 1 .. D - 1 are read */
  uint8_t* best_plan;                        /* device [D * segment][n] out */
  uint8_t* action;                           /* device [n] out */
  float* best_return;                        /* device [n] out */
  float* q;                                  /* device [n][3] out, or NULL */
  int32_t* visits;                           /* device [n][3] out, or NULL */
};
int ble_tree_finish_f32(const struct ble_tree_finish* fin, void* stream);

/* ------------------------------------------------------------------------------ beam search in scenario winds
 * The tree above flown in the M = scn->num scenario winds of ble_gp_fit_scenarios_f32.  A GROUP (e, c) is M scenario nodes, node
 * (e, c, m) at index (e * C_d + c) * M + m of the level's arena; the arenas of `ex` hold n * 3 * beam * M nodes, and the last level's
 * is a leaf arena of C_D * M leaves per environment.  Added without a new ABI version.
 *
 * ble_tree_expand_scenarios_f32: one lane per (e, r, a, m), lane index = destination node index.  The lane loads node
 * (e * C_{d-1} + parent[e][r]) * M + m of `src` -- at level 1 environment e of `st`, with acc 0, disc 1, flown 0 --, flies the edge with
 * ble_rollout_scenarios_f32's loop body in scenario m of environment e and stores the child as ble_tree_expand_f32 does.  A scenario
 * node is STOPPED when its status is not OK or its acc is NaN: it flies nothing and is carried on unchanged (state, acc, disc, flown)
 * under EVERY action, as a frozen lane of ble_rollout_scenarios_f32 is.  A group whose M nodes are all stopped is SPENT: its a = 0 child
 * group is the carry, its a = 1 and a = 2 child groups are VOID -- the same copies with acc = NaN in all M nodes.  A void group is spent,
 * so all its descendants are void.  At level 1 the group is spent exactly when st->status[e] is not OK.  A node of a non-void group
 * reached by (a_1 .. a_d) holds, bit for bit, the ret, steps_flown and final_state words ble_rollout_scenarios_f32 gives the plan
 * a_1 x segment, .., a_d x segment in scenario m from environment e, and as its state what ble_gp_scenario_wind_f32 followed by
 * ble_step_f32 leave on a copy.  A level's ret is [n][C_d][M]: ble_plan_risk_f32 (n_plans = C_d) maps it to the [n][C_d] that
 * ble_tree_select_f32 and ble_tree_finish_f32 take.  st, the history, the slab and every cache are never written; flags go to err_flags
 * -- give it a word of its own.
 * BLE_E_INVALID_ARG before any HIP call: everything ble_tree_expand_f32 refuses of st and ex, with the bound n * 3 * beam * num >= 2^31;
 * what ble_gp_fit_scenarios_f32 refuses of scn and gen; scn->n other than ex->n.  n == 0: BLE_OK without a launch.  A fleet has no form
 * of this call.
 */
int ble_tree_expand_scenarios_f32(const ble_state_f32* st, const struct ble_tree_expand* ex, const ble_gp_scenarios* scn,
                                  const ble_scenario_gen* gen, uint32_t* err_flags, void* stream);

/* ------------------------------------------------------------------------------------------- guided tree search
 * PUCT over a persistent node pool: R rounds of L descents per environment, every new node evaluated once by the caller's network, mean
 * backups, the root's visit counts as the answer.  Deterministic: no random stream.  Added without a new ABI version.
 *
 * The pool (ble_mcts_pool) holds cap = 1 + 3 L R node ids per environment.  Id 0 is the root: environment e of `st` itself, never copied,
 * read as level 1 of ble_tree_expand_f32 reads st.  Id 1 + r 3L + 3l + a is the child under action a of the l-th leaf chosen in round r.
 * `nodes` is a ble_tree_arena of R * n * 3L entries stored round-major, [R][n][3L]: node id >= 1 of environment e lies at
 * ((id - 1) / 3L * n + e) * 3L + (id - 1) % 3L, so the nodes born in round r are the contiguous slice [r n 3L, (r + 1) n 3L) -- a leaf
 * arena of 3L leaves per environment (ble_observe_leaves_f32 takes it as it is).  The statistics lie [n][cap]: parent (-1: the root, or
 * a node that was never grown), first_child (0: not expanded), depth, visits, pending (int32), value_sum and g (fp64), prior [n][cap][3]
 * (fp32); per environment g_range [n][2] = (g_lo, g_hi), the smallest and largest G seen; leaf and kind [n][L] are the round's slots.
 * G = acc + disc * V(node), fp64, the product and the sum two statements; V = 0 where the node's status is not OK and where there is no
 * value.  A node whose acc is NaN is VOID: no G, visits 0, never selected.
 *
 * ble_mcts_select_f32(round): L descents per environment in order l = 0 .. L - 1; round 0 first initialises the root (visits 0, prior
 * root_prior[e] or, NULL, uniform; g_range empty).  At an expanded node a descent takes the non-void child of the largest
 *   score = Qn + c_puct * prior[a] * sqrt(Nv(node)) / (1 + Nv(child)),   Nv = visits + pending,
 *   Qn = (value_sum / visits - g_lo) / (g_hi - g_lo) * (visits / Nv)      (0 unless g_hi > g_lo)
 * in fp64, one operation per statement, ties to the lower action.  It ends as kind[e][l] =
 *   BLE_MCTS_EXPAND   at a node that is not expanded, OK, of depth < max_depth, not chosen by an earlier slot of this round; pending += 3
 *                     on the node and all its ancestors
 *   BLE_MCTS_EMPTY    at a node an earlier slot of this round chose (and every slot of a root that is not OK or has three void children)
 *   BLE_MCTS_REVISIT  at a node that cannot grow: status not OK, depth == max_depth, or three void children; pending += 1 on its path
 * with leaf[e][l] the node.  source_status: st->status.
 *
 * ble_mcts_expand_f32(round): one lane per (e, l, a).  The lanes of an EXPAND slot load node leaf[e][l] (id 0: environment e of st, acc 0,
 * disc 1, flown 0), fly one edge of segment * action_repeat agent steps under action a with ble_rollout_f32's loop body in environment e's
 * wind, and store the child -- state, acc, disc, flown, ret -- at index e 3L + 3l + a of the round's slice.  The lanes of any other slot
 * fly nothing and store void nodes (the source's words, acc NaN).  A non-void node reached by (a_1 .. a_d) holds, bit for bit, the state,
 * (float)acc and flown ble_rollout_leaves_f32 gives the plan a_1 x segment, .., a_d x segment from environment e in the same wind.  st,
 * the history, the belief slab and every cache are never written; flags go to err_flags.  noise / belief: ble_tree_expand_f32's winds.
 *
 * ble_mcts_backup_f32(round): per environment, slots in order l, then a.  value [n 3L] and probs [n 3L][3] are the network's answers
 * on the round's slice (both NULL: V = 0, uniform priors).  A non-void newborn gets parent, depth, first_child 0, prior = its probs row (a
 * row with a non-finite or negative entry: uniform), g = G, visits 1, value_sum G; g_range takes G; every ancestor gets visits += 1 and
 * value_sum += G; the leaf's first_child is set.  A REVISIT slot adds (1, g of its node) to the node and its ancestors.  pending is cleared.
 * After any round visits[node] is the number of non-void nodes in its subtree (itself included; the root: excluded) plus the revisits in
 * it, and value_sum the sum of their G in backup order.
 *
 * ble_mcts_finish_f32: visits [n][3] and q [n][3] of the root's children (q: the mean value as fp32, -Inf for a void child: the encoding
 * of ble_tree_finish_f32); action: the child with the most visits, ties to the larger q, then to the lower action; best_return =
 * q[action]; the principal variation -- that rule followed down to a node without visited children -- as best_plan [D * segment][n],
 * padded with STAY, and pv_length [n] (edges).  A source that is not OK: all STAY, +0.0f; a root without a visited child: all STAY, -Inf.
 *
 * BLE_E_INVALID_ARG before any HIP call, all four: NULL pool or any pointer of it (nodes.state or an array of it, acc, disc, flown, ret
 * included); n < 0; num_rounds < 1, leaves_per_round < 1 or their product > BLE_MCTS_MAX_LEAVES; max_depth < 1, segment < 1 or
 * max_depth * segment > BLE_ROLLOUT_MAX_STEPS; n * cap >= 2^31; reserved_ != 0.  select, expand, backup: round outside 0 .. num_rounds - 1.
 * select: NULL source_status; c_puct NaN, infinite or negative.  backup: exactly one of value and probs.  finish: NULL fin or any pointer
 * of it.  expand: NULL st, state array, ex or wind_grid; action_repeat < 1 or max_depth * segment * action_repeat >
 * BLE_ROLLOUT_MAX_STEPS; substeps outside 1 .. BLE_MAX_SUBSTEPS; gamma NaN or outside [0, 1]; a negative grid_env_stride or
 * noise->env_offset; both noise and belief; what ble_rollout_belief_f32 refuses of a belief, a belief whose n is not the pool's included;
 * an invalid st->vehicle; ex->reserved_ != 0; an array of nodes.state that is the same array of st.  n == 0: BLE_OK without a launch.
 * A fleet has no form of these calls.
 */
#define BLE_MCTS_MAX_LEAVES 256
#define BLE_MCTS_EMPTY 0
#define BLE_MCTS_EXPAND 1
#define BLE_MCTS_REVISIT 2
struct ble_mcts_pool {
  int64_t n;                                 /* source environments */
  int32_t num_rounds;                        /* R >= 1 */
  int32_t leaves_per_round;                  /* L >= 1, L * R <= BLE_MCTS_MAX_LEAVES */
  int32_t max_depth;                         /* D >= 1 edges */
  int32_t segment;                           /* >= 1 plan entries per edge */
  int64_t reserved_;                         /* 0 */
  struct ble_tree_arena nodes;               /* R * n * 3L entries, [R][n][3L] */
  int32_t* parent;                           /* device [n][cap] */
  int32_t* first_child;                      /* device [n][cap] */
  int32_t* depth;                            /* device [n][cap] */
  int32_t* visits;                           /* device [n][cap] */
  int32_t* pending;                          /* device [n][cap] */
  double* value_sum;                         /* device [n][cap] */
  double* g;                                 /* device [n][cap] */
  float* prior;                              /* device [n][cap][3] */
  double* g_range;                           /* device [n][2] */
  int32_t* leaf;                             /* device [n][L] */
  int32_t* kind;                             /* device [n][L] */
};
struct ble_mcts_expand {
  int32_t round;                             /* 0 .. R - 1 */
  int32_t action_repeat;                     /* >= 1 agent steps per plan entry */
  int32_t substeps;                          /* 1 .. BLE_MAX_SUBSTEPS */
  int32_t reserved_;                         /* 0 */
  double gamma;                              /* finite, 0 <= gamma <= 1 */
  const float* wind_grid;                    /* as for ble_step_f32 */
  int64_t grid_env_stride;
};
struct ble_mcts_finish {
  const uint8_t* source_status;              /* device [n]: st->status */
  uint8_t* best_plan;                        /* device [D * segment][n] out */
  uint8_t* action;                           /* device [n] out */
  float* best_return;                        /* device [n] out */
  float* q;                                  /* device [n][3] out */
  int32_t* visits;                           /* device [n][3] out */
  int32_t* pv_length;                        /* device [n] out */
};
int ble_mcts_select_f32(const struct ble_mcts_pool* pool, int32_t round, double c_puct, const uint8_t* source_status, const float* root_prior,
                        void* stream);
int ble_mcts_expand_f32(const ble_state_f32* st, const struct ble_mcts_pool* pool, const struct ble_mcts_expand* ex, const ble_noise_gen* noise,
                        const ble_gp_belief* belief, uint32_t* err_flags, void* stream);
int ble_mcts_backup_f32(const struct ble_mcts_pool* pool, int32_t round, const float* value, const float* probs, void* stream);
int ble_mcts_finish_f32(const struct ble_mcts_pool* pool, const struct ble_mcts_finish* fin, void* stream);

/* ---------------------------------------------------------------------------- guided tree search in scenario winds
 * The search above flown in the M = scn->num scenario winds of ble_gp_fit_scenarios_f32.  Added without a new ABI version.
 *
 * The pool of groups.  Node id i of environment e is a GROUP of M scenario nodes.  `nodes` of the ble_mcts_pool holds R * n * 3L * M
 * entries laid out [R][n][3L][M]: node (id, m) lies at (((id - 1) / 3L * n + e) * 3L + (id - 1) % 3L) * M + m, so the nodes born in
 * round r are one contiguous leaf arena of 3L * M leaves per environment (ble_observe_leaves_f32 takes the slice as it is).  Id 0 is
 * environment e of `st` itself for every m, with acc 0, disc 1, flown 0.  The statistics, leaf and kind stay per group, [n][cap] with
 * cap = 1 + 3 L R, and mean what they mean above.  Two more arrays per group, each [R][n][3L] (a group's index is its node index
 * without M): group_status (uint8; 0: live, 1: spent) and group_g (fp64).
 *
 * Stopped, spent, void (§3u's definitions).  A scenario node is STOPPED when its status is not OK or its acc is NaN.  A group is SPENT
 * when all M of its nodes are stopped, VOID when its acc is NaN in all M nodes.  For the select a group's "status OK" is "not spent": a
 * spent group is never EXPAND, it is REVISIT.
 *
 * ble_mcts_expand_scenarios_f32(round): one lane per (e, l, a, m); the lane index within the round's slice, (e * 3L + 3l + a) * M + m,
 * is the destination node index.  The lanes of an EXPAND slot take their rule from the parent group's M status bytes and acc words
 * (the root: st->status[e]): a live node flies one edge of segment * action_repeat agent steps under action a in scenario m of
 * environment e, with ble_rollout_scenarios_f32's loop body; a stopped node inside a live group is carried on unchanged -- state, acc,
 * disc, flown -- under every action.  The lanes of any other slot fly nothing and store void nodes (the source's words, acc NaN).  No
 * arithmetic of its own: a node of a non-void group reached by (a_1 .. a_d) holds, bit for bit, the state words, (float)acc and flown
 * ble_rollout_scenarios_f32 gives the plan a_1 x segment, .., a_d x segment in scenario m from environment e.  st, the history, the
 * scenario slab and every cache are never written; flags go to err_flags -- give it a word of its own.
 *
 * ble_mcts_backup_scenarios_f32(round): per environment, slots in order l, then a; per group first the group step over its M nodes:
 *   G_m = acc_m + disc_m * V_m, fp64, the product and the sum two statements; V_m = value[node] where value is given and the node's
 *         status is OK, else 0 (a value on a node that is not OK is never read into G);
 *   G   = the mean of the `tail` smallest G_m in ble_plan_risk_f32's order -- G_m ascending with -0 equal to +0, then m ascending --,
 *         summed in that order in double from 0.0 and divided by tail once; kept in fp64, never rounded to float.  tail = num: the
 *         expectation; tail = 1: the worst case.  Any non-finite G_m: the group is treated as void -- visits 0, g NaN, never selected;
 *   prior = uniform where probs is NULL; else the mean of the probs rows of the group's nodes whose status is OK, m ascending, each
 *         component summed in double from 0.0, divided by their number once and rounded to float once; uniform if there is no such
 *         node or if one of those rows has a non-finite or negative entry;
 *   group_status = 1 if all M nodes are stopped, else 0; group_g = G (NaN: void).
 * Then ble_mcts_backup_f32's rules with that G, prior and status: parent, depth, first_child, visits, value_sum, g, g_range, the path
 * to the root, REVISIT, pending cleared.  value [n * 3L * M] and probs [n * 3L * M][3] are the network's answers on the round's slice,
 * both NULL or both given.  q and best_return of the finish are means of group Gs: risk scores.
 *
 * Select and finish: ble_mcts_select_f32 and ble_mcts_finish_f32 on a second ble_mcts_pool -- the same statistics, leaf and kind --
 * whose nodes.state->status points at group_status (the other arrays of that state are not read; they must not be NULL).
 *
 * BLE_E_INVALID_ARG before any HIP call: expand -- everything ble_mcts_expand_f32 refuses of st, pool and ex; what
 * ble_gp_fit_scenarios_f32 refuses of scn and gen; scn->n other than pool->n; n * 3L * num >= 2^31.  backup -- everything
 * ble_mcts_backup_f32 refuses; num outside 1 .. BLE_SCENARIO_MAX; tail outside 1 .. num; n * 3L * num >= 2^31; NULL group_status or
 * group_g.  n == 0: BLE_OK without a launch.  A fleet has no form of these calls.
 */
int ble_mcts_expand_scenarios_f32(const ble_state_f32* st, const struct ble_mcts_pool* pool, const struct ble_mcts_expand* ex,
                                  const ble_gp_scenarios* scn, const ble_scenario_gen* gen, uint32_t* err_flags, void* stream);
int ble_mcts_backup_scenarios_f32(const struct ble_mcts_pool* pool, int32_t round, int32_t num, int32_t tail, const float* value,
                                  const float* probs, uint8_t* group_status, double* group_g, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BLE_ABI_H_ */
