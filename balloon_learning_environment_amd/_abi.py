"""ctypes mirror of include/ble_abi.h (struct ble_state_f32 and field metadata)."""
import ctypes

import numpy as np

# (name, numpy dtype, ctypes scalar type, mutable?) in the order of struct ble_state_f32.
STATE_FIELDS = (
    ('x', np.float32, ctypes.c_float), ('y', np.float32, ctypes.c_float),
    ('pressure', np.float32, ctypes.c_float), ('ambient_temperature', np.float32, ctypes.c_float),
    ('internal_temperature', np.float32, ctypes.c_float), ('envelope_volume', np.float32, ctypes.c_float),
    ('superpressure', np.float32, ctypes.c_float), ('mols_air', np.float32, ctypes.c_float),
    ('battery_charge', np.float32, ctypes.c_float),
    ('acs_power', np.float32, ctypes.c_float), ('acs_mass_flow', np.float32, ctypes.c_float),
    ('solar_charging', np.float32, ctypes.c_float), ('power_load', np.float32, ctypes.c_float),
    ('center_lat_deg', np.float32, ctypes.c_float), ('center_lng_deg', np.float32, ctypes.c_float),
    ('upwelling_infrared', np.float32, ctypes.c_float), ('alpha', np.float32, ctypes.c_float),
    ('start_unix', np.int64, ctypes.c_int64),
    ('time_elapsed_s', np.int32, ctypes.c_int32),
    ('sunrise_h_rel', np.int32, ctypes.c_int32), ('sunset_rel', np.int32, ctypes.c_int32),
    ('status', np.uint8, ctypes.c_uint8), ('last_command', np.uint8, ctypes.c_uint8),
    ('alt_fsm', np.uint8, ctypes.c_uint8), ('env_fsm', np.uint8, ctypes.c_uint8),
    ('power_paused', np.uint8, ctypes.c_uint8),
)
FIELD_NAMES = tuple(f[0] for f in STATE_FIELDS)
FIELD_DTYPES = {f[0]: f[1] for f in STATE_FIELDS}
MUTABLE_FLOATS = FIELD_NAMES[:9]
DERIVED_FLOATS = FIELD_NAMES[9:13]
EPISODE_CONSTS = FIELD_NAMES[13:18]


EPISODE_CACHE_ROWS = 7     # BLE_EPISODE_CACHE_ROWS


class BleVehicle(ctypes.Structure):
  """struct ble_vehicle (ABI 5): BalloonState's flight-vehicle constants (reference env/balloon/balloon.py:156-173), mols_lift_gas
  (:183) and power_safety_layer_enabled (:200) -- a HOST struct of doubles, one per call."""
  _fields_ = [('envelope_volume_base', ctypes.c_double), ('envelope_volume_dv_pressure', ctypes.c_double), ('envelope_mass', ctypes.c_double),
              ('envelope_max_superpressure', ctypes.c_double), ('envelope_cod', ctypes.c_double), ('payload_mass', ctypes.c_double),
              ('nighttime_power_load_w', ctypes.c_double), ('daytime_power_load_w', ctypes.c_double),
              ('acs_valve_hole_diameter_m', ctypes.c_double), ('battery_capacity_wh', ctypes.c_double), ('mols_lift_gas', ctypes.c_double),
              ('power_safety_layer_enabled', ctypes.c_int32), ('reserved_', ctypes.c_int32)]


VEHICLE_FIELDS = tuple(f[0] for f in BleVehicle._fields_[:-1])
# the reference's defaults (balloon.py:156-173,183,200) == what ble_vehicle_default() writes (tests/test_host_api.py)
VEHICLE_DEFAULTS = dict(envelope_volume_base=1804.0, envelope_volume_dv_pressure=0.0199, envelope_mass=68.5, envelope_max_superpressure=2380.0,
                        envelope_cod=0.25, payload_mass=92.5, nighttime_power_load_w=183.7, daytime_power_load_w=120.4,
                        acs_valve_hole_diameter_m=0.04, battery_capacity_wh=3058.56, mols_lift_gas=6830.0, power_safety_layer_enabled=1)


def vehicle_struct(**overrides):
  """A BleVehicle with the reference's defaults and the given fields replaced; None when nothing differs from the defaults
  (ble_state_f32.vehicle == NULL: the kernels with compile-time vehicle constants)."""
  unknown = set(overrides) - set(VEHICLE_DEFAULTS)
  if unknown:
    raise TypeError(f'unknown vehicle field(s) {sorted(unknown)}')
  values = dict(VEHICLE_DEFAULTS)
  values.update({k: (int(bool(v)) if k == 'power_safety_layer_enabled' else float(v)) for k, v in overrides.items()})
  if values == VEHICLE_DEFAULTS:
    return None
  return BleVehicle(reserved_=0, **values)


class BleStateF32(ctypes.Structure):
  # the per-env arrays, then the optional [EPISODE_CACHE_ROWS][n] float64 cache of per-episode derived constants, then the optional
  # HOST pointer to the vehicle (ABI 5)
  _fields_ = ([(name, ctypes.POINTER(ct)) for name, _, ct in STATE_FIELDS] + [('episode_cache', ctypes.POINTER(ctypes.c_double))] +
              [('vehicle', ctypes.POINTER(BleVehicle))])


def state_struct(pointers, episode_cache: int = 0, vehicle=None):
  """Builds a BleStateF32 from a {field: integer address} mapping (+ the address of the optional episode cache, + an optional
  BleVehicle, which the returned struct keeps alive)."""
  st = BleStateF32()
  for name, _, ct in STATE_FIELDS:
    setattr(st, name, ctypes.cast(ctypes.c_void_p(int(pointers[name])), ctypes.POINTER(ct)))
  st.episode_cache = ctypes.cast(ctypes.c_void_p(int(episode_cache) or None), ctypes.POINTER(ctypes.c_double))
  set_vehicle(st, vehicle)
  return st


def set_vehicle(st, vehicle) -> None:
  """Points st.vehicle at `vehicle` (a BleVehicle, kept alive by `st`) or at NULL (None: the reference's defaults)."""
  st._vehicle_keepalive = vehicle
  st.vehicle = ctypes.pointer(vehicle) if vehicle is not None else ctypes.POINTER(BleVehicle)()


class BleGpHistoryF32(ctypes.Structure):
  """struct ble_gp_history_f32."""
  _fields_ = [('xyp', ctypes.POINTER(ctypes.c_float)), ('elapsed_s', ctypes.POINTER(ctypes.c_int32)),
              ('err_uv', ctypes.POINTER(ctypes.c_float)), ('count', ctypes.POINTER(ctypes.c_int32)),
              ('chol', ctypes.POINTER(ctypes.c_double)), ('n_chol', ctypes.POINTER(ctypes.c_int32)),
              ('chol_stride', ctypes.c_int64)]


class BleGpQueryF32(ctypes.Structure):
  """struct ble_gp_query_f32: q query points per environment for ble_gp_query_f32 (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('q', ctypes.c_int32), ('add_forecast', ctypes.c_int32), ('xyp', ctypes.c_void_p),
              ('time_s', ctypes.c_void_p), ('wind_grid', ctypes.c_void_p), ('grid_env_stride', ctypes.c_int64),
              ('mean_uv', ctypes.c_void_p), ('deviation', ctypes.c_void_p)]


class BleRolloutF32(ctypes.Structure):
  """struct ble_rollout_f32: K action plans per environment for ble_rollout_f32 (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('n_plans', ctypes.c_int32), ('n_plan_steps', ctypes.c_int32), ('action_repeat', ctypes.c_int32),
              ('substeps', ctypes.c_int32), ('gamma', ctypes.c_double), ('plans', ctypes.c_void_p), ('wind_grid', ctypes.c_void_p),
              ('grid_env_stride', ctypes.c_int64), ('ret', ctypes.c_void_p), ('steps_flown', ctypes.c_void_p), ('reward', ctypes.c_void_p),
              ('final_state', ctypes.c_void_p)]


ROLLOUT_MAX_STEPS = 960      # BLE_ROLLOUT_MAX_STEPS
GP_BELIEF_DOUBLES = 720      # BLE_GP_BELIEF_DOUBLES


class BleGpBelief(ctypes.Structure):
  """struct ble_gp_belief: a fitted WindGP kept on the device (ble_gp_fit_f32): the slab [n][stride] of float64 and n_obs [n] int32,
  device pointers, and the number of environments (the sizes of the belief's calls travel in the struct)."""
  _fields_ = [('slab', ctypes.c_void_p), ('stride', ctypes.c_int64), ('n_obs', ctypes.c_void_p), ('n', ctypes.c_int64)]


PLAN_MAX_PLANS, PLAN_MAX_ITERATIONS = 1024, 16      # BLE_PLAN_MAX_PLANS, BLE_PLAN_MAX_ITERATIONS


class BlePlanSample(ctypes.Structure):
  """struct ble_plan_sample: K piecewise-constant action plans per environment for ble_plan_sample_u8 (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('n_plans', ctypes.c_int32), ('n_plan_steps', ctypes.c_int32), ('segment', ctypes.c_int32),
              ('iteration', ctypes.c_int32), ('seed', ctypes.c_uint64), ('env_seed', ctypes.c_void_p), ('env_offset', ctypes.c_int64),
              ('decision_counter', ctypes.c_void_p), ('elite_counts', ctypes.c_void_p), ('best_plan', ctypes.c_void_p),
              ('plans', ctypes.c_void_p)]


class BlePlanSelect(ctypes.Structure):
  """struct ble_plan_select: the returns of those plans and what ble_plan_select_f32 writes (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('n_plans', ctypes.c_int32), ('n_plan_steps', ctypes.c_int32), ('segment', ctypes.c_int32),
              ('iteration', ctypes.c_int32), ('elite', ctypes.c_int32), ('reserved_', ctypes.c_int32), ('ret', ctypes.c_void_p),
              ('plans', ctypes.c_void_p), ('best_return', ctypes.c_void_p), ('best_k', ctypes.c_void_p), ('best_plan', ctypes.c_void_p),
              ('action', ctypes.c_void_p), ('elite_counts', ctypes.c_void_p), ('advance_counter', ctypes.c_void_p)]


class BlePlanPrior(ctypes.Structure):
  """struct ble_plan_prior: probs [n][3] -> prior counts [n][segments][3] for ble_plan_prior_u16 (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('segments', ctypes.c_int32), ('strength', ctypes.c_int32), ('probs', ctypes.c_void_p),
              ('prior_counts', ctypes.c_void_p)]


class BlePlanSamplePrior(ctypes.Structure):
  """struct ble_plan_sample_prior: BlePlanSample's fields, then the prior counts iteration 0 draws from (ble_plan_sample_prior_u8)."""
  _fields_ = BlePlanSample._fields_ + [('prior_counts', ctypes.c_void_p)]


class BlePlanActionValues(ctypes.Structure):
  """struct ble_plan_action_values: ret [n][K] and the plans' first actions -> q, q_k, visits [n][3] (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('n_plans', ctypes.c_int32), ('accumulate', ctypes.c_int32), ('ret', ctypes.c_void_p),
              ('first_action', ctypes.c_void_p), ('q', ctypes.c_void_p), ('q_k', ctypes.c_void_p), ('visits', ctypes.c_void_p)]


class BlePlanBootstrap(ctypes.Structure):
  """struct ble_plan_bootstrap: ret [n][K], steps_flown [n][K], the leaves' status and value [n K] -> score [n][K] (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('n_plans', ctypes.c_int32), ('reserved_', ctypes.c_int32), ('gamma', ctypes.c_double),
              ('ret', ctypes.c_void_p), ('steps_flown', ctypes.c_void_p), ('leaf_status', ctypes.c_void_p), ('value', ctypes.c_void_p),
              ('score', ctypes.c_void_p)]


TREE_MAX_BEAM = 256         # BLE_TREE_MAX_BEAM


class BleTreeArena(ctypes.Structure):
  """struct ble_tree_arena: the nodes of one level of a beam search: a leaf arena's state and, per node, the rollout lane's acc and disc
  (float64), flown (int32) and ret = (float)acc (device pointers)."""
  _fields_ = [('state', ctypes.POINTER(BleStateF32)), ('acc', ctypes.c_void_p), ('disc', ctypes.c_void_p), ('flown', ctypes.c_void_p),
              ('ret', ctypes.c_void_p)]


class BleTreeExpand(ctypes.Structure):
  """struct ble_tree_expand: one level of a beam search: every selected parent's three children flown for one edge (ble_tree_expand_f32;
  ble_tree_expand_scenarios_f32 takes the same struct with arenas of n * 3 * beam * M nodes, node (e, c, m) at (e C + c) M + m)."""
  _fields_ = [('n', ctypes.c_int64), ('beam', ctypes.c_int32), ('depth', ctypes.c_int32), ('n_parents', ctypes.c_int32),
              ('parent_children', ctypes.c_int32), ('segment', ctypes.c_int32), ('action_repeat', ctypes.c_int32), ('substeps', ctypes.c_int32),
              ('reserved_', ctypes.c_int32), ('gamma', ctypes.c_double), ('wind_grid', ctypes.c_void_p), ('grid_env_stride', ctypes.c_int64),
              ('parent', ctypes.c_void_p), ('src', BleTreeArena), ('dst', BleTreeArena)]


class BleTreeSelect(ctypes.Structure):
  """struct ble_tree_select: a level's returns [n][C] -> the next level's parents and this level's choice list [n][beam]."""
  _fields_ = [('n', ctypes.c_int64), ('n_children', ctypes.c_int32), ('beam', ctypes.c_int32), ('ret', ctypes.c_void_p),
              ('parent', ctypes.c_void_p), ('choice', ctypes.c_void_p)]


class BleTreeFinish(ctypes.Structure):
  """struct ble_tree_finish: the last level's returns (and optional scores) and the choice lists -> best_plan, action, best_return and,
  on request, q and visits [n][3] (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('n_children', ctypes.c_int32), ('beam', ctypes.c_int32), ('depth', ctypes.c_int32),
              ('segment', ctypes.c_int32), ('ret', ctypes.c_void_p), ('score', ctypes.c_void_p), ('source_status', ctypes.c_void_p),
              ('choice', ctypes.c_void_p), ('best_plan', ctypes.c_void_p), ('action', ctypes.c_void_p), ('best_return', ctypes.c_void_p),
              ('q', ctypes.c_void_p), ('visits', ctypes.c_void_p)]


MCTS_MAX_LEAVES = 256       # BLE_MCTS_MAX_LEAVES
MCTS_EMPTY, MCTS_EXPAND, MCTS_REVISIT = 0, 1, 2      # BLE_MCTS_EMPTY / EXPAND / REVISIT


class BleMctsPool(ctypes.Structure):
  """struct ble_mcts_pool: the node pool of a guided tree search: cap = 1 + 3 L R ids per environment, the nodes [R][n][3L] as a
  ble_tree_arena, the statistics [n][cap], the round's slots [n][L] (device pointers).  In scenario winds (ble_mcts_expand_scenarios_f32,
  ble_mcts_backup_scenarios_f32) a node id is a group of M scenario nodes: the nodes are [R][n][3L][M], the statistics stay per group, and
  select and finish take a copy of the struct whose nodes.state->status is the groups' status [R][n][3L]."""
  _fields_ = [('n', ctypes.c_int64), ('num_rounds', ctypes.c_int32), ('leaves_per_round', ctypes.c_int32), ('max_depth', ctypes.c_int32),
              ('segment', ctypes.c_int32), ('reserved_', ctypes.c_int64), ('nodes', BleTreeArena), ('parent', ctypes.c_void_p),
              ('first_child', ctypes.c_void_p), ('depth', ctypes.c_void_p), ('visits', ctypes.c_void_p), ('pending', ctypes.c_void_p),
              ('value_sum', ctypes.c_void_p), ('g', ctypes.c_void_p), ('prior', ctypes.c_void_p), ('g_range', ctypes.c_void_p),
              ('leaf', ctypes.c_void_p), ('kind', ctypes.c_void_p)]


class BleMctsExpand(ctypes.Structure):
  """struct ble_mcts_expand: what one round's flights need beside the pool (ble_mcts_expand_f32)."""
  _fields_ = [('round', ctypes.c_int32), ('action_repeat', ctypes.c_int32), ('substeps', ctypes.c_int32), ('reserved_', ctypes.c_int32),
              ('gamma', ctypes.c_double), ('wind_grid', ctypes.c_void_p), ('grid_env_stride', ctypes.c_int64)]


class BleMctsFinish(ctypes.Structure):
  """struct ble_mcts_finish: the source's status and what ble_mcts_finish_f32 writes (device pointers)."""
  _fields_ = [('source_status', ctypes.c_void_p), ('best_plan', ctypes.c_void_p), ('action', ctypes.c_void_p), ('best_return', ctypes.c_void_p),
              ('q', ctypes.c_void_p), ('visits', ctypes.c_void_p), ('pv_length', ctypes.c_void_p)]


SCENARIO_MAX = 16           # BLE_SCENARIO_MAX


def gp_scenario_doubles(num: int) -> int:
  """BLE_GP_SCENARIO_DOUBLES(num): the window's 120 x 4 coordinates, then 120 x 2 weights per scenario."""
  return 480 + 240 * int(num)


class BleGpScenarios(ctypes.Structure):
  """struct ble_gp_scenarios: num scenario winds per environment (ble_gp_fit_scenarios_f32): the slab [n][stride] of float64 and
  n_obs [n] int32, device pointers, the number of environments and the number of scenarios."""
  _fields_ = [('slab', ctypes.c_void_p), ('stride', ctypes.c_int64), ('n_obs', ctypes.c_void_p), ('n', ctypes.c_int64),
              ('num', ctypes.c_int32), ('reserved_', ctypes.c_int32)]


class BleScenarioGen(ctypes.Structure):
  """struct ble_scenario_gen: where the scenario streams come from: the batch's seed and env_offset, or a device seed per environment;
  the device episode counters."""
  _fields_ = [('seed', ctypes.c_uint64), ('env_seed', ctypes.c_void_p), ('episode', ctypes.c_void_p), ('env_offset', ctypes.c_int64)]


class BlePlanRisk(ctypes.Structure):
  """struct ble_plan_risk: ret [n][K][M] -> score [n][K], the mean of the `tail` smallest scenario returns (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('n_plans', ctypes.c_int32), ('num', ctypes.c_int32), ('tail', ctypes.c_int32),
              ('reserved_', ctypes.c_int32), ('ret', ctypes.c_void_p), ('score', ctypes.c_void_p)]


class BleNoiseGen(ctypes.Structure):
  """struct ble_noise_gen: the wind-noise generator of a fused rollout (ble_step_n_f32, ABI 3)."""
  _fields_ = [('seed', ctypes.c_uint64), ('episode', ctypes.c_void_p), ('harmonic_cache', ctypes.c_void_p),
              ('env_offset', ctypes.c_int64)]       # (ABI 4: the shard's first environment in the global batch; default 0)


class BleEvalAcc(ctypes.Structure):
  """struct ble_eval_acc: the per-environment accumulators of an evaluation (ble_eval_accumulate_f32), device pointers."""
  _fields_ = [('cumulative_reward', ctypes.c_void_p), ('steps_within_radius', ctypes.c_void_p), ('final_timestep', ctypes.c_void_p),
              ('done', ctypes.c_void_p), ('end_status', ctypes.c_void_p)]


FLEET_MAX_VEHICLES = 16      # BLE_FLEET_MAX_VEHICLES


class BleFleet(ctypes.Structure):
  """struct ble_fleet: a palette of up to FLEET_MAX_VEHICLES vehicles (a HOST array of BleVehicle, read when a call is made) and the
  DEVICE uint8 index of the entry each environment flies; sample_index makes ble_reset_fleet_at_f32 draw the index per episode."""
  _fields_ = [('palette', ctypes.POINTER(BleVehicle)), ('n_vehicles', ctypes.c_int32), ('sample_index', ctypes.c_int32),
              ('vehicle_index', ctypes.c_void_p)]


def vehicle_full(**overrides) -> 'BleVehicle':
  """A BleVehicle with the reference's defaults and the given fields replaced -- always a struct (a fleet's palette entry), unlike
  vehicle_struct."""
  return vehicle_struct(**overrides) or BleVehicle(reserved_=0, **VEHICLE_DEFAULTS)


def fleet_struct(vehicles, index_ptr: int, sample_index: bool = False) -> BleFleet:
  """A BleFleet over the vehicles (override dicts in set_vehicle's form); the struct keeps its palette array alive."""
  n = len(vehicles)
  palette = (BleVehicle * max(n, 1))(*[vehicle_full(**v) for v in vehicles])
  f = BleFleet(ctypes.cast(palette, ctypes.POINTER(BleVehicle)), n, 1 if sample_index else 0, int(index_ptr) or None)
  f._palette_keepalive = palette
  return f


class BleQnetF32(ctypes.Structure):
  """struct ble_qnet_f32: the shape of a QuantileNetwork / MLPNetwork and the DEVICE pointer to its packed weights
  (ble_qnet_pack_f32's image)."""
  _fields_ = [('num_layers', ctypes.c_int32), ('input_dim', ctypes.c_int32), ('hidden_units', ctypes.c_int32),
              ('num_actions', ctypes.c_int32), ('num_atoms', ctypes.c_int32), ('reserved_', ctypes.c_int32),
              ('weights', ctypes.c_void_p)]


class BleReplayF32(ctypes.Structure):
  """struct ble_replay_f32: the per-environment n-step replay ring (device pointers) and its sizes."""
  _fields_ = [('capacity', ctypes.c_int64), ('num_envs', ctypes.c_int64), ('update_horizon', ctypes.c_int32),
              ('obs_stride', ctypes.c_int32), ('gamma', ctypes.c_double), ('max_tries', ctypes.c_int32),
              ('reserved_', ctypes.c_int32),
              ('obs', ctypes.c_void_p), ('action', ctypes.c_void_p), ('reward', ctypes.c_void_p), ('terminal', ctypes.c_void_p),
              ('episode_end', ctypes.c_void_p), ('count', ctypes.c_void_p), ('counter', ctypes.c_void_p)]


class BleTrainBatchF32(ctypes.Structure):
  """struct ble_train_batch_f32: one batch of B transitions (device pointers)."""
  _fields_ = [('batch', ctypes.c_int64), ('state_stride', ctypes.c_int64), ('state', ctypes.c_void_p), ('next_state', ctypes.c_void_p),
              ('ret', ctypes.c_void_p), ('discount', ctypes.c_void_p), ('action', ctypes.c_void_p), ('index', ctypes.c_void_p)]


class BleQnetTrainF32(ctypes.Structure):
  """struct ble_qnet_train_f32: the trainer's device buffers and Adam's hyperparameters."""
  _fields_ = [('net', BleQnetF32), ('target', ctypes.c_void_p), ('weights_t', ctypes.c_void_p), ('grad', ctypes.c_void_p),
              ('adam_m', ctypes.c_void_p), ('adam_v', ctypes.c_void_p), ('adam_step', ctypes.c_void_p), ('workspace', ctypes.c_void_p),
              ('adam_b1', ctypes.c_double), ('adam_b2', ctypes.c_double), ('lr', ctypes.c_float), ('adam_eps', ctypes.c_float),
              ('kappa', ctypes.c_float), ('apply_update', ctypes.c_int32)]


class BleQnetTrainLayout(ctypes.Structure):
  """struct ble_qnet_train_layout: offsets, in floats, into the trainer's workspace."""
  _fields_ = [(name, ctypes.c_int64) for name in ('ld', 'acts', 'target_logits', 'targets', 'dlogits', 'scratch', 'partial', 'slabs',
                                                  'corrections', 'total', 'transposed_floats')]


TD_DQN_MSE, TD_DQN_HUBER, TD_SARSA_MSE = 0, 1, 2     # BLE_TD_*
TD_OPT_ADAM, TD_OPT_SGD = 0, 1                        # BLE_TD_OPT_*


class BleTdF32(ctypes.Structure):
  """struct ble_td_f32: the loss kind and optimiser of ble_qnet_td_step_f32, SARSA's gamma and device pointers."""
  _fields_ = [('kind', ctypes.c_int32), ('optimizer', ctypes.c_int32), ('gamma', ctypes.c_float), ('reserved_', ctypes.c_int32),
              ('next_action', ctypes.c_void_p), ('mask', ctypes.c_void_p)]


class BleExploreF32(ctypes.Structure):
  """struct ble_explore_f32: epsilon-greedy over n actions, keyed by (seed, env, step)."""
  _fields_ = [('n', ctypes.c_int64), ('epsilon', ctypes.c_float), ('reserved_', ctypes.c_int32), ('seed', ctypes.c_uint64),
              ('step', ctypes.c_uint64)]


class BleSumTreeF64(ctypes.Structure):
  """struct ble_sum_tree_f64: the prioritized replay's fp64 sum tree (device pointers) and its sizes."""
  _fields_ = [('leaves', ctypes.c_int64), ('padded', ctypes.c_int64), ('nodes', ctypes.c_void_p), ('max_priority', ctypes.c_void_p)]


class BleMarcoPoloF32(ctypes.Structure):
  """struct ble_marco_polo_f32: Marco Polo exploration over n environments (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('obs_stride', ctypes.c_int32), ('reserved_', ctypes.c_int32),
              ('exploratory_episode_probability', ctypes.c_double), ('seed', ctypes.c_uint64), ('obs', ctypes.c_void_p),
              ('begin', ctypes.c_void_p), ('step', ctypes.c_void_p), ('phase_clock', ctypes.c_void_p), ('walk_clock', ctypes.c_void_p),
              ('exploratory_episode', ctypes.c_void_p), ('exploratory_phase', ctypes.c_void_p), ('target', ctypes.c_void_p)]


class BleAcRowsF32(ctypes.Structure):
  """struct ble_ac_rows_f32: n observation rows and what ble_ac_act_f32 writes for each (device pointers)."""
  _fields_ = [('n', ctypes.c_int64), ('obs_row_stride', ctypes.c_int64), ('obs', ctypes.c_void_p), ('action', ctypes.c_void_p),
              ('logp', ctypes.c_void_p), ('value', ctypes.c_void_p), ('probs', ctypes.c_void_p)]


class BleAcSample(ctypes.Structure):
  """struct ble_ac_sample: the sampled head's stream, keyed by (seed, env_offset + row, *step); step is a device pointer."""
  _fields_ = [('seed', ctypes.c_uint64), ('env_offset', ctypes.c_int64), ('step', ctypes.c_void_p), ('reserved_', ctypes.c_int64)]


class BleGaeBlockF32(ctypes.Structure):
  """struct ble_gae_block_f32: a rollout block of T steps of N environments, arrays [T][N] (device pointers)."""
  _fields_ = [('steps', ctypes.c_int64), ('num_envs', ctypes.c_int64), ('gamma', ctypes.c_float), ('lam', ctypes.c_float),
              ('reward', ctypes.c_void_p), ('value', ctypes.c_void_p), ('boot_value', ctypes.c_void_p), ('terminal', ctypes.c_void_p),
              ('episode_end', ctypes.c_void_p), ('advantage', ctypes.c_void_p), ('ret', ctypes.c_void_p)]


class BlePpoF32(ctypes.Structure):
  """struct ble_ppo_f32: the clipped-PPO loss's coefficients and the batch rows' old log-probabilities and advantages (device)."""
  _fields_ = [('clip', ctypes.c_float), ('value_coef', ctypes.c_float), ('entropy_coef', ctypes.c_float), ('reserved_', ctypes.c_int32),
              ('old_logp', ctypes.c_void_p), ('advantage', ctypes.c_void_p)]


class BleBcF32(ctypes.Structure):
  """struct ble_bc_f32: the cloning loss's label smoothing and value coefficient."""
  _fields_ = [('label_smoothing', ctypes.c_float), ('value_coef', ctypes.c_float), ('reserved_', ctypes.c_int64)]


class BleSoftBcF32(ctypes.Structure):
  """struct ble_soft_bc_f32: the soft cloning loss's inverse temperature, label smoothing and value coefficient, and the rows'
  per-action values target_q [B][3] (device)."""
  _fields_ = [('inv_temperature', ctypes.c_float), ('label_smoothing', ctypes.c_float), ('value_coef', ctypes.c_float),
              ('reserved_', ctypes.c_int32), ('target_q', ctypes.c_void_p)]


class BleDaggerMixF32(ctypes.Structure):
  """struct ble_dagger_mix_f32: the DAgger mixture of n learner and expert actions, keyed by (seed, env_offset + row, *step); step,
  learner, expert, action and took_expert are device pointers."""
  _fields_ = [('n', ctypes.c_int64), ('beta', ctypes.c_float), ('reserved_', ctypes.c_int32), ('seed', ctypes.c_uint64),
              ('env_offset', ctypes.c_int64), ('step', ctypes.c_void_p), ('learner', ctypes.c_void_p), ('expert', ctypes.c_void_p),
              ('action', ctypes.c_void_p), ('took_expert', ctypes.c_void_p)]


POP_HEAD_Q, POP_HEAD_ACTOR_GREEDY = 0, 1             # BLE_POP_HEAD_*


class BleQnetGroupedF32(ctypes.Structure):
  """struct ble_qnet_grouped_f32: P networks of one shape over P * R rows, rows [p R, (p + 1) R) through image p (device pointers)."""
  _fields_ = [('net', BleQnetF32), ('members', ctypes.c_int32), ('head', ctypes.c_int32), ('member_stride', ctypes.c_int64),
              ('rows_per_member', ctypes.c_int64), ('obs_row_stride', ctypes.c_int64), ('obs', ctypes.c_void_p),
              ('scratch', ctypes.c_void_p), ('action', ctypes.c_void_p), ('q_values', ctypes.c_void_p), ('value', ctypes.c_void_p),
              ('probs', ctypes.c_void_p)]


class BleEsF32(ctypes.Structure):
  """struct ble_es_f32: an evolution strategy's centre image (net.weights), its population of images, sigma, weight decay, the seed and
  the device generation counter."""
  _fields_ = [('net', BleQnetF32), ('members', ctypes.c_int32), ('antithetic', ctypes.c_int32), ('member_stride', ctypes.c_int64),
              ('population', ctypes.c_void_p), ('sigma', ctypes.c_float), ('weight_decay', ctypes.c_float), ('seed', ctypes.c_uint64),
              ('generation', ctypes.c_void_p)]


class BlePpoGroupedF32(ctypes.Structure):
  """struct ble_ppo_grouped_f32: a grouped PPO update of P networks of one shape on P * B rows: member 0's buffers and the strides
  between members, the per-member hyperparameters [P] and the rows' old log-probabilities and advantages [P * B] (device pointers)."""
  _fields_ = [('tr', BleQnetTrainF32), ('members', ctypes.c_int32), ('reserved_', ctypes.c_int32), ('member_stride', ctypes.c_int64),
              ('transposed_stride', ctypes.c_int64), ('rows_per_member', ctypes.c_int64), ('lr', ctypes.c_void_p),
              ('clip', ctypes.c_void_p), ('value_coef', ctypes.c_void_p), ('entropy_coef', ctypes.c_void_p), ('old_logp', ctypes.c_void_p),
              ('advantage', ctypes.c_void_p)]


TD_GROUPED_QUANTILE = 0                              # BLE_TD_GROUPED_QUANTILE; the DQN kinds are TD_DQN_* + 1


class BleTdGroupedF32(ctypes.Structure):
  """struct ble_td_grouped_f32: a grouped QR-DQN / DQN update of P networks of one shape on P * B rows: member 0's buffers (the target
  image among them) and the strides between members, the loss kind and the per-member learning rates and Huber thresholds [P] (device
  pointers)."""
  _fields_ = [('tr', BleQnetTrainF32), ('members', ctypes.c_int32), ('reserved_', ctypes.c_int32), ('member_stride', ctypes.c_int64),
              ('transposed_stride', ctypes.c_int64), ('rows_per_member', ctypes.c_int64), ('kind', ctypes.c_int32),
              ('reserved2_', ctypes.c_int32), ('lr', ctypes.c_void_p), ('kappa', ctypes.c_void_p)]


class BleExploreGroupedF32(ctypes.Structure):
  """struct ble_explore_grouped_f32: epsilon-greedy over n = P * R actions, row p R + r keyed by (seed[p], r, step) at epsilon[p];
  epsilon (float32 [P]) and seed (uint64 [P]) are device pointers."""
  _fields_ = [('n', ctypes.c_int64), ('members', ctypes.c_int32), ('reserved_', ctypes.c_int32), ('epsilon', ctypes.c_void_p),
              ('seed', ctypes.c_void_p), ('step', ctypes.c_uint64)]


class BleSumTreeGroupedF64(ctypes.Structure):
  """struct ble_sum_tree_grouped_f64: P solo sum-tree images over one population ring; leaves and padded are per member, member_stride
  the doubles between trees; nodes [P][member_stride] and max_priority [P] are device pointers."""
  _fields_ = [('members', ctypes.c_int64), ('leaves', ctypes.c_int64), ('padded', ctypes.c_int64), ('member_stride', ctypes.c_int64),
              ('nodes', ctypes.c_void_p), ('max_priority', ctypes.c_void_p)]


class BleMarcoPoloGroupedF32(ctypes.Structure):
  """struct ble_marco_polo_grouped_f32: Marco Polo exploration over n = P * R lanes, lane p R + r keyed by (seed[p], r, *step) at
  probability[p]; probability (float64 [P]) and seed (uint64 [P]) are device pointers."""
  _fields_ = [('n', ctypes.c_int64), ('obs_stride', ctypes.c_int32), ('reserved_', ctypes.c_int32), ('members', ctypes.c_int64),
              ('probability', ctypes.c_void_p), ('seed', ctypes.c_void_p), ('obs', ctypes.c_void_p), ('begin', ctypes.c_void_p),
              ('step', ctypes.c_void_p), ('phase_clock', ctypes.c_void_p), ('walk_clock', ctypes.c_void_p),
              ('exploratory_episode', ctypes.c_void_p), ('exploratory_phase', ctypes.c_void_p), ('target', ctypes.c_void_p)]
