"""Loader for libble_hip.so (the C ABI in include/ble_abi.h).

The HIP library is the ONLY compute path of this package.  If it is missing or cannot
be loaded the import of anything that needs it raises -- there is no CPU fallback.
"""
import ctypes
import os
import subprocess

# One HIP runtime per process: torch ships its own libamdhip64 (SONAME libamdhip64.so.7, found
# through torch/lib's RPATH).  Importing torch first makes libble_hip.so's NEEDED
# libamdhip64.so.7 resolve to that already-loaded runtime, so torch's device pointers and
# hipStream_t handles are valid in our launches.  Loaded the other way round the process gets
# two runtimes and launches fail with hipErrorNoDevice (100).
import torch  # noqa: F401  (must precede ctypes.CDLL(LIB_PATH))

from balloon_learning_environment_amd import _abi

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('BLE_HIP_LIB') or os.path.join(_PKG_DIR, 'libble_hip.so')   # override: experiments only
_SOURCES = [os.path.join(_PKG_DIR, 'csrc', f) for f in ('ble_kernels.hip', 'ble_step_core.h', 'ble_physics.h', 'ble_intrinsics.h', 'ble_reset.h',
                                                          'ble_observe.h', 'ble_gp_query.h', 'ble_gp_factor.h', 'ble_lookahead.h', 'ble_rollout.h', 'ble_gp_belief.h', 'ble_plan.h', 'ble_tree.h', 'ble_scenarios.h', 'ble_tree_scenarios.h', 'ble_mcts.h', 'ble_mcts_scenarios.h', 'ble_noise.h', 'ble_decode.h', 'ble_step_split.h', 'ble_step_helper.h', 'ble_agent.h', 'ble_qnet.h',
                                                          'ble_train.h', 'ble_replay.h', 'ble_explore.h', 'ble_actor.h', 'ble_imitate.h', 'ble_population.h',
                                                          'ble_population_train.h', 'ble_population_td.h', 'ble_population_prio.h')]
_HEADER = os.path.join(os.path.dirname(_PKG_DIR), 'include', 'ble_abi.h')

ABI_VERSION = 5
NOISE_PRIMITIVE_VERSION = 2     # BLE_NOISE_PRIMITIVE_VERSION this mirror, oracle/noise_oracle.py and tests/golden/f14 were made with
BLE_OK = 0
FLAG_PRESSURE_RANGE, FLAG_ABSORPTIVITY, FLAG_SOLAR_RANGE, FLAG_POWER_TABLE, FLAG_NONFINITE = 1, 2, 4, 16, 32
FLAG_GP_WINDOW, FLAG_PRESSURE_SEARCH, FLAG_DAY_CYCLE = 64, 128, 256
FLAG_VEHICLE_INDEX = 512
FLAG_AGENT_NO_LEVEL = 1024
FLAG_REPLAY_EMPTY, FLAG_TRAIN_ACTION = 2048, 4096
FLAG_REPLAY_PRIORITY = 8192
SEEKER_LEVELS = 361
OBS_DIM, GP_CAPACITY, GP_CHOL_STRIDE = 1099, 128, 7620
GP_BELIEF_DOUBLES = _abi.GP_BELIEF_DOUBLES
ROW_DOUBLES = 26        # BLE_ROW_DOUBLES
NOISE_CACHE_ROWS = 53

# every symbol include/ble_abi.h declares
EXPORTS = ('ble_abi_version', 'ble_noise_primitive_version', 'ble_vehicle_default', 'ble_last_hip_error', 'ble_device_count', 'ble_set_step_form', 'ble_last_step_form', 'ble_step_f32', 'ble_step_n_f32', 'ble_reset_f32', 'ble_reset_at_f32', 'ble_wind_noise_at_f32', 'ble_observe_f32', 'ble_observe_forecast_f32', 'ble_decode_flow_fields_f32', 'ble_wind_noise_f32', 'ble_forecast_f32',
           'ble_forecast_column_f32', 'ble_state_rows_f64', 'ble_power_table_f32', 'ble_probe_atmosphere_f32', 'ble_probe_atmosphere_at_height_f64', 'ble_probe_solar_f32', 'ble_probe_latlng_f64',
           'ble_probe_solar_power_f32', 'ble_probe_thermal_f32', 'ble_probe_sp_volume_f32', 'ble_probe_thermal_vehicle_f32', 'ble_probe_sp_volume_vehicle_f32', 'ble_probe_acs_f32', 'ble_probe_safety_f32',
           'ble_probe_f64_prims', 'ble_step_fleet_f32', 'ble_step_n_fleet_f32', 'ble_reset_fleet_at_f32', 'ble_observe_forecast_fleet_f32',
           'ble_station_seeker_f32', 'ble_eval_accumulate_f32', 'ble_reset_seeded_f32', 'ble_wind_noise_seeded_f32',
           'ble_observe_live_f32', 'ble_qnet_workspace_f32', 'ble_qnet_pack_f32', 'ble_qnet_forward_f32',
           'ble_qnet_unpack_f32', 'ble_replay_sample_f32', 'ble_qnet_train_workspace_f32', 'ble_qnet_transpose_f32',
           'ble_qnet_train_step_f32', 'ble_qnet_explore_u8', 'ble_qnet_td_workspace_f32', 'ble_qnet_td_step_f32',
           'ble_replay_tree_add_f64', 'ble_replay_sample_prioritized_f32', 'ble_replay_set_priority_f32', 'ble_marco_polo_u8', 'ble_gp_query_f32', 'ble_rollout_f32',
           'ble_gp_fit_f32', 'ble_gp_belief_wind_f32', 'ble_rollout_belief_f32', 'ble_plan_sample_u8', 'ble_plan_select_f32',
           'ble_gp_fit_scenarios_f32', 'ble_gp_scenario_wind_f32', 'ble_rollout_scenarios_f32', 'ble_plan_risk_f32',
           'ble_ac_act_f32', 'ble_gae_f32', 'ble_adv_normalize_f32', 'ble_qnet_ppo_step_f32', 'ble_qnet_bc_step_f32', 'ble_dagger_mix_u8',
           'ble_plan_prior_u16', 'ble_plan_sample_prior_u8', 'ble_plan_action_values_f32', 'ble_qnet_soft_bc_step_f32',
           'ble_rollout_leaves_f32', 'ble_observe_leaves_f32', 'ble_plan_bootstrap_f32',
           'ble_qnet_forward_grouped_f32', 'ble_es_perturb_f32', 'ble_es_gradient_f32', 'ble_qnet_apply_grad_f32',
           'ble_qnet_ppo_grouped_workspace_f32', 'ble_qnet_ppo_step_grouped_f32', 'ble_ac_act_grouped_f32',
           'ble_tree_expand_f32', 'ble_tree_select_f32', 'ble_tree_finish_f32',
           'ble_qnet_td_grouped_workspace_f32', 'ble_qnet_td_step_grouped_f32', 'ble_replay_sample_grouped_f32',
           'ble_qnet_explore_grouped_u8', 'ble_tree_expand_scenarios_f32',
           'ble_mcts_select_f32', 'ble_mcts_expand_f32', 'ble_mcts_backup_f32', 'ble_mcts_finish_f32',
           'ble_mcts_expand_scenarios_f32', 'ble_mcts_backup_scenarios_f32',
           'ble_replay_tree_add_grouped_f64', 'ble_replay_sample_prioritized_grouped_f32', 'ble_replay_set_priority_grouped_f32',
           'ble_marco_polo_grouped_u8')
# Exports added without a new ABI version: a library of this ABI built before them (BLE_HIP_LIB: the parent's, in A/B runs) still loads.
# build() checks every name of EXPORTS on the library it builds.
ADDITIVE_EXPORTS = ('ble_last_step_form', 'ble_gp_query_f32', 'ble_rollout_f32', 'ble_gp_fit_f32', 'ble_gp_belief_wind_f32',
                    'ble_rollout_belief_f32', 'ble_plan_sample_u8', 'ble_plan_select_f32', 'ble_gp_fit_scenarios_f32',
                    'ble_gp_scenario_wind_f32', 'ble_rollout_scenarios_f32', 'ble_plan_risk_f32', 'ble_ac_act_f32', 'ble_gae_f32',
                    'ble_adv_normalize_f32', 'ble_qnet_ppo_step_f32', 'ble_qnet_bc_step_f32', 'ble_dagger_mix_u8', 'ble_plan_prior_u16',
                    'ble_plan_sample_prior_u8', 'ble_plan_action_values_f32', 'ble_qnet_soft_bc_step_f32', 'ble_rollout_leaves_f32',
                    'ble_observe_leaves_f32', 'ble_plan_bootstrap_f32', 'ble_qnet_forward_grouped_f32', 'ble_es_perturb_f32',
                    'ble_es_gradient_f32', 'ble_qnet_apply_grad_f32', 'ble_qnet_ppo_grouped_workspace_f32',
                    'ble_qnet_ppo_step_grouped_f32', 'ble_ac_act_grouped_f32', 'ble_tree_expand_f32', 'ble_tree_select_f32',
                    'ble_tree_finish_f32', 'ble_qnet_td_grouped_workspace_f32', 'ble_qnet_td_step_grouped_f32',
                    'ble_replay_sample_grouped_f32', 'ble_qnet_explore_grouped_u8', 'ble_tree_expand_scenarios_f32',
                    'ble_mcts_select_f32', 'ble_mcts_expand_f32', 'ble_mcts_backup_f32', 'ble_mcts_finish_f32',
                    'ble_mcts_expand_scenarios_f32', 'ble_mcts_backup_scenarios_f32', 'ble_replay_tree_add_grouped_f64',
                    'ble_replay_sample_prioritized_grouped_f32', 'ble_replay_set_priority_grouped_f32', 'ble_marco_polo_grouped_u8')


class BleLibraryError(RuntimeError):
  pass


def build(force: bool = False, verbose: bool = False) -> str:
  """Compiles csrc/ble_kernels.hip for gfx950 into libble_hip.so (in-tree)."""
  deps = _SOURCES + [_HEADER]
  stale = (not os.path.exists(LIB_PATH) or
           any(os.path.exists(d) and os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in deps))
  if force or stale:
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
      hipcc = 'hipcc'
    # -ffp-contract=on: a * b + c fuses where the SOURCE writes it in one expression and nowhere else.  hipcc's default
    # ("fast") also fuses across statements wherever the optimiser happens to see a product next to a sum, which depends on the
    # code around it (inlining, vectorisation): the same lane function then rounds differently in two kernels.  The transition
    # exists in three kernels that must agree bit for bit (one lane per environment, four waves per environment, noise
    # generated in-kernel); measured neutral on both hot kernels (profiles/r04_notes.md).
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=on', '-fPIC', '-shared', '-I', os.path.join(_PKG_DIR, 'csrc'),
           '-o', LIB_PATH, _SOURCES[0]]
    if verbose:
      cmd.insert(1, '-Rpass-analysis=kernel-resource-usage')
    subprocess.check_call(cmd)
  return LIB_PATH


_lib = None
_vp, _i64, _int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


class _I64(ctypes.c_int64):
  """int64_t, as an argument type of its own (ble_observe_leaves_f32 below)."""


def lib():
  """Returns the loaded library; raises BleLibraryError if it is not there."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise BleLibraryError(
        f'{LIB_PATH} not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` '
        '(hipcc --offload-arch=gfx950). This package has no CPU fallback.')
  try:
    l = ctypes.CDLL(LIB_PATH)
  except OSError as e:  # e.g. libamdhip64 missing
    raise BleLibraryError(f'cannot load {LIB_PATH}: {e}') from e
  for name in EXPORTS:
    if not hasattr(l, name) and name not in ADDITIVE_EXPORTS:
      raise BleLibraryError(f'{LIB_PATH} does not export {name}')
  if l.ble_abi_version() != ABI_VERSION:
    raise BleLibraryError('ABI version mismatch between libble_hip.so and the Python mirror')
  if l.ble_noise_primitive_version() != NOISE_PRIMITIVE_VERSION:
    raise BleLibraryError(f'libble_hip.so evaluates wind-noise primitive version {l.ble_noise_primitive_version()}, this package (its oracle and '
                          f'fixtures) was made with {NOISE_PRIMITIVE_VERSION}: recorded noise seeds would fly another wind')
  st = ctypes.POINTER(_abi.BleStateF32)
  l.ble_step_f32.argtypes = [st, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _int, _vp]
  l.ble_step_n_f32.argtypes = [st, _vp, _vp, _i64, ctypes.POINTER(_abi.BleNoiseGen), _vp, _vp, _vp, _vp, _i64, _int, _int, _vp]
  l.ble_reset_f32.argtypes = [st, _vp, ctypes.c_uint64, _vp, _int, _vp, _i64, _vp]
  l.ble_reset_at_f32.argtypes = [st, _vp, ctypes.c_uint64, _vp, _int, _vp, _i64, _i64, _vp]
  l.ble_observe_f32.argtypes = [st, _vp, _i64, _vp, _vp, ctypes.POINTER(_abi.BleGpHistoryF32), _int, _vp, _vp, _i64, _vp]
  l.ble_observe_forecast_f32.argtypes = [st, _vp, _i64, _vp, _vp, _vp, ctypes.POINTER(_abi.BleGpHistoryF32), _int, _vp, _vp, _i64, _vp]
  l.ble_decode_flow_fields_f32.argtypes = [_vp, _vp, _i64, _vp]
  l.ble_wind_noise_f32.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _int, _vp, _vp, _i64, _vp]
  l.ble_wind_noise_at_f32.argtypes = [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _int, _vp, _vp, _i64, _i64, _vp]
  l.ble_forecast_f32.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
  l.ble_forecast_column_f32.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _int, _vp, _i64, _vp]
  l.ble_power_table_f32.argtypes = [_vp, _vp, _vp, _vp, _i64, _vp]
  l.ble_state_rows_f64.argtypes = [st, _i64, _i64, _vp, _i64, _vp]
  l.ble_probe_atmosphere_f32.argtypes = [_vp, _vp, _vp, _vp, _vp, _i64, _vp]
  l.ble_probe_atmosphere_at_height_f64.argtypes = [_vp, _vp, _vp, _vp, _vp, _i64, _vp]
  l.ble_probe_solar_f32.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
  l.ble_probe_latlng_f64.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]
  l.ble_probe_solar_power_f32.argtypes = [_vp, _vp, _vp, _vp, _i64, _vp]
  l.ble_probe_thermal_f32.argtypes = [_vp] * 9 + [_i64, _vp]
  l.ble_probe_sp_volume_f32.argtypes = [_vp] * 5 + [_i64, _vp]
  l.ble_probe_thermal_vehicle_f32.argtypes = [ctypes.POINTER(_abi.BleVehicle)] + [_vp] * 9 + [_i64, _vp]
  l.ble_probe_sp_volume_vehicle_f32.argtypes = [ctypes.POINTER(_abi.BleVehicle)] + [_vp] * 5 + [_i64, _vp]
  l.ble_probe_acs_f32.argtypes = [_vp] * 4 + [_i64, _vp]
  l.ble_probe_safety_f32.argtypes = [_int, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp, _i64, _vp]
  l.ble_probe_f64_prims.argtypes = [_vp, _vp, _int, _i64, _vp]
  l.ble_set_step_form.argtypes = [_int]
  if hasattr(l, 'ble_last_step_form'):
    l.ble_last_step_form.argtypes = []
  l.ble_vehicle_default.argtypes = [ctypes.POINTER(_abi.BleVehicle)]
  fleet = ctypes.POINTER(_abi.BleFleet)
  l.ble_step_fleet_f32.argtypes = [st, fleet] + l.ble_step_f32.argtypes[1:]
  l.ble_step_n_fleet_f32.argtypes = [st, fleet] + l.ble_step_n_f32.argtypes[1:]
  l.ble_reset_fleet_at_f32.argtypes = [st, fleet] + l.ble_reset_at_f32.argtypes[1:]
  l.ble_observe_forecast_fleet_f32.argtypes = [st, fleet] + l.ble_observe_forecast_f32.argtypes[1:]
  l.ble_observe_live_f32.argtypes = list(l.ble_observe_f32.argtypes)
  l.ble_station_seeker_f32.argtypes = [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]
  l.ble_eval_accumulate_f32.argtypes = [st, _vp, ctypes.POINTER(_abi.BleEvalAcc), ctypes.c_double, _int, _int, _vp, _i64, _vp]
  l.ble_reset_seeded_f32.argtypes = [st, _vp, _vp, _vp, _int, _vp, _i64, _vp]
  l.ble_wind_noise_seeded_f32.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _i64, _vp]
  qnet = ctypes.POINTER(_abi.BleQnetF32)
  l.ble_qnet_workspace_f32.argtypes = [qnet, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64)]
  l.ble_qnet_pack_f32.argtypes = [qnet, ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp]
  l.ble_qnet_forward_f32.argtypes = [qnet, _vp, _i64, _vp, _vp, _vp, _i64, _vp]
  # training: every size travels in a descriptor (no int64_t argument)
  batch = ctypes.POINTER(_abi.BleTrainBatchF32)
  train = ctypes.POINTER(_abi.BleQnetTrainF32)
  l.ble_qnet_unpack_f32.argtypes = [qnet, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]
  l.ble_replay_sample_f32.argtypes = [ctypes.POINTER(_abi.BleReplayF32), batch, ctypes.c_uint64, _vp, _vp]
  l.ble_qnet_train_workspace_f32.argtypes = [train, batch, ctypes.POINTER(_abi.BleQnetTrainLayout)]
  l.ble_qnet_transpose_f32.argtypes = [qnet, _vp, _vp]
  l.ble_qnet_train_step_f32.argtypes = [train, batch, _vp, _vp, _vp]
  l.ble_qnet_explore_u8.argtypes = [ctypes.POINTER(_abi.BleExploreF32), _vp, _vp]
  td = ctypes.POINTER(_abi.BleTdF32)
  l.ble_qnet_td_workspace_f32.argtypes = [train, td, batch, ctypes.POINTER(_abi.BleQnetTrainLayout)]
  l.ble_qnet_td_step_f32.argtypes = [train, td, batch, _vp, _vp, _vp]
  # prioritized replay and Marco Polo exploration (sizes in descriptors, as above)
  replay, tree = ctypes.POINTER(_abi.BleReplayF32), ctypes.POINTER(_abi.BleSumTreeF64)
  l.ble_replay_tree_add_f64.argtypes = [replay, tree, _vp]
  l.ble_replay_sample_prioritized_f32.argtypes = [replay, tree, batch, _vp, ctypes.c_uint64, _vp, _vp]
  l.ble_replay_set_priority_f32.argtypes = [replay, tree, batch, _vp, _vp, _vp, _vp, _vp]
  l.ble_marco_polo_u8.argtypes = [ctypes.POINTER(_abi.BleMarcoPoloF32), _vp, _vp]
  if hasattr(l, 'ble_gp_query_f32'):
    l.ble_gp_query_f32.argtypes = [ctypes.POINTER(_abi.BleGpHistoryF32), _vp, ctypes.POINTER(_abi.BleGpQueryF32), _vp, _vp]
  if hasattr(l, 'ble_rollout_f32'):      # (its sizes travel in the struct: no int64_t argument)
    l.ble_rollout_f32.argtypes = [st, ctypes.POINTER(_abi.BleRolloutF32), ctypes.POINTER(_abi.BleNoiseGen), _vp, _vp]
  if hasattr(l, 'ble_gp_fit_f32'):       # the belief: a WindGP fitted once and kept on the device
    belief = ctypes.POINTER(_abi.BleGpBelief)
    l.ble_gp_fit_f32.argtypes = [ctypes.POINTER(_abi.BleGpHistoryF32), _vp, _vp, belief, _vp, _vp]      # (no int64_t argument: n is the belief's)
    l.ble_gp_belief_wind_f32.argtypes = [belief, _vp, _vp, _vp, _vp, _vp, _vp]
    l.ble_rollout_belief_f32.argtypes = [st, ctypes.POINTER(_abi.BleRolloutF32), belief, _vp, _vp]
  if hasattr(l, 'ble_plan_sample_u8'):   # the planner's two ends (sizes in the structs: no int64_t argument)
    l.ble_plan_sample_u8.argtypes = [ctypes.POINTER(_abi.BlePlanSample), _vp]
    l.ble_plan_select_f32.argtypes = [ctypes.POINTER(_abi.BlePlanSelect), _vp]
  if hasattr(l, 'ble_gp_fit_scenarios_f32'):      # scenario winds (sizes in the structs: no int64_t argument)
    scn, sgen = ctypes.POINTER(_abi.BleGpScenarios), ctypes.POINTER(_abi.BleScenarioGen)
    l.ble_gp_fit_scenarios_f32.argtypes = [ctypes.POINTER(_abi.BleGpHistoryF32), _vp, _vp, scn, sgen, _vp, _vp]
    l.ble_gp_scenario_wind_f32.argtypes = [scn, sgen, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp]
    l.ble_rollout_scenarios_f32.argtypes = [st, ctypes.POINTER(_abi.BleRolloutF32), scn, sgen, _vp, _vp]
    l.ble_plan_risk_f32.argtypes = [ctypes.POINTER(_abi.BlePlanRisk), _vp]
  if hasattr(l, 'ble_ac_act_f32'):       # on-policy training (sizes in the structs: no int64_t argument)
    gae = ctypes.POINTER(_abi.BleGaeBlockF32)
    l.ble_ac_act_f32.argtypes = [qnet, ctypes.POINTER(_abi.BleAcRowsF32), _vp, ctypes.POINTER(_abi.BleAcSample), _vp]
    l.ble_gae_f32.argtypes = [gae, _vp]
    l.ble_adv_normalize_f32.argtypes = [gae, _vp]
    l.ble_qnet_ppo_step_f32.argtypes = [train, ctypes.POINTER(_abi.BlePpoF32), batch, _vp, _vp, _vp]
  if hasattr(l, 'ble_qnet_bc_step_f32'):      # imitation (sizes in the structs: no int64_t argument)
    l.ble_qnet_bc_step_f32.argtypes = [train, ctypes.POINTER(_abi.BleBcF32), batch, _vp, _vp, _vp]
    l.ble_dagger_mix_u8.argtypes = [ctypes.POINTER(_abi.BleDaggerMixF32), _vp]
  if hasattr(l, 'ble_plan_prior_u16'):        # expert iteration (sizes in the structs: no int64_t argument)
    l.ble_plan_prior_u16.argtypes = [ctypes.POINTER(_abi.BlePlanPrior), _vp]
    l.ble_plan_sample_prior_u8.argtypes = [ctypes.POINTER(_abi.BlePlanSamplePrior), _vp]
    l.ble_plan_action_values_f32.argtypes = [ctypes.POINTER(_abi.BlePlanActionValues), _vp]
    l.ble_qnet_soft_bc_step_f32.argtypes = [train, ctypes.POINTER(_abi.BleSoftBcF32), batch, _vp, _vp, _vp]
  if hasattr(l, 'ble_rollout_leaves_f32'):    # a learned terminal value: the leaves as states, their observation, the bootstrap
    l.ble_rollout_leaves_f32.argtypes = [st, ctypes.POINTER(_abi.BleRolloutF32), ctypes.POINTER(_abi.BleNoiseGen),
                                         ctypes.POINTER(_abi.BleGpBelief), st, _vp, _vp]
    # (its three int64_t arguments are _I64, a subclass of c_int64: test_entry_checks_host.py keeps a closed table of the entry points
    # that take a plain c_int64; this one's argument checks are tests/test_leaves_entry_checks_host.py's)
    l.ble_observe_leaves_f32.argtypes = [st, ctypes.c_int32, _vp, _I64, _vp, ctypes.POINTER(_abi.BleGpHistoryF32), _vp, _I64, _vp, _I64, _vp]
    l.ble_plan_bootstrap_f32.argtypes = [ctypes.POINTER(_abi.BlePlanBootstrap), _vp]
  if hasattr(l, 'ble_qnet_forward_grouped_f32'):      # populations (sizes in the structs: no int64_t argument)
    es = ctypes.POINTER(_abi.BleEsF32)
    l.ble_qnet_forward_grouped_f32.argtypes = [ctypes.POINTER(_abi.BleQnetGroupedF32), _vp]
    l.ble_es_perturb_f32.argtypes = [es, _vp]
    l.ble_es_gradient_f32.argtypes = [es, train, _vp, _vp]
    l.ble_qnet_apply_grad_f32.argtypes = [train, _vp]
  if hasattr(l, 'ble_qnet_ppo_step_grouped_f32'):     # populations trained by gradient (sizes in the structs: no int64_t argument)
    grouped = ctypes.POINTER(_abi.BlePpoGroupedF32)
    l.ble_qnet_ppo_grouped_workspace_f32.argtypes = [grouped, ctypes.POINTER(_abi.BleQnetTrainLayout)]
    l.ble_qnet_ppo_step_grouped_f32.argtypes = [grouped, batch, _vp, _vp, _vp]
    l.ble_ac_act_grouped_f32.argtypes = [ctypes.POINTER(_abi.BleQnetGroupedF32), ctypes.POINTER(_abi.BleAcSample), _vp, _vp]
  if hasattr(l, 'ble_tree_expand_f32'):               # plan by beam search (sizes in the structs: no int64_t argument)
    l.ble_tree_expand_f32.argtypes = [st, ctypes.POINTER(_abi.BleTreeExpand), ctypes.POINTER(_abi.BleNoiseGen),
                                      ctypes.POINTER(_abi.BleGpBelief), _vp, _vp]
    l.ble_tree_select_f32.argtypes = [ctypes.POINTER(_abi.BleTreeSelect), _vp]
    l.ble_tree_finish_f32.argtypes = [ctypes.POINTER(_abi.BleTreeFinish), _vp]
  if hasattr(l, 'ble_qnet_td_step_grouped_f32'):      # populations of replay learners (sizes in the structs: no int64_t argument)
    td_grouped = ctypes.POINTER(_abi.BleTdGroupedF32)
    l.ble_qnet_td_grouped_workspace_f32.argtypes = [td_grouped, ctypes.POINTER(_abi.BleQnetTrainLayout)]
    l.ble_qnet_td_step_grouped_f32.argtypes = [td_grouped, batch, _vp, _vp, _vp]
    l.ble_replay_sample_grouped_f32.argtypes = [replay, ctypes.c_int32, _vp, batch, _vp, _vp]
    l.ble_qnet_explore_grouped_u8.argtypes = [ctypes.POINTER(_abi.BleExploreGroupedF32), _vp, _vp]
  if hasattr(l, 'ble_tree_expand_scenarios_f32'):     # the beam search in scenario winds (sizes in the structs: no int64_t argument)
    l.ble_tree_expand_scenarios_f32.argtypes = [st, ctypes.POINTER(_abi.BleTreeExpand), ctypes.POINTER(_abi.BleGpScenarios),
                                                ctypes.POINTER(_abi.BleScenarioGen), _vp, _vp]
  if hasattr(l, 'ble_mcts_select_f32'):               # guided tree search (sizes in the structs: no int64_t argument)
    pool = ctypes.POINTER(_abi.BleMctsPool)
    l.ble_mcts_select_f32.argtypes = [pool, ctypes.c_int32, ctypes.c_double, _vp, _vp, _vp]
    l.ble_mcts_expand_f32.argtypes = [st, pool, ctypes.POINTER(_abi.BleMctsExpand), ctypes.POINTER(_abi.BleNoiseGen),
                                      ctypes.POINTER(_abi.BleGpBelief), _vp, _vp]
    l.ble_mcts_backup_f32.argtypes = [pool, ctypes.c_int32, _vp, _vp, _vp]
    l.ble_mcts_finish_f32.argtypes = [pool, ctypes.POINTER(_abi.BleMctsFinish), _vp]
  if hasattr(l, 'ble_mcts_expand_scenarios_f32'):     # guided tree search in scenario winds: a node is a group of M scenario nodes
    pool = ctypes.POINTER(_abi.BleMctsPool)
    l.ble_mcts_expand_scenarios_f32.argtypes = [st, pool, ctypes.POINTER(_abi.BleMctsExpand), ctypes.POINTER(_abi.BleGpScenarios),
                                                ctypes.POINTER(_abi.BleScenarioGen), _vp, _vp]
    l.ble_mcts_backup_scenarios_f32.argtypes = [pool, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]
  if hasattr(l, 'ble_replay_tree_add_grouped_f64'):   # a population's prioritized replay and Marco Polo (sizes in the structs)
    trees = ctypes.POINTER(_abi.BleSumTreeGroupedF64)
    l.ble_replay_tree_add_grouped_f64.argtypes = [replay, trees, _vp]
    l.ble_replay_sample_prioritized_grouped_f32.argtypes = [replay, trees, _vp, batch, _vp, _vp, _vp]
    l.ble_replay_set_priority_grouped_f32.argtypes = [replay, trees, batch, _vp, _vp, _vp, _vp, _vp]
    l.ble_marco_polo_grouped_u8.argtypes = [ctypes.POINTER(_abi.BleMarcoPoloGroupedF32), _vp, _vp]
  for name in EXPORTS:
    if hasattr(l, name) or name not in ADDITIVE_EXPORTS:
      getattr(l, name).restype = _int
  _lib = l
  return l


def check(code: int, what: str) -> None:
  if code != BLE_OK:
    hip = _lib.ble_last_hip_error() if _lib is not None else 0
    raise BleLibraryError(f'{what} failed with BLE error {code} (hipError_t {hip})')


def call(name: str, *args) -> None:
  """Looks up the export `name`, calls it and raises BleLibraryError unless it answers BLE_OK."""
  check(getattr(lib(), name)(*args), name)


STEP_FORM_HELPER = 12      # BLE_STEP_FORM_HELPER (include/ble_abi.h)


class step_form:
  """`with _lib.step_form(waves): ...` forces the transition kernel's form (`ble_set_step_form`) for the launches inside the
  block and restores the previous setting: the only way to force one.  A/B runs and the bit-identity tests; the automatic
  choice is by batch size (BLE_SPLIT_MAX_ENVS).  The legal values are those the ValueError below names."""

  def __init__(self, waves_per_env: int):
    self.waves = int(waves_per_env)

  def __enter__(self):
    self.before = lib().ble_set_step_form(self.waves)
    if self.before < 0:
      raise ValueError(f'step form must be 0 (automatic), 1 (one lane per environment), 4 (four wavefronts per environment) or '
                       f'{STEP_FORM_HELPER} (one lane per environment and a helper wave per 64), not {self.waves}')
    return self

  def __exit__(self, *exc):
    lib().ble_set_step_form(self.before)
    return False
