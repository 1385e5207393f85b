"""Every host-side argument check of every entry point that takes `n`, CPU only: an invalid argument answers BLE_E_INVALID_ARG before
any HIP call, so these run on a machine without a GPU.  No call below has valid arguments and n > 0 (that would launch).

Each entry point is a list of (parameter, valid value); a case replaces some of them.  Valid arguments with n == 0 answer BLE_OK; every
case answers BLE_E_INVALID_ARG with n == 0 and with n == 64 -- the checks come before the early return on an empty batch."""
import ctypes

import pytest

from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE, _qnet
MAX_SUBSTEPS = 60         # BLE_MAX_SUBSTEPS


def _state(vehicle=None, null=None):
  return _abi.state_struct({name: 0 if name == null else _FAKE for name in _abi.FIELD_NAMES}, 0, vehicle)


def _bad_vehicle():
  return _abi.vehicle_full(envelope_volume_base=-1.0)


def _hist(null=None, **fields):
  h = _abi.BleGpHistoryF32()
  for name, ct in (('xyp', ctypes.c_float), ('elapsed_s', ctypes.c_int32), ('err_uv', ctypes.c_float), ('count', ctypes.c_int32)):
    setattr(h, name, ctypes.cast(ctypes.c_void_p(None if name == null else _FAKE), ctypes.POINTER(ct)))
  if 'chol_stride' in fields:         # a carried factor: chol (and n_chol unless it is the case) given
    h.chol = ctypes.cast(ctypes.c_void_p(_FAKE), ctypes.POINTER(ctypes.c_double))
    if not fields.get('no_n_chol'):
      h.n_chol = ctypes.cast(ctypes.c_void_p(_FAKE), ctypes.POINTER(ctypes.c_int32))
    h.chol_stride = fields['chol_stride']
  return h


def _noise(env_offset=0):
  return _abi.BleNoiseGen(1, None, None, env_offset)


def _fleet():
  return _abi.fleet_struct([{}, {'envelope_mass': 75.0}], _FAKE)


def _acc(null=None):
  return _abi.BleEvalAcc(*[None if name == null else _FAKE for name, _ in _abi.BleEvalAcc._fields_])


def _nulls(*params):
  return {f'null_{p}': {p: None} for p in params}


# ---- the entry points: (parameters with valid values, cases) ---------------------------------------------------------------------
_STEP = [('st', _state), ('action', _FAKE), ('wind_grid', _FAKE), ('grid_env_stride', 0), ('noise_uv', None), ('reward', _FAKE),
         ('terminal', _FAKE), ('effective_action', None), ('err_flags', None), ('active_count', None), ('n', 0), ('substeps', 18),
         ('stream', None)]
_STEP_CASES = {**_nulls('st', 'action', 'wind_grid', 'reward', 'terminal'), 'null_state_field': {'st': lambda: _state(null='power_paused')},
               'substeps_0': {'substeps': 0}, 'substeps_max_plus_1': {'substeps': MAX_SUBSTEPS + 1}, 'negative_stride': {'grid_env_stride': -1},
               'bad_vehicle': {'st': lambda: _state(_bad_vehicle())}}
_STEP_N = [('st', _state), ('action', _FAKE), ('wind_grid', _FAKE), ('grid_env_stride', 0), ('noise', _noise), ('reward', _FAKE),
           ('terminal', _FAKE), ('err_flags', None), ('active_count', None), ('n', 0), ('substeps', 18), ('n_steps', 4), ('stream', None)]
_STEP_N_CASES = {**_STEP_CASES, 'negative_n_steps': {'n_steps': -1}, 'negative_env_offset': {'noise': lambda: _noise(-1)}}
_RESET_AT = [('st', _state), ('mask', None), ('seed', 1), ('episode', None), ('sample', 1), ('err_flags', None), ('env_offset', 0), ('n', 0),
             ('stream', None)]
_RESET_CASES = {**_nulls('st'), 'null_state_field': {'st': lambda: _state(null='x')}, 'bad_vehicle': {'st': lambda: _state(_bad_vehicle())}}
_RESET_AT_CASES = {**_RESET_CASES, 'negative_env_offset': {'env_offset': -1}}
_OBSERVE = [('st', _state), ('wind_grid', _FAKE), ('grid_env_stride', 0), ('noise_uv', None), ('reset_mask', None), ('hist', _hist),
            ('append', 1), ('obs', _FAKE), ('err_flags', None), ('n', 0), ('stream', None)]
_OBSERVE_FORECAST = _OBSERVE[:3] + [('forecast_levels', None)] + _OBSERVE[3:]
_OBSERVE_CASES = {**_nulls('st', 'wind_grid', 'hist', 'obs'), 'null_state_field': {'st': lambda: _state(null='status')},
                  **{f'null_hist_{f}': {'hist': (lambda f=f: _hist(null=f))} for f in ('xyp', 'elapsed_s', 'err_uv', 'count')},
                  'negative_stride': {'grid_env_stride': -1},
                  'chol_without_n_chol': {'hist': lambda: _hist(chol_stride=7620, no_n_chol=True)},
                  'chol_stride_short': {'hist': lambda: _hist(chol_stride=7618)},
                  'chol_stride_odd': {'hist': lambda: _hist(chol_stride=7621)},
                  'bad_vehicle': {'st': lambda: _state(_bad_vehicle())}}
_NOISE = [('x_m', _FAKE), ('y_m', _FAKE), ('pressure', _FAKE), ('elapsed_s', _FAKE), ('seed', 1), ('episode', None), ('mode', 0),
          ('harmonic_cache', None), ('noise_uv', _FAKE), ('n', 0), ('stream', None)]
_NOISE_CASES = {**_nulls('x_m', 'y_m', 'pressure', 'elapsed_s', 'noise_uv'), 'mode_negative': {'mode': -1}, 'mode_2': {'mode': 2}}
_THERMAL = [('volume', _FAKE), ('t_int', _FAKE), ('t_amb', _FAKE), ('pressure', _FAKE), ('el_deg', _FAKE), ('flux', _FAKE),
            ('upwelling_ir', _FAKE), ('dtdt', _FAKE), ('err_flags', None), ('n', 0), ('stream', None)]
_THERMAL_CASES = _nulls('volume', 't_int', 't_amb', 'pressure', 'el_deg', 'flux', 'upwelling_ir', 'dtdt')
_SP_VOLUME = [('mols_air', _FAKE), ('t_int', _FAKE), ('pressure', _FAKE), ('volume', _FAKE), ('superpressure', _FAKE), ('n', 0),
              ('stream', None)]
_SP_VOLUME_CASES = _nulls('mols_air', 't_int', 'pressure', 'volume', 'superpressure')
_BAD_VEHICLE_ARG = {'bad_vehicle': {'vehicle': _bad_vehicle}}


def _with_fleet(params, cases):
  """A fleet entry point: the single-vehicle counterpart's parameters with `fleet` after `st`; its cases, a state vehicle standing for
  the bad vehicle (a fleet refuses any), and no fleet."""
  cases = {**cases, 'bad_vehicle': {'st': lambda: _state(_abi.vehicle_full(envelope_mass=70.0))}, 'null_fleet': {'fleet': None}}
  return params[:1] + [('fleet', _fleet)] + params[1:], cases


ENTRIES = {
    'ble_step_f32': (_STEP, _STEP_CASES),
    'ble_step_n_f32': (_STEP_N, _STEP_N_CASES),
    'ble_step_fleet_f32': _with_fleet(_STEP, _STEP_CASES),
    'ble_step_n_fleet_f32': _with_fleet(_STEP_N, _STEP_N_CASES),
    'ble_reset_f32': ([p for p in _RESET_AT if p[0] != 'env_offset'], _RESET_CASES),
    'ble_reset_at_f32': (_RESET_AT, _RESET_AT_CASES),
    'ble_reset_fleet_at_f32': _with_fleet(_RESET_AT, _RESET_AT_CASES),
    'ble_reset_seeded_f32': ([('st', _state), ('mask', None), ('env_seed', _FAKE), ('episode', None), ('sample', 1), ('err_flags', None),
                              ('n', 0), ('stream', None)], {**_RESET_CASES, **_nulls('env_seed')}),
    'ble_observe_f32': (_OBSERVE, _OBSERVE_CASES),
    'ble_observe_live_f32': (_OBSERVE, _OBSERVE_CASES),
    'ble_observe_forecast_f32': (_OBSERVE_FORECAST, _OBSERVE_CASES),
    'ble_observe_forecast_fleet_f32': _with_fleet(_OBSERVE_FORECAST, _OBSERVE_CASES),
    'ble_decode_flow_fields_f32': ([('flow', _FAKE), ('wind_grid', _FAKE), ('n', 0), ('stream', None)],
                                   {**_nulls('flow', 'wind_grid'), 'n_above_int32': {'n': 2 ** 31}}),
    'ble_wind_noise_f32': (_NOISE, _NOISE_CASES),
    'ble_wind_noise_at_f32': (_NOISE[:9] + [('env_offset', 0)] + _NOISE[9:], {**_NOISE_CASES, 'negative_env_offset': {'env_offset': -1}}),
    'ble_wind_noise_seeded_f32': ([('x_m', _FAKE), ('y_m', _FAKE), ('pressure', _FAKE), ('elapsed_s', _FAKE), ('env_seed', _FAKE),
                                   ('episode', None), ('mode', 0), ('noise_uv', _FAKE), ('n', 0), ('stream', None)],
                                  {**_NOISE_CASES, **_nulls('env_seed')}),
    'ble_forecast_f32': ([('wind_grid', _FAKE), ('grid_env_stride', 0), ('x_m', _FAKE), ('y_m', _FAKE), ('pressure', _FAKE),
                          ('elapsed_s', _FAKE), ('u', _FAKE), ('v', _FAKE), ('n', 0), ('stream', None)],
                         {**_nulls('wind_grid', 'x_m', 'y_m', 'pressure', 'elapsed_s', 'u', 'v'), 'negative_stride': {'grid_env_stride': -1}}),
    'ble_forecast_column_f32': ([('wind_grid', _FAKE), ('grid_env_stride', 0), ('x_m', _FAKE), ('y_m', _FAKE), ('elapsed_s', _FAKE),
                                 ('levels_pa', _FAKE), ('n_levels', 181), ('out_uv', _FAKE), ('n', 0), ('stream', None)],
                                {**_nulls('wind_grid', 'x_m', 'y_m', 'elapsed_s', 'levels_pa', 'out_uv'), 'n_levels_0': {'n_levels': 0},
                                 'negative_stride': {'grid_env_stride': -1}}),
    'ble_state_rows_f64': ([('st', _state), ('first', 0), ('count', 0), ('out', _FAKE), ('n', 0), ('stream', None)],
                           {**_nulls('st', 'out'), 'null_state_field': {'st': lambda: _state(null='y')}, 'negative_first': {'first': -1},
                            'negative_count': {'count': -1}, 'rows_past_n': {'first': 60, 'count': 5}}),
    'ble_power_table_f32': ([('pressure_ratio', _FAKE), ('state_of_charge', _FAKE), ('watts', _FAKE), ('err_flags', None), ('n', 0),
                             ('stream', None)], _nulls('pressure_ratio', 'state_of_charge', 'watts')),
    'ble_probe_atmosphere_f32': ([('alpha', _FAKE), ('pressure', _FAKE), ('height', _FAKE), ('temperature', _FAKE), ('err_flags', None),
                                  ('n', 0), ('stream', None)], _nulls('alpha', 'pressure', 'height', 'temperature')),
    'ble_probe_atmosphere_at_height_f64': ([('alpha', _FAKE), ('height_m', _FAKE), ('pressure', _FAKE), ('temperature', _FAKE),
                                            ('err_flags', None), ('n', 0), ('stream', None)],
                                           _nulls('alpha', 'height_m', 'pressure', 'temperature')),
    'ble_probe_solar_f32': ([('center_lat_deg', _FAKE), ('center_lng_deg', _FAKE), ('x_m', _FAKE), ('y_m', _FAKE), ('unix_s', _FAKE),
                             ('el_deg', _FAKE), ('flux', _FAKE), ('n', 0), ('stream', None)],
                            _nulls('center_lat_deg', 'center_lng_deg', 'x_m', 'y_m', 'unix_s', 'el_deg', 'flux')),
    'ble_probe_latlng_f64': ([('center_lat_deg', _FAKE), ('center_lng_deg', _FAKE), ('x_m', _FAKE), ('y_m', _FAKE), ('lat_deg', _FAKE),
                              ('lng_deg', _FAKE), ('n', 0), ('stream', None)],
                             _nulls('center_lat_deg', 'center_lng_deg', 'x_m', 'y_m', 'lat_deg', 'lng_deg')),
    'ble_probe_solar_power_f32': ([('el_deg', _FAKE), ('pressure', _FAKE), ('attenuation', _FAKE), ('power_w', _FAKE), ('n', 0),
                                   ('stream', None)], _nulls('el_deg', 'pressure', 'attenuation', 'power_w')),
    'ble_probe_thermal_f32': (_THERMAL, _THERMAL_CASES),
    'ble_probe_thermal_vehicle_f32': ([('vehicle', None)] + _THERMAL, {**_THERMAL_CASES, **_BAD_VEHICLE_ARG}),
    'ble_probe_sp_volume_f32': (_SP_VOLUME, _SP_VOLUME_CASES),
    'ble_probe_sp_volume_vehicle_f32': ([('vehicle', None)] + _SP_VOLUME, {**_SP_VOLUME_CASES, **_BAD_VEHICLE_ARG}),
    'ble_probe_acs_f32': ([('pressure_ratio', _FAKE), ('power_w', _FAKE), ('efficiency', _FAKE), ('mass_flow', _FAKE), ('n', 0),
                           ('stream', None)], _nulls('pressure_ratio', 'power_w', 'efficiency', 'mass_flow')),
    'ble_probe_safety_f32': ([('layer', 2), ('action', _FAKE), ('value', _FAKE), ('alpha', _FAKE), ('clocks', _FAKE), ('night_load_w', 183.7),
                              ('capacity_wh', 3058.56), ('fsm', _FAKE), ('effective_action', _FAKE), ('err_flags', None), ('n', 0),
                              ('stream', None)],
                             {**_nulls('action', 'value', 'fsm', 'effective_action'), 'layer_negative': {'layer': -1}, 'layer_3': {'layer': 3},
                              'layer_0_null_alpha': {'layer': 0, 'alpha': None}, 'layer_2_null_clocks': {'clocks': None},
                              'layer_2_capacity_0': {'capacity_wh': 0.0}, 'layer_2_capacity_nan': {'capacity_wh': float('nan')}}),
    'ble_probe_f64_prims': ([('x', _FAKE), ('y', _FAKE), ('op', 0), ('n', 0), ('stream', None)],
                            {**_nulls('x', 'y'), 'op_negative': {'op': -1}, 'op_9': {'op': 9}}),
    'ble_station_seeker_f32': ([('obs', _FAKE), ('obs_row_stride', _lib.OBS_DIM), ('action', _FAKE), ('level', None), ('scores', None),
                                ('err_flags', None), ('n', 0), ('stream', None)],
                               {**_nulls('obs', 'action'), 'stride_below_obs_dim': {'obs_row_stride': _lib.OBS_DIM - 1},
                                'n_above_four_int32': {'n': 4 * (2 ** 31 - 1) + 1}}),
    'ble_eval_accumulate_f32': ([('st', _state), ('reward', _FAKE), ('acc', _acc), ('radius_m', 50000.0), ('step_index', 0), ('max_steps', 10),
                                 ('flight_path', None), ('n', 0), ('stream', None)],
                                {**_nulls('st', 'reward', 'acc'), 'null_state_field': {'st': lambda: _state(null='alpha')},
                                 **{f'null_acc_{f}': {'acc': (lambda f=f: _acc(null=f))} for f, _ in _abi.BleEvalAcc._fields_},
                                 'negative_step_index': {'step_index': -1}, 'max_steps_not_above_step': {'max_steps': 0},
                                 'bad_vehicle': {'st': lambda: _state(_bad_vehicle())}}),
    'ble_qnet_workspace_f32': ([('net', _qnet), ('n', 0), ('packed_floats', None), ('scratch_floats', None)],
                               {**_nulls('net'), 'layers_0': {'net': lambda: _qnet(num_layers=0)},
                                'layers_65': {'net': lambda: _qnet(num_layers=65)}, 'actions_2': {'net': lambda: _qnet(num_actions=2)}}),
    'ble_qnet_forward_f32': ([('net', _qnet), ('obs', _FAKE), ('obs_row_stride', _lib.OBS_DIM), ('scratch', _FAKE), ('action', _FAKE),
                              ('q_values', None), ('n', 0), ('stream', None)],
                             {**_nulls('net', 'obs', 'scratch', 'action'), 'null_weights': {'net': lambda: _qnet(weights=None)},
                              'layers_0': {'net': lambda: _qnet(num_layers=0)}, 'layers_65': {'net': lambda: _qnet(num_layers=65)},
                              'hidden_0': {'net': lambda: _qnet(hidden_units=0)}, 'atoms_0': {'net': lambda: _qnet(num_atoms=0)},
                              'input_dim': {'net': lambda: _qnet(input_dim=_lib.OBS_DIM - 1)},
                              'stride_below_obs_dim': {'obs_row_stride': _lib.OBS_DIM - 1},
                              'misaligned_weights': {'net': lambda: _qnet(weights=_FAKE + 4)}, 'misaligned_scratch': {'scratch': _FAKE + 8}}),
}


def _call(entry, n, case=None):
  params, cases = ENTRIES[entry]
  values = dict(params)
  values['n'] = n
  values.update(cases[case] if case is not None else {})
  args = []
  for name, _ in params:
    v = values[name]
    v = v() if callable(v) else v
    args.append(ctypes.byref(v) if isinstance(v, ctypes.Structure) else v)
  return getattr(_lib.lib(), entry)(*args)


def test_every_entry_point_that_takes_n_is_covered():
  lib = _lib.lib()
  takes_n = {name for name in _lib.EXPORTS if getattr(lib, name).argtypes and ctypes.c_int64 in getattr(lib, name).argtypes}
  assert takes_n == set(ENTRIES), takes_n ^ set(ENTRIES)
  for name, (params, _) in ENTRIES.items():
    assert len(params) == len(getattr(lib, name).argtypes), name


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_valid_arguments_and_no_environments(entry):
  assert _call(entry, 0) == 0


_CASES = [(entry, case) for entry in sorted(ENTRIES) for case in ENTRIES[entry][1]]


@pytest.mark.parametrize('entry,case', _CASES, ids=[f'{e}-{c}' for e, c in _CASES])
def test_invalid_argument(entry, case):
  for n in (0,) if 'n' in ENTRIES[entry][1][case] else (0, 64):       # (a case about n itself sets it)
    assert _call(entry, n, case) == E_INVALID_ARG, (entry, case, n)


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_negative_n(entry):
  assert _call(entry, -1) == E_INVALID_ARG
