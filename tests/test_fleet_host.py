"""Fleets (include/ble_abi.h::ble_fleet), CPU only: the header <-> ctypes mirror, the exports, and every host-side argument check of the
four fleet entry points -- they answer BLE_E_INVALID_ARG before any HIP call, so they run on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib, vec_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
FLEET_ENTRY_POINTS = ('ble_step_fleet_f32', 'ble_step_n_fleet_f32', 'ble_reset_fleet_at_f32', 'ble_observe_forecast_fleet_f32')
E_INVALID_ARG = -1


def _define(name):
  return int(re.search(r'#define ' + name + r' \(?(-?\d+)u?\)?', HEADER).group(1))


def test_fleet_struct_matches_header():
  body = HEADER[HEADER.index('typedef struct ble_fleet {'):HEADER.index('} ble_fleet;')]
  names = re.findall(r'(\w+);', body)
  assert names == [f[0] for f in _abi.BleFleet._fields_]
  assert _define('BLE_FLEET_MAX_VEHICLES') == _abi.FLEET_MAX_VEHICLES == 16
  assert _define('BLE_FLAG_VEHICLE_INDEX') == _lib.FLAG_VEHICLE_INDEX == 512
  # pointer, two int32, pointer: the C layout on x86-64
  assert ctypes.sizeof(_abi.BleFleet) == 24
  assert [getattr(_abi.BleFleet, n).offset for n in names] == [0, 8, 12, 16]


def test_fleet_entry_points_declared_and_exported():
  declared = set(re.findall(r'^int (ble_\w+)\(', HEADER, re.M))
  assert set(FLEET_ENTRY_POINTS) <= declared
  assert set(FLEET_ENTRY_POINTS) <= set(_lib.EXPORTS)
  path = _lib.build()
  out = subprocess.check_output(['nm', '-D', '--defined-only', path]).decode()
  exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
  assert set(FLEET_ENTRY_POINTS) <= exported


def test_fleet_struct_builder():
  f = _abi.fleet_struct([{}, {'envelope_mass': 70.0, 'power_safety_layer_enabled': False}], 0x1000, sample_index=True)
  assert f.n_vehicles == 2 and f.sample_index == 1 and f.vehicle_index == 0x1000
  assert f.palette[0].envelope_volume_base == 1804.0 and f.palette[0].power_safety_layer_enabled == 1
  assert f.palette[1].envelope_mass == 70.0 and f.palette[1].power_safety_layer_enabled == 0
  assert vec_state.VecSimulator.vehicle_overrides({'envelope_mass': 68.5, 'payload_mass': 90}) == {'payload_mass': 90.0}
  with pytest.raises(TypeError):
    _abi.fleet_struct([{'no_such_field': 1.0}], 0x1000)


def test_vehicle_index_flag_raises_value_error():
  with pytest.raises(ValueError, match='palette'):
    vec_state.raise_for_flags(_lib.FLAG_VEHICLE_INDEX)


# ---- argument checks through ctypes (never dereferenced: the checks answer first) ------------------------------------------------
_FAKE = 0x100000          # a non-NULL address for every device pointer


def _state(vehicle=None):
  return _abi.state_struct({name: _FAKE for name in _abi.FIELD_NAMES}, 0, vehicle)


def _hist():
  h = _abi.BleGpHistoryF32()
  for name, ct in (('xyp', ctypes.c_float), ('elapsed_s', ctypes.c_int32), ('err_uv', ctypes.c_float), ('count', ctypes.c_int32)):
    setattr(h, name, ctypes.cast(ctypes.c_void_p(_FAKE), ctypes.POINTER(ct)))
  return h


def _call(name, st, fleet, n):
  l = _lib.lib()
  f = None if fleet is None else ctypes.byref(fleet)
  if name == 'ble_step_fleet_f32':
    return l.ble_step_fleet_f32(ctypes.byref(st), f, _FAKE, _FAKE, 0, None, _FAKE, _FAKE, None, None, None, n, 18, None)
  if name == 'ble_step_n_fleet_f32':
    return l.ble_step_n_fleet_f32(ctypes.byref(st), f, _FAKE, _FAKE, 0, None, _FAKE, _FAKE, None, None, n, 18, 4, None)
  if name == 'ble_reset_fleet_at_f32':
    return l.ble_reset_fleet_at_f32(ctypes.byref(st), f, None, 1, None, 1, None, 0, n, None)
  hist = _hist()
  return l.ble_observe_forecast_fleet_f32(ctypes.byref(st), f, _FAKE, 0, None, None, None, ctypes.byref(hist), 1, _FAKE, None, n, None)


def _fleet(vehicles=({}, {'envelope_mass': 75.0}), index=_FAKE, n_vehicles=None):
  f = _abi.fleet_struct(list(vehicles), index)
  if n_vehicles is not None:
    f.n_vehicles = n_vehicles
  return f


@pytest.mark.parametrize('entry', FLEET_ENTRY_POINTS)
def test_fleet_valid_arguments_pass_the_checks(entry):
  # n == 0 returns before any launch: BLE_OK shows that the arguments below differ from these in the fleet alone
  assert _call(entry, _state(), _fleet(), 0) == 0
  assert _call(entry, _state(), _fleet([{}] * 16), 0) == 0


@pytest.mark.parametrize('entry', FLEET_ENTRY_POINTS)
@pytest.mark.parametrize('case', ['no_fleet', 'bad_palette_entry', 'nan_palette_entry', 'zero_vehicles', 'seventeen_vehicles',
                                  'null_index', 'null_palette', 'state_vehicle_too'])
def test_fleet_argument_checks(entry, case):
  st, fleet = _state(), _fleet()
  if case == 'no_fleet':
    fleet = None
  elif case == 'bad_palette_entry':
    fleet = _fleet([{}, {'envelope_volume_base': -1.0}])
  elif case == 'nan_palette_entry':
    fleet = _fleet([{'battery_capacity_wh': float('nan')}])
  elif case == 'zero_vehicles':
    fleet = _fleet(n_vehicles=0)
  elif case == 'seventeen_vehicles':
    fleet = _fleet([{}] * 17)
  elif case == 'null_index':
    fleet = _fleet(index=0)
  elif case == 'null_palette':
    fleet.palette = ctypes.POINTER(_abi.BleVehicle)()
  elif case == 'state_vehicle_too':
    st = _state(_abi.vehicle_full(envelope_mass=70.0))
  for n in (0, 64):
    assert _call(entry, st, fleet, n) == E_INVALID_ARG, (entry, case, n)
