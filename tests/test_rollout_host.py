"""ble_rollout_f32 on a machine without a GPU: the entry is declared, exported and mirrored, its sizes travel in the struct (no int64
argument), and every invalid argument answers BLE_E_INVALID_ARG before any HIP call, with n == 0 and with n == 64 (no call below has
valid arguments and n > 0: that would launch)."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID_ARG = -1
_FAKE = 0x1000          # a non-NULL address that is never dereferenced (the checks come before any HIP call)
MAX_SUBSTEPS, MAX_STEPS = 60, 960         # BLE_MAX_SUBSTEPS, BLE_ROLLOUT_MAX_STEPS
_HEADER_FIELDS = ['n', 'n_plans', 'n_plan_steps', 'action_repeat', 'substeps', 'gamma', 'plans', 'wind_grid', 'grid_env_stride', 'ret',
                  'steps_flown', 'reward', 'final_state']


def _state(vehicle=None, null=None):
  return _abi.state_struct({name: 0 if name == null else _FAKE for name in _abi.FIELD_NAMES}, 0, vehicle)


def _ro(**over):
  f = dict(n=0, n_plans=4, n_plan_steps=6, action_repeat=1, substeps=18, gamma=0.99, plans=_FAKE, wind_grid=_FAKE, grid_env_stride=0,
           ret=_FAKE, steps_flown=_FAKE, reward=None, final_state=None)
  f.update(over)
  return _abi.BleRolloutF32(**f)


def _noise(env_offset=0):
  return _abi.BleNoiseGen(1, None, None, env_offset)


def _call(st, ro, noise=None):
  return _lib.lib().ble_rollout_f32(None if st is None else ctypes.byref(st), None if ro is None else ctypes.byref(ro),
                                    None if noise is None else ctypes.byref(noise), None, None)


def test_declared_exported_and_mirrored():
  header = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
  assert re.search(r'\bint ble_rollout_f32\(const ble_state_f32\* st, const struct ble_rollout_f32\* ro, const ble_noise_gen\* noise,', header)
  assert 'struct ble_rollout_f32 {' in header
  assert re.search(r'#define BLE_ROLLOUT_MAX_STEPS 960\b', header) and _abi.ROLLOUT_MAX_STEPS == MAX_STEPS
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header)            # additive: the ABI stays 5
  assert 'ble_rollout_f32' in _lib.EXPORTS and 'ble_rollout_f32' in _lib.ADDITIVE_EXPORTS and _lib.ABI_VERSION == 5
  assert any(s.endswith('ble_rollout.h') for s in _lib._SOURCES)
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  assert re.search(r' T ble_rollout_f32$', symbols, re.M)


def test_sizes_travel_in_the_struct():
  argtypes = _lib.lib().ble_rollout_f32.argtypes
  assert argtypes is not None and len(argtypes) == 5 and ctypes.c_int64 not in argtypes


def test_struct_layout_matches_the_header():
  header = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
  body = re.search(r'struct ble_rollout_f32 \{(.*?)\n\};', header, re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  declared = [re.search(r'(\w+)\s*$', d).group(1) for d in body.split(';') if d.strip()]
  assert declared == _HEADER_FIELDS
  assert [f[0] for f in _abi.BleRolloutF32._fields_] == _HEADER_FIELDS
  # int64, 4 x int32, double, 2 pointers, int64, 4 pointers: no padding anywhere
  assert ctypes.sizeof(_abi.BleRolloutF32) == 8 + 4 * 4 + 8 + 2 * 8 + 8 + 4 * 8
  assert _abi.BleRolloutF32.gamma.offset == 24 and _abi.BleRolloutF32.plans.offset == 32 and _abi.BleRolloutF32.ret.offset == 56


def test_empty_batch_is_ok_without_a_launch():
  assert _call(_state(), _ro()) == _lib.BLE_OK
  assert _call(_state(), _ro(), _noise()) == _lib.BLE_OK
  assert _call(_state(), _ro(reward=_FAKE, final_state=_FAKE, grid_env_stride=79380)) == _lib.BLE_OK
  assert _call(_state(_abi.vehicle_full(envelope_mass=70.0)), _ro()) == _lib.BLE_OK
  # the bounds themselves are legal: gamma 0 and 1, H * repeat == 960, n * K == 2^31 - 1 (n == 0: only the product's bound is in play)
  assert _call(_state(), _ro(gamma=0.0)) == _lib.BLE_OK and _call(_state(), _ro(gamma=1.0)) == _lib.BLE_OK
  assert _call(_state(), _ro(n_plan_steps=480, action_repeat=2)) == _lib.BLE_OK
  assert _call(_state(), _ro(n_plans=2 ** 31 - 1)) == _lib.BLE_OK
  assert _call(_state(), _ro(substeps=1)) == _lib.BLE_OK and _call(_state(), _ro(substeps=MAX_SUBSTEPS)) == _lib.BLE_OK


_CASES = {
    'null_st': lambda n: (None, _ro(n=n), None),
    **{f'null_state_{f}': (lambda n, f=f: (_state(null=f), _ro(n=n), None)) for f in ('x', 'start_unix', 'power_paused')},
    'null_ro': lambda n: (_state(), None, None),
    **{f'null_{f}': (lambda n, f=f: (_state(), _ro(n=n, **{f: None}), None)) for f in ('plans', 'wind_grid', 'ret', 'steps_flown')},
    'negative_n': lambda n: (_state(), _ro(n=-1), None),
    'plans_0': lambda n: (_state(), _ro(n=n, n_plans=0), None),
    'plans_negative': lambda n: (_state(), _ro(n=n, n_plans=-2), None),
    'plan_steps_0': lambda n: (_state(), _ro(n=n, n_plan_steps=0), None),
    'plan_steps_negative': lambda n: (_state(), _ro(n=n, n_plan_steps=-1), None),
    'repeat_0': lambda n: (_state(), _ro(n=n, action_repeat=0), None),
    'repeat_negative': lambda n: (_state(), _ro(n=n, action_repeat=-1), None),
    'steps_961': lambda n: (_state(), _ro(n=n, n_plan_steps=961), None),
    'steps_times_repeat_962': lambda n: (_state(), _ro(n=n, n_plan_steps=481, action_repeat=2), None),
    'steps_times_repeat_wraps_int32': lambda n: (_state(), _ro(n=n, n_plan_steps=2 ** 16, action_repeat=2 ** 16), None),
    'n_times_k_2_31': lambda n: (_state(), _ro(n=2 ** 20, n_plans=2 ** 11), None),
    'n_2_31': lambda n: (_state(), _ro(n=2 ** 31, n_plans=1), None),
    'n_times_k_wraps_int64': lambda n: (_state(), _ro(n=2 ** 62, n_plans=4), None),
    'substeps_0': lambda n: (_state(), _ro(n=n, substeps=0), None),
    'substeps_max_plus_1': lambda n: (_state(), _ro(n=n, substeps=MAX_SUBSTEPS + 1), None),
    'negative_stride': lambda n: (_state(), _ro(n=n, grid_env_stride=-1), None),
    'negative_env_offset': lambda n: (_state(), _ro(n=n), _noise(-1)),
    'gamma_nan': lambda n: (_state(), _ro(n=n, gamma=float('nan')), None),
    'gamma_negative': lambda n: (_state(), _ro(n=n, gamma=-1e-9), None),
    'gamma_above_1': lambda n: (_state(), _ro(n=n, gamma=1.0000001), None),
    'gamma_inf': lambda n: (_state(), _ro(n=n, gamma=float('inf')), None),
    'bad_vehicle': lambda n: (_state(_abi.vehicle_full(envelope_volume_base=-1.0)), _ro(n=n), None),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  st, ro, noise = _CASES[case](n)
  assert _call(st, ro, noise) == E_INVALID_ARG
