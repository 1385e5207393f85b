"""Every host-side argument check of the learned terminal value's entry points (ble_rollout_leaves_f32, ble_observe_leaves_f32,
ble_plan_bootstrap_f32), CPU only, in the style of test_exit_entry_checks_host.py: an invalid argument answers
BLE_E_INVALID_ARG before any HIP call, with an empty batch and with a non-empty one.  ble_rollout_f32, ble_rollout_belief_f32 and
ble_observe_f32, whose checks the new entry points share, answer on the same descriptors as they did.  No call below launches."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float('nan'), float('inf')
ENTRIES = ('ble_rollout_leaves_f32', 'ble_observe_leaves_f32', 'ble_plan_bootstrap_f32')
_LEAF = _FAKE + 0x10000        # the leaf arena's arrays: not the source's


def _header():
  return open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()


def _ref(x):
  return ctypes.byref(x) if x is not None else None


def _state(address=_FAKE, null=None, vehicle=None, same_as_source=None):
  fields = {name: 0 if name == null else (_FAKE if name == same_as_source else address) for name in _abi.FIELD_NAMES}
  return _abi.state_struct(fields, 0, vehicle)


def _ro(**over):
  f = dict(n=0, n_plans=4, n_plan_steps=6, action_repeat=1, substeps=18, gamma=0.99, plans=_FAKE, wind_grid=_FAKE, grid_env_stride=0,
           ret=_FAKE, steps_flown=_FAKE, reward=None, final_state=None)
  f.update(over)
  return _abi.BleRolloutF32(**f)


def _belief(**over):
  f = dict(slab=_FAKE, stride=720, n_obs=_FAKE, n=0)
  f.update(over)
  return _abi.BleGpBelief(**f)


def _gen(**over):
  f = dict(seed=3, episode=_FAKE, harmonic_cache=None, env_offset=0)
  f.update(over)
  return _abi.BleNoiseGen(**f)


def _hist(null=None):
  h = _abi.BleGpHistoryF32()
  for name, ct in (('xyp', ctypes.c_float), ('elapsed_s', ctypes.c_int32), ('err_uv', ctypes.c_float), ('count', ctypes.c_int32)):
    if name != null:
      setattr(h, name, ctypes.cast(ctypes.c_void_p(_FAKE), ctypes.POINTER(ct)))
  return h


def _boot(**over):
  f = dict(n=0, n_plans=8, reserved_=0, gamma=0.993, ret=_FAKE, steps_flown=_FAKE, leaf_status=_FAKE, value=_FAKE, score=_FAKE)
  f.update(over)
  return _abi.BlePlanBootstrap(**f)


_DEFAULT = object()


def _rollout(st=_DEFAULT, ro=_DEFAULT, noise=None, belief=None, leaves=_DEFAULT):
  st = _state() if st is _DEFAULT else st
  ro = _ro() if ro is _DEFAULT else ro
  leaves = _state(_LEAF) if leaves is _DEFAULT else leaves
  return _lib.lib().ble_rollout_leaves_f32(_ref(st), _ref(ro), _ref(noise), _ref(belief), _ref(leaves), None, None)


def _observe(leaves=_DEFAULT, per_env=4, grid=_FAKE, grid_stride=0, mask=None, hist=_DEFAULT, obs=_FAKE, stride=1099, n=0):
  leaves = _state(_LEAF) if leaves is _DEFAULT else leaves
  hist = _hist() if hist is _DEFAULT else hist
  return _lib.lib().ble_observe_leaves_f32(_ref(leaves), per_env, grid, grid_stride, mask, _ref(hist), obs, stride, None, n, None)


def _bootstrap(b):
  return _lib.lib().ble_plan_bootstrap_f32(_ref(b), None)


# ---- declared, exported, mirrored ----------------------------------------------------------------------------------------------------
def test_declared_exported_and_mirrored():
  header = _header()
  assert re.search(r'\bint ble_rollout_leaves_f32\(const ble_state_f32\* st, const struct ble_rollout_f32\* ro, const ble_noise_gen\* noise,\s*'
                   r'const ble_gp_belief\* belief, const ble_state_f32\* leaves, uint32_t\* err_flags, void\* stream\);', header)
  assert re.search(r'\bint ble_observe_leaves_f32\(const ble_state_f32\* leaves, int32_t leaves_per_env, const float\* wind_grid, '
                   r'int64_t grid_env_stride,\s*const uint8_t\* reset_mask, const ble_gp_history_f32\* hist, float\* obs, '
                   r'int64_t obs_row_stride,\s*uint32_t\* err_flags, int64_t n_leaves, void\* stream\);', header)
  assert re.search(r'\bint ble_plan_bootstrap_f32\(const struct ble_plan_bootstrap\* b, void\* stream\);', header)
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header) and _lib.ABI_VERSION == 5            # additive: the ABI stays 5
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  for name in ENTRIES:
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert re.search(r' T ' + name + r'$', symbols, re.M), name
    fn = getattr(_lib.lib(), name)
    assert fn.argtypes is not None and fn.restype is ctypes.c_int


def test_struct_layout_matches_the_header():
  body = re.search(r'struct ble_plan_bootstrap \{(.*?)\n\}', _header(), re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  declared = [re.search(r'(\w+)\s*$', d).group(1) for d in body.split(';') if d.strip()]
  assert declared == [f[0] for f in _abi.BlePlanBootstrap._fields_]
  assert ctypes.sizeof(_abi.BlePlanBootstrap) == 64
  for name, kind in _abi.BlePlanBootstrap._fields_:
    if kind in (ctypes.c_void_p, ctypes.c_int64, ctypes.c_double):
      assert getattr(_abi.BlePlanBootstrap, name).offset % 8 == 0, name


# ---- empty batches -------------------------------------------------------------------------------------------------------------------
def test_empty_batch_is_ok_without_a_launch():
  assert _rollout() == _lib.BLE_OK                                         # the forecast
  assert _rollout(noise=_gen()) == _lib.BLE_OK
  assert _rollout(belief=_belief()) == _lib.BLE_OK
  leaves = _state(_LEAF)
  leaves.episode_cache = None                                              # (not read, not written)
  assert _rollout(leaves=leaves) == _lib.BLE_OK
  assert _rollout(ro=_ro(reward=_FAKE, final_state=_FAKE, n_plan_steps=480, action_repeat=2, gamma=0.0)) == _lib.BLE_OK
  assert _observe() == _lib.BLE_OK
  assert _observe(per_env=1, mask=_FAKE, stride=1104, grid_stride=79380) == _lib.BLE_OK
  assert _observe(per_env=1024) == _lib.BLE_OK
  for gamma in (0.0, 0.993, 1.0):
    assert _bootstrap(_boot(gamma=gamma)) == _lib.BLE_OK
  assert _bootstrap(_boot(n_plans=1024)) == _lib.BLE_OK
  assert _bootstrap(_boot(n_plans=1)) == _lib.BLE_OK


# ---- invalid arguments ---------------------------------------------------------------------------------------------------------------
_RO_BAD = {                     # what ble_rollout_f32 refuses of its struct
    'null_plans': dict(plans=None), 'null_grid': dict(wind_grid=None), 'null_ret': dict(ret=None), 'null_steps_flown': dict(steps_flown=None),
    'plans_0': dict(n_plans=0), 'plans_negative': dict(n_plans=-1), 'steps_0': dict(n_plan_steps=0), 'repeat_0': dict(action_repeat=0),
    'steps_961': dict(n_plan_steps=961), 'steps_times_repeat_962': dict(n_plan_steps=481, action_repeat=2),
    'substeps_0': dict(substeps=0), 'substeps_huge': dict(substeps=10 ** 6), 'negative_grid_stride': dict(grid_env_stride=-1),
    'gamma_nan': dict(gamma=NAN), 'gamma_negative': dict(gamma=-0.1), 'gamma_above_1': dict(gamma=1.0001), 'gamma_inf': dict(gamma=INF),
    'negative_n': dict(n=-1), 'n_2_31': dict(n=2 ** 31, n_plans=1), 'n_times_k_2_31': dict(n=2 ** 29, n_plans=4),
}

_CASES = {
    # -- the rollout with leaves
    **{f'rollout_{k}': (lambda n, k=k: _rollout(ro=_ro(**{'n': n, **_RO_BAD[k]}))) for k in _RO_BAD},
    **{f'rollout_belief_{k}': (lambda n, k=k: _rollout(ro=_ro(**{'n': n, **_RO_BAD[k]}), belief=_belief(n=_RO_BAD[k].get('n', n))))
       for k in _RO_BAD},
    'rollout_null_state': lambda n: _rollout(st=None, ro=_ro(n=n)),
    'rollout_null_state_array': lambda n: _rollout(st=_state(null='pressure'), ro=_ro(n=n)),
    'rollout_null_ro': lambda n: _rollout(ro=None),
    'rollout_both_winds': lambda n: _rollout(ro=_ro(n=n), noise=_gen(), belief=_belief(n=n)),
    'rollout_null_leaves': lambda n: _rollout(ro=_ro(n=n), leaves=None),
    'rollout_null_leaf_array': lambda n: _rollout(ro=_ro(n=n), leaves=_state(_LEAF, null='last_command')),
    'rollout_null_leaf_constant': lambda n: _rollout(ro=_ro(n=n), leaves=_state(_LEAF, null='start_unix')),
    'rollout_leaf_array_is_the_sources': lambda n: _rollout(ro=_ro(n=n), leaves=_state(_LEAF, same_as_source='x')),
    'rollout_leaf_status_is_the_sources': lambda n: _rollout(ro=_ro(n=n), leaves=_state(_LEAF, same_as_source='status')),
    'rollout_leaves_are_the_source': lambda n: _rollout(ro=_ro(n=n), leaves=_state()),
    'rollout_negative_noise_offset': lambda n: _rollout(ro=_ro(n=n), noise=_gen(env_offset=-1)),
    'rollout_bad_vehicle': lambda n: _rollout(st=_state(vehicle=_abi.vehicle_struct(envelope_mass=-1.0)), ro=_ro(n=n)),
    'rollout_belief_of_another_batch': lambda n: _rollout(ro=_ro(n=n), belief=_belief(n=n + 1)),
    'rollout_belief_null_slab': lambda n: _rollout(ro=_ro(n=n), belief=_belief(n=n, slab=None)),
    'rollout_belief_short_stride': lambda n: _rollout(ro=_ro(n=n), belief=_belief(n=n, stride=718)),
    'rollout_belief_misaligned_slab': lambda n: _rollout(ro=_ro(n=n), belief=_belief(n=n, slab=_FAKE + 8)),
    # -- the observation of leaves
    'observe_null_leaves': lambda n: _observe(leaves=None, n=n),
    'observe_null_leaf_array': lambda n: _observe(leaves=_state(_LEAF, null='superpressure'), n=n),
    'observe_null_hist': lambda n: _observe(hist=None, n=n),
    **{f'observe_null_ring_{f}': (lambda n, f=f: _observe(hist=_hist(null=f), n=n)) for f in ('xyp', 'elapsed_s', 'err_uv', 'count')},
    'observe_null_grid': lambda n: _observe(grid=None, n=n),
    'observe_null_obs': lambda n: _observe(obs=None, n=n),
    'observe_per_env_0': lambda n: _observe(per_env=0, n=n),
    'observe_per_env_negative': lambda n: _observe(per_env=-4, n=n),
    'observe_negative_n': lambda n: _observe(n=-4),
    'observe_n_2_31': lambda n: _observe(n=2 ** 31),
    'observe_n_not_a_multiple': lambda n: _observe(per_env=4, n=n + 6),
    'observe_stride_1098': lambda n: _observe(stride=1098, n=n),
    'observe_stride_0': lambda n: _observe(stride=0, n=n),
    'observe_negative_grid_stride': lambda n: _observe(grid_stride=-1, n=n),
    'observe_bad_vehicle': lambda n: _observe(leaves=_state(_LEAF, vehicle=_abi.vehicle_struct(battery_capacity_wh=0.0)), n=n),
    # -- the bootstrap
    'bootstrap_null_struct': lambda n: _lib.lib().ble_plan_bootstrap_f32(None, None),
    **{f'bootstrap_null_{f}': (lambda n, f=f: _bootstrap(_boot(n=n, **{f: None}))) for f in ('ret', 'steps_flown', 'leaf_status', 'value', 'score')},
    'bootstrap_plans_0': lambda n: _bootstrap(_boot(n=n, n_plans=0)),
    'bootstrap_plans_negative': lambda n: _bootstrap(_boot(n=n, n_plans=-1)),
    'bootstrap_plans_1025': lambda n: _bootstrap(_boot(n=n, n_plans=1025)),
    'bootstrap_negative_n': lambda n: _bootstrap(_boot(n=-1)),
    'bootstrap_n_2_31': lambda n: _bootstrap(_boot(n=2 ** 31, n_plans=1)),
    'bootstrap_n_times_k_2_31': lambda n: _bootstrap(_boot(n=2 ** 21, n_plans=1024)),
    'bootstrap_gamma_nan': lambda n: _bootstrap(_boot(n=n, gamma=NAN)),
    'bootstrap_gamma_negative': lambda n: _bootstrap(_boot(n=n, gamma=-1e-9)),
    'bootstrap_gamma_above_1': lambda n: _bootstrap(_boot(n=n, gamma=1.0 + 1e-12)),
    'bootstrap_gamma_inf': lambda n: _bootstrap(_boot(n=n, gamma=INF)),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG


# ---- the entry points next to them keep their answers ---------------------------------------------------------------------------------
def test_the_existing_entry_points_keep_their_answers():
  """The checks of ble_rollout_f32 and ble_rollout_belief_f32 moved into launchers they share with the leaf form: the same answers on
  the same descriptors, and ble_observe_f32 -- whose kernel gained the leaf form -- refuses what it refused."""
  lib = _lib.lib()
  st = _state()
  assert lib.ble_rollout_f32(_ref(st), _ref(_ro()), None, None, None) == _lib.BLE_OK
  assert lib.ble_rollout_f32(_ref(st), _ref(_ro()), _ref(_gen()), None, None) == _lib.BLE_OK
  assert lib.ble_rollout_belief_f32(_ref(st), _ref(_ro()), _ref(_belief()), None, None) == _lib.BLE_OK
  for n in (0, 64):
    for k, bad in _RO_BAD.items():
      ro = _ro(**{'n': n, **bad})
      assert lib.ble_rollout_f32(_ref(st), _ref(ro), None, None, None) == E_INVALID_ARG, k
      assert lib.ble_rollout_belief_f32(_ref(st), _ref(ro), _ref(_belief(n=bad.get('n', n))), None, None) == E_INVALID_ARG, k
    assert lib.ble_rollout_f32(None, _ref(_ro(n=n)), None, None, None) == E_INVALID_ARG
    assert lib.ble_rollout_f32(_ref(_state(null='x')), _ref(_ro(n=n)), None, None, None) == E_INVALID_ARG
    assert lib.ble_rollout_f32(_ref(st), _ref(_ro(n=n)), _ref(_gen(env_offset=-1)), None, None) == E_INVALID_ARG
    assert lib.ble_rollout_belief_f32(_ref(st), _ref(_ro(n=n)), None, None, None) == E_INVALID_ARG
    assert lib.ble_rollout_belief_f32(_ref(st), _ref(_ro(n=n)), _ref(_belief(n=n + 1)), None, None) == E_INVALID_ARG
    # ble_observe_f32(st, grid, stride, noise_uv, reset_mask, hist, append, obs, err_flags, n, stream)
    assert lib.ble_observe_f32(_ref(st), _FAKE, 0, None, None, None, 1, _FAKE, None, n, None) == E_INVALID_ARG
    assert lib.ble_observe_f32(_ref(st), _FAKE, 0, None, None, _ref(_hist(null='count')), 1, _FAKE, None, n, None) == E_INVALID_ARG
    assert lib.ble_observe_f32(_ref(st), None, 0, None, None, _ref(_hist()), 1, _FAKE, None, n, None) == E_INVALID_ARG
    assert lib.ble_observe_f32(_ref(st), _FAKE, 0, None, None, _ref(_hist()), 1, None, None, n, None) == E_INVALID_ARG
    assert lib.ble_observe_f32(_ref(st), _FAKE, -1, None, None, _ref(_hist()), 1, _FAKE, None, n, None) == E_INVALID_ARG
    assert lib.ble_observe_f32(_ref(_state(null='alpha')), _FAKE, 0, None, None, _ref(_hist()), 1, _FAKE, None, n, None) == E_INVALID_ARG
  assert lib.ble_observe_f32(_ref(st), _FAKE, 0, None, None, _ref(_hist()), 1, _FAKE, None, -1, None) == E_INVALID_ARG
  assert lib.ble_observe_f32(_ref(st), _FAKE, 0, None, None, _ref(_hist()), 1, _FAKE, None, 0, None) == _lib.BLE_OK
  assert lib.ble_observe_f32(_ref(st), _FAKE, 0, None, None, _ref(_hist()), 0, _FAKE, None, 0, None) == _lib.BLE_OK
