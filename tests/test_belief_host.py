"""The belief -- ble_gp_fit_f32, ble_gp_belief_wind_f32, ble_rollout_belief_f32 -- on a machine without a GPU: the entries are declared,
exported and mirrored (their sizes travel in struct ble_gp_belief: no int64 argument), every invalid argument answers BLE_E_INVALID_ARG before any HIP call, with n == 0 and with n == 64 (no call below
has valid arguments and n > 0: that would launch), and the lane function gp_belief_mean, built for the host, agrees with a NumPy
restatement of the posterior mean.

The numerics check: 40 random windows of 1, 2, 17, 64 and 120 observations (the spread of test_gpu_gp_query.py::_observations: positions
within +-200 km, pressures 5 .. 14 kPa, 180 s apart, errors ~ N(0, 2 m/s)), 32 points each at times from an hour before the anchor to
twelve hours after it.  Reference: alpha = cho_solve(chol(K + 0.05 I), y) and mean = K* alpha in float64 (tests/wind_gp_host.py's
kernel); both sides get the same alpha, so what is compared is the evaluation of K* alpha alone.  Bar: the project's 1e-5 m/s absolute
(DESIGN 5); the float32 rounding of a mean of a few m/s is 2.4e-7, the lane function's exponential is good to ~1e-14 relative."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg

import wind_gp_host
from balloon_learning_environment_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID_ARG = -1
_FAKE = 0x1000          # a non-NULL, 16-byte aligned address that is never dereferenced (the checks come before any HIP call)
MAX_SUBSTEPS = 60
ENTRIES = ('ble_gp_fit_f32', 'ble_gp_belief_wind_f32', 'ble_rollout_belief_f32')
TOL = 1e-5


def _header():
  return open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()


def _state(vehicle=None, null=None):
  return _abi.state_struct({name: 0 if name == null else _FAKE for name in _abi.FIELD_NAMES}, 0, vehicle)


def _ro(**over):
  f = dict(n=0, n_plans=4, n_plan_steps=6, action_repeat=1, substeps=18, gamma=0.99, plans=_FAKE, wind_grid=_FAKE, grid_env_stride=0,
           ret=_FAKE, steps_flown=_FAKE, reward=None, final_state=None)
  f.update(over)
  return _abi.BleRolloutF32(**f)


def _belief(**over):
  f = dict(slab=_FAKE, stride=720, n_obs=_FAKE, n=0)
  f.update(over)
  return _abi.BleGpBelief(**f)


def _hist(null=None):
  h = _abi.BleGpHistoryF32()
  for name, ct in (('xyp', ctypes.c_float), ('elapsed_s', ctypes.c_int32), ('err_uv', ctypes.c_float), ('count', ctypes.c_int32)):
    if name != null:
      setattr(h, name, ctypes.cast(ctypes.c_void_p(_FAKE), ctypes.POINTER(ct)))
  return h


def _ref(x):
  return None if x is None else ctypes.byref(x)


def _fit(hist, time_s, belief):
  return _lib.lib().ble_gp_fit_f32(_ref(hist), None, time_s, _ref(belief), None, None)


def _wind(belief, null=None):
  args = [None if k == null else _FAKE for k in ('x', 'y', 'pressure', 'elapsed_s', 'uv')]
  return _lib.lib().ble_gp_belief_wind_f32(_ref(belief), *args, None)


def _rollout(st, ro, belief):
  return _lib.lib().ble_rollout_belief_f32(_ref(st), _ref(ro), _ref(belief), None, None)


def test_declared_exported_and_mirrored():
  header = _header()
  assert re.search(r'\bint ble_gp_fit_f32\(const ble_gp_history_f32\* hist, const uint8_t\* reset_mask, const int32_t\* time_s, '
                   r'const ble_gp_belief\* belief,', header)
  assert re.search(r'\bint ble_gp_belief_wind_f32\(const ble_gp_belief\* belief, const float\* x_m, const float\* y_m, const float\* pressure, '
                   r'const int32_t\* elapsed_s,', header)
  assert re.search(r'\bint ble_rollout_belief_f32\(const ble_state_f32\* st, const struct ble_rollout_f32\* ro, const ble_gp_belief\* belief, '
                   r'uint32_t\* err_flags,', header)
  assert re.search(r'#define BLE_GP_BELIEF_DOUBLES 720\b', header) and _abi.GP_BELIEF_DOUBLES == 720 == _lib.GP_BELIEF_DOUBLES
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header) and _lib.ABI_VERSION == 5            # additive: the ABI stays 5
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  for name in ENTRIES:
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS, name
    assert re.search(r' T ' + name + r'$', symbols, re.M), name
    assert getattr(_lib.lib(), name).argtypes is not None and getattr(_lib.lib(), name).restype is ctypes.c_int
  assert any(s.endswith('ble_gp_belief.h') for s in _lib._SOURCES)
  for name in ENTRIES:          # sizes travel in the structs
    assert ctypes.c_int64 not in getattr(_lib.lib(), name).argtypes, name


def test_struct_layout_matches_the_header():
  body = re.search(r'typedef struct ble_gp_belief \{(.*?)\n\} ble_gp_belief;', _header(), re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  declared = [re.search(r'(\w+)\s*$', d).group(1) for d in body.split(';') if d.strip()]
  assert declared == ['slab', 'stride', 'n_obs', 'n'] == [f[0] for f in _abi.BleGpBelief._fields_]
  assert ctypes.sizeof(_abi.BleGpBelief) == 32 and _abi.BleGpBelief.stride.offset == 8 and _abi.BleGpBelief.n_obs.offset == 16
  assert _abi.BleGpBelief.n.offset == 24
  # ble_rollout_f32 travels unchanged
  assert ctypes.sizeof(_abi.BleRolloutF32) == 8 + 4 * 4 + 8 + 2 * 8 + 8 + 4 * 8


def test_empty_batch_is_ok_without_a_launch():
  assert _fit(_hist(), _FAKE, _belief()) == _lib.BLE_OK
  assert _fit(_hist(), _FAKE, _belief(stride=722)) == _lib.BLE_OK
  assert _wind(_belief()) == _lib.BLE_OK
  assert _rollout(_state(), _ro(), _belief()) == _lib.BLE_OK
  assert _rollout(_state(), _ro(reward=_FAKE, final_state=_FAKE, grid_env_stride=79380), _belief(stride=7620)) == _lib.BLE_OK
  assert _rollout(_state(_abi.vehicle_full(envelope_mass=70.0)), _ro(), _belief()) == _lib.BLE_OK


_BAD_BELIEFS = {
    'null_belief': lambda n: None,
    'null_slab': lambda n: _belief(n=n, slab=None),
    'null_n_obs': lambda n: _belief(n=n, n_obs=None),
    'stride_719': lambda n: _belief(n=n, stride=719),
    'stride_721': lambda n: _belief(n=n, stride=721),
    'stride_0': lambda n: _belief(n=n, stride=0),
    'slab_misaligned': lambda n: _belief(n=n, slab=_FAKE + 8),
}

_CASES = {
    # ---- ble_gp_fit_f32
    **{f'fit_{k}': (lambda n, k=k: _fit(_hist(), _FAKE, _BAD_BELIEFS[k](n))) for k in _BAD_BELIEFS},
    'fit_null_hist': lambda n: _fit(None, _FAKE, _belief(n=n)),
    **{f'fit_null_ring_{f}': (lambda n, f=f: _fit(_hist(null=f), _FAKE, _belief(n=n))) for f in ('xyp', 'elapsed_s', 'err_uv', 'count')},
    'fit_null_time_s': lambda n: _fit(_hist(), None, _belief(n=n)),
    'fit_negative_n': lambda n: _fit(_hist(), _FAKE, _belief(n=-1)),
    'fit_n_2_31': lambda n: _fit(_hist(), _FAKE, _belief(n=2 ** 31)),
    # ---- ble_gp_belief_wind_f32
    **{f'wind_{k}': (lambda n, k=k: _wind(_BAD_BELIEFS[k](n))) for k in _BAD_BELIEFS},
    **{f'wind_null_{f}': (lambda n, f=f: _wind(_belief(n=n), null=f)) for f in ('x', 'y', 'pressure', 'elapsed_s', 'uv')},
    'wind_negative_n': lambda n: _wind(_belief(n=-1)),
    'wind_n_2_31': lambda n: _wind(_belief(n=2 ** 31)),
    # ---- ble_rollout_belief_f32: the belief's cases, then ble_rollout_f32's own through the new entry
    **{f'rollout_{k}': (lambda n, k=k: _rollout(_state(), _ro(n=n), _BAD_BELIEFS[k](n))) for k in _BAD_BELIEFS},
    'rollout_null_st': lambda n: _rollout(None, _ro(n=n), _belief(n=n)),
    **{f'rollout_null_state_{f}': (lambda n, f=f: _rollout(_state(null=f), _ro(n=n), _belief(n=n))) for f in ('x', 'start_unix', 'power_paused')},
    'rollout_null_ro': lambda n: _rollout(_state(), None, _belief()),
    **{f'rollout_null_{f}': (lambda n, f=f: _rollout(_state(), _ro(n=n, **{f: None}), _belief(n=n))) for f in ('plans', 'wind_grid', 'ret', 'steps_flown')},
    'rollout_negative_n': lambda n: _rollout(_state(), _ro(n=-1), _belief(n=-1)),
    'rollout_belief_of_another_batch': lambda n: _rollout(_state(), _ro(n=n), _belief(n=n + 1)),
    'rollout_plans_0': lambda n: _rollout(_state(), _ro(n=n, n_plans=0), _belief(n=n)),
    'rollout_plan_steps_0': lambda n: _rollout(_state(), _ro(n=n, n_plan_steps=0), _belief(n=n)),
    'rollout_repeat_0': lambda n: _rollout(_state(), _ro(n=n, action_repeat=0), _belief(n=n)),
    'rollout_steps_961': lambda n: _rollout(_state(), _ro(n=n, n_plan_steps=961), _belief(n=n)),
    'rollout_steps_times_repeat_wraps_int32': lambda n: _rollout(_state(), _ro(n=n, n_plan_steps=2 ** 16, action_repeat=2 ** 16), _belief(n=n)),
    'rollout_n_times_k_2_31': lambda n: _rollout(_state(), _ro(n=2 ** 20, n_plans=2 ** 11), _belief(n=2 ** 20)),
    'rollout_n_2_31': lambda n: _rollout(_state(), _ro(n=2 ** 31, n_plans=1), _belief(n=2 ** 31)),
    'rollout_substeps_0': lambda n: _rollout(_state(), _ro(n=n, substeps=0), _belief(n=n)),
    'rollout_substeps_max_plus_1': lambda n: _rollout(_state(), _ro(n=n, substeps=MAX_SUBSTEPS + 1), _belief(n=n)),
    'rollout_negative_stride': lambda n: _rollout(_state(), _ro(n=n, grid_env_stride=-1), _belief(n=n)),
    'rollout_gamma_nan': lambda n: _rollout(_state(), _ro(n=n, gamma=float('nan')), _belief(n=n)),
    'rollout_gamma_above_1': lambda n: _rollout(_state(), _ro(n=n, gamma=1.0000001), _belief(n=n)),
    'rollout_bad_vehicle': lambda n: _rollout(_state(_abi.vehicle_full(envelope_volume_base=-1.0)), _ro(n=n), _belief(n=n)),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG


def test_python_signatures():
  from balloon_learning_environment_amd import vec_state
  from balloon_learning_environment_amd.env import balloon_arena, balloon_env
  p = inspect.signature(vec_state.VecSimulator.rollout_plans).parameters
  assert list(p)[-1] == 'belief' and p['belief'].default is None
  assert list(p)[:9] == ['self', 'plans', 'gamma', 'action_repeat', 'noise_seed', 'substeps', 'want_rewards', 'want_final', 'out']
  assert inspect.signature(balloon_env.VecBalloonEnv.lookahead).parameters['wind'].default == 'truth'
  assert vec_state.WindBelief._fields == ('slab', 'n_obs')
  p = inspect.signature(vec_state.VecSimulator.fit_wind_belief).parameters
  assert list(p) == ['self', 'time_s', 'out'] and p['time_s'].default is None and p['out'].default is None
  p = inspect.signature(vec_state.VecSimulator.belief_wind).parameters
  assert list(p) == ['self', 'belief', 'x', 'y', 'pressure', 'elapsed_s', 'out'] and all(p[k].default is None for k in list(p)[2:])
  for name in ('fit_wind_belief', 'belief_wind'):
    assert callable(getattr(balloon_arena.VecBalloonArena, name))
  p = inspect.signature(balloon_arena.VecBalloonArena.lookahead).parameters
  assert list(p)[-1] == 'belief' and p['belief'].default is None


# ---------------------------------------------------------------------------------------------- the lane function on the host
SIZES = (1, 2, 17, 64, 120)
N_WINDOWS, N_POINTS = 40, 32


def _window(rng, m):
  """m observations, float32 values as the ring holds them: (loc [m, 4] float64: x, y, p, t; err [m, 2] float64)."""
  xyp = np.column_stack([rng.uniform(-2.0e5, 2.0e5, m), rng.uniform(-2.0e5, 2.0e5, m), rng.uniform(5000.0, 14000.0, m)]).astype(np.float32)
  t = (180 * np.arange(m)).astype(np.int32)
  err = rng.normal(0.0, 2.0, (m, 2)).astype(np.float32)
  return np.column_stack([xyp.astype(np.float64), t.astype(np.float64)]), err.astype(np.float64)


def _alpha(loc, err):
  k = wind_gp_host._kernel(loc, loc)
  k[np.diag_indices_from(k)] += wind_gp_host._SIGMA_NOISE_SQUARED
  return scipy.linalg.cho_solve((scipy.linalg.cholesky(k, lower=True), True), err)


def test_lane_function_against_numpy():
  from emul import belief_emul
  rng = np.random.default_rng(2026)
  worst = 0.0
  for w in range(N_WINDOWS):
    m = SIZES[w % len(SIZES)]
    loc, err = _window(rng, m)
    alpha = _alpha(loc, err)
    anchor = int(loc[-1, 3])
    pts = np.column_stack([rng.uniform(-2.5e5, 2.5e5, N_POINTS), rng.uniform(-2.5e5, 2.5e5, N_POINTS),
                           rng.uniform(4000.0, 15000.0, N_POINTS)]).astype(np.float32)
    t = rng.integers(anchor - 3600, anchor + 12 * 3600 + 1, N_POINTS).astype(np.int32)
    t[0], t[1], t[2] = anchor - 3600, anchor, anchor + 12 * 3600
    slab = belief_emul.pack(loc, alpha)
    got = belief_emul.mean(slab, m, pts, t).astype(np.float64)
    want = wind_gp_host._kernel(np.column_stack([pts.astype(np.float64), t.astype(np.float64)]), loc) @ alpha
    e = float(np.max(np.abs(got - want)))
    worst = max(worst, e)
    assert np.isfinite(got).all() and e <= TOL, (w, m, e)
    # the zero padding: a longer loop gives the same bits
    assert np.array_equal(belief_emul.mean(slab, m, pts, t, n_trip=120).view(np.uint32), got.astype(np.float32).view(np.uint32)), (w, m)
  print(f'gp_belief_mean on the host: max |lane function - NumPy| = {worst:.3e} m/s over {N_WINDOWS} windows x {N_POINTS} points')


def test_lane_function_without_a_posterior():
  from emul import belief_emul
  rng = np.random.default_rng(7)
  loc, err = _window(rng, 17)
  slab = belief_emul.pack(loc, _alpha(loc, err))
  pts = np.array([[1.0e4, -2.0e4, 9000.0], [np.nan, 0.0, 9000.0]], np.float32)
  t = np.array([600, 600], np.int32)
  zero = belief_emul.mean(np.zeros_like(slab), 0, pts, t, n_trip=120)
  assert np.array_equal(zero.view(np.uint32), np.zeros((2, 2), np.uint32))          # exactly +0.0f, whatever the point and the loop
  assert np.isnan(belief_emul.mean(np.zeros_like(slab), -1, pts, t)).all()
  assert np.isfinite(belief_emul.mean(slab, 17, pts[:1], t[:1])).all() and np.isnan(belief_emul.mean(slab, 17, pts[1:], t[1:])).all()
