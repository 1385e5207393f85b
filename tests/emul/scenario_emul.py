"""ctypes loader for tests/emul/libscenario_emul.so: the host build of csrc/ble_scenarios.h's lane functions (scenario_emul.cpp).

TEST TOOLING ONLY, next to plan_emul.py and belief_emul.py and with their compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libscenario_emul.so')
_vp = ctypes.c_void_p
_u64, _u32, _int, _ll = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_longlong
M64 = 2 ** 64 - 1


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'scenario_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h')] + [
      os.path.join(csrc, f) for f in ('ble_scenarios.h', 'ble_gp_belief.h', 'ble_noise.h', 'ble_reset.h', 'ble_physics.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', os.path.join(_HERE, 'ble_intrinsics.h'),
                           '-o', _SO, srcs[0]])
  return _SO


_lib = None


def lib():
  global _lib
  if _lib is None:
    _lib = ctypes.CDLL(build())
    _lib.emul_scenario_draws.argtypes = [_u64, _u64, _u32, _int, _vp]
    _lib.emul_scenario_harmonic.argtypes = [_u64, _u64, _u32, _int, _int, _vp]
    _lib.emul_truth_draws.argtypes = [_u64, _u64, _u32, _vp]
    _lib.emul_risk_ranks.argtypes = [_vp, _int]
    _lib.emul_risk_ranks.restype = _u64
    _lib.emul_risk_score.argtypes = [_vp, _int, _int]
    _lib.emul_risk_score.restype = ctypes.c_float
    _lib.emul_scenario_prior.argtypes = [_vp, _ll] + [_vp] * 6
    _lib.emul_scenario_correction.argtypes = [_vp, _int, _int, _int, _ll] + [_vp] * 5
    for f in (_lib.emul_scenario_draws, _lib.emul_scenario_harmonic, _lib.emul_truth_draws, _lib.emul_scenario_prior,
              _lib.emul_scenario_correction):
      f.restype = None
  return _lib


def draws(seed, key, episode, m):
  """The 50 harmonic words of scenario m: uint32 [10, 5] = (seed, ox, oy, op, ot bits) of harmonic k = 5 comp + h."""
  out = np.empty(50, np.uint32)
  lib().emul_scenario_draws(int(seed) & M64, int(key), int(episode), int(m), out.ctypes.data)
  return out.reshape(10, 5)


def harmonic(seed, key, episode, m, k):
  out = np.empty(5, np.uint32)
  lib().emul_scenario_harmonic(int(seed) & M64, int(key), int(episode), int(m), int(k), out.ctypes.data)
  return out


def truth_draws(seed, key, episode):
  out = np.empty(50, np.uint32)
  lib().emul_truth_draws(int(seed) & M64, int(key), int(episode), out.ctypes.data)
  return out.reshape(10, 5)


def risk_ranks(ret):
  """The rank of every scenario return: int [M]."""
  ret = np.ascontiguousarray(ret, np.float32)
  word = int(lib().emul_risk_ranks(ret.ctypes.data, len(ret)))
  return np.array([(word >> (4 * m)) & 15 for m in range(len(ret))])


def risk_score(ret, tail):
  ret = np.ascontiguousarray(ret, np.float32)
  return np.float32(lib().emul_risk_score(ret.ctypes.data, len(ret), int(tail)))


def _points(x, y, p, t):
  return (np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32), np.ascontiguousarray(p, np.float32),
          np.ascontiguousarray(t, np.int32))


def prior(words, x, y, p, t):
  """f_m at the points from the 50 words: (uv [q, 2] float32 by wind_noise_from_rows, the same component by component)."""
  words = np.ascontiguousarray(np.asarray(words, np.uint32).reshape(50))
  x, y, p, t = _points(x, y, p, t)
  uv, by = np.empty((len(x), 2), np.float32), np.empty((len(x), 2), np.float32)
  lib().emul_scenario_prior(words.ctypes.data, len(x), x.ctypes.data, y.ctypes.data, p.ctypes.data, t.ctypes.data, uv.ctypes.data, by.ctypes.data)
  return uv, by


def correction(slab, num, m, n_obs, x, y, p, t):
  slab = np.ascontiguousarray(slab, np.float64)
  assert slab.size >= 480 + 240 * num
  x, y, p, t = _points(x, y, p, t)
  uv = np.empty((len(x), 2), np.float32)
  lib().emul_scenario_correction(slab.ctypes.data, num, m, n_obs, len(x), x.ctypes.data, y.ctypes.data, p.ctypes.data, t.ctypes.data, uv.ctypes.data)
  return uv
