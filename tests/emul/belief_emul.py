"""ctypes loader for tests/emul/libbelief_emul.so: the host build of csrc/ble_gp_belief.h's lane function (belief_emul.cpp).

TEST TOOLING ONLY, next to emul.py and with its compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libbelief_emul.so')
_vp = ctypes.c_void_p


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'belief_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h'), os.path.join(csrc, 'ble_gp_belief.h'),
          os.path.join(csrc, 'ble_physics.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', os.path.join(_HERE, 'ble_intrinsics.h'),
                           '-o', _SO, srcs[0]])
  return _SO


_lib = None


def lib():
  global _lib
  if _lib is None:
    _lib = ctypes.CDLL(build())
    _lib.emul_belief_pack.argtypes = [ctypes.c_int, _vp, _vp, _vp]
    _lib.emul_belief_mean.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, _vp, _vp, _vp, _vp, _vp]
    _lib.emul_belief_pack.restype = _lib.emul_belief_mean.restype = None
  return _lib


def pack(loc, alpha):
  """loc [m, 4] (x m, y m, pressure Pa, t s), alpha [m, 2] -> the slab (float64 array) of that window."""
  loc, alpha = np.ascontiguousarray(loc, np.float64), np.ascontiguousarray(alpha, np.float64)
  slab = np.empty(lib().emul_belief_doubles(), np.float64)
  lib().emul_belief_pack(len(loc), loc.ctypes.data, alpha.ctypes.data, slab.ctypes.data)
  return slab


def mean(slab, n_obs, points, t, n_trip=-1):
  """gp_belief_mean at points [q, 3] float32 and times t [q] int32: [q, 2] float32."""
  points = np.asarray(points, np.float32)
  x, y, p = (np.ascontiguousarray(points[:, k]) for k in range(3))
  t = np.ascontiguousarray(t, np.int32)
  uv = np.empty((len(t), 2), np.float32)
  slab = np.ascontiguousarray(slab, np.float64)
  lib().emul_belief_mean(slab.ctypes.data, int(n_obs), int(n_trip), len(t), x.ctypes.data, y.ctypes.data, p.ctypes.data, t.ctypes.data,
                         uv.ctypes.data)
  return uv
