"""ctypes loader for tests/emul/libleaves_emul.so: the host build of the bootstrap lane function of csrc/ble_plan.h (leaves_emul.cpp).

TEST TOOLING ONLY, next to exit_emul.py and with its compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libleaves_emul.so')
_vp = ctypes.c_void_p


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'leaves_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h'), os.path.join(csrc, 'ble_plan.h'),
          os.path.join(csrc, 'ble_reset.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', os.path.join(_HERE, 'ble_intrinsics.h'),
                           '-o', _SO, srcs[0]])
  return _SO


_lib = None


def lib():
  global _lib
  if _lib is None:
    _lib = ctypes.CDLL(build())
    _lib.emul_plan_bootstrap.argtypes = [ctypes.c_int, ctypes.c_double] + [_vp] * 5
    _lib.emul_plan_bootstrap.restype = None
  return _lib


def bootstrap(ret, steps_flown, leaf_status, value, gamma):
  """plan_bootstrap_lane over flat arrays: float32 [total]."""
  ret = np.ascontiguousarray(ret, np.float32).ravel()
  steps = np.ascontiguousarray(steps_flown, np.int32).ravel()
  status = np.ascontiguousarray(leaf_status, np.uint8).ravel()
  value = np.ascontiguousarray(value, np.float32).ravel()
  score = np.empty_like(ret)
  lib().emul_plan_bootstrap(ret.size, float(gamma), ret.ctypes.data, steps.ctypes.data, status.ctypes.data, value.ctypes.data, score.ctypes.data)
  return score
