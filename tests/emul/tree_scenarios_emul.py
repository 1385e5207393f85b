"""ctypes loader for tests/emul/libtree_scenarios_emul.so: the host build of csrc/ble_tree_scenarios.h's lane function and of one level's
risk -> select (tree_scenarios_emul.cpp).

TEST TOOLING ONLY, next to tree_emul.py and scenario_emul.py and with their compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libtree_scenarios_emul.so')
_vp, _int = ctypes.c_void_p, ctypes.c_int
FLY, CARRY, VOID = 0, 1, 2


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'tree_scenarios_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h')] + [
      os.path.join(csrc, f) for f in ('ble_tree_scenarios.h', 'ble_tree.h', 'ble_plan.h', 'ble_scenarios.h', 'ble_gp_belief.h', 'ble_noise.h',
                                      'ble_reset.h', 'ble_physics.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', os.path.join(_HERE, 'ble_intrinsics.h'),
                           '-o', _SO, srcs[0]])
  return _SO


_lib = None


def lib():
  global _lib
  if _lib is None:
    _lib = ctypes.CDLL(build())
    _lib.emul_tree_scenario_lane.argtypes = [_vp, _vp, _int, _int, _int]
    _lib.emul_tree_scenario_lane.restype = _int
    _lib.emul_tree_scenarios_level.argtypes = [_int] * 4 + [_vp] * 4
    _lib.emul_tree_scenarios_level.restype = None
  return _lib


def lane(status, acc, m, act):
  """The parent group's status [M] uint8 and acc [M] float64 (None: level 1, status[0] the environment's byte) -> FLY, CARRY or VOID."""
  status = np.ascontiguousarray(status, np.uint8)
  if acc is None:
    return lib().emul_tree_scenario_lane(status.ctypes.data, None, 0, m, act)
  acc = np.ascontiguousarray(acc, np.float64)
  assert len(acc) == len(status)
  return lib().emul_tree_scenario_lane(status.ctypes.data, acc.ctypes.data, len(status), m, act)


def level(ret, tail, beam):
  """One environment: ret [C, M] float32 -> (score [C] float32, parent, choice: int32 [min(C, beam)] each)."""
  ret = np.ascontiguousarray(ret, np.float32)
  C, num = ret.shape
  score = np.zeros(C, np.float32)
  parent, choice = np.full(beam, -7, np.int32), np.full(beam, -7, np.int32)
  lib().emul_tree_scenarios_level(C, num, tail, beam, ret.ctypes.data, score.ctypes.data, parent.ctypes.data, choice.ctypes.data)
  keep = min(C, beam)
  assert np.all(parent[keep:] == -7) and np.all(choice[keep:] == -7)
  return score, parent[:keep], choice[:keep]
