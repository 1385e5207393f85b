"""ctypes loader for tests/emul/libplan_emul.so: the host build of csrc/ble_plan.h's lane functions (plan_emul.cpp).

TEST TOOLING ONLY, next to belief_emul.py and with its compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libplan_emul.so')
_vp = ctypes.c_void_p


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'plan_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h'), os.path.join(csrc, 'ble_plan.h'),
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
    _lib.emul_plan_sample.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_int] * 4 + [_vp, _vp, _vp]
    _lib.emul_plan_draw.argtypes = [ctypes.c_uint32] + [ctypes.c_int] * 3
    _lib.emul_plan_select.argtypes = [ctypes.c_int] * 5 + [_vp] * 7
    _lib.emul_plan_sample.restype = _lib.emul_plan_select.restype = None
    _lib.emul_plan_draw.restype = ctypes.c_int
  return _lib


def sample(seed, key, decision, iteration, n_plans, n_entries, segment, counts=None, prev=None):
  """The K plans of one environment: uint8 [H, K].  counts: uint16 [segments, 3] (iteration > 0); prev: uint8 [H] or None (all STAY)."""
  plans = np.empty((n_entries, n_plans), np.uint8)
  counts = None if counts is None else np.ascontiguousarray(counts, np.uint16)
  prev = None if prev is None else np.ascontiguousarray(prev, np.uint8)
  lib().emul_plan_sample(int(seed) & (2 ** 64 - 1), int(key), int(decision) & (2 ** 64 - 1), iteration, n_plans, n_entries, segment,
                         None if counts is None else counts.ctypes.data, None if prev is None else prev.ctypes.data, plans.ctypes.data)
  return plans


def draw(word, c0, c1, c2):
  return lib().emul_plan_draw(int(word), c0, c1, c2)


def select(ret, plans, iteration, elite, segment, best_return=None, best_plan=None):
  """One environment: ret [K] float32, plans uint8 [H, K]; the incumbent (iteration > 0): best_return, best_plan [H].
  -> (best_return, best_k, best_plan [H], action, counts [segments, 3] or None)."""
  ret = np.ascontiguousarray(ret, np.float32)
  plans = np.ascontiguousarray(plans, np.uint8)
  h, k = plans.shape
  br = np.array([0.0 if best_return is None else best_return], np.float32)
  bk = np.zeros(1, np.int32)
  bp = np.zeros(h, np.uint8) if best_plan is None else np.array(best_plan, np.uint8)
  act = np.zeros(1, np.uint8)
  counts = np.zeros((-(-h // segment), 3), np.uint16)
  lib().emul_plan_select(k, h, segment, iteration, elite, ret.ctypes.data, plans.ctypes.data, br.ctypes.data, bk.ctypes.data, bp.ctypes.data,
                         act.ctypes.data, counts.ctypes.data)
  return br[0], int(bk[0]), bp, int(act[0]), (counts if elite >= 1 else None)
