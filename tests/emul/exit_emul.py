"""ctypes loader for tests/emul/libexit_emul.so: the host build of the expert-iteration lane functions of csrc/ble_plan.h
(exit_emul.cpp).

TEST TOOLING ONLY, next to plan_emul.py and with its compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libexit_emul.so')
_vp = ctypes.c_void_p


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'exit_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h'), os.path.join(csrc, 'ble_plan.h'),
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
    _lib.emul_plan_prior.argtypes = [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]
    _lib.emul_plan_sample_prior.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_int] * 4 + [_vp] * 4
    _lib.emul_plan_action_values.argtypes = [ctypes.c_int, ctypes.c_int] + [_vp] * 5
    _lib.emul_plan_prior.restype = _lib.emul_plan_sample_prior.restype = _lib.emul_plan_action_values.restype = None
  return _lib


def prior_counts(probs, strength, segments):
  """uint16 [n, segments, 3] of probs float32 [n, 3]."""
  probs = np.ascontiguousarray(probs, np.float32)
  n = len(probs)
  counts = np.zeros((n, segments, 3), np.uint16)
  lib().emul_plan_prior(probs.ctypes.data, int(strength), int(segments), n, counts.ctypes.data)
  return counts


def sample_prior(seed, key, decision, iteration, n_plans, n_entries, segment, prior, counts=None, prev=None):
  """The K plans of one environment: uint8 [H, K].  prior: uint16 [segments, 3]; counts (iteration > 0) and prev as plan_emul.sample."""
  plans = np.empty((n_entries, n_plans), np.uint8)
  prior = np.ascontiguousarray(prior, np.uint16)
  counts = None if counts is None else np.ascontiguousarray(counts, np.uint16)
  prev = None if prev is None else np.ascontiguousarray(prev, np.uint8)
  lib().emul_plan_sample_prior(int(seed) & (2 ** 64 - 1), int(key), int(decision) & (2 ** 64 - 1), iteration, n_plans, n_entries, segment,
                               None if counts is None else counts.ctypes.data, prior.ctypes.data,
                               None if prev is None else prev.ctypes.data, plans.ctypes.data)
  return plans


def action_values(ret, first, stored=None):
  """One environment: ret float32 [K], first uint8 [K]; stored = (q [3], q_k [3], visits [3]) to accumulate into, or None.
  -> (q float32 [3], q_k int32 [3], visits int32 [3])."""
  ret = np.ascontiguousarray(ret, np.float32)
  first = np.ascontiguousarray(first, np.uint8)
  if stored is None:
    q, q_k, visits = np.zeros(3, np.float32), np.zeros(3, np.int32), np.zeros(3, np.int32)
  else:
    q, q_k, visits = (np.array(stored[0], np.float32), np.array(stored[1], np.int32), np.array(stored[2], np.int32))
  lib().emul_plan_action_values(len(ret), 0 if stored is None else 1, ret.ctypes.data, first.ctypes.data, q.ctypes.data, q_k.ctypes.data,
                                visits.ctypes.data)
  return q, q_k, visits
