"""ctypes loader for tests/emul/libmcts_scenarios_emul.so: the host build of csrc/ble_mcts_scenarios.h's group functions
(mcts_scenarios_emul.cpp), one environment at a time.  Select and finish are mcts_emul.Pool's, fed the groups' status.

TEST TOOLING ONLY, next to mcts_emul.py and with its compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

from emul import mcts_emul

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libmcts_scenarios_emul.so')
_vp = ctypes.c_void_p


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'mcts_scenarios_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h')] + [
      os.path.join(csrc, f) for f in ('ble_mcts_scenarios.h', 'ble_mcts.h', 'ble_tree_scenarios.h', 'ble_tree.h', 'ble_plan.h', 'ble_scenarios.h',
                                      'ble_gp_belief.h', 'ble_noise.h', 'ble_reset.h', 'ble_physics.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', os.path.join(_HERE, 'ble_intrinsics.h'),
                           '-o', _SO, srcs[0]])
  return _SO


_lib = None


def lib():
  global _lib
  if _lib is None:
    _lib = ctypes.CDLL(build())
    i = ctypes.c_int
    _lib.emul_mcts_backup_scenarios.argtypes = [ctypes.POINTER(mcts_emul._Stats), i, i, i, i, i] + [_vp] * 9
    _lib.emul_mcts_backup_scenarios.restype = None
    _lib.emul_mcts_group.argtypes = [_vp] * 5 + [i, i, _vp, _vp]
    _lib.emul_mcts_group.restype = ctypes.c_double
    _lib.emul_mcts_lane_rule.argtypes = [_vp, _vp, i, i, i]
    _lib.emul_mcts_lane_rule.restype = i
  return _lib


def group(acc, disc, status, value, probs, tail):
  """The group step on one group's M nodes -> (G, prior [3] f32, spent)."""
  acc, disc = np.ascontiguousarray(acc, np.float64), np.ascontiguousarray(disc, np.float64)
  status = np.ascontiguousarray(status, np.uint8)
  value = None if value is None else np.ascontiguousarray(value, np.float32)
  probs = None if probs is None else np.ascontiguousarray(probs, np.float32)
  prior, spent = np.zeros(3, np.float32), np.zeros(1, np.uint8)
  g = lib().emul_mcts_group(acc.ctypes.data, disc.ctypes.data, status.ctypes.data, None if value is None else value.ctypes.data,
                            None if probs is None else probs.ctypes.data, len(acc), int(tail), prior.ctypes.data, spent.ctypes.data)
  return g, prior, int(spent[0])


def lane_rule(status, acc, m, act):
  status = np.ascontiguousarray(status, np.uint8)
  acc = None if acc is None else np.ascontiguousarray(acc, np.float64)
  return lib().emul_mcts_lane_rule(status.ctypes.data, None if acc is None else acc.ctypes.data, len(status), int(m), int(act))


class Pool(mcts_emul.Pool):
  """One environment's pool of groups as the device keeps it: mcts_emul.Pool's statistics and slots; `status` [R, 3L] is the GROUPS'
  (what select and finish read), the nodes' acc, disc, node_status are [R, 3L, M], group_g [R, 3L].  Garbage until written."""

  def __init__(self, rounds, leaves, max_depth, c_puct, num, tail, source_status=0, root_prior=None):
    super().__init__(rounds, leaves, max_depth, c_puct, source_status, root_prior)
    self.M, self.tail = int(num), int(tail)
    shape = (self.R, 3 * self.L, self.M)
    junk = lambda shape, dtype: np.frombuffer(b'\x5a' * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()
    self.acc, self.disc, self.node_status = junk(shape, np.float64), junk(shape, np.float64), junk(shape, np.uint8)
    self.group_g = junk(shape[:2], np.float64)

  def backup(self, r, acc, disc, status, value=None, probs=None):
    """The round's 3L M nodes as the expansion stored them ([3L, M]; value [3L, M], probs [3L, M, 3]), then the backup of groups."""
    self.acc[r], self.disc[r], self.node_status[r] = acc, disc, status
    value = None if value is None else np.ascontiguousarray(value, np.float32)
    probs = None if probs is None else np.ascontiguousarray(probs, np.float32)
    lib().emul_mcts_backup_scenarios(ctypes.byref(self._stats), r, self.L, self.D, self.M, self.tail, self.acc.ctypes.data,
                                     self.disc.ctypes.data, self.node_status.ctypes.data, None if value is None else value.ctypes.data,
                                     None if probs is None else probs.ctypes.data, self.leaf.ctypes.data, self.kind.ctypes.data,
                                     self.status.ctypes.data, self.group_g.ctypes.data)
