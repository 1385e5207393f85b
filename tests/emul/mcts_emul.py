"""ctypes loader for tests/emul/libmcts_emul.so: the host build of csrc/ble_mcts.h's select, backup and finish lane functions
(mcts_emul.cpp), one environment at a time.

TEST TOOLING ONLY, next to tree_emul.py and with its compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libmcts_emul.so')
_vp = ctypes.c_void_p


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'mcts_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h'), os.path.join(csrc, 'ble_mcts.h'),
          os.path.join(csrc, 'ble_tree.h'), os.path.join(csrc, 'ble_plan.h'), os.path.join(csrc, 'ble_reset.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', os.path.join(_HERE, 'ble_intrinsics.h'),
                           '-o', _SO, srcs[0]])
  return _SO


class _Stats(ctypes.Structure):
  _fields_ = [(name, _vp) for name in ('parent', 'first_child', 'depth', 'visits', 'pending', 'value_sum', 'g', 'prior', 'g_range')]


_lib = None


def lib():
  global _lib
  if _lib is None:
    _lib = ctypes.CDLL(build())
    i, d = ctypes.c_int, ctypes.c_double
    _lib.emul_mcts_select.argtypes = [ctypes.POINTER(_Stats), i, i, i, d, i, _vp, _vp, _vp, _vp]
    _lib.emul_mcts_backup.argtypes = [ctypes.POINTER(_Stats), i, i, i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    _lib.emul_mcts_finish.argtypes = [ctypes.POINTER(_Stats), i, i, i, i, i] + [_vp] * 6
    _lib.emul_mcts_score.argtypes = [d, i, i, d, d, d, ctypes.c_float, i]
    _lib.emul_mcts_select.restype = _lib.emul_mcts_backup.restype = _lib.emul_mcts_finish.restype = None
    _lib.emul_mcts_score.restype = d
  return _lib


def score(value_sum, visits, pending, g_lo, g_hi, c_puct, prior, nv_node):
  return lib().emul_mcts_score(value_sum, visits, pending, g_lo, g_hi, c_puct, prior, nv_node)


class Pool:
  """One environment's pool as the device keeps it: the statistics [cap], the nodes' acc, disc, status [R, 3L], the slots [L].
  Every array starts as garbage a search must not read (0x5A bytes): what a round reads, an earlier call has written."""

  def __init__(self, rounds, leaves, max_depth, c_puct, source_status=0, root_prior=None):
    self.R, self.L, self.D, self.c, self.source_status = int(rounds), int(leaves), int(max_depth), float(c_puct), int(source_status)
    cap = self.cap = 1 + 3 * self.L * self.R

    def junk(shape, dtype):
      return np.frombuffer(b'\x5a' * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype).reshape(shape).copy()
    self.parent, self.first_child, self.depth, self.visits, self.pending = (junk(cap, np.int32) for _ in range(5))
    self.value_sum, self.g = junk(cap, np.float64), junk(cap, np.float64)
    self.prior, self.g_range = junk((cap, 3), np.float32), junk(2, np.float64)
    self.acc, self.disc = junk((self.R, 3 * self.L), np.float64), junk((self.R, 3 * self.L), np.float64)
    self.status = junk((self.R, 3 * self.L), np.uint8)
    self.leaf, self.kind = junk(self.L, np.int32), junk(self.L, np.int32)
    self.root_prior = None if root_prior is None else np.ascontiguousarray(root_prior, np.float32)
    self._stats = _Stats(*(a.ctypes.data for a in (self.parent, self.first_child, self.depth, self.visits, self.pending, self.value_sum,
                                                    self.g, self.prior, self.g_range)))

  def select(self, r):
    lib().emul_mcts_select(ctypes.byref(self._stats), r, self.L, self.D, self.c, self.source_status, self.status.ctypes.data,
                           None if self.root_prior is None else self.root_prior.ctypes.data, self.leaf.ctypes.data, self.kind.ctypes.data)
    return self.leaf.copy(), self.kind.copy()

  def backup(self, r, acc, disc, status, value=None, probs=None):
    """The round's 3L nodes as the expansion stored them, then the backup."""
    self.acc[r], self.disc[r], self.status[r] = acc, disc, status
    value = None if value is None else np.ascontiguousarray(value, np.float32)
    probs = None if probs is None else np.ascontiguousarray(probs, np.float32)
    lib().emul_mcts_backup(ctypes.byref(self._stats), r, self.L, self.D, self.acc.ctypes.data, self.disc.ctypes.data, self.status.ctypes.data,
                           None if value is None else value.ctypes.data, None if probs is None else probs.ctypes.data,
                           self.leaf.ctypes.data, self.kind.ctypes.data)

  def finish(self, segment):
    best_plan, action, best_return = np.zeros(self.D * segment, np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.float32)
    q, visits, length = np.zeros(3, np.float32), np.zeros(3, np.int32), np.zeros(1, np.int32)
    lib().emul_mcts_finish(ctypes.byref(self._stats), self.R, self.L, self.D, segment, self.source_status, best_plan.ctypes.data,
                           action.ctypes.data, best_return.ctypes.data, q.ctypes.data, visits.ctypes.data, length.ctypes.data)
    return dict(action=int(action[0]), best_return=best_return[0], q=q, visits=visits, best_plan=best_plan, pv_length=int(length[0]))
