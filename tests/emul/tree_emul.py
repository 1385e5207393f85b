"""ctypes loader for tests/emul/libtree_emul.so: the host build of csrc/ble_tree.h's select and finish lane functions (tree_emul.cpp).

TEST TOOLING ONLY, next to plan_emul.py and with its compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libtree_emul.so')
_vp = ctypes.c_void_p


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'tree_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h'), os.path.join(csrc, 'ble_tree.h'),
          os.path.join(csrc, 'ble_plan.h'), os.path.join(csrc, 'ble_reset.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', os.path.join(_HERE, 'ble_intrinsics.h'),
                           '-o', _SO, srcs[0]])
  return _SO


_lib = None


def lib():
  global _lib
  if _lib is None:
    _lib = ctypes.CDLL(build())
    _lib.emul_tree_select.argtypes = [ctypes.c_int] * 2 + [_vp] * 3
    _lib.emul_tree_finish.argtypes = [ctypes.c_int] * 4 + [_vp, _vp, ctypes.c_int] + [_vp] * 6
    _lib.emul_tree_select.restype = _lib.emul_tree_finish.restype = None
  return _lib


def select(ret, beam):
  """One environment: ret [C] float32 -> (parent, choice), int32 [min(C, beam)] each (the slots beyond are not written)."""
  ret = np.ascontiguousarray(ret, np.float32)
  parent, choice = np.full(beam, -7, np.int32), np.full(beam, -7, np.int32)
  lib().emul_tree_select(len(ret), beam, ret.ctypes.data, parent.ctypes.data, choice.ctypes.data)
  keep = min(len(ret), beam)
  assert np.all(parent[keep:] == -7) and np.all(choice[keep:] == -7)
  return parent[:keep], choice[:keep]


def finish(ret, choice, depth, segment, beam, source_ok=True, score=None, want_q=True):
  """One environment: ret [C], score [C] or None, choice int32 [depth, beam] -> (best_plan [depth * segment], action, best_return, q [3]
  or None, visits [3] or None)."""
  ret = np.ascontiguousarray(ret, np.float32)
  score = ret if score is None else np.ascontiguousarray(score, np.float32)
  choice = np.ascontiguousarray(choice, np.int32)
  assert choice.shape == (depth, beam)
  best_plan, action, best_return = np.zeros(depth * segment, np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.float32)
  q, visits = (np.zeros(3, np.float32), np.zeros(3, np.int32)) if want_q else (None, None)
  lib().emul_tree_finish(len(ret), beam, depth, segment, ret.ctypes.data, score.ctypes.data, 1 if source_ok else 0, choice.ctypes.data,
                         best_plan.ctypes.data, action.ctypes.data, best_return.ctypes.data, None if q is None else q.ctypes.data,
                         None if visits is None else visits.ctypes.data)
  return best_plan, int(action[0]), best_return[0], q, visits
