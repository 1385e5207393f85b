"""ctypes loader for tests/emul/libes_emul.so: the host build of csrc/ble_population.h's lane functions (es_emul.cpp).

TEST TOOLING ONLY, next to plan_emul.py and with its compiler flags."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, 'libes_emul.so')
_vp = ctypes.c_void_p
_U64 = 2 ** 64 - 1


def build():
  csrc = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
  srcs = [os.path.join(_HERE, 'es_emul.cpp'), os.path.join(_HERE, 'ble_intrinsics.h'), os.path.join(csrc, 'ble_population.h'),
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
    u64, i64, f32 = ctypes.c_uint64, ctypes.c_int64, ctypes.c_float
    _lib.emul_es_address.argtypes = [u64, u64, u64, u64, _vp, _vp]
    _lib.emul_es_noise.argtypes = [u64, u64, ctypes.c_int, i64, i64, _vp]
    _lib.emul_es_perturb.argtypes = [_vp, f32, _vp, i64, _vp, _vp]
    _lib.emul_es_gradient.argtypes = [_vp, _vp, ctypes.c_int, i64, f32, f32, _vp, _vp]
    for f in (_lib.emul_es_address, _lib.emul_es_noise, _lib.emul_es_perturb, _lib.emul_es_gradient):
      f.restype = None
  return _lib


def address(seed, pair, generation, q):
  """-> (key0, key1, c0, c1, c2, c3) uint32 [6], the block's words uint32 [4]."""
  kc, words = np.zeros(6, np.uint32), np.zeros(4, np.uint32)
  lib().emul_es_address(int(seed) & _U64, int(pair), int(generation) & _U64, int(q), kc.ctypes.data, words.ctypes.data)
  return kc, words


def noise(seed, generation, streams, d, q0=0):
  """eps float32 [streams, d]: logical parameters q0 .. q0 + d - 1."""
  eps = np.zeros((streams, d), np.float32)
  lib().emul_es_noise(int(seed) & _U64, int(generation) & _U64, streams, q0, d, eps.ctypes.data)
  return eps


def perturb(theta, sigma, eps):
  theta, eps = np.ascontiguousarray(theta, np.float32), np.ascontiguousarray(eps, np.float32)
  plus, minus = np.zeros_like(theta), np.zeros_like(theta)
  lib().emul_es_perturb(theta.ctypes.data, float(sigma), eps.ctypes.data, theta.size, plus.ctypes.data, minus.ctypes.data)
  return plus, minus


def gradient(w, eps, sigma, weight_decay, theta):
  w, eps, theta = (np.ascontiguousarray(a, np.float32) for a in (w, eps, theta))
  grad = np.zeros(theta.size, np.float32)
  lib().emul_es_gradient(w.ctypes.data, eps.ctypes.data, eps.shape[0], eps.shape[1], float(sigma), float(weight_decay), theta.ctypes.data,
                         grad.ctypes.data)
  return grad
