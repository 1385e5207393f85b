"""ctypes loader for tests/emul/libqnet_emul.so: the fma-chain twin of the Q-network kernels (qnet_emul.cpp), written from the order
DESIGN §3f / §3g document and from no kernel's text.

TEST TOOLING ONLY, next to es_emul.py and with its compiler flags, plus -O3 -mfma so that the independent chains of a row vectorise
(std::fmaf is correctly rounded either way).  Everything here works on logical arrays: kernels [k, m] and biases [m] as
ble_qnet_unpack_f32 hands them out, activation rows padded to round64(m) columns."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, 'libqnet_emul.so')
_vp = ctypes.c_void_p

CONTRACT, ASCENDING, HALVES_SWAPPED, UNFUSED, COLUMN_DROPPED, EVEN_FIRST, SLABS_DESCENDING = range(7)
FORWARD_MUTANTS = (ASCENDING, HALVES_SWAPPED, UNFUSED, COLUMN_DROPPED)
WGRAD_MUTANTS = (HALVES_SWAPPED, UNFUSED, EVEN_FIRST)      # ASCENDING is dW's contract already: the rows run in ascending order
WGRAD_SLAB_ROWS, WGRAD_MAX_SLABS = 256, 16


def build():
  srcs = [os.path.join(_HERE, 'qnet_emul.cpp')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O3', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-mfma', '-o', _SO, srcs[0]])
  return _SO


_lib = None


def lib():
  global _lib
  if _lib is None:
    _lib = ctypes.CDLL(build())
    i32, i64, f32 = ctypes.c_int, ctypes.c_int64, ctypes.c_float
    _lib.emul_qnet_dense.argtypes = [_vp, i64, i64, i32, i32, _vp, _vp, i32, i32, i32, i32, _vp]
    _lib.emul_qnet_head.argtypes = [_vp, i64, i64, i32, i32, i32, _vp, _vp]
    _lib.emul_qnet_dgrad.argtypes = [_vp, i64, i64, i32, i32, _vp, _vp, i64, i32, i32, _vp]
    _lib.emul_qnet_wgrad.argtypes = [_vp, i64, i32, _vp, i64, i32, i64, i32, i64, i32, _vp, _vp]
    _lib.emul_qr_loss.argtypes = [_vp, _vp, i64, i32, i32, _vp, _vp, _vp, f32, i64, _vp, _vp, _vp, _vp, _vp]
    _lib.emul_td_loss.argtypes = [i32, _vp, _vp, i64, i32, _vp, _vp, _vp, i64, _vp, _vp, _vp, _vp]
    for f in (_lib.emul_qnet_dense, _lib.emul_qnet_head, _lib.emul_qnet_dgrad, _lib.emul_qnet_wgrad, _lib.emul_qr_loss, _lib.emul_td_loss):
      f.restype = None
  return _lib


def _f32(a):
  return np.ascontiguousarray(a, np.float32)


def round_up(v, m):
  return (v + m - 1) // m * m


def layers_of(params):
  """[(kernel [k, m], bias [m])] float32 of a {'params': {'Dense_i': ...}} tree."""
  tree = params.get('params', params)
  return [(_f32(tree[f'Dense_{i}']['kernel']), _f32(tree[f'Dense_{i}']['bias'])) for i in range(len(tree))]


def dense(x, kernel, bias, first, relu, order=CONTRACT, skip=-1):
  """y float32 [n, round64(m)].  x: [n, >= k] rows (first: observations, columns >= k not read; else the previous layer's padded
  output, columns up to round8(k) read)."""
  x, kernel, bias = _f32(x), _f32(kernel), _f32(bias)
  k, m = kernel.shape
  assert x.ndim == 2 and x.shape[1] >= (k if first else round_up(k, 8)) and bias.shape == (m,)
  y = np.empty((x.shape[0], round_up(m, 64)), np.float32)
  lib().emul_qnet_dense(x.ctypes.data, x.shape[1], x.shape[0], k, m, kernel.ctypes.data, bias.ctypes.data, int(first), int(relu), order, skip,
                        y.ctypes.data)
  return y


def smallest_column(x):
  """The input column with the smallest mean |x|: the one mutant 4 leaves out."""
  return int(np.argmin(np.abs(np.asarray(x, np.float64)).mean(axis=0)))


def forward(layers, x, order=CONTRACT):
  """Every layer's padded output [n, round64(m_l)], the last being the logits.  COLUMN_DROPPED drops its column from layer 0 only."""
  x = _f32(x)
  outs, h = [], x
  for l, (kernel, bias) in enumerate(layers):
    skip = smallest_column(x[:, :kernel.shape[0]]) if order == COLUMN_DROPPED and l == 0 else -1
    o = order if order != COLUMN_DROPPED or l == 0 else CONTRACT
    h = dense(h, kernel, bias, l == 0, l < len(layers) - 1, o, skip)
    outs.append(h)
  return outs


def head(logits, atoms, actions=3, order=CONTRACT):
  """(q float32 [n, actions], action uint8 [n]) of padded logits rows."""
  logits = _f32(logits)
  n = logits.shape[0]
  q, action = np.empty((n, actions), np.float32), np.empty(n, np.uint8)
  lib().emul_qnet_head(logits.ctypes.data, logits.shape[1], n, actions, atoms, order, q.ctypes.data, action.ctypes.data)
  return q, action


def dgrad(dy, kernel, xin, order=CONTRACT):
  """dX float32 [n, round64(k)] of a layer >= 1 from its dY rows (padded) and its padded input xin."""
  dy, kernel, xin = _f32(dy), _f32(kernel), _f32(xin)
  k, m = kernel.shape
  assert dy.shape[1] >= round_up(m, 8) and xin.shape[1] >= round_up(k, 64)
  dx = np.empty((dy.shape[0], round_up(k, 64)), np.float32)
  lib().emul_qnet_dgrad(dy.ctypes.data, dy.shape[1], dy.shape[0], k, m, kernel.ctypes.data, xin.ctypes.data, xin.shape[1], order, -1,
                        dx.ctypes.data)
  return dx


def wgrad_slabs(b):
  """(slabs, slab_rows) of a batch: the host's rule (B // 256 slabs, 1 .. 16, of ceil(B / slabs) rows)."""
  slabs = min(max(b // WGRAD_SLAB_ROWS, 1), WGRAD_MAX_SLABS)
  return slabs, (b if slabs == 1 else (b + slabs - 1) // slabs)


def wgrad(x, dy, k, m, order=CONTRACT):
  """(dW float32 [k, m], db float32 [m]) over the batch rows of x [B, >= k] and dy [B, >= m]."""
  x, dy = _f32(x), _f32(dy)
  b = x.shape[0]
  assert dy.shape[0] == b and x.shape[1] >= k and dy.shape[1] >= m
  slabs, slab_rows = wgrad_slabs(b)
  dw, db = np.empty((k, m), np.float32), np.empty(m, np.float32)
  lib().emul_qnet_wgrad(x.ctypes.data, x.shape[1], k, dy.ctypes.data, dy.shape[1], m, b, slabs, slab_rows, order, dw.ctypes.data,
                        db.ctypes.data)
  return dw, db


def backward(layers, x, acts, dlogits, order=CONTRACT):
  """{'params': {'Dense_l': {'kernel': dW, 'bias': db}}} from the padded layer outputs `acts` (forward()) and the padded dlogits rows.
  The mutant applies to dW / db only; dX stays the contract's, so that a layer's change is its own."""
  dy, tree = _f32(dlogits), {}
  for l in range(len(layers) - 1, -1, -1):
    k, m = layers[l][0].shape
    dw, db = wgrad(x if l == 0 else acts[l - 1], dy, k, m, order)
    tree[f'Dense_{l}'] = {'kernel': dw, 'bias': db}
    if l > 0:
      dy = dgrad(dy, layers[l][0], acts[l - 1])
  return {'params': {f'Dense_{l}': tree[f'Dense_{l}'] for l in range(len(layers))}}


def qr_loss(logits, target_logits, ret, discount, action, atoms, batch=None, kappa=1.0, actions=3):
  """(targets [B, atoms], loss [B], dlogits [B, ld], a* uint8 [B], flag) of padded logits rows [B, ld]."""
  logits, target_logits, ret, discount = _f32(logits), _f32(target_logits), _f32(ret), _f32(discount)
  action = np.ascontiguousarray(action, np.uint8)
  b, ld = logits.shape
  assert target_logits.shape == (b, ld) and ld >= actions * atoms
  targets, loss, dlogits = np.empty((b, atoms), np.float32), np.empty(b, np.float32), np.empty((b, ld), np.float32)
  best, flag = np.empty(b, np.uint8), ctypes.c_int(0)
  lib().emul_qr_loss(logits.ctypes.data, target_logits.ctypes.data, ld, actions, atoms, ret.ctypes.data, discount.ctypes.data,
                     action.ctypes.data, float(kappa), b if batch is None else batch, targets.ctypes.data, dlogits.ctypes.data,
                     loss.ctypes.data, best.ctypes.data, ctypes.byref(flag))
  return targets, loss, dlogits, best, bool(flag.value)


def td_loss(kind, logits, target_logits, ret, discount, action, actions=3):
  """DQN's 'mse' / 'huber' on one-atom padded logits rows: (targets [B], loss [B], dlogits [B, ld], flag)."""
  logits, target_logits, ret, discount = _f32(logits), _f32(target_logits), _f32(ret), _f32(discount)
  action = np.ascontiguousarray(action, np.uint8)
  b, ld = logits.shape
  targets, loss, dlogits = np.empty(b, np.float32), np.empty(b, np.float32), np.empty((b, ld), np.float32)
  flag = ctypes.c_int(0)
  lib().emul_td_loss({'mse': 0, 'huber': 1}[kind], logits.ctypes.data, target_logits.ctypes.data, ld, actions, ret.ctypes.data,
                     discount.ctypes.data, action.ctypes.data, b, targets.ctypes.data, dlogits.ctypes.data, loss.ctypes.data,
                     ctypes.byref(flag))
  return targets, loss, dlogits, bool(flag.value)
