"""Host-side parts of the device trainer, CPU only: the packed image's inverse (ble_qnet_unpack_f32), the transposed image, the argument
checks of the training entry points (every one answers BLE_E_INVALID_ARG before any HIP call), and the float64 oracle's gradient against
central finite differences."""
import ctypes

import numpy as np
import pytest

import train_host
from balloon_learning_environment_amd import _abi, _lib
from balloon_learning_environment_amd.agents import qnet, qnet_train

E_INVALID_ARG = -1
_FAKE = 0x100000          # a non-NULL, 16-byte aligned address for every device pointer (never dereferenced)


def _random_params(layers, hidden, atoms, seed=0):
  rng = np.random.default_rng(seed)
  dims = [_lib.OBS_DIM] + [hidden] * (layers - 1) + [3 * atoms]
  return {'params': {f'Dense_{i}': {'kernel': rng.standard_normal((dims[i], dims[i + 1])).astype(np.float32),
                                    'bias': rng.standard_normal(dims[i + 1]).astype(np.float32)} for i in range(layers)}}


@pytest.mark.parametrize('layers,hidden,atoms', [(8, 600, 51), (1, 0, 1), (3, 37, 7), (2, 5, 3)])
def test_unpack_inverts_pack(layers, hidden, atoms):
  params = _random_params(layers, hidden, atoms)
  net = qnet.QNetwork.from_params(params)
  back = qnet_train.unpack(net._struct, net.packed_host)
  for name, leaf in params['params'].items():
    for k in ('kernel', 'bias'):
      got = back['params'][name][k]
      assert got.dtype == np.float32 and got.shape == leaf[k].shape
      assert np.array_equal(got.view(np.uint32), leaf[k].view(np.uint32)), (name, k)


@pytest.mark.parametrize('layers,hidden,atoms', [(3, 37, 7), (2, 70, 3)])
def test_transposed_image(layers, hidden, atoms):
  """ble_qnet_transpose_f32 packs W^T of layers 1 .. L-1: packing W_l^T as a layer of its own gives the same floats."""
  params = _random_params(layers, hidden, atoms, seed=1)
  net = qnet.QNetwork.from_params(params)
  tr = _abi.BleQnetTrainF32(net._struct)
  lay = _abi.BleQnetTrainLayout()
  assert _lib.lib().ble_qnet_train_workspace_f32(ctypes.byref(tr), ctypes.byref(_abi.BleTrainBatchF32(0, 1104)), ctypes.byref(lay)) == 0
  out = np.full(lay.transposed_floats, np.nan, np.float32)
  assert _lib.lib().ble_qnet_transpose_f32(ctypes.byref(net._struct), net.packed_host.ctypes.data, out.ctypes.data) == 0
  off = 0
  for l in range(1, layers):
    w = params['params'][f'Dense_{l}']['kernel']
    k, m = w.shape
    kp, mp = -(-m // 8) * 8, -(-k // 64) * 64
    block = out[off:off + kp * mp].reshape(mp // 64, kp // 8, 2, 64, 4)
    for g in range(mp // 64):
      for c in range(kp // 8):
        for t in range(2):
          lane = np.arange(64)[:, None]
          j = np.arange(4)[None, :]
          kk, mm = 8 * c + 4 * (lane >> 5) + j, 64 * g + 32 * t + (lane & 31)      # row kk, column mm of W^T
          want = np.where((kk < m) & (mm < k), w.T[np.minimum(kk, m - 1), np.minimum(mm, k - 1)], 0.0)
          assert np.array_equal(block[g, c, t], want.astype(np.float32)), (l, g, c, t)
    off += kp * mp
  assert off == lay.transposed_floats


def test_oracle_gradient_matches_finite_differences():
  """train_host.backward against central differences of the float64 objective on a tiny network (x away from every kink: the
  differences are taken at a point where no u_ij, ReLU input or |u| - kappa is near 0)."""
  rng = np.random.default_rng(5)
  atoms, hidden, b = 3, 4, 5
  params = {'params': {'Dense_0': {'kernel': rng.standard_normal((_lib.OBS_DIM, hidden)) * 0.05, 'bias': rng.standard_normal(hidden) * 0.1},
                       'Dense_1': {'kernel': rng.standard_normal((hidden, 3 * atoms)), 'bias': rng.standard_normal(3 * atoms)}}}
  x = rng.random((b, _lib.OBS_DIM))
  action = rng.integers(0, 3, b)
  tgt = rng.standard_normal((b, atoms)) * 2.0
  logits = train_host.forward_all(params, x)[-1]
  _, dlog = train_host.quantile_loss(logits, tgt, action, atoms)
  grads = train_host.backward(params, x, dlog)
  h = 1e-6
  checked = 0
  for l, name in enumerate(('Dense_0', 'Dense_1')):
    for leaf, gi in (('kernel', 0), ('bias', 1)):
      arr = params['params'][name][leaf]
      idx = [tuple(rng.integers(0, s) for s in arr.shape) for _ in range(6)]
      for ix in idx:
        old = arr[ix]
        arr[ix] = old + h
        fp = train_host.loss_of_params(params, x, tgt, action, atoms)
        arr[ix] = old - h
        fm = train_host.loss_of_params(params, x, tgt, action, atoms)
        arr[ix] = old
        fd = (fp - fm) / (2 * h)
        assert abs(fd - grads[l][gi][ix]) <= 1e-6 * max(1.0, abs(fd)), (name, leaf, ix, fd, grads[l][gi][ix])
        checked += 1
  assert checked == 24


def test_oracle_adam_is_optax():
  """Two steps by hand: the first Adam step moves every non-zero-gradient weight by lr * g / (|g| + eps)."""
  g = np.array([1e-3, -2.0, 0.0])
  w, m, v = train_host.adam(np.zeros(3), g, np.zeros(3), np.zeros(3), 1, lr=0.1, eps=1e-8)
  assert np.allclose(w, -0.1 * g / (np.abs(g) + 1e-8)) and w[2] == 0.0
  w2, _, _ = train_host.adam(w, g, m, v, 2, lr=0.1, eps=1e-8)
  assert np.allclose(w2, 2 * w)


# ---- argument checks: no call below launches (invalid arguments, or B == 0 / n == 0)
def _qnet(**fields):
  d = dict(num_layers=2, input_dim=_lib.OBS_DIM, hidden_units=64, num_actions=3, num_atoms=51, reserved_=0, weights=_FAKE)
  d.update(fields)
  return _abi.BleQnetF32(**d)


def _replay(**fields):
  d = dict(capacity=16, num_envs=4, update_horizon=5, obs_stride=1104, gamma=0.993, max_tries=64, obs=_FAKE, action=_FAKE, reward=_FAKE,
           terminal=_FAKE, episode_end=_FAKE, count=_FAKE, counter=_FAKE)
  d.update(fields)
  return _abi.BleReplayF32(**d)


def _batch(**fields):
  d = dict(batch=0, state_stride=1104, state=_FAKE, next_state=_FAKE, ret=_FAKE, discount=_FAKE, action=_FAKE, index=None)
  d.update(fields)
  return _abi.BleTrainBatchF32(**d)


def _train(**fields):
  net = fields.pop('net', None) or _qnet()
  d = dict(net=net, target=_FAKE, weights_t=_FAKE, grad=_FAKE, adam_m=_FAKE, adam_v=_FAKE, adam_step=_FAKE, workspace=_FAKE, lr=2e-6,
           adam_b1=0.9, adam_b2=0.999, adam_eps=2e-5, kappa=1.0, apply_update=1)
  d.update(fields)
  return _abi.BleQnetTrainF32(**d)


def _sample(rp=None, bt=None):
  return _lib.lib().ble_replay_sample_f32(ctypes.byref(rp or _replay()), ctypes.byref(bt or _batch()), 1, None, None)


def _step(tr=None, bt=None, loss=_FAKE):
  return _lib.lib().ble_qnet_train_step_f32(ctypes.byref(tr or _train()), ctypes.byref(bt or _batch()), loss, None, None)


def test_no_new_entry_point_takes_an_int64():
  lib = _lib.lib()
  for name in ('ble_qnet_unpack_f32', 'ble_replay_sample_f32', 'ble_qnet_train_workspace_f32', 'ble_qnet_transpose_f32',
               'ble_qnet_train_step_f32', 'ble_qnet_explore_u8'):
    assert name in _lib.EXPORTS
    assert ctypes.c_int64 not in getattr(lib, name).argtypes, name


def test_empty_batch_is_ok():
  assert _sample() == 0
  assert _step() == 0
  assert _step(_train(apply_update=0)) == 0
  ex = _abi.BleExploreF32(0, 0.1, 0, 1, 0)
  assert _lib.lib().ble_qnet_explore_u8(ctypes.byref(ex), _FAKE, None) == 0


_REPLAY_CASES = {
    **{f'null_{p}': {p: None} for p in ('obs', 'action', 'reward', 'terminal', 'episode_end', 'count', 'counter')},
    'horizon_0': {'update_horizon': 0}, 'horizon_65': {'update_horizon': 65}, 'capacity_short': {'capacity': 5},
    'negative_capacity': {'capacity': -1}, 'envs_0': {'num_envs': 0}, 'negative_envs': {'num_envs': -4},
    'obs_stride_short': {'obs_stride': 1098}, 'obs_stride_unaligned': {'obs_stride': 1099}, 'tries_0': {'max_tries': 0},
    'tries_1025': {'max_tries': 1025}, 'gamma_nan': {'gamma': float('nan')}, 'misaligned_obs': {'obs': _FAKE + 4}}
_BATCH_CASES = {
    **{f'null_{p}': {p: None} for p in ('state', 'next_state', 'ret', 'discount', 'action')},
    'negative_batch': {'batch': -1}, 'batch_too_large': {'batch': 1048577}, 'stride_short': {'state_stride': 1096},
    'stride_unaligned': {'state_stride': 1102}, 'misaligned_state': {'state': _FAKE + 8}, 'misaligned_next_state': {'next_state': _FAKE + 4}}
_TRAIN_CASES = {
    **{f'null_{p}': {p: None} for p in ('target', 'weights_t', 'grad', 'adam_m', 'adam_v', 'adam_step', 'workspace')},
    'null_weights': {'net': _qnet(weights=None)}, 'layers_0': {'net': _qnet(num_layers=0)}, 'atoms_0': {'net': _qnet(num_atoms=0)},
    'input_dim': {'net': _qnet(input_dim=1098)}, 'kappa_0': {'kappa': 0.0}, 'kappa_nan': {'kappa': float('nan')},
    'lr_inf': {'lr': float('inf')}, 'misaligned_weights': {'net': _qnet(weights=_FAKE + 4)}, 'misaligned_grad': {'grad': _FAKE + 4},
    'misaligned_workspace': {'workspace': _FAKE + 8}, 'misaligned_m': {'adam_m': _FAKE + 4}}


@pytest.mark.parametrize('case', sorted(_REPLAY_CASES))
@pytest.mark.parametrize('b', [0, 64])
def test_replay_sample_invalid(case, b):
  assert _sample(_replay(**_REPLAY_CASES[case]), _batch(batch=b)) == E_INVALID_ARG


@pytest.mark.parametrize('case', sorted(_BATCH_CASES))
def test_batch_invalid(case):
  fields = dict(_BATCH_CASES[case])
  for b in ((fields.pop('batch'),) if 'batch' in fields else (0, 64)):
    assert _sample(bt=_batch(batch=b, **fields)) == E_INVALID_ARG, b
    assert _step(bt=_batch(batch=b, **fields)) == E_INVALID_ARG, b


@pytest.mark.parametrize('case', sorted(_TRAIN_CASES))
@pytest.mark.parametrize('b', [0, 64])
def test_train_step_invalid(case, b):
  assert _step(_train(**_TRAIN_CASES[case]), _batch(batch=b)) == E_INVALID_ARG


def test_train_step_null_loss_and_gradient_only_mode():
  assert _step(loss=None) == E_INVALID_ARG
  # the gradient alone needs no Adam state ...
  assert _step(_train(apply_update=0, adam_m=None, adam_v=None, adam_step=None)) == 0
  # ... but the transposed image whenever there is a hidden layer
  assert _step(_train(apply_update=0, weights_t=None)) == E_INVALID_ARG
  assert _step(_train(net=_qnet(num_layers=1), weights_t=None)) == 0


def test_workspace_and_host_entries_invalid():
  lib = _lib.lib()
  lay = _abi.BleQnetTrainLayout()
  assert lib.ble_qnet_train_workspace_f32(ctypes.byref(_train()), ctypes.byref(_batch(batch=32)), ctypes.byref(lay)) == 0
  assert lay.total > 0 and lay.slabs == 1 and lay.ld == 192
  assert lib.ble_qnet_train_workspace_f32(ctypes.byref(_train()), ctypes.byref(_batch(batch=4096)), ctypes.byref(lay)) == 0
  assert lay.slabs == 16
  assert lib.ble_qnet_train_workspace_f32(ctypes.byref(_train()), ctypes.byref(_batch(batch=-1)), ctypes.byref(lay)) == E_INVALID_ARG
  assert lib.ble_qnet_train_workspace_f32(ctypes.byref(_train(net=_qnet(num_layers=0))), ctypes.byref(_batch()), ctypes.byref(lay)) == E_INVALID_ARG
  assert lib.ble_qnet_train_workspace_f32(ctypes.byref(_train()), ctypes.byref(_batch()), None) == E_INVALID_ARG
  k = (ctypes.c_void_p * 2)(_FAKE, None)
  assert lib.ble_qnet_unpack_f32(ctypes.byref(_qnet()), _FAKE, k, k) == E_INVALID_ARG       # a NULL layer pointer
  assert lib.ble_qnet_unpack_f32(ctypes.byref(_qnet()), None, k, k) == E_INVALID_ARG
  assert lib.ble_qnet_transpose_f32(ctypes.byref(_qnet(num_actions=2)), _FAKE, _FAKE) == E_INVALID_ARG
  assert lib.ble_qnet_transpose_f32(ctypes.byref(_qnet()), None, _FAKE) == E_INVALID_ARG


@pytest.mark.parametrize('n,eps', [(-1, 0.1), (4, -0.1), (4, 1.5), (4, float('nan'))])
def test_explore_invalid(n, eps):
  ex = _abi.BleExploreF32(n, eps, 0, 1, 0)
  assert _lib.lib().ble_qnet_explore_u8(ctypes.byref(ex), _FAKE, None) == E_INVALID_ARG
  assert _lib.lib().ble_qnet_explore_u8(ctypes.byref(_abi.BleExploreF32(0, 0.1, 0, 1, 0)), None, None) == E_INVALID_ARG
