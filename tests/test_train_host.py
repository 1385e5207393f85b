"""Host-side parts of the device trainer, CPU only: the packed image's inverse (ble_qnet_unpack_f32), the transposed image, the argument
checks of the training entry points (every one answers BLE_E_INVALID_ARG before any HIP call), and the float64 oracle's gradient against
central finite differences."""
import ctypes

import numpy as np
import pytest

import train_host
from balloon_learning_environment_amd import _abi, _lib
from balloon_learning_environment_amd.agents import qnet, qnet_train
from descriptors_host import E_INVALID_ARG, _FAKE, _batch, _qnet, _train


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


@pytest.mark.parametrize('layers,hidden,atoms', [(8, 600, 51), (1, 0, 1), (3, 37, 7), (2, 5, 3)])
def test_pack_is_the_layout_formula(layers, hidden, atoms):
  """ble_qnet_pack_f32 against the layout written in numpy: block l is [mp / 64][kp / 8][2][64 lanes][4] floats, element
  (g, c, t, lane, j) = W[8c + 4 (lane >> 5) + j][64g + 32t + (lane & 31)], then the bias padded to mp -- bit for bit, padding zeros
  (+0.0) included."""
  params = _random_params(layers, hidden, atoms, seed=2)
  got = qnet.QNetwork.from_params(params).packed_host
  t, lane, j = np.arange(2).reshape(-1, 1, 1), np.arange(64).reshape(-1, 1), np.arange(4)
  off = 0
  for l in range(layers):
    w, b = params['params'][f'Dense_{l}']['kernel'], params['params'][f'Dense_{l}']['bias']
    k, m = w.shape
    kp, mp = -(-k // 8) * 8, -(-m // 64) * 64
    g, c = np.arange(mp // 64).reshape(-1, 1, 1, 1, 1), np.arange(kp // 8).reshape(1, -1, 1, 1, 1)
    kk, mm = 8 * c + 4 * (lane >> 5) + j, 64 * g + 32 * t + (lane & 31)
    want = np.where((kk < k) & (mm < m), w[np.minimum(kk, k - 1), np.minimum(mm, m - 1)], np.float32(0.0)).astype(np.float32)
    assert want.shape == (mp // 64, kp // 8, 2, 64, 4)
    assert np.array_equal(got[off:off + kp * mp].view(np.uint32), want.ravel().view(np.uint32)), l
    off += kp * mp
    want_b = np.zeros(mp, np.float32)
    want_b[:m] = b
    assert np.array_equal(got[off:off + mp].view(np.uint32), want_b.view(np.uint32)), l
    off += mp
  assert off == got.size


# Every size the Q-network entry points answer, per network shape and batch size: (every field of ble_qnet_train_layout in declaration
# order, (packed_floats, scratch_floats) of ble_qnet_workspace_f32).  The literals were printed by the library built from the commit
# before the host code got its one shape table, loaded through BLE_HIP_LIB: they pin the ABI's sizes, not this build's arithmetic.
_LAYOUT_FIELDS = ('ld', 'acts', 'target_logits', 'targets', 'dlogits', 'scratch', 'partial', 'slabs', 'corrections', 'total',
                  'transposed_floats')
_SIZE_BATCHES = (0, 1, 32, 300, 4096, 5000)
_SIZES = {
    (8, 600, 51): [
        ((640, 0, 0, 0, 0, 0, 0, 1, 0, 64, 2406400), (3130432, 0)),      # B = 0
        ((640, 0, 5120, 5760, 5824, 6464, 9024, 1, 9024, 9088, 2406400), (3130432, 1280)),      # B = 1
        ((640, 0, 163840, 184320, 185984, 206464, 288384, 1, 288384, 288448, 2406400), (3130432, 40960)),      # B = 32
        ((640, 0, 1536000, 1728000, 1743360, 1935360, 2703360, 1, 2703360, 2703424, 2406400), (3130432, 384000)),      # B = 300
        ((640, 0, 20971520, 23592960, 23801856, 26423296, 36909056, 16, 48224256, 48224320, 2406400), (3130432, 5242880)),      # B = 4096
        ((640, 0, 25600000, 28800000, 29055040, 32255040, 45055040, 16, 56370240, 56370304, 2406400), (3130432, 6400000)),      # B = 5000
    ],
    (1, 0, 1): [
        ((64, 0, 0, 0, 0, 0, 0, 1, 0, 64, 0), (70720, 0)),      # B = 0
        ((64, 0, 64, 128, 192, 256, 512, 1, 512, 576, 0), (70720, 128)),      # B = 1
        ((64, 0, 2048, 4096, 4160, 6208, 14400, 1, 14400, 14464, 0), (70720, 4096)),      # B = 32
        ((64, 0, 19200, 38400, 38720, 57920, 134720, 1, 134720, 134784, 0), (70720, 38400)),      # B = 300
        ((64, 0, 262144, 524288, 528384, 790528, 1839104, 16, 2970624, 2970688, 0), (70720, 524288)),      # B = 4096
        ((64, 0, 320000, 640000, 645056, 965056, 2245056, 16, 3376576, 3376640, 0), (70720, 640000)),      # B = 5000
    ],
    (3, 37, 7): [
        ((64, 0, 0, 0, 0, 0, 0, 1, 0, 64, 4096), (75968, 0)),      # B = 0
        ((64, 0, 192, 256, 320, 384, 640, 1, 640, 704, 4096), (75968, 128)),      # B = 1
        ((64, 0, 6144, 8192, 8448, 10496, 18688, 1, 18688, 18752, 4096), (75968, 4096)),      # B = 32
        ((64, 0, 57600, 76800, 78912, 98112, 174912, 1, 174912, 174976, 4096), (75968, 38400)),      # B = 300
        ((64, 0, 786432, 1048576, 1077248, 1339392, 2387968, 16, 3519488, 3519552, 4096), (75968, 524288)),      # B = 4096
        ((64, 0, 960000, 1280000, 1315008, 1635008, 2915008, 16, 4046528, 4046592, 4096), (75968, 640000)),      # B = 5000
    ],
    (2, 5, 3): [
        ((64, 0, 0, 0, 0, 0, 0, 1, 0, 64, 1024), (71296, 0)),      # B = 0
        ((64, 0, 128, 192, 256, 320, 576, 1, 576, 640, 1024), (71296, 128)),      # B = 1
        ((64, 0, 4096, 6144, 6272, 8320, 16512, 1, 16512, 16576, 1024), (71296, 4096)),      # B = 32
        ((64, 0, 38400, 57600, 58560, 77760, 154560, 1, 154560, 154624, 1024), (71296, 38400)),      # B = 300
        ((64, 0, 524288, 786432, 798720, 1060864, 2109440, 16, 3240960, 3241024, 1024), (71296, 524288)),      # B = 4096
        ((64, 0, 640000, 960000, 975040, 1295040, 2575040, 16, 3706560, 3706624, 1024), (71296, 640000)),      # B = 5000
    ],
    (2, 70, 3): [
        ((128, 0, 0, 0, 0, 0, 0, 1, 0, 64, 2048), (146112, 0)),      # B = 0
        ((128, 0, 256, 384, 448, 576, 1088, 1, 1088, 1152, 2048), (146112, 256)),      # B = 1
        ((128, 0, 8192, 12288, 12416, 16512, 32896, 1, 32896, 32960, 2048), (146112, 8192)),      # B = 32
        ((128, 0, 76800, 115200, 116160, 154560, 308160, 1, 308160, 308224, 2048), (146112, 76800)),      # B = 300
        ((128, 0, 1048576, 1572864, 1585152, 2109440, 4206592, 16, 6469632, 6469696, 2048), (146112, 1048576)),      # B = 4096
        ((128, 0, 1280000, 1920000, 1935040, 2575040, 5135040, 16, 7398080, 7398144, 2048), (146112, 1280000)),      # B = 5000
    ],
}


@pytest.mark.parametrize('shape', sorted(_SIZES))
def test_sizes_are_pinned(shape):
  assert _LAYOUT_FIELDS == tuple(name for name, _ in _abi.BleQnetTrainLayout._fields_)
  lib = _lib.lib()
  layers, hidden, atoms = shape
  net = _abi.BleQnetF32(layers, _lib.OBS_DIM, hidden, 3, atoms, 0, None)
  for b, (want_layout, want_workspace) in zip(_SIZE_BATCHES, _SIZES[shape]):
    lay = _abi.BleQnetTrainLayout()
    assert lib.ble_qnet_train_workspace_f32(ctypes.byref(_abi.BleQnetTrainF32(net)), ctypes.byref(_abi.BleTrainBatchF32(b, 1104)),
                                            ctypes.byref(lay)) == 0
    assert tuple(getattr(lay, name) for name in _LAYOUT_FIELDS) == want_layout, b
    packed, scratch = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.ble_qnet_workspace_f32(ctypes.byref(net), b, ctypes.byref(packed), ctypes.byref(scratch)) == 0
    assert (packed.value, scratch.value) == want_workspace, b


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
def _replay(**fields):
  d = dict(capacity=16, num_envs=4, update_horizon=5, obs_stride=1104, gamma=0.993, max_tries=64, obs=_FAKE, action=_FAKE, reward=_FAKE,
           terminal=_FAKE, episode_end=_FAKE, count=_FAKE, counter=_FAKE)
  d.update(fields)
  return _abi.BleReplayF32(**d)


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
