"""Host-side parts of the DQN / SARSA learners, CPU only: the float64 twins' hand-derived gradients (td_host.py) against torch.autograd,
ble_td_f32's ctypes mirror against the header, every host refusal of ble_qnet_td_step_f32 (BLE_E_INVALID_ARG before any HIP call), the
workspace sizes, and the agent registry."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import descriptors_host
import td_host
import train_host
from balloon_learning_environment_amd import _abi, _lib
from descriptors_host import E_INVALID_ARG, _FAKE, _batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the twins against autograd ---------------------------------------------------------------------------------------------------
def _net(rng, hidden=11):
  dims = [_lib.OBS_DIM, hidden, hidden, 3]
  return {'params': {f'Dense_{i}': {'kernel': rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i]),
                                    'bias': rng.standard_normal(dims[i + 1]) * 0.1} for i in range(3)}}


def _torch_forward(leaves, x):
  h = x
  for i, (k, b) in enumerate(leaves):
    h = h @ k + b
    if i < len(leaves) - 1:
      h = torch.relu(h)
  return h


def _leaves(params):
  return [(torch.tensor(params['params'][f'Dense_{i}']['kernel'], dtype=torch.float64, requires_grad=True),
           torch.tensor(params['params'][f'Dense_{i}']['bias'], dtype=torch.float64, requires_grad=True)) for i in range(3)]


def _assert_grads(leaves, grads):
  for l, (k, b) in enumerate(leaves):
    for got, want in ((grads[l][0], k.grad.numpy()), (grads[l][1], b.grad.numpy())):
      scale = np.abs(want).max()
      assert scale > 0
      assert np.abs(got - want).max() <= 1e-10 * scale, (l, np.abs(got - want).max() / scale)


@pytest.mark.parametrize('kind', ['mse', 'huber'])
def test_dqn_gradient_matches_autograd(kind):
  """A 3-layer network, the target a constant (stop_gradient), u on both sides of the Huber threshold."""
  rng = np.random.default_rng(1)
  b = 24
  params = _net(rng)
  x = rng.random((b, _lib.OBS_DIM))
  action = rng.integers(0, 3, b)
  target_q, ret, disc = rng.standard_normal((b, 3)), rng.standard_normal(b) * 2.0, np.where(rng.random(b) < 0.3, 0.0, 0.96)
  tgt = td_host.dqn_targets(target_q, ret, disc)
  assert np.allclose(tgt, ret + disc * target_q.max(axis=1), rtol=0, atol=0)
  q = train_host.forward_all(params, x)[-1]
  loss, dq = td_host.dqn_loss(q, tgt, action, kind)
  u = np.abs(tgt - q[np.arange(b), action])
  assert (u > 1.0).any() and (u < 1.0).any()
  grads = train_host.backward(params, x, dq)
  leaves = _leaves(params)
  qt = _torch_forward(leaves, torch.tensor(x))[torch.arange(b), torch.tensor(action)]
  ut = torch.tensor(tgt) - qt
  lt = ut * ut if kind == 'mse' else torch.where(ut.abs() <= 1.0, 0.5 * ut * ut, ut.abs() - 0.5)
  assert np.abs(lt.detach().numpy() - loss).max() <= 1e-12 * np.abs(loss).max()
  lt.mean().backward()
  _assert_grads(leaves, grads)


def test_sarsa_gradient_matches_autograd():
  """Both Q terms come from the same parameters and both carry gradient (the reference's loss_fn); masked rows add nothing but count
  in the mean."""
  rng = np.random.default_rng(2)
  b, gamma = 24, 0.9
  params = _net(rng)
  xs, xn = rng.random((b, _lib.OBS_DIM)), rng.random((b, _lib.OBS_DIM))
  action, next_action = rng.integers(0, 3, b), rng.integers(0, 3, b)
  reward = rng.standard_normal(b)
  mask = (rng.random(b) < 0.25).astype(np.uint8)
  assert mask.any() and not mask.all()
  qs, qn = train_host.forward_all(params, xs)[-1], train_host.forward_all(params, xn)[-1]
  tgt, loss, ds, dn = td_host.sarsa_loss(qs, qn, reward, action, next_action, gamma, mask)
  assert not loss[mask != 0].any() and not ds[mask != 0].any() and not dn[mask != 0].any()
  grads = td_host.sarsa_backward(params, xs, xn, ds, dn)
  leaves = _leaves(params)
  rows = torch.arange(b)
  q_val = _torch_forward(leaves, torch.tensor(xs))[rows, torch.tensor(action)]
  next_val = _torch_forward(leaves, torch.tensor(xn))[rows, torch.tensor(next_action)]
  target = torch.tensor(reward) + gamma * next_val
  lt = (q_val - target) ** 2 * torch.tensor((mask == 0).astype(np.float64))
  assert np.abs(target.detach().numpy() - tgt).max() <= 1e-12
  assert np.abs(lt.detach().numpy() - loss).max() <= 1e-12 * np.abs(loss).max()
  lt.mean().backward()
  _assert_grads(leaves, grads)
  # and the unmasked form
  _, loss1, ds1, dn1 = td_host.sarsa_loss(qs, qn, reward, action, next_action, gamma)
  leaves = _leaves(params)
  q_val = _torch_forward(leaves, torch.tensor(xs))[rows, torch.tensor(action)]
  next_val = _torch_forward(leaves, torch.tensor(xn))[rows, torch.tensor(next_action)]
  ((q_val - (torch.tensor(reward) + gamma * next_val)) ** 2).mean().backward()
  _assert_grads(leaves, td_host.sarsa_backward(params, xs, xn, ds1, dn1))


def test_sgd_is_optax():
  assert np.array_equal(td_host.sgd(np.array([1.0, -2.0]), np.array([0.5, 0.0]), 0.1), np.array([0.95, -2.0]))


# ---- the descriptor ---------------------------------------------------------------------------------------------------------------
def test_td_struct_matches_header():
  header = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
  body = header[header.index('typedef struct ble_td_f32 {'):header.index('} ble_td_f32;')]
  fields = re.findall(r'^\s*(const uint8_t\*|int32_t|float)\s+(\w+);', body, re.M)
  ctype = {'int32_t': ctypes.c_int32, 'float': ctypes.c_float, 'const uint8_t*': ctypes.c_void_p}
  assert [(n, ctype[t]) for t, n in fields] == list(_abi.BleTdF32._fields_)
  assert len(fields) == 6 and ctypes.sizeof(_abi.BleTdF32) == 32
  for name in ('TD_DQN_MSE', 'TD_DQN_HUBER', 'TD_SARSA_MSE', 'TD_OPT_ADAM', 'TD_OPT_SGD'):
    assert int(re.search(rf'#define BLE_{name} (\d+)', header).group(1)) == getattr(_abi, name)
  lib = _lib.lib()
  for name in ('ble_qnet_td_step_f32', 'ble_qnet_td_workspace_f32'):
    assert name in _lib.EXPORTS and ctypes.c_int64 not in getattr(lib, name).argtypes, name


# ---- argument checks: no call below launches (invalid arguments, or B == 0) -------------------------------------------------------
def _qnet(**fields):
  return descriptors_host._qnet(**{'num_atoms': 1, **fields})


def _train(**fields):
  return descriptors_host._train(**{'net': _qnet(), **fields})


def _td(**fields):
  d = dict(kind=_abi.TD_DQN_MSE, optimizer=_abi.TD_OPT_ADAM, gamma=0.9, reserved_=0, next_action=None, mask=None)
  d.update(fields)
  return _abi.BleTdF32(**d)


def _sarsa(**fields):
  return _td(**{**dict(kind=_abi.TD_SARSA_MSE, optimizer=_abi.TD_OPT_SGD, next_action=_FAKE), **fields})


def _step(tr=None, td=None, bt=None, loss=_FAKE):
  return _lib.lib().ble_qnet_td_step_f32(ctypes.byref(tr or _train()), ctypes.byref(td or _td()), ctypes.byref(bt or _batch()), loss, None,
                                         None)


def test_empty_batch_is_ok():
  for kind in (_abi.TD_DQN_MSE, _abi.TD_DQN_HUBER):
    for opt in (_abi.TD_OPT_ADAM, _abi.TD_OPT_SGD):
      assert _step(td=_td(kind=kind, optimizer=opt)) == 0
  assert _step(td=_sarsa()) == 0 and _step(td=_sarsa(mask=_FAKE, optimizer=_abi.TD_OPT_ADAM)) == 0
  # SGD needs no Adam state, SARSA no target image, a one-layer network no transposed image
  assert _step(_train(adam_m=None, adam_v=None, adam_step=None, target=None), _sarsa()) == 0
  assert _step(_train(net=_qnet(num_layers=1, hidden_units=0), weights_t=None, target=None), _sarsa()) == 0
  assert _step(_train(apply_update=0, adam_m=None, adam_v=None, adam_step=None)) == 0


_CASES = {
    'atoms_51': dict(tr={'net': _qnet(num_atoms=51)}), 'atoms_2': dict(tr={'net': _qnet(num_atoms=2)}),
    'kind_3': dict(td={'kind': 3}), 'kind_negative': dict(td={'kind': -1}), 'optimizer_2': dict(td={'optimizer': 2}),
    'optimizer_negative': dict(td={'optimizer': -1}),
    'sarsa_without_next_action': dict(td={'kind': _abi.TD_SARSA_MSE}),
    'sarsa_gamma_nan': dict(td={'kind': _abi.TD_SARSA_MSE, 'next_action': _FAKE, 'gamma': float('nan')}),
    'sarsa_gamma_inf': dict(td={'kind': _abi.TD_SARSA_MSE, 'next_action': _FAKE, 'gamma': float('inf')}),
    'lr_nan': dict(tr={'lr': float('nan')}), 'lr_inf': dict(tr={'lr': float('inf')}),
    'sgd_lr_inf': dict(tr={'lr': float('-inf')}, td={'optimizer': _abi.TD_OPT_SGD}),
    'misaligned_weights': dict(tr={'net': _qnet(weights=_FAKE + 4)}), 'misaligned_target': dict(tr={'target': _FAKE + 8}),
    'misaligned_grad': dict(tr={'grad': _FAKE + 4}), 'misaligned_weights_t': dict(tr={'weights_t': _FAKE + 4}),
    'misaligned_workspace': dict(tr={'workspace': _FAKE + 8}), 'misaligned_state': dict(bt={'state': _FAKE + 8}),
    'null_target_dqn': dict(tr={'target': None}), 'null_weights': dict(tr={'net': _qnet(weights=None)}), 'null_grad': dict(tr={'grad': None}),
    'null_workspace': dict(tr={'workspace': None}), 'null_weights_t': dict(tr={'weights_t': None}),
    'adam_without_state': dict(tr={'adam_m': None}), 'negative_batch': dict(bt={'batch': -1}), 'null_ret': dict(bt={'ret': None}),
}


@pytest.mark.parametrize('case', sorted(_CASES))
def test_td_step_invalid(case):
  c = _CASES[case]
  for b in ((c['bt']['batch'],) if 'batch' in c.get('bt', {}) else (0, 64)):
    bt = _batch(**{'batch': b, **c.get('bt', {})})
    assert _step(_train(**dict(c.get('tr', {}))), _td(**c.get('td', {})), bt) == E_INVALID_ARG, b


def test_td_step_null_arguments():
  assert _step(loss=None) == E_INVALID_ARG
  lib = _lib.lib()
  assert lib.ble_qnet_td_step_f32(None, ctypes.byref(_td()), ctypes.byref(_batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_td_step_f32(ctypes.byref(_train()), None, ctypes.byref(_batch()), _FAKE, None, None) == E_INVALID_ARG
  assert lib.ble_qnet_td_step_f32(ctypes.byref(_train()), ctypes.byref(_td()), None, _FAKE, None, None) == E_INVALID_ARG


@pytest.mark.parametrize('layers,hidden', [(1, 0), (2, 64), (8, 600)])
def test_td_workspace(layers, hidden):
  """The DQN kinds answer the trainer's own layout; SARSA's holds both branches: 2 L B ld of activations, 2 B ld of dlogits, two
  2 B-row dY buffers and two branches' slabs of partial sums, every part a multiple of 64 floats."""
  lib = _lib.lib()
  tr = _train(net=_qnet(num_layers=layers, hidden_units=hidden))
  names = [n for n, _ in _abi.BleQnetTrainLayout._fields_]
  for b in (0, 1, 32, 300, 4096):
    want, got, sar = _abi.BleQnetTrainLayout(), _abi.BleQnetTrainLayout(), _abi.BleQnetTrainLayout()
    assert lib.ble_qnet_train_workspace_f32(ctypes.byref(tr), ctypes.byref(_batch(batch=b)), ctypes.byref(want)) == 0
    assert lib.ble_qnet_td_workspace_f32(ctypes.byref(tr), ctypes.byref(_td(kind=_abi.TD_DQN_HUBER)), ctypes.byref(_batch(batch=b)),
                                         ctypes.byref(got)) == 0
    assert [getattr(got, n) for n in names] == [getattr(want, n) for n in names]
    assert lib.ble_qnet_td_workspace_f32(ctypes.byref(tr), ctypes.byref(_sarsa()), ctypes.byref(_batch(batch=b)), ctypes.byref(sar)) == 0
    up = lambda x: -(-x // 64) * 64
    ld, slabs = want.ld, want.slabs
    assert (sar.ld, sar.slabs, sar.transposed_floats) == (ld, slabs, want.transposed_floats)
    assert sar.acts == 0 and sar.target_logits == sar.targets == up(2 * layers * b * ld)
    assert sar.dlogits - sar.targets == up(b) and sar.scratch - sar.dlogits == up(2 * b * ld) and sar.partial - sar.scratch == up(4 * b * ld)
    assert (sar.corrections - sar.partial) % (2 * slabs) == 0 and sar.corrections - sar.partial >= 2 * slabs * 64 and sar.total == sar.corrections + 64
    if slabs > 1:
      assert sar.corrections - sar.partial == 2 * (want.corrections - want.partial)
  bad = _abi.BleQnetTrainLayout()
  assert lib.ble_qnet_td_workspace_f32(ctypes.byref(_train(net=_qnet(num_atoms=51))), ctypes.byref(_td()), ctypes.byref(_batch()),
                                       ctypes.byref(bad)) == E_INVALID_ARG
  assert lib.ble_qnet_td_workspace_f32(ctypes.byref(tr), ctypes.byref(_td(kind=7)), ctypes.byref(_batch()), ctypes.byref(bad)) == E_INVALID_ARG
  assert lib.ble_qnet_td_workspace_f32(ctypes.byref(tr), None, ctypes.byref(_batch()), ctypes.byref(bad)) == E_INVALID_ARG
  assert lib.ble_qnet_td_workspace_f32(ctypes.byref(tr), ctypes.byref(_td()), ctypes.byref(_batch(batch=-1)), ctypes.byref(bad)) == E_INVALID_ARG
  assert lib.ble_qnet_td_workspace_f32(ctypes.byref(tr), ctypes.byref(_td()), ctypes.byref(_batch()), None) == E_INVALID_ARG


# ---- the registry and the Python refusals -----------------------------------------------------------------------------------------
def test_registry_names_and_error():
  from balloon_learning_environment_amd.agents import (agent_registry, dqn_agent, mlp_agent, perciatelli44, quantile_agent,
                                                       station_seeker_agent)
  assert set(agent_registry.REGISTRY) == {'mlp', 'dqn', 'quantile', 'finetune_perciatelli', 'perciatelli44', 'station_seeker'}
  want = {'mlp': mlp_agent.MLPAgent, 'dqn': dqn_agent.DQNAgent, 'quantile': quantile_agent.QuantileAgent,
          'finetune_perciatelli': quantile_agent.QuantileAgent, 'perciatelli44': perciatelli44.Perciatelli44,
          'station_seeker': station_seeker_agent.StationSeekerAgent}
  for name, cls in want.items():
    assert agent_registry.agent_constructor(name) is cls
  for name in ('random', 'random_walk', 'acme_eval_agent', 'nope'):
    with pytest.raises(ValueError, match=f'Agent {name} not recognized'):
      agent_registry.agent_constructor(name)


def test_trainer_refuses_before_touching_the_device():
  from balloon_learning_environment_amd.agents import dqn_agent, mlp_agent, qnet
  quantile = qnet.QNetwork.from_params(qnet.init_params('quantile', 0, 2, 8, 5))
  mlp = qnet.QNetwork.from_params(qnet.init_params('mlp', 0, 2, 8))
  with pytest.raises(ValueError, match='one-atom'):
    dqn_agent.DQNTrainer(quantile)
  with pytest.raises(ValueError, match='loss_type'):
    dqn_agent.DQNTrainer(mlp, loss_type='l1')
  with pytest.raises(ValueError, match='one-atom'):
    mlp_agent.VecMLPAgent(4, quantile)
  with pytest.raises(ValueError, match='3 actions'):
    mlp_agent.MLPAgent(4, [1099])
