"""The float64 restatement of the imitation kernels (imitation_host.py), CPU only: loss and dL/dlogits against torch autograd of
mean_b(CE_smooth + c_v (v - R)^2), agree against ppo_host.greedy with tied logits, the mixture on the DAGGER stream's Philox words and
at its beta edges, the descriptors against the header and the library's exports."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import imitation_host
import ppo_host
from balloon_learning_environment_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autograd(z, act, ret, s, cv):
  zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
  lp = torch.log_softmax(zt[:, [0, 2, 4]], dim=1)
  q = torch.full((len(act), 3), s / 3.0, dtype=torch.float64)
  q[torch.arange(len(act)), torch.tensor(act)] += 1.0 - s
  loss = -(q * lp).sum(dim=1) + cv * (zt[:, 1] - torch.tensor(ret)) ** 2
  loss.mean().backward()
  return loss.detach().numpy(), zt.grad.numpy()


@pytest.mark.parametrize('b', [1, 32])
@pytest.mark.parametrize('cv', [0.0, 0.5])
@pytest.mark.parametrize('s', [0.0, 0.1])
def test_bc_loss_gradient_against_autograd(s, cv, b):
  rng = np.random.default_rng(100 * b + int(10 * s) + int(cv * 2))
  z = rng.standard_normal((b, 6)) * 1.5
  act = rng.integers(0, 3, b)
  ret = rng.standard_normal(b)
  s32, cv32 = float(np.float32(s)), float(np.float32(cv))          # (the twin takes the float32 the descriptor carries)
  loss, aux, d = imitation_host.bc_loss(z, act, None if cv == 0.0 else ret, s, cv)
  want_loss, want_d = _autograd(z, act, ret, s32, cv32)
  assert np.allclose(loss, want_loss, rtol=1e-13, atol=1e-15)
  assert np.allclose(d, want_d, rtol=1e-12, atol=1e-16), np.abs(d - want_d).max()
  assert not d[:, [3, 5]].any()
  if cv == 0.0:
    assert not d[:, 1].any()                                       # exactly 0, and ret was never read
    ce = -(imitation_host.smoothed_target(act, s) * ppo_host.log_softmax(z[:, [0, 2, 4]])[0])
    assert np.allclose(loss, ce.sum(axis=1), rtol=1e-13)
  lp, _ = ppo_host.log_softmax(z[:, [0, 2, 4]])
  assert np.array_equal(aux[:, 0], lp[np.arange(b), act])
  assert np.array_equal(aux[:, 1], (z[:, [0, 2, 4]].argmax(axis=1) == act).astype(np.float64))
  if s == 0.0:
    assert np.allclose(loss - (cv32 * (z[:, 1] - ret) ** 2 if cv else 0.0), -aux[:, 0], rtol=1e-12, atol=1e-15)


def test_smoothed_target_sums_to_one():
  q = imitation_host.smoothed_target([0, 1, 2, 2], 0.1)
  assert np.allclose(q.sum(axis=1), 1.0, atol=1e-15) and q.argmax(axis=1).tolist() == [0, 1, 2, 2]
  assert np.array_equal(imitation_host.smoothed_target([1], 0.0), [[0.0, 1.0, 0.0]])


def test_agree_follows_the_greedy_rule_with_ties():
  rows = [[1, 2, 3], [2, 2, 1], [0, 0, 0], [1, 3, 3], [-1, -1, -2], [3, 3, 3], [5, 1, 0], [0, 7, 0], [-2, -1, -1]]
  z = np.zeros((len(rows), 6))
  z[:, [0, 2, 4]] = rows
  z[:, [1, 3, 5]] = 99.0                                            # the value and the unread columns do not vote
  g = ppo_host.greedy(z)
  assert g.tolist() == [2, 0, 0, 1, 0, 0, 0, 1, 1]                  # the lowest index among equal maxima
  for label in range(3):
    act = np.full(len(rows), label)
    aux = imitation_host.bc_loss(z, act)[1]
    assert np.array_equal(aux[:, 1], (g == label).astype(np.float64)), label
  zn = z.copy()
  zn[0, 2] = np.nan                                                 # the first NaN is the greedy action
  assert imitation_host.bc_loss(zn, np.array([1] + [0] * 8))[1][0, 1] == 1.0
  assert imitation_host.bc_loss(zn, np.array([2] + [0] * 8))[1][0, 1] == 0.0


def test_invalid_label_zeroes_its_row_only():
  rng = np.random.default_rng(3)
  z = rng.standard_normal((5, 6))
  act = np.array([0, 3, 2, 200, 1])
  loss, aux, d = imitation_host.bc_loss(z, act, rng.standard_normal(5), 0.1, 0.5)
  assert not loss[[1, 3]].any() and not aux[[1, 3]].any() and not d[[1, 3]].any()
  assert loss[[0, 2, 4]].all() and d[[0, 2, 4]][:, [0, 1, 2, 4]].all()


# ---- the mixture ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def draws(tmp_path_factory):
  return ppo_host.build_actor_draws(tmp_path_factory.mktemp('dgd'))


def test_dagger_stream_is_its_own(draws):
  """The DAGGER words are the epsilon-greedy keying under seed ^ "DAGGER": apart from the actor's and the epsilon-greedy stream of the
  same seed, a function of (seed, environment, step) alone, the step's high word included."""
  w = imitation_host.dagger_words(draws, 5, 0, 500, 7)
  assert not np.array_equal(w, draws(5, 0, 500, 7)) and not np.array_equal(w, draws.explore(5, 0, 500, 7))
  assert np.array_equal(w, draws.explore(5 ^ 0x444147474552, 0, 500, 7))
  assert np.array_equal(imitation_host.dagger_words(draws, 5, 300, 200, 7), w[300:])      # a shard draws what the whole draws
  assert not np.array_equal(imitation_host.dagger_words(draws, 5, 0, 500, 8), w)
  assert not np.array_equal(imitation_host.dagger_words(draws, 6, 0, 500, 7), w)
  assert not np.array_equal(imitation_host.dagger_words(draws, 5, 0, 500, 2 ** 32 + 7), w)


def test_mix_twin_and_beta_edges(draws):
  rng = np.random.default_rng(0)
  n = 4096
  learner, expert = rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 3, n).astype(np.uint8)
  w = imitation_host.dagger_words(draws, 9, 0, n, 3)
  u = ppo_host.uniform24(w)
  assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
  a, took = imitation_host.mix(learner, expert, 0.0, w)
  assert np.array_equal(a, learner) and not took.any()              # u < 0 never
  a, took = imitation_host.mix(learner, expert, 1.0, w)
  assert np.array_equal(a, expert) and took.all()                   # u < 1 always
  a, took = imitation_host.mix(learner, expert, 0.3, w)
  assert np.array_equal(took, (u < np.float32(0.3)).astype(np.uint8))
  assert np.array_equal(a[took == 1], expert[took == 1]) and np.array_equal(a[took == 0], learner[took == 0])
  sigma = np.sqrt(n * 0.3 * 0.7)
  assert abs(int(took.sum()) - 0.3 * n) <= 4 * sigma, took.sum()
  # the largest uniform a word can give is 1 - 2^-24: still below beta = 1
  assert imitation_host.mix([0], [2], 1.0, np.array([0xFFFFFFFF], np.uint32))[0].tolist() == [2]
  assert imitation_host.mix([0], [2], 0.0, np.array([0], np.uint32))[0].tolist() == [0]


# ---- the descriptors and the module --------------------------------------------------------------------------------------------------
def _struct_fields(name):
  header = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
  body = re.search(r'typedef struct ' + name + r' \{(.*?)\} ' + name + ';', header, re.S).group(1)
  body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
  return [re.search(r'(\w+)$', decl.strip()).group(1) for decl in body.split(';') if decl.strip()]      # (one field per declaration)


def test_descriptors_match_the_header():
  assert [f[0] for f in _abi.BleBcF32._fields_] == _struct_fields('ble_bc_f32') == ['label_smoothing', 'value_coef', 'reserved_']
  assert [f[0] for f in _abi.BleDaggerMixF32._fields_] == _struct_fields('ble_dagger_mix_f32')
  assert ctypes.sizeof(_abi.BleBcF32) == 16 and ctypes.sizeof(_abi.BleDaggerMixF32) == 72
  assert _abi.BleDaggerMixF32.step.offset == 32 and _abi.BleDaggerMixF32.took_expert.offset == 64


def test_exports_and_module():
  lib = _lib.lib()
  for name in ('ble_qnet_bc_step_f32', 'ble_dagger_mix_u8'):
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS and hasattr(lib, name)
  assert _lib.ABI_VERSION == 5                                      # additive: the version stays
  from balloon_learning_environment_amd.agents import agent_registry, imitation
  assert 'agent_registry' in imitation.__doc__                      # the module says why it has no registry entry
  assert not any('imitat' in k.lower() or k.lower().startswith('bc') for k in getattr(agent_registry, 'REGISTRY', {}))
  assert issubclass(imitation.BCTrainer, imitation.qnet_train.QNetworkLearner)
  assert imitation.BCTrainer._TENSORS == ('weights', 'adam_m', 'adam_v', 'adam_step', 'act_step', 'mix_step')
