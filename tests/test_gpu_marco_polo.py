"""Marco Polo exploration on the device (ble_marco_polo_u8, agents/marco_polo.py) against the restatement (marco_polo_host.py) with the
same Philox draws made on the host by a g++ build, and run_training_loop_vec end to end with prioritized replay and Marco Polo."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import marco_polo_host as mh

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def draws(tmp_path_factory):
  so = str(tmp_path_factory.mktemp('mpd') / 'libmarco_polo_draws.so')
  subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include',
                         os.path.join(_HERE, 'emul', 'ble_intrinsics.h'), '-o', so, os.path.join(_HERE, 'marco_polo_draws.cpp')])
  lib = ctypes.CDLL(so)
  lib.marco_polo_draws.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint64] + [ctypes.c_void_p] * 3

  def draw(seed, n, step):
    out = [np.empty(n) for _ in range(3)]
    lib.marco_polo_draws(seed, n, step, *[o.ctypes.data for o in out])
    return out
  return draw


@pytest.fixture(scope='module')
def mp():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import marco_polo
  return marco_polo


def test_kernel_equals_restatement(mp, draws):
  n, steps, seed = 4096, 2000, 17
  ex = mp.VecMarcoPoloExploration(n, 0.8, seed=seed)
  host = mh.MarcoPolo(n, 0.8)
  rng = np.random.default_rng(0)
  obs = torch.zeros(n, 1104, dtype=torch.float32, device='cuda')
  mismatched_targets = 0
  for s in range(steps):
    begin = (rng.random(n) < 1 / 150).astype(np.uint8) if s else np.ones(n, np.uint8)
    f0 = (rng.random(n) * 0.8 + 0.1).astype(np.float32)
    agent = rng.integers(0, 3, n).astype(np.uint8)
    obs[:, 0].copy_(torch.from_numpy(f0))
    act = torch.from_numpy(agent).cuda()
    ex(obs, act, torch.from_numpy(begin).cuda())
    ut, ue, z = draws(seed, n, s)
    want = host(f0, agent, begin, mh.u24(ut), mh.u24(ue), z)
    got = act.cpu().numpy()
    assert np.array_equal(got, want), (s, np.flatnonzero(got != want)[:5])
    if s % 97 == 0 or s == steps - 1:
      assert np.array_equal(ex.phase_clock.cpu().numpy(), host.phase_clock)
      assert np.array_equal(ex.walk_clock.cpu().numpy(), host.walk_clock)
      assert np.array_equal(ex.exploratory_episode.cpu().numpy(), host.exploratory_episode)
      assert np.array_equal(ex.exploratory_phase.cpu().numpy(), host.exploratory_phase)
      # (the host's normals use libm for the device's log / sincos approximations: the targets agree to rounding)
      np.testing.assert_allclose(ex.target.cpu().numpy(), host.target, rtol=1e-12, atol=1e-9)
  assert ex.step.item() == steps
  assert 0.5 < host.exploratory_episode.mean() < 0.95 and host.walk_clock.max() > 40


class _Recording:
  """Wraps an explorer and records the share of lanes in the exploratory phase after each call (device scalars)."""

  def __init__(self, ex):
    self.ex, self.share = ex, []

  def __call__(self, obs, actions, begin):
    self.ex(obs, actions, begin)
    self.share.append(self.ex.exploratory_phase.float().mean())
    return actions


@pytest.mark.parametrize('layers,hidden,steps', [(2, 64, 360), (8, 600, 130)])
def test_training_loop_with_prioritized_replay_and_marco_polo(mp, layers, hidden, steps):
  from balloon_learning_environment_amd import train_lib
  from balloon_learning_environment_amd.agents import qnet, qnet_train
  from balloon_learning_environment_amd.env import balloon_env
  n = 256
  env = balloon_env.VecBalloonEnv(n, seed=1)
  tr = qnet_train.QNetworkTrainer(qnet.QNetwork.from_params(qnet.init_params('quantile', 3, layers, hidden, 51)), lr=1e-4, seed=2)
  rp = qnet_train.VecPrioritizedReplayBuffer(n, 64, update_horizon=5, gamma=0.993)
  ex = _Recording(mp.VecMarcoPoloExploration(n, 0.8, seed=4))
  stats = train_lib.run_training_loop_vec(env, tr, rp, num_iterations=1, steps_per_iteration=steps, min_replay_history=n * 8,
                                          updates_per_step=2, epsilon=0.0, seed=3, exploration=ex)
  assert stats[0]['updates'] > 0 and np.isfinite(stats[0]['mean_loss'])
  leaves = rp.leaf_priorities()
  moved = leaves[(leaves > 0) & (leaves != 1.0)]
  assert moved.numel() > 0 and rp.max_priority.item() >= 1.0
  share = torch.stack(ex.share).cpu().numpy()
  assert share[:80].max() == 0.0                           # every episode starts in the RL phase (4 h)
  if steps >= 360:
    steady = share[120:360].mean()                         # two full RL + exploratory periods
    assert 0.15 < steady < 0.4, steady                     # ~ 0.8 x 40 / 120
  else:
    assert share[80:120].mean() > 0.5                      # the exploratory episodes' first walk
