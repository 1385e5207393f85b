"""A NumPy twin of train_lib.pbt_decide, written from its contract, and recording fakes of a population trainer, its rollout buffer and
an environment on CPU tensors for run_pbt_loop_vec's schedule (in the manner of loop_fakes.py).  TEST TOOLING."""
import numpy as np
import torch

import loop_fakes as lf


def pbt_decide(fitness, truncation, src_draws, factor_draws):
  """(src, dst, factor_index) from fitness [P] (NaN: no finished episode) and the draws the decision consumes: src_draws [k] in
  [0, k), factor_draws [k, E] in {0, 1}.  Best first; among equal fitness the lower member index first; NaN last."""
  f = np.asarray(fitness, np.float64)
  p = len(f)
  k = min(int(np.floor(truncation * p + 1e-9)), p // 2)
  if k == 0:
    return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, np.asarray(factor_draws).shape[-1]), np.int64)
  with_episodes = [i for i in range(p) if not np.isnan(f[i])]
  order = sorted(with_episodes, key=lambda i: (-f[i], i)) + [i for i in range(p) if np.isnan(f[i])]
  top, bottom = order[:k], order[p - k:]
  return np.array([top[j] for j in src_draws], np.int64), np.array(bottom, np.int64), np.asarray(factor_draws, np.int64).reshape(k, -1)


# ---- run_pbt_loop_vec on fakes ---------------------------------------------------------------------------------------------------------
P, R, T, LIMIT = 4, 2, 2, 2                     # every environment finishes one episode of LIMIT = T steps per iteration
# the reward of member p's environments in iteration i (both steps): the episode's return is twice that
REWARD = {0: (0.0, 1.0, 2.0, 3.0), 1: (0.0, 1.0, 2.0, 3.0), 2: (5.0, 1.0, 0.0, 2.0), 3: (5.0, 1.0, 0.0, 2.0), 4: (1.0, 1.0, 1.0, 1.0)}


class FakePopEnv:
  num_envs, device = P * R, torch.device('cpu')

  def __init__(self, log):
    self.log, self.s = log, 0

  def _obs(self):
    return torch.full((P * R, 2), float(self.s))

  def reset(self):
    self.log.append(('reset',))
    return self._obs()

  def step(self, actions, end_mask=None):
    reward = torch.tensor(REWARD[self.s // T], dtype=torch.float32).repeat_interleave(R)
    self.log.append(('step', self.s, actions.clone(), end_mask.clone()))
    self.s += 1
    return self._obs(), reward, torch.zeros(P * R, dtype=torch.uint8)

  def check_errors(self):
    self.log.append(('env_check',))


class FakePopTrainer:
  """PopulationPPOTrainer's face towards run_pbt_loop_vec; the hyperparameter tensors are real (CPU), copy and scale act on them."""
  gamma, lam, normalize_advantage, members = 0.75, 0.5, True, P

  def __init__(self, log):
    self.log, self.acts = log, 0
    self.lr = torch.tensor([1.0, 2.0, 4.0, 8.0])
    self.entropy_coef = torch.tensor([0.5, 0.25, 0.125, 0.0625])

  def act(self, obs, out, logp, value):
    out.fill_(self.acts % 3)
    logp.fill_(-float(self.acts))
    value.fill_(float(self.acts))
    self.log.append(('act', self.acts, obs.clone()))
    self.acts += 1
    return out

  def capture(self, batch):
    self.log.append(('update', 'capture', batch))
    return torch.ones(P * 2)

  def train_step(self, batch):
    self.log.append(('update', 'train_step', batch))
    return torch.full((P * 2,), 3.0)

  def copy_members(self, src, dst):
    self.log.append(('copy', src.tolist(), dst.tolist()))
    for t in (self.lr, self.entropy_coef):
      t[dst] = t[src]

  def scale_hyper(self, name, dst, factor):
    self.log.append(('scale', name, dst.tolist(), factor.tolist()))
    getattr(self, name)[dst] *= factor

  def check_errors(self):
    self.log.append(('trainer_check',))


class FakePopRollout:
  members, rows_per_member, horizon, num_envs = P, R, T, P * R

  def __init__(self, log):
    self.log, self.passes = log, 0

  def add(self, t, obs, action, logp, value, reward, terminal, episode_end=None):
    self.log.append(('add', t, action.clone(), reward.clone(), terminal.clone(), episode_end.clone()))

  def finish(self, boot_value, gamma, lam, normalize=True):
    self.log.append(('finish', boot_value.clone(), gamma, lam, normalize))

  def minibatches(self, batch_size):
    self.log.append(('pass', self.passes, batch_size))
    p, self.passes = self.passes, self.passes + 1
    for k in range(T * R // batch_size):
      yield (p, k)


Log = lf.Log
