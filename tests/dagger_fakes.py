"""Recording fakes of an imitation learner and an expert on CPU tensors, beside loop_fakes.py (whose environment, rollout and log they
share), for the schedule of train_lib.run_dagger_loop_vec (test_dagger_loop_host.py).  TEST TOOLING."""
import torch

import loop_fakes as lf

N_ENV = lf.N_ENV


def label_of(obs):
  """What FakeExpert says on an observation (FakeEnv's is full of the step index s): (2 s + e + 1) % 3 -- it differs from one
  observation to the next in every environment."""
  s = int(obs[0, 0].item())
  return lf.u8([(2 * s + e + 1) % 3 for e in range(N_ENV)])


def took_of(k):
  """The draw of FakeBCTrainer's mix number k: environment e flies the expert's action when (k + e) is even."""
  return lf.u8([(k + e + 1) % 2 for e in range(N_ENV)])


def agree_of(k):
  """aux[:, 1] after update number k (four rows)."""
  return torch.tensor([1.0, 1.0, 0.0, 1.0]) if k % 2 else torch.tensor([0.0, 1.0, 0.0, 0.0])


class FakeExpert:
  def __init__(self, log, checks=True):
    self.log = log
    if checks:
      self.check_errors = lambda: self.log.append(('expert_check',))

  def act(self, obs, out):
    out.copy_(label_of(obs))
    self.log.append(('expert', obs.clone()))
    return out


class FakeBCTrainer:
  """BCTrainer's face towards run_dagger_loop_vec: act k writes loop_fakes.ppo_act(k); mix k flies took_of(k)."""

  def __init__(self, log):
    self.log, self.acts, self.mixes, self.updates = log, 0, 0, 0

  def act(self, obs, out, logp, value):
    a, l, v = lf.ppo_act(self.acts)
    out.copy_(a)
    logp.copy_(l)
    value.copy_(v)
    self.log.append(('act', self.acts, obs.clone()))
    self.acts += 1
    return out

  def mix(self, learner_actions, expert_actions, beta, out=None, took_expert=None):
    took = took_of(self.mixes)
    self.log.append(('mix', self.mixes, learner_actions.clone(), expert_actions.clone(), beta))
    out.copy_(torch.where(took.bool(), expert_actions, learner_actions))
    if took_expert is not None:
      took_expert.copy_(took)
    self.mixes += 1
    return out

  def _update(self, kind, batch):
    self.log.append(('update', kind, batch))
    self.updates += 1

  def capture(self, batch):
    self._update('capture', batch)
    return torch.ones(4)

  def train_step(self, batch):
    self._update('train_step', batch)
    return torch.full((4,), 3.0)

  def views(self, batch_size):
    assert self.updates > 0
    self.log.append(('views', batch_size))
    agree = agree_of(self.updates - 1)
    return {'aux': torch.stack([torch.full((4,), -1.0), agree], dim=1)}

  def check_errors(self):
    self.log.append(('trainer_check',))
