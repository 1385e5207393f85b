"""Recording fakes of an environment, the learners and their buffers on CPU tensors, for the schedules of train_lib's loops
(test_collect_host.py: run_training_loop_vec; test_ppo_host.py: run_ppo_loop_vec).  Every call appends a tuple to one shared log, with
clones of the tensors it was handed.  TEST TOOLING."""
import torch

N_ENV = 3
TERMINALS = {(0, 1), (1, 2), (5, 0)}                   # (step, env): staggers the three episode clocks
# max_episode_length = 4: an environment's end_mask is set on the 4th step of its own episode
END_MASK = {3: (1, 0, 0), 4: (0, 1, 0), 5: (0, 0, 1), 8: (0, 1, 0), 9: (1, 0, 1), 12: (0, 1, 0), 13: (1, 0, 1)}


class Log(list):
  def named(self, name):
    return [e[1:] for e in self if e[0] == name]


def u8(values):
  return torch.tensor(values, dtype=torch.uint8)


def reward_of(step):
  return torch.tensor([1.0, 0.25, 0.0]) + step


class FakeEnv:
  """Step s returns the observation full of s + 1 (reset: 0), reward_of(s) and the terminals of TERMINALS."""
  num_envs, device = N_ENV, torch.device('cpu')

  def __init__(self, log):
    self.log, self.s = log, 0

  def _obs(self):
    return torch.full((N_ENV, 2), float(self.s))

  def reset(self):
    self.log.append(('reset',))
    return self._obs()

  def step(self, actions, end_mask=None):
    s = self.s
    terminal = torch.tensor([1 if (s, e) in TERMINALS else 0 for e in range(N_ENV)], dtype=torch.uint8)
    reward = reward_of(s)
    self.log.append(('step', s, actions.clone(), end_mask.clone(), terminal.clone()))
    self.s += 1
    return self._obs(), reward, terminal

  def check_errors(self):
    self.log.append(('env_check',))


class FakeTrainer:
  """A replay learner: act k writes the actions (k + e) % 3."""

  def __init__(self, log):
    self.log, self.acts = log, 0

  def act(self, obs, out):
    out.copy_(torch.tensor([(self.acts + e) % 3 for e in range(N_ENV)], dtype=torch.uint8))
    self.log.append(('act', self.acts, obs.clone()))
    self.acts += 1
    return out

  def capture(self, replay, batch_size):
    self.log.append(('update', 'capture', batch_size))
    return torch.ones(batch_size)

  def train_step(self, replay, batch_size):
    self.log.append(('update', 'train_step', batch_size))
    return torch.full((batch_size,), 3.0)

  def sync_target(self):
    self.log.append(('sync',))

  def check_errors(self):
    self.log.append(('trainer_check',))


class FakeReplay:
  num_envs = N_ENV

  def __init__(self, log, update_horizon=4):
    self.log, self.cursor, self.update_horizon = log, 0, update_horizon

  def add(self, obs, action, reward, terminal, episode_end=None):
    self.log.append(('add', obs.clone(), action.clone(), reward.clone(), terminal.clone(), episode_end.clone()))
    self.cursor += 1

  def check_errors(self):
    self.log.append(('replay_check',))


# ---- the on-policy loop --------------------------------------------------------------------------------------------------------------
def ppo_act(k):
  """What FakePPOTrainer's act k writes: (actions, logp, value)."""
  e = torch.arange(N_ENV, dtype=torch.float32)
  return u8([(k + i) % 3 for i in range(N_ENV)]), -(k + e / 8), 100.0 * k + e


class FakePPOTrainer:
  """PPOTrainer's face towards run_ppo_loop_vec: act k writes ppo_act(k) into the loop's static buffers."""
  gamma, lam, normalize_advantage = 0.75, 0.5, True

  def __init__(self, log):
    self.log, self.acts = log, 0

  def act(self, obs, out, logp, value):
    a, l, v = ppo_act(self.acts)
    out.copy_(a)
    logp.copy_(l)
    value.copy_(v)
    self.log.append(('act', self.acts, obs.clone()))
    self.acts += 1
    return out

  def capture(self, batch):
    self.log.append(('update', 'capture', batch))
    return torch.ones(4)

  def train_step(self, batch):
    self.log.append(('update', 'train_step', batch))
    return torch.full((4,), 3.0)

  def check_errors(self):
    self.log.append(('trainer_check',))


class FakeRollout:
  """VecRolloutBuffer's face towards the loop: a pass yields T N // batch_size tokens (pass, k)."""
  num_envs = N_ENV

  def __init__(self, log, horizon):
    self.log, self.horizon, self.passes = log, horizon, 0

  def add(self, t, obs, action, logp, value, reward, terminal, episode_end=None):
    self.log.append(('add', t, obs.clone(), action.clone(), logp.clone(), value.clone(), reward.clone(), terminal.clone(),
                     episode_end.clone()))

  def finish(self, boot_value, gamma, lam, normalize=True):
    self.log.append(('finish', boot_value.clone(), gamma, lam, normalize))

  def minibatches(self, batch_size):
    self.log.append(('pass', self.passes, batch_size))
    p, self.passes = self.passes, self.passes + 1
    for k in range(self.horizon * N_ENV // batch_size):
      yield (p, k)
