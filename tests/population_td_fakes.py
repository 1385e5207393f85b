"""Recording fakes of a population's environment, replay learner and replay ring on CPU tensors, for the schedule of
train_lib.run_population_training_loop_vec (test_population_td_loop_host.py), in the manner of loop_fakes.py and pbt_host.py: every call
appends a tuple to one shared log, with clones of the tensors it was handed.  TEST TOOLING."""
import torch

from loop_fakes import Log                              # noqa: F401  (re-exported: the tests build one)

P, R = 2, 3                                             # members, environments per member
N = P * R
LIMIT = 4                                               # max_episode_length: every environment's episode ends on its 4th step
BATCH = 2                                               # rows per member of an update
FIRST_LOSS, LATER_LOSS = (1.0, 5.0), (3.0, 7.0)         # per member: the captured (first) update's row losses, every later one's


def reward_of(step):
  """Environment e earns e at every step: member 0's episodes return 0, 4, 8 (mean 4), member 1's 12, 16, 20 (mean 16)."""
  return torch.arange(N, dtype=torch.float32)


class FakePopEnv:
  """Step s returns the observation full of s + 1 (reset: 0), reward_of(s) and no terminal."""
  num_envs, device = N, torch.device('cpu')

  def __init__(self, log):
    self.log, self.s = log, 0

  def _obs(self):
    return torch.full((N, 2), float(self.s))

  def reset(self):
    self.log.append(('reset',))
    return self._obs()

  def step(self, actions, end_mask=None):
    s = self.s
    self.log.append(('step', s, actions.clone(), end_mask.clone()))
    self.s += 1
    return self._obs(), reward_of(s), torch.zeros(N, dtype=torch.uint8)

  def check_errors(self):
    self.log.append(('env_check',))


def _losses(per_member, batch_size):
  return torch.cat([torch.full((batch_size,), v) for v in per_member])


class FakePopQTrainer:
  """PopulationQTrainer's face towards the loop: act k writes the actions (k + e) % 3; copy_members and scale_hyper act on lr."""
  members = P

  def __init__(self, log):
    self.log, self.acts = log, 0
    self.seeds = torch.tensor([11, 12], dtype=torch.int64)
    self.lr = torch.tensor([1.0, 2.0])

  def act(self, obs, out):
    out.copy_(torch.tensor([(self.acts + e) % 3 for e in range(N)], dtype=torch.uint8))
    self.log.append(('act', self.acts, obs.clone()))
    self.acts += 1
    return out

  def capture(self, replay, batch_size):
    self.log.append(('update', 'capture', batch_size))
    return _losses(FIRST_LOSS, batch_size)

  def train_step(self, replay, batch_size):
    self.log.append(('update', 'train_step', batch_size))
    return _losses(LATER_LOSS, batch_size)

  def sync_target(self):
    self.log.append(('sync',))

  def check_errors(self):
    self.log.append(('trainer_check',))

  def copy_members(self, src, dst):
    self.log.append(('copy', src.tolist(), dst.tolist()))
    self.lr.index_copy_(0, dst, self.lr.index_select(0, src))

  def scale_hyper(self, name, dst, factor):
    self.log.append(('scale', name, dst.tolist(), factor.tolist()))
    assert name == 'lr'
    self.lr.index_copy_(0, dst, self.lr.index_select(0, dst) * factor)


class FakePopReplay:
  members, rows_per_member, num_envs = P, R, N

  def __init__(self, log, update_horizon=1):
    self.log, self.cursor, self.update_horizon = log, 0, update_horizon

  def add(self, obs, action, reward, terminal, episode_end=None):
    self.log.append(('add', obs.clone(), action.clone(), reward.clone(), terminal.clone(), episode_end.clone()))
    self.cursor += 1

  def check_errors(self):
    self.log.append(('replay_check',))


def recording_explore(log):
  """A stand-in for qnet_train.explore_grouped: records (epsilon as a list, the seeds, the step); the actions stay."""
  def explore_grouped(actions, epsilon, seeds, step):
    eps = epsilon.tolist() if isinstance(epsilon, torch.Tensor) else epsilon
    log.append(('explore', eps, seeds.tolist(), step, actions.clone()))
    return actions
  return explore_grouped
