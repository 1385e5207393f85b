"""Marco Polo exploration on the device: the reference's MarcoPoloExploration over a RandomWalkAgent (configs/quantile.gin), one lane
per environment of a VecBalloonEnv (ble_marco_polo_u8, csrc/ble_explore.h).

An episode is exploratory with probability exploratory_episode_probability.  It starts in the RL phase (the agent's actions), and an
exploratory episode alternates 4 h of RL with 2 h of a random walk in pressure: a target drawn in [6500, 11400) Pa at the episode's
begin drifts by (seconds walked) x 0.1666 x N(0, 1) per exploratory step, and the balloon goes UP / DOWN / STAY with 100 Pa of
hysteresis around it.  The draws come from Philox keyed by (seed, environment, step), not from JAX's stream.
"""
import ctypes

import numpy as np
import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import qnet_train


class VecMarcoPoloExploration:
  """explorer(obs, actions, begin) rewrites the uint8 device actions in place: begin (uint8 [N], nonzero where obs is an episode's
  first observation) runs begin_episode on those lanes, every other lane steps.  No host synchronisation: capturable in a graph (the
  step counter that keys the draws is device memory)."""

  def __init__(self, num_envs: int, exploratory_episode_probability: float = 0.8, seed: int = 0, device='cuda:0'):
    self.device = dev.require_gpu(device)
    self.num_envs, self.probability, self.seed = int(num_envs), float(exploratory_episode_probability), int(seed)
    if not 0.0 <= self.probability <= 1.0:
      raise ValueError('exploratory_episode_probability must be in [0, 1]')
    n, d = self.num_envs, self.device
    with torch.cuda.device(d):
      self.step = torch.zeros(1, dtype=torch.int64, device=d)          # (read as uint64 by the kernel)
      self.phase_clock = torch.zeros(n, dtype=torch.int32, device=d)
      self.walk_clock = torch.zeros(n, dtype=torch.int32, device=d)
      self.exploratory_episode = torch.zeros(n, dtype=torch.uint8, device=d)
      self.exploratory_phase = torch.zeros(n, dtype=torch.uint8, device=d)
      self.target = torch.zeros(n, dtype=torch.float64, device=d)

  @dev.on_own_device
  def __call__(self, obs: torch.Tensor, actions: torch.Tensor, begin: torch.Tensor) -> torch.Tensor:
    n = self.num_envs
    assert obs.shape[0] == n and actions.numel() == n and begin.numel() == n, 'one lane per environment'
    assert obs.dtype == torch.float32 and actions.dtype == torch.uint8 and begin.dtype == torch.uint8
    stride = obs.stride(0) if obs.dim() > 1 else 1
    mp = _abi.BleMarcoPoloF32(n, stride, 0, self.probability, self.seed & (2 ** 64 - 1), obs.data_ptr(), begin.data_ptr(),
                              self.step.data_ptr(), self.phase_clock.data_ptr(), self.walk_clock.data_ptr(),
                              self.exploratory_episode.data_ptr(), self.exploratory_phase.data_ptr(), self.target.data_ptr())
    _lib.call('ble_marco_polo_u8', ctypes.byref(mp), actions.data_ptr(), dev.stream_ptr(self.device))
    return actions

  _STATE = ('step', 'phase_clock', 'walk_clock', 'exploratory_episode', 'exploratory_phase', 'target')

  def state_dict(self) -> dict:
    return {'num_envs': self.num_envs, 'probability': self.probability, 'seed': self.seed,
            **{k: getattr(self, k).clone() for k in self._STATE}}

  def load_state_dict(self, d: dict) -> None:
    """Restores in place (tensors keep their addresses)."""
    assert int(d['num_envs']) == self.num_envs
    self.probability, self.seed = float(d['probability']), int(d['seed'])
    for k in self._STATE:
      getattr(self, k).copy_(d[k])


def _probabilities(probability, members: int) -> np.ndarray:
  """A scalar or a length-P sequence as float64 [P], each in [0, 1] (the entry point cannot see device values)."""
  a = np.asarray(probability, np.float64)
  a = np.full(members, float(a)) if a.ndim == 0 else a.reshape(-1)
  if a.shape != (members,):
    raise ValueError(f'exploratory_episode_probability: a scalar or {members} values, not {a.shape[0]}')
  if not ((a >= 0.0) & (a <= 1.0)).all():
    raise ValueError(f'exploratory_episode_probability must be in [0, 1], not {a.tolist()}')
  return a


class VecPopulationMarcoPoloExploration:
  """Marco Polo exploration for a population of P members of R environments each (ble_marco_polo_grouped_u8):
  explorer(obs, actions, begin) is VecMarcoPoloExploration's call over the P * R rows of the population's VecBalloonEnv, rows
  [p R, (p + 1) R) member p's.  Row p R + r draws from the stream of (seeds[p], r, step) and its episodes are exploratory with
  probability[p]: member p's rows and state hold the bytes its own VecMarcoPoloExploration(R, probability[p], seeds[p]) holds
  (member(p)).  exploratory_episode_probability: a scalar or P values in [0, 1], validated here, then uploaded; seeds: a device int64
  [P] tensor (qnet_train.member_seeds; a PopulationQTrainer's `seeds` may be passed) or what member_seeds takes.  The state belongs to
  the environment rows: a PBT copy of a member's parameters leaves it where it is."""

  def __init__(self, members: int, rows_per_member: int, exploratory_episode_probability=0.8, seeds=0, device='cuda:0'):
    self.device = dev.require_gpu(device)
    self.members, self.rows_per_member = int(members), int(rows_per_member)
    if self.members < 1 or self.rows_per_member < 1:
      raise ValueError('a population explorer has at least one member of at least one environment')
    self.num_envs = n = self.members * self.rows_per_member
    d = self.device
    host = _probabilities(exploratory_episode_probability, self.members)
    with torch.cuda.device(d):
      self.probability = torch.from_numpy(host).to(d)
      if isinstance(seeds, torch.Tensor):
        if seeds.dtype != torch.int64 or seeds.numel() != self.members:
          raise ValueError(f'seeds: an int64 tensor of {self.members} values')
        self.seeds = seeds.detach().to(d).contiguous().clone()
      else:
        self.seeds = qnet_train.member_seeds(seeds, self.members, d)
      self.step = torch.zeros(1, dtype=torch.int64, device=d)          # (read as uint64 by the kernel)
      self.phase_clock = torch.zeros(n, dtype=torch.int32, device=d)
      self.walk_clock = torch.zeros(n, dtype=torch.int32, device=d)
      self.exploratory_episode = torch.zeros(n, dtype=torch.uint8, device=d)
      self.exploratory_phase = torch.zeros(n, dtype=torch.uint8, device=d)
      self.target = torch.zeros(n, dtype=torch.float64, device=d)

  @dev.on_own_device
  def __call__(self, obs: torch.Tensor, actions: torch.Tensor, begin: torch.Tensor) -> torch.Tensor:
    n = self.num_envs
    assert obs.shape[0] == n and actions.numel() == n and begin.numel() == n, 'one lane per environment'
    assert obs.dtype == torch.float32 and actions.dtype == torch.uint8 and begin.dtype == torch.uint8
    stride = obs.stride(0) if obs.dim() > 1 else 1
    mp = _abi.BleMarcoPoloGroupedF32(n, stride, 0, self.members, self.probability.data_ptr(), self.seeds.data_ptr(), obs.data_ptr(),
                                     begin.data_ptr(), self.step.data_ptr(), self.phase_clock.data_ptr(), self.walk_clock.data_ptr(),
                                     self.exploratory_episode.data_ptr(), self.exploratory_phase.data_ptr(), self.target.data_ptr())
    _lib.call('ble_marco_polo_grouped_u8', ctypes.byref(mp), actions.data_ptr(), dev.stream_ptr(self.device))
    return actions

  _LANES = ('phase_clock', 'walk_clock', 'exploratory_episode', 'exploratory_phase', 'target')
  _STATE = ('step',) + _LANES + ('probability', 'seeds')

  def member(self, p: int) -> VecMarcoPoloExploration:
    """Member p's explorer on its own: a VecMarcoPoloExploration(R, probability[p], seeds[p]) holding a copy of the slice's state."""
    p = int(p)
    if not 0 <= p < self.members:
      raise IndexError(f'member {p} of a population of {self.members}')
    r = self.rows_per_member
    solo = VecMarcoPoloExploration(r, float(self.probability[p].item()), int(self.seeds[p].item()) & (2 ** 64 - 1), self.device)
    solo.step.copy_(self.step)
    for k in self._LANES:
      getattr(solo, k).copy_(getattr(self, k)[p * r:(p + 1) * r])
    return solo

  def state_dict(self) -> dict:
    return {'members': self.members, 'rows_per_member': self.rows_per_member, **{k: getattr(self, k).clone() for k in self._STATE}}

  def load_state_dict(self, d: dict) -> None:
    """Restores in place (tensors keep their addresses: captured graphs stay valid)."""
    assert (int(d['members']), int(d['rows_per_member'])) == (self.members, self.rows_per_member), 'checkpoint of another population'
    for k in self._STATE:
      getattr(self, k).copy_(d[k])
