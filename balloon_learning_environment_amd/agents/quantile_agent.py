"""QuantileAgent (agents/quantile_agent.py of the reference) in eval mode: the greedy policy of a QR-DQN network on the device.

The reference's agent trains Dopamine's JaxQuantileAgent; here only its eval-mode decision exists (epsilon_eval = 0: q = the mean of
each action's atoms, argmax), on `ble_qnet_forward_f32` at N = 1 -- the kernel VecQNetworkAgent runs on a batch, so a serial decision
is the batched one bit for bit.  This agent does not train: set_mode('train') raises NotImplementedError.  Batched training
(replay, optimiser, target network, exploration) is agents/qnet_train.py with train_lib.run_training_loop_vec; its
QNetworkTrainer.network() loads here through params=.
"""
from typing import Optional, Sequence, Union

import numpy as np
import torch

from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd.agents import agent
from balloon_learning_environment_amd.agents import qnet


class QuantileAgent(agent.Agent):
  """A QR-DQN (or, with one atom, DQN) policy in eval mode.

  params: the network's flax parameter tree ({'params': {'Dense_i': {'kernel', 'bias'}}}, see qnet.QNetwork.from_params) or a
  QNetwork; num_atoms: as QNetwork.from_params (default: the last layer's width / 3)."""

  def __init__(self, num_actions: int, observation_shape: Sequence[int], *, params=None, num_atoms: Optional[int] = None,
               device='cuda:0'):
    if num_actions != qnet.NUM_ACTIONS:
      raise ValueError(f'{type(self).__name__} only supports {qnet.NUM_ACTIONS} actions.')
    if list(observation_shape) != [_lib.OBS_DIM]:
      raise ValueError(f'{type(self).__name__} only supports {_lib.OBS_DIM} dimensional input.')
    if params is None:
      raise ValueError(f'{type(self).__name__} needs the network parameters (params=...): this package does not train')
    network = params if isinstance(params, qnet.QNetwork) else qnet.QNetwork.from_params(params, num_atoms=num_atoms, device=device)
    self._vec = qnet.VecQNetworkAgent(network)
    self.network = network
    self.device = self._vec.device
    with torch.cuda.device(self.device):
      self._obs = torch.zeros(1, _lib.OBS_DIM, dtype=torch.float32, device=self.device)
      self._action = torch.zeros(1, dtype=torch.uint8, device=self.device)
      self._q = torch.zeros(1, qnet.NUM_ACTIONS, dtype=torch.float32, device=self.device)
    super().__init__(num_actions, observation_shape)
    self.set_mode(agent.AgentMode.EVAL)

  def set_mode(self, mode: Union[agent.AgentMode, str]) -> None:
    mode = agent.AgentMode(mode)
    if mode != agent.AgentMode.EVAL:
      if getattr(self, '_constructed', False):
        raise NotImplementedError(f'{type(self).__name__} runs in eval mode only: this package does not train')
      return                       # (the base class's constructor sets TRAIN before the agent has its network)
    self._constructed = True
    self.eval_mode = True

  def q_values(self, observation) -> np.ndarray:
    """The network's q-values [3] for one observation (float32)."""
    self._run(observation)
    return self._q[0].cpu().numpy()

  def _run(self, observation) -> int:
    if isinstance(observation, torch.Tensor):
      o = observation.detach().to(self.device, torch.float32).reshape(1, -1)
    else:
      o = torch.from_numpy(np.ascontiguousarray(np.asarray(observation, np.float32).reshape(1, -1)))
    self._obs.copy_(o)
    self._vec.act(self._obs, out=self._action, q_values=self._q)
    return int(self._action.item())

  def begin_episode(self, observation: np.ndarray) -> int:
    self.action = self._run(observation)
    return self.action

  def step(self, reward: float, observation: np.ndarray) -> int:
    del reward
    self.action = self._run(observation)
    return self.action

  def end_episode(self, reward: float, terminal: bool = True) -> None:
    pass
