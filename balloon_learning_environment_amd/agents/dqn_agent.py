"""DQN on the device: Dopamine 4.0.0's JaxDQNAgent update (configs/dqn.gin of the reference) without JAX, and the reference-shaped
eval-mode agent.

`DQNTrainer` is a `QNetworkTrainer` (agents/qnet_train.py) for one-atom networks whose loss is DQN's own: the TD error
u = ret + discount max_a q_target(s')[a] - q(s)[action] through 'mse' (dqn.gin) or 'huber' (JaxDQNAgent's default), by
`ble_qnet_td_step_f32` (csrc/ble_train.h).  Everything else -- the uniform n-step replay, the target and online forwards,
backprop, Adam, graph capture, checkpoints -- is the parent's:

    trainer = DQNTrainer(qnet.QNetwork.from_params(qnet.init_params('mlp')))
    train_lib.run_training_loop_vec(env, trainer, VecReplayBuffer(env.num_envs, 1024), num_iterations=..., steps_per_iteration=...)

is configs/dqn.gin (Adam 2e-6 / 2e-5, gamma 0.993, horizon 5, epsilon 0.01, 500 / 4 / 100).
"""
from typing import Sequence

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import qnet_train
from balloon_learning_environment_amd.agents import quantile_agent

_KINDS = {'mse': _abi.TD_DQN_MSE, 'huber': _abi.TD_DQN_HUBER}


class DQNTrainer(qnet_train.QNetworkTrainer):
  """DQN training of a one-atom QNetwork's parameters on its device (defaults: configs/dqn.gin).  JaxDQNAgent has no priority rule,
  so a VecPrioritizedReplayBuffer is refused."""

  def __init__(self, network: qnet.QNetwork, *, loss_type: str = 'mse', lr: float = 2e-6, eps: float = 2e-5, gamma: float = 0.993,
               update_horizon: int = 5, seed: int = 0, b1: float = 0.9, b2: float = 0.999):
    if network.num_atoms != 1:
      raise ValueError(f'DQNTrainer trains one-atom networks (an MLPNetwork), not {network.num_atoms} atoms: QNetworkTrainer is QR-DQN')
    if loss_type not in _KINDS:
      raise ValueError(f"loss_type is 'mse' or 'huber', not {loss_type!r}")
    self.loss_type = loss_type
    super().__init__(network, lr=lr, eps=eps, gamma=gamma, update_horizon=update_horizon, seed=seed, b1=b1, b2=b2)

  def _td(self) -> _abi.BleTdF32:
    return _abi.BleTdF32(_KINDS[self.loss_type], _abi.TD_OPT_ADAM, 0.0, 0, None, None)

  def _update(self, replay: qnet_train.VecReplayBuffer, batch_size: int) -> torch.Tensor:
    if replay.prioritized:
      raise ValueError('DQNTrainer samples uniformly (JaxDQNAgent sets no priorities): use a VecReplayBuffer')
    return super()._update(replay, batch_size)

  def state_dict(self) -> dict:
    return {**super().state_dict(), 'loss_type': self.loss_type}

  def load_state_dict(self, d: dict) -> None:
    loss_type = d.get('loss_type', self.loss_type)
    if loss_type not in _KINDS:
      raise ValueError(f"loss_type is 'mse' or 'huber', not {loss_type!r}")
    if loss_type != self.loss_type:
      self._graphs.clear()                     # (the loss kind is an argument of the captured launches)
    self.loss_type = loss_type
    super().load_state_dict(d)


class DQNAgent(quantile_agent.QuantileAgent):
  """The reference's DQNAgent (agents/dqn_agent.py) in eval mode: the greedy policy of a one-atom network, one decision per call.
  Training is DQNTrainer with train_lib.run_training_loop_vec; its network() loads here through params=."""

  def __init__(self, num_actions: int, observation_shape: Sequence[int], *, params=None, device='cuda:0'):
    super().__init__(num_actions, observation_shape, params=params, num_atoms=1, device=device)
    if self.network.num_atoms != 1:
      raise ValueError(f'DQNAgent needs a one-atom network, not {self.network.num_atoms} atoms (QuantileAgent is QR-DQN)')
