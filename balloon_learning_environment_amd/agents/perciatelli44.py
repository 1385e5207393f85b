"""Perciatelli44 (agents/perciatelli44.py of the reference): the frozen QR-DQN agent of Bellemare et al. (2020), in eval mode.

The reference loads a serialised TensorFlow graph shipped with its package; that graph -- the weights -- is not part of this
package.  Pass the parameters in the flax form QuantileAgent.load_perciatelli_weights builds (8 Dense layers: 1099 -> 600 x 7 -> 3 x 51),
as a tree (params=...) or as qnet.QNetwork.save_npz's file (params_path=...).
"""
from typing import Sequence

from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import quantile_agent


class Perciatelli44(quantile_agent.QuantileAgent):
  """Perciatelli44 Agent: frozen weights, for comparison in evaluation, not for retraining."""

  def __init__(self, num_actions: int, observation_shape: Sequence[int], params=None, params_path=None, device='cuda:0'):
    if num_actions != 3:
      raise ValueError('Perciatelli44 only supports 3 actions.')
    if list(observation_shape) != [1099]:
      raise ValueError('Perciatelli44 only supports 1099 dimensional input.')
    if params is None and params_path is None:
      raise FileNotFoundError('Perciatelli44: its weights are not shipped with this package; pass params= (the flax parameter tree) '
                              'or params_path= (a file written by qnet.QNetwork.save_npz)')
    if params is None:
      params = qnet.QNetwork.from_npz(params_path, device=device)
    super().__init__(num_actions, observation_shape, params=params, device=device)
