"""The MLP agent (agents/mlp_agent.py of the reference) on the device: online SARSA with optax.sgd, the gradient through both Q terms.

The reference's agent acts greedily, then trains on (last_state, last_action, reward, state, action) with
loss = (q(s)[a] - (r + gamma q(s')[a']))^2, both terms from the parameters being differentiated, and plain SGD.  `VecMLPAgent` does
that for N environments that share one network: one `ble_qnet_forward_f32` for the actions (the pre-update parameters: the reference
selects, then trains) and one `ble_qnet_td_step_f32` (csrc/ble_train.h) for the update, whose objective is the mean of the
N rows' losses -- at N = 1 the reference's update exactly.  A row whose episode has just ended is masked (the reference's end_episode
does not train, and the next call is begin_episode): it adds nothing to the gradient but still counts in N.  `MLPAgent` is the
reference's class over VecMLPAgent(1).
"""
import time
from typing import Optional, Sequence, Union

import numpy as np
import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import agent
from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import qnet_train

ROW_FLOATS = qnet_train.ROW_FLOATS


class VecMLPAgent(qnet_train.QNetworkLearner):
  """SARSA over N environments and one shared one-atom network (default: the reference's mlp.gin, a single Dense 1099 -> 3).

    agent = VecMLPAgent(env.num_envs)
    actions = agent.begin_episode(env.reset())
    obs, reward, terminal = env.step(actions)
    actions = agent.step(reward, obs, episode_end=terminal)      # acts, then (train mode) one SARSA update + SGD

  The actions returned are a uint8 [N] device buffer the next call overwrites; `loss` holds the last update's per-row losses.  No call
  synchronises with the host.  capture() records step()'s device work as one HIP graph that later steps replay."""

  _TENSORS = ('weights', 'last_obs', 'last_action')

  def __init__(self, num_envs: int, network: Optional[qnet.QNetwork] = None, *, gamma: float = 0.9, learning_rate: float = 0.001,
               seed: int = 0, device='cuda:0'):
    if network is None:
      network = qnet.QNetwork.from_params(qnet.init_params('mlp', seed, num_layers=1), device=device)
    if network.num_atoms != 1:
      raise ValueError(f'VecMLPAgent trains one-atom networks (an MLPNetwork), not {network.num_atoms} atoms')
    self.num_envs = n = int(num_envs)
    if n < 1:
      raise ValueError('num_envs >= 1')
    self.gamma, self.lr, self.seed = float(gamma), float(learning_rate), int(seed)
    self._sarsa = _abi.BleTdF32(_abi.TD_SARSA_MSE, _abi.TD_OPT_SGD, self.gamma, 0, None, None)
    super().__init__(network)
    d = self.device
    with torch.cuda.device(d):
      self.last_obs = torch.zeros(n, ROW_FLOATS, dtype=torch.float32, device=d)      # s, then (after a step) s'
      self.obs = torch.zeros(n, ROW_FLOATS, dtype=torch.float32, device=d)           # s'
      self.last_action = torch.zeros(n, dtype=torch.uint8, device=d)
      self.action = torch.zeros(n, dtype=torch.uint8, device=d)
      self.reward = torch.zeros(n, dtype=torch.float32, device=d)
      self.mask = torch.zeros(n, dtype=torch.uint8, device=d)
      self.loss = torch.zeros(n, dtype=torch.float32, device=d)
      self._sarsa.next_action, self._sarsa.mask = self.action.data_ptr(), self.mask.data_ptr()
      self._batch = _abi.BleTrainBatchF32(n, ROW_FLOATS, self.last_obs.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(),
                                          self.reward.data_ptr(), self.last_action.data_ptr(), None)      # (discount is not read)
      self.layout = self._layout(n)
      self.workspace = torch.zeros(max(self.layout.total, 64), dtype=torch.float32, device=d)
    self._mode = agent.AgentMode.TRAIN
    self._begun = False

  learning_rate = property(lambda self: self.lr)

  # ---- plumbing
  def _td(self) -> _abi.BleTdF32:
    return self._sarsa

  def _load(self, dst: torch.Tensor, obs: torch.Tensor) -> None:
    assert obs.dim() == 2 and obs.shape[0] == self.num_envs and obs.shape[1] >= _lib.OBS_DIM, tuple(obs.shape)
    dst[:, :_lib.OBS_DIM].copy_(obs[:, :_lib.OBS_DIM])

  def views(self) -> dict:
    """The workspace's tensors of the last update: 'acts' (layer l: [2, N, ld], the state branch then the next_state branch), 'logits'
    [2, N, 3], 'targets' [N], 'dlogits' [2, N, ld], 'loss' [N]."""
    n, lay, ws = self.num_envs, self.layout, self.workspace
    ld = lay.ld
    acts = [ws[lay.acts + 2 * l * n * ld:lay.acts + 2 * (l + 1) * n * ld].view(2, n, ld) for l in range(self.num_layers)]
    return {'acts': acts, 'logits': acts[-1][:, :, :qnet.NUM_ACTIONS], 'targets': ws[lay.targets:lay.targets + n],
            'dlogits': ws[lay.dlogits:lay.dlogits + 2 * n * ld].view(2, n, ld), 'loss': self.loss}

  # ---- the agent
  def set_mode(self, mode: Union[agent.AgentMode, str]) -> None:
    self._mode = agent.AgentMode(mode)

  @dev.on_own_device
  def begin_episode(self, obs: torch.Tensor) -> torch.Tensor:
    """The first observations of N episodes [N, >= 1099] -> their greedy actions (uint8 [N], a buffer the next call overwrites)."""
    self._load(self.last_obs, obs)
    self._forward(self.last_obs, self.last_action)
    self._begun = True
    return self.last_action

  @dev.on_own_device
  def train_on_transitions(self, apply_update: bool = True) -> torch.Tensor:
    """One SARSA update on the agent's own buffers (last_obs, last_action, reward, obs, action, mask): the per-row losses [N]."""
    self._launch_update(self.workspace, self._batch, self.loss, apply_update)
    return self.loss

  def _body(self, train: bool) -> None:
    """step()'s device work on the input buffers: the actions with the pre-update parameters, the update, then s, a <- s', a'."""
    self._forward(self.obs, self.action)
    if train:
      self.train_on_transitions()
    self.last_obs.copy_(self.obs)
    self.last_action.copy_(self.action)

  @dev.on_own_device
  def step(self, reward: torch.Tensor, obs: torch.Tensor, episode_end: Optional[torch.Tensor] = None) -> torch.Tensor:
    """reward [N] and obs [N, >= 1099] of the step just taken -> the next greedy actions.  episode_end[i] != 0: that step ended
    environment i's episode and obs[i] opens a new one -- row i is not trained on."""
    if not self._begun:
      raise RuntimeError('VecMLPAgent.step before begin_episode')
    self._load(self.obs, obs)
    self.reward.copy_(reward)
    if episode_end is None:
      self.mask.zero_()
    else:
      self.mask.copy_(episode_end)
    train = self._mode == agent.AgentMode.TRAIN
    graph = self._graphs.get(train)
    if graph is not None:
      graph.replay()
    else:
      self._body(train)
    return self.last_action

  @dev.on_own_device
  def capture(self) -> None:
    """Records step()'s device work in the current mode into a HIP graph that step() replays from then on (the inputs are copied into
    the agent's own buffers first, so any tensors can be passed).  Call after begin_episode; the capture itself runs nothing."""
    if not self._begun:
      raise RuntimeError('VecMLPAgent.capture before begin_episode (the forward scratch is allocated there)')
    train = self._mode == agent.AgentMode.TRAIN
    graph, _ = dev.capture(self.device, lambda: self._body(train))
    self._graphs[train] = graph

  # ---- checkpoints
  def state_dict(self) -> dict:
    return {**super().state_dict(), 'num_envs': self.num_envs, 'hyper': (self.gamma, self.lr), 'begun': self._begun,
            'mode': self._mode.value}

  def load_state_dict(self, d: dict) -> None:
    assert int(d['num_envs']) == self.num_envs, 'checkpoint of another number of environments'
    hyper = tuple(float(h) for h in d['hyper'])
    if hyper != (self.gamma, self.lr):
      self._graphs.clear()                     # (the hyperparameters are arguments of the captured launches)
    self.gamma, self.lr = hyper
    self._sarsa.gamma = self.gamma
    self._begun, self._mode = bool(d['begun']), agent.AgentMode(d['mode'])
    super().load_state_dict(d)


class MLPAgent(agent.Agent):
  """The reference's MLPAgent: one environment, host observations in, an int action out; trains from construction (mode 'train')."""

  def __init__(self, num_actions: int, observation_shape: Sequence[int], gamma: float = 0.9, seed: Optional[int] = None):
    if num_actions != qnet.NUM_ACTIONS:
      raise ValueError(f'MLPAgent only supports {qnet.NUM_ACTIONS} actions.')
    if list(observation_shape) != [_lib.OBS_DIM]:
      raise ValueError(f'MLPAgent only supports {_lib.OBS_DIM} dimensional input.')
    seed = int(time.time() * 1e6) if seed is None else seed
    self._vec = VecMLPAgent(1, gamma=gamma, seed=seed)
    self.device = self._vec.device
    self._reward = torch.zeros(1, dtype=torch.float32, device=self.device)
    super().__init__(num_actions, observation_shape)

  def _obs(self, observation) -> torch.Tensor:
    if isinstance(observation, torch.Tensor):
      return observation.detach().to(self.device, torch.float32).reshape(1, -1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(observation, np.float32).reshape(1, -1))).to(self.device)

  def begin_episode(self, observation: np.ndarray) -> int:
    return int(self._vec.begin_episode(self._obs(observation)).item())

  def step(self, reward: float, observation: np.ndarray) -> int:
    self._reward.fill_(float(reward))
    return int(self._vec.step(self._reward, self._obs(observation)).item())

  def end_episode(self, reward: float, terminal: bool = True) -> None:
    pass

  def set_mode(self, mode: Union[agent.AgentMode, str]) -> None:
    self._vec.set_mode(mode)

  def network(self) -> qnet.QNetwork:
    return self._vec.network()
