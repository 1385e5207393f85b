"""Training QR-DQN / DQN policies on the device: Dopamine 4.0.0's JaxQuantileAgent update (configs/quantile.gin) without JAX.

`VecReplayBuffer` is an n-step replay ring of N environments stepped in lockstep (VecBalloonEnv's tensors, one ring column per
environment); `QNetworkLearner` is what every device learner holds (the online image, its gradient and transposed image, the update's
descriptors, acting, export, checkpoints); `QNetworkTrainer` adds the target image, Adam's moments and the device counters, and runs one
update -- uniform n-step sample, target and online forward, quantile Huber loss, backprop, Adam -- as a handful of HIP kernels
(csrc/ble_train.h) with no host synchronisation, capturable as one graph.  Every reduction has one order fixed by the
shapes and no kernel uses floating-point atomics: a run is a pure function of (initial parameters, replay contents, seeds).

With num_atoms == 1 the loss is the one-quantile QR loss, i.e. half the Huber loss of DQN's TD error (tau = 1/2); DQN's own losses
(Dopamine's 'mse' and 'huber') are agents/dqn_agent.py's DQNTrainer, a subclass of the trainer here.
"""
import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import qnet

ROW_FLOATS = 1104          # a stored observation row: the 1099 features zero-padded to a multiple of 4 (aligned float4 rows)
MAX_TRIES = 64


def _check_flags(flags: torch.Tensor) -> None:
  f = int(flags.item())
  if f:
    flags.zero_()
  if f & _lib.FLAG_REPLAY_EMPTY:
    raise RuntimeError('replay: no valid n-step window to sample (too few steps written, or every window crosses a time-limit end)')
  if f & _lib.FLAG_TRAIN_ACTION:
    raise ValueError('train step: a batch action is not below num_actions')
  if f & _lib.FLAG_REPLAY_PRIORITY:
    raise ValueError('set_priority: a non-finite or negative loss (its leaf was left unchanged)')


class TrainBatch:
  """One batch of B transitions on the device (what the sampler writes, what the train step reads).  A prioritized batch also holds
  each row's sampled priority and the weighted losses set_priority reports; both are None otherwise."""

  def __init__(self, batch_size: int, device, prioritized: bool = False):
    b = int(batch_size)
    self.batch_size = b
    self.state = torch.zeros(b, ROW_FLOATS, dtype=torch.float32, device=device)
    self.next_state = torch.zeros(b, ROW_FLOATS, dtype=torch.float32, device=device)
    self.ret = torch.zeros(b, dtype=torch.float32, device=device)
    self.discount = torch.zeros(b, dtype=torch.float32, device=device)
    self.action = torch.zeros(b, dtype=torch.uint8, device=device)
    self.index = torch.zeros(b, 2, dtype=torch.int64, device=device)
    self.priority = torch.zeros(max(b, 1), dtype=torch.float32, device=device)[:b] if prioritized else None
    self.weighted_loss = torch.zeros(max(b, 1), dtype=torch.float32, device=device)[:b] if prioritized else None
    self.struct = _abi.BleTrainBatchF32(b, ROW_FLOATS, self.state.data_ptr(), self.next_state.data_ptr(), self.ret.data_ptr(),
                                        self.discount.data_ptr(), self.action.data_ptr(), self.index.data_ptr())

  @classmethod
  def from_tensors(cls, state, next_state, ret, discount, action, device) -> 'TrainBatch':
    """A batch given on the host or device (state rows of 1099 features); for tests and offline data."""
    bt = cls(len(action), device)
    bt.state[:, :_lib.OBS_DIM].copy_(torch.as_tensor(np.asarray(state, np.float32)))
    bt.next_state[:, :_lib.OBS_DIM].copy_(torch.as_tensor(np.asarray(next_state, np.float32)))
    bt.ret.copy_(torch.as_tensor(np.asarray(ret, np.float32)))
    bt.discount.copy_(torch.as_tensor(np.asarray(discount, np.float32)))
    bt.action.copy_(torch.as_tensor(np.asarray(action, np.uint8)))
    bt.index.fill_(-1)
    return bt


class VecReplayBuffer:
  """The replay memory of N environments: a ring of capacity_steps vector steps (capacity_steps x num_envs transitions).

  add(obs, action, reward, terminal, episode_end) appends one VecBalloonEnv step: obs is the observation the actions were taken on,
  episode_end marks the steps that end an episode (a terminal or the time limit; default: terminal).  sample(B, seed, counter) draws B
  valid n-step windows uniformly (ble_replay_sample_f32): a window never reads past an episode's end, and one that reaches a time-limit
  end without a terminal is not drawn."""

  prioritized = False
  _TENSORS = ('obs', 'action', 'reward', 'terminal', 'episode_end', 'counter')      # the checkpoint's tensors

  def __init__(self, num_envs: int, capacity_steps: int, update_horizon: int = 5, gamma: float = 0.993, device='cuda:0'):
    self.device = dev.require_gpu(device)
    self.num_envs, self.capacity = int(num_envs), int(capacity_steps)
    self.update_horizon, self.gamma = int(update_horizon), float(gamma)
    if self.capacity < self.update_horizon + 1:
      raise ValueError(f'capacity_steps must be at least update_horizon + 1 = {self.update_horizon + 1}')
    t, n, d = self.capacity, self.num_envs, self.device
    with torch.cuda.device(d):
      self.obs = torch.zeros(t, n, ROW_FLOATS, dtype=torch.float32, device=d)
      self.action = torch.zeros(t, n, dtype=torch.uint8, device=d)
      self.reward = torch.zeros(t, n, dtype=torch.float32, device=d)
      self.terminal = torch.zeros(t, n, dtype=torch.uint8, device=d)
      self.episode_end = torch.zeros(t, n, dtype=torch.uint8, device=d)
      self.count = torch.zeros(1, dtype=torch.int64, device=d)
      self.counter = torch.zeros(1, dtype=torch.int64, device=d)        # (read as uint64 by the kernel)
      self.err_flags = torch.zeros(1, dtype=torch.int32, device=d)
    self.cursor = 0                      # host mirror of count
    self._batches: Dict[int, TrainBatch] = {}

  def __len__(self) -> int:
    """Transitions held."""
    return min(self.cursor, self.capacity) * self.num_envs

  def struct(self, counter: torch.Tensor) -> _abi.BleReplayF32:
    return _abi.BleReplayF32(self.capacity, self.num_envs, self.update_horizon, ROW_FLOATS, self.gamma, MAX_TRIES, 0, self.obs.data_ptr(),
                             self.action.data_ptr(), self.reward.data_ptr(), self.terminal.data_ptr(), self.episode_end.data_ptr(),
                             self.count.data_ptr(), counter.data_ptr())

  @dev.on_own_device
  def add(self, obs: torch.Tensor, action: torch.Tensor, reward: torch.Tensor, terminal: torch.Tensor,
          episode_end: Optional[torch.Tensor] = None) -> None:
    row = self.cursor % self.capacity
    self.obs[row, :, :_lib.OBS_DIM].copy_(obs[:, :_lib.OBS_DIM])
    self.action[row].copy_(action)
    self.reward[row].copy_(reward)
    self.terminal[row].copy_(terminal)
    self.episode_end[row].copy_(terminal if episode_end is None else episode_end)
    self.count.add_(1)
    self.cursor += 1

  def batch_buffers(self, batch_size: int) -> TrainBatch:
    return dev.first_use(self._batches, batch_size, lambda: TrainBatch(batch_size, self.device, self.prioritized),
                         f'VecReplayBuffer: sample once at batch size {batch_size} before capturing it in a graph')

  @dev.on_own_device
  def sample(self, batch_size: int, seed: int, counter: Optional[torch.Tensor] = None) -> TrainBatch:
    """B transitions into this buffer's batch buffers of that size (overwritten by the next sample at that size).  counter: the
    int64 [1] device update counter the draw is keyed by and advances (default: the buffer's own)."""
    bt = self.batch_buffers(int(batch_size))
    self._draw(self.struct(self.counter if counter is None else counter), bt, int(seed) & (2 ** 64 - 1))
    return bt

  def _draw(self, rp: _abi.BleReplayF32, bt: TrainBatch, seed: int) -> None:
    _lib.call('ble_replay_sample_f32', ctypes.byref(rp), ctypes.byref(bt.struct), seed, self.err_flags.data_ptr(),
              dev.stream_ptr(self.device))

  def check_errors(self) -> None:
    _check_flags(self.err_flags)

  def state_dict(self) -> dict:
    return {'num_envs': self.num_envs, 'capacity': self.capacity, 'update_horizon': self.update_horizon, 'gamma': self.gamma,
            'cursor': self.cursor, **{k: getattr(self, k).clone() for k in self._TENSORS}}

  def load_state_dict(self, d: dict) -> None:
    assert (d['num_envs'], d['capacity'], d['update_horizon']) == (self.num_envs, self.capacity, self.update_horizon)
    for k in self._TENSORS:
      getattr(self, k).copy_(d[k])
    self.cursor = int(d['cursor'])
    self.count.fill_(self.cursor)


class VecPrioritizedReplayBuffer(VecReplayBuffer):
  """VecReplayBuffer with Dopamine's prioritized replay (configs/quantile.gin's OutOfGraphPrioritizedReplayBuffer), DESIGN §3g.

  An fp64 sum tree over capacity_steps x num_envs leaves (one per n-step window).  add() also enters the windows that have just become
  complete at the max recorded priority (ble_replay_tree_add_f64); sample() draws stratified by priority and the batch carries each
  row's priority (batch.priority); set_priority(batch, loss) sets leaf = sqrt(loss + 1e-10) and returns the importance-weighted
  per-row losses Dopamine reports (the gradient itself is not weighted)."""

  prioritized = True
  _TENSORS = VecReplayBuffer._TENSORS + ('tree', 'max_priority')

  def __init__(self, num_envs: int, capacity_steps: int, update_horizon: int = 5, gamma: float = 0.993, device='cuda:0'):
    super().__init__(num_envs, capacity_steps, update_horizon, gamma, device)
    leaves = self.capacity * self.num_envs
    if leaves > 2 ** 31:
      raise ValueError('capacity_steps x num_envs must be at most 2^31')
    self.padded = 1 << (leaves - 1).bit_length()
    with torch.cuda.device(self.device):
      self.tree = torch.zeros(2 * self.padded, dtype=torch.float64, device=self.device)
      self.max_priority = torch.ones(1, dtype=torch.float64, device=self.device)
    self._tree = _abi.BleSumTreeF64(leaves, self.padded, self.tree.data_ptr(), self.max_priority.data_ptr())

  def leaf_priorities(self) -> torch.Tensor:
    """The leaves as [capacity_steps, num_envs] (a view)."""
    return self.tree[self.padded:self.padded + self.capacity * self.num_envs].view(self.capacity, self.num_envs)

  @dev.on_own_device
  def add(self, obs, action, reward, terminal, episode_end=None) -> None:
    super().add(obs, action, reward, terminal, episode_end)
    _lib.call('ble_replay_tree_add_f64', ctypes.byref(self.struct(self.counter)), ctypes.byref(self._tree), dev.stream_ptr(self.device))

  def _draw(self, rp: _abi.BleReplayF32, bt: TrainBatch, seed: int) -> None:
    """sample()'s draw: B stratified prioritized draws (ble_replay_sample_prioritized_f32); batch.priority [B] holds each row's leaf
    (fp32)."""
    _lib.call('ble_replay_sample_prioritized_f32', ctypes.byref(rp), ctypes.byref(self._tree), ctypes.byref(bt.struct),
              bt.priority.data_ptr(), seed, self.err_flags.data_ptr(), dev.stream_ptr(self.device))

  @dev.on_own_device
  def set_priority(self, batch: TrainBatch, loss: torch.Tensor) -> torch.Tensor:
    """Leaves of the batch's rows = sqrt(loss + 1e-10) (ble_replay_set_priority_f32); returns the weighted per-row losses [B] (a
    buffer the next call at this size overwrites)."""
    _lib.call('ble_replay_set_priority_f32', ctypes.byref(self.struct(self.counter)), ctypes.byref(self._tree), ctypes.byref(batch.struct),
              batch.priority.data_ptr(), loss.data_ptr(), batch.weighted_loss.data_ptr(), self.err_flags.data_ptr(),
              dev.stream_ptr(self.device))
    return batch.weighted_loss


class QNetworkLearner:
  """What the device learners share: a network's online image with its gradient and transposed image on the network's device, the
  descriptors of one update (ble_qnet_train_step_f32, or ble_qnet_td_step_f32 when _td() gives a BleTdF32), acting, export and the
  tensors of a checkpoint (_TENSORS).  A subclass sets the optimiser state it has; what it lacks stays None / 0."""

  _TENSORS = ('weights',)      # the checkpoint's tensors
  target = adam_m = adam_v = adam_step = None
  lr = eps = b1 = b2 = kappa = 0.0

  def __init__(self, network: qnet.QNetwork):
    self.device = d = dev.require_gpu(network.device)
    self.num_layers, self.hidden_units, self.num_atoms = network.num_layers, network.hidden_units, network.num_atoms
    self._net = _abi.BleQnetF32(self.num_layers, _lib.OBS_DIM, self.hidden_units, qnet.NUM_ACTIONS, self.num_atoms, 0, None)
    with torch.cuda.device(d):
      self.weights = torch.from_numpy(network.packed_host.copy()).to(d)
      self.grad = torch.zeros_like(self.weights)
      self.err_flags = torch.zeros(1, dtype=torch.int32, device=d)
      self.weights_t = torch.zeros(max(self._layout(0).transposed_floats, 4), dtype=torch.float32, device=d)
    self._net.weights = self.weights.data_ptr()
    self._retranspose()
    self._forward = qnet.Forward(self._net, d, type(self).__name__)
    self._graphs: dict = {}

  # ---- plumbing
  def _td(self) -> Optional[_abi.BleTdF32]:
    """The TD descriptor of this learner's update; None: the QR-DQN update, which has none."""
    return None

  def _struct(self, workspace: Optional[torch.Tensor], apply_update: bool = True) -> _abi.BleQnetTrainF32:
    return _abi.BleQnetTrainF32(self._net, dev.ptr(self.target), self.weights_t.data_ptr(), self.grad.data_ptr(), dev.ptr(self.adam_m),
                                dev.ptr(self.adam_v), dev.ptr(self.adam_step), dev.ptr(workspace), self.b1, self.b2, self.lr,
                                self.eps, self.kappa, 1 if apply_update else 0)

  def _layout(self, batch_size: int) -> _abi.BleQnetTrainLayout:
    bt = _abi.BleTrainBatchF32(int(batch_size), ROW_FLOATS)
    out = _abi.BleQnetTrainLayout()
    tr, td = _abi.BleQnetTrainF32(self._net), self._td()
    if td is None:
      _lib.call('ble_qnet_train_workspace_f32', ctypes.byref(tr), ctypes.byref(bt), ctypes.byref(out))
    else:
      _lib.call('ble_qnet_td_workspace_f32', ctypes.byref(tr), ctypes.byref(td), ctypes.byref(bt), ctypes.byref(out))
    return out

  def _launch_update(self, workspace: torch.Tensor, batch: _abi.BleTrainBatchF32, loss: torch.Tensor, apply_update: bool = True) -> None:
    """One update on a batch descriptor, the per-row losses into `loss`."""
    tr, td = self._struct(workspace, apply_update), self._td()
    head = ('ble_qnet_train_step_f32', ctypes.byref(tr)) if td is None else ('ble_qnet_td_step_f32', ctypes.byref(tr), ctypes.byref(td))
    _lib.call(*head, ctypes.byref(batch), loss.data_ptr(), self.err_flags.data_ptr(), dev.stream_ptr(self.device))

  def _retranspose(self) -> None:
    """weights_t from the online image (host transpose; at construction and after a load)."""
    host_t = np.zeros(self.weights_t.numel(), np.float32)
    w = self.weights.cpu().numpy()
    _lib.call('ble_qnet_transpose_f32', ctypes.byref(self._net), w.ctypes.data, host_t.ctypes.data)
    self.weights_t.copy_(torch.from_numpy(host_t))

  def check_errors(self) -> None:
    _check_flags(self.err_flags)

  # ---- acting
  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """The online network's greedy actions (ble_qnet_forward_f32 on the live image) into out (uint8 [N])."""
    return self._forward(obs, out)

  # ---- export and checkpoints
  def params(self) -> dict:
    """The flax-shaped tree of the online parameters (ble_qnet_unpack_f32)."""
    return unpack(self._net, self.weights.cpu().numpy())

  def network(self, device=None) -> qnet.QNetwork:
    return qnet.QNetwork.from_params(self.params(), num_atoms=self.num_atoms, device=self.device if device is None else device)

  def state_dict(self) -> dict:
    return {'shape': (self.num_layers, self.hidden_units, self.num_atoms), 'seed': self.seed,
            **{k: getattr(self, k).clone() for k in self._TENSORS}}

  def load_state_dict(self, d: dict) -> None:
    """Restores in place (every tensor keeps its address: captured graphs stay valid)."""
    assert tuple(d['shape']) == (self.num_layers, self.hidden_units, self.num_atoms), 'checkpoint of another network shape'
    self.seed = int(d['seed'])
    for k in self._TENSORS:
      getattr(self, k).copy_(d[k])
    self._retranspose()


class QNetworkTrainer(QNetworkLearner):
  """QR-DQN training of a QNetwork's parameters on its device (defaults: configs/quantile.gin -- Adam lr 2e-6, eps 2e-5, gamma 0.993,
  update horizon 5, kappa 1).

    trainer = QNetworkTrainer(QNetwork.from_params(init_params('quantile')))
    loss = trainer.train_step(replay, 32)          # per-row losses [32], on the device
    trainer.sync_target()
    policy = trainer.network()                     # a QNetwork: VecQNetworkAgent, QuantileAgent, eval_agent_vec, save_npz
  """

  _TENSORS = ('weights', 'target', 'adam_m', 'adam_v', 'adam_step', 'counter')

  def __init__(self, network: qnet.QNetwork, *, lr: float = 2e-6, eps: float = 2e-5, gamma: float = 0.993, update_horizon: int = 5,
               kappa: float = 1.0, seed: int = 0, b1: float = 0.9, b2: float = 0.999):
    super().__init__(network)
    self.lr, self.eps, self.b1, self.b2, self.kappa = float(lr), float(eps), float(b1), float(b2), float(kappa)
    self.gamma, self.update_horizon, self.seed = float(gamma), int(update_horizon), int(seed)
    d = self.device
    with torch.cuda.device(d):
      self.target = self.weights.clone()
      self.adam_m = torch.zeros_like(self.weights)
      self.adam_v = torch.zeros_like(self.weights)
      self.adam_step = torch.zeros(1, dtype=torch.int64, device=d)
      self.counter = torch.zeros(1, dtype=torch.int64, device=d)      # the update counter the replay draw is keyed by
    self._ws: Dict[int, tuple] = {}

  def workspace(self, batch_size: int):
    """(workspace tensor, layout) of a batch size (allocated on first use, which must not be inside a graph capture)."""
    def make():
      lay = self._layout(batch_size)
      with torch.cuda.device(self.device):
        return (torch.zeros(max(lay.total, 64), dtype=torch.float32, device=self.device), lay,
                torch.zeros(max(batch_size, 1), dtype=torch.float32, device=self.device))
    return dev.first_use(self._ws, batch_size, make, f'QNetworkTrainer: run one update at batch size {batch_size} before capturing it')

  def views(self, batch_size: int) -> dict:
    """The workspace's tensors of the last update at this batch size: 'acts' (every online layer's output, [B, ld] each), 'logits'
    [B, 3 * atoms] (online), 'target_logits',
    'targets' [B, atoms], 'dlogits' [B, 3 * atoms], 'loss' [B]."""
    ws, lay, loss = self.workspace(batch_size)
    b, ld, out = batch_size, lay.ld, qnet.NUM_ACTIONS * self.num_atoms

    def mat(off, cols, width):
      return ws[off:off + b * cols].view(b, cols)[:, :width]
    return {'acts': [mat(lay.acts + l * b * ld, ld, ld) for l in range(self.num_layers)],
            'logits': mat(lay.acts + (self.num_layers - 1) * b * ld, ld, out), 'target_logits': mat(lay.target_logits, ld, out),
            'targets': mat(lay.targets, self.num_atoms, self.num_atoms), 'dlogits': mat(lay.dlogits, ld, ld), 'loss': loss[:b]}

  # ---- the update
  @dev.on_own_device
  def train_on_batch(self, batch: TrainBatch, apply_update: bool = True) -> torch.Tensor:
    """One update on a given batch: the per-row losses [B] (a view of a buffer the next update at this size overwrites)."""
    ws, _, loss = self.workspace(batch.batch_size)
    self._launch_update(ws, batch.struct, loss, apply_update)
    return loss[:batch.batch_size]

  @dev.on_own_device
  def train_step(self, replay: VecReplayBuffer, batch_size: int = 32) -> torch.Tensor:
    """Sample a batch (keyed by (seed, update counter)) and update: per-row losses [B] on the device, no host synchronisation.  A
    captured graph of this batch size (capture()) replays it.  With a VecPrioritizedReplayBuffer the update is followed by
    set_priority and the losses returned are the importance-weighted ones (Dopamine's reported QuantileLoss)."""
    g = self._graphs.get(batch_size)
    if g is not None and g[1] is replay:
      g[0].replay()
      return g[2]
    return self._update(replay, batch_size)

  def _update(self, replay: VecReplayBuffer, batch_size: int) -> torch.Tensor:
    batch = replay.sample(batch_size, self.seed, self.counter)
    loss = self.train_on_batch(batch)
    if replay.prioritized:                          # sample -> update -> set_priority; the reported loss is the weighted one
      return replay.set_priority(batch, loss)
    return loss

  def capture(self, replay: VecReplayBuffer, batch_size: int = 32) -> torch.Tensor:
    """Records one update (sample + train step, + set_priority with a VecPrioritizedReplayBuffer) into a HIP graph that
    train_step(replay, batch_size) replays from then on: the counters are device memory, so each replay draws a new batch and takes a
    new Adam step.  Runs one eager update first (the lazy allocations) -- that is a real update; returns its per-row losses."""
    first = self.train_step(replay, batch_size)
    graph, loss = dev.capture(self.device, lambda: self._update(replay, batch_size))
    self._graphs[batch_size] = (graph, replay, loss)
    return first

  def sync_target(self) -> None:
    self.target.copy_(self.weights)

  def state_dict(self) -> dict:
    return {**super().state_dict(), 'hyper': (self.lr, self.eps, self.b1, self.b2, self.kappa, self.gamma, self.update_horizon)}

  def load_state_dict(self, d: dict) -> None:
    hyper = tuple(d['hyper'])
    if int(d['seed']) != self.seed or hyper != (self.lr, self.eps, self.b1, self.b2, self.kappa, self.gamma, self.update_horizon):
      self._graphs.clear()                     # (the seed and hyperparameters are arguments of the captured launches)
    self.lr, self.eps, self.b1, self.b2, self.kappa, self.gamma, self.update_horizon = hyper
    super().load_state_dict(d)


def unpack(net: _abi.BleQnetF32, packed: np.ndarray) -> dict:
  """The flax-shaped tree {'params': {'Dense_i': {'kernel', 'bias'}}} of a host packed image (ble_qnet_unpack_f32)."""
  packed = np.ascontiguousarray(packed, np.float32)
  dims = [net.input_dim] + [net.hidden_units] * (net.num_layers - 1) + [net.num_actions * net.num_atoms]
  kernels = [np.zeros((dims[i], dims[i + 1]), np.float32) for i in range(net.num_layers)]
  biases = [np.zeros(dims[i + 1], np.float32) for i in range(net.num_layers)]
  kp = (ctypes.c_void_p * net.num_layers)(*[k.ctypes.data for k in kernels])
  bp = (ctypes.c_void_p * net.num_layers)(*[b.ctypes.data for b in biases])
  _lib.call('ble_qnet_unpack_f32', ctypes.byref(net), packed.ctypes.data, kp, bp)
  return {'params': {f'Dense_{i}': {'kernel': k, 'bias': b} for i, (k, b) in enumerate(zip(kernels, biases))}}


def explore(actions: torch.Tensor, epsilon: float, seed: int, step: int) -> torch.Tensor:
  """epsilon-greedy in place on uint8 device actions (ble_qnet_explore_u8): keyed by (seed, environment, step)."""
  if actions.dtype != torch.uint8 or not actions.is_contiguous():
    raise ValueError('explore: actions must be a contiguous uint8 tensor (the kernel writes numel() bytes from data_ptr())')
  ex = _abi.BleExploreF32(actions.numel(), float(epsilon), 0, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1))
  _lib.call('ble_qnet_explore_u8', ctypes.byref(ex), actions.data_ptr(), dev.stream_ptr(actions.device))
  return actions


def member_seeds(seed, members: int, device) -> torch.Tensor:
  """The per-member seeds of a population as a device int64 [P] tensor (the kernels read the bits as uint64): a scalar s gives member p
  s + p, a length-P sequence is taken as given; both modulo 2^64."""
  a = np.asarray(seed, dtype=object)
  vals = [int(a) + p for p in range(members)] if a.ndim == 0 else [int(v) for v in a.reshape(-1)]
  if len(vals) != members:
    raise ValueError(f'seed: a scalar or {members} values, not {len(vals)}')
  return torch.from_numpy(np.array([v & (2 ** 64 - 1) for v in vals], np.uint64).view(np.int64)).to(device)


class VecPopulationReplayBuffer(VecReplayBuffer):
  """The replay memory of a population of P learners of R environments each: ONE VecReplayBuffer ring of P * R columns,
  columns [p R, (p + 1) R) member p's, filled by add() with the P * R rows of a VecBalloonEnv step.  sample(B, seeds, counter) draws B
  rows PER MEMBER into a TrainBatch of P * B rows (ble_replay_sample_grouped_f32): rows [p B, (p + 1) B) are what member p's own
  VecReplayBuffer of its R columns (member_buffer(p)) gives sample(B, seeds[p], counter), with the index's column + p R.  Prioritized
  replay per member is VecPopulationPrioritizedReplayBuffer's."""

  def __init__(self, members: int, rows_per_member: int, capacity_steps: int, update_horizon: int = 5, gamma: float = 0.993,
               device='cuda:0'):
    self.members, self.rows_per_member = int(members), int(rows_per_member)
    if self.members < 1 or self.rows_per_member < 1:
      raise ValueError('a population replay has at least one member of at least one environment')
    super().__init__(self.members * self.rows_per_member, capacity_steps, update_horizon, gamma, device)

  def batch_buffers(self, batch_size: int) -> TrainBatch:
    """The TrainBatch of P * B rows of B rows per member."""
    rows = self.members * int(batch_size)
    return dev.first_use(self._batches, rows, lambda: TrainBatch(rows, self.device),
                         f'VecPopulationReplayBuffer: sample once at {batch_size} rows per member before capturing it in a graph')

  @dev.on_own_device
  def sample(self, batch_size: int, seeds: torch.Tensor, counter: Optional[torch.Tensor] = None) -> TrainBatch:
    """B transitions per member into this buffer's batch of P * B rows (overwritten by the next sample at that size).  seeds: device
    int64 [P] (member_seeds), read as uint64; counter: the int64 [1] device update counter every member's draw is keyed by, advanced
    once (default: the buffer's own).  No host synchronisation."""
    assert seeds.dtype == torch.int64 and seeds.is_contiguous() and seeds.numel() == self.members and seeds.device == self.device
    bt = self.batch_buffers(int(batch_size))
    rp = self.struct(self.counter if counter is None else counter)
    _lib.call('ble_replay_sample_grouped_f32', ctypes.byref(rp), self.members, seeds.data_ptr(), ctypes.byref(bt.struct),
              self.err_flags.data_ptr(), dev.stream_ptr(self.device))
    return bt

  def member_buffer(self, p: int) -> VecReplayBuffer:
    """A copy of member p's R columns as a VecReplayBuffer of its own (same steps written, its own update counter at 0)."""
    if not 0 <= int(p) < self.members:
      raise IndexError(f'member {p} of a population of {self.members}')
    r = self.rows_per_member
    cols = slice(int(p) * r, (int(p) + 1) * r)
    solo = VecReplayBuffer(r, self.capacity, self.update_horizon, self.gamma, self.device)
    for k in ('obs', 'action', 'reward', 'terminal', 'episode_end'):
      getattr(solo, k).copy_(getattr(self, k)[:, cols])
    solo.cursor = self.cursor
    solo.count.fill_(self.cursor)
    return solo

  def state_dict(self) -> dict:
    return {**super().state_dict(), 'members': self.members}

  def load_state_dict(self, d: dict) -> None:
    assert int(d['members']) == self.members, 'checkpoint of another population'
    super().load_state_dict(d)


class VecPopulationPrioritizedReplayBuffer(VecPopulationReplayBuffer):
  """VecPopulationReplayBuffer with prioritized replay per member: P fp64 sum trees, `tree` [P, 2 * padded], each a solo
  VecPrioritizedReplayBuffer's tree image over capacity_steps x R leaves -- leaf (t % T) R + r the window of column p R + r -- with its
  own max recorded priority, `max_priority` [P].  add() also enters every member's newly complete windows at that member's max priority
  (ble_replay_tree_add_grouped_f64); sample(B, seeds, counter) draws B rows per member stratified by its own priorities, the batch
  carrying each row's priority; set_priority(batch, loss) sets the leaves per member and returns the importance-weighted losses
  [P * B], each member's normalised by its own largest weight.  Rows [p B, (p + 1) B), tree p and max_priority[p] hold the bytes
  member_buffer(p) -- a VecPrioritizedReplayBuffer of member p's columns -- holds after the same calls with seeds[p]."""

  prioritized = True
  _TENSORS = VecPopulationReplayBuffer._TENSORS + ('tree', 'max_priority')

  def __init__(self, members: int, rows_per_member: int, capacity_steps: int, update_horizon: int = 5, gamma: float = 0.993,
               device='cuda:0'):
    super().__init__(members, rows_per_member, capacity_steps, update_horizon, gamma, device)
    leaves = self.capacity * self.rows_per_member
    if leaves > 2 ** 31:
      raise ValueError('capacity_steps x rows_per_member must be at most 2^31')
    self.padded = 1 << (leaves - 1).bit_length()
    with torch.cuda.device(self.device):
      self.tree = torch.zeros(self.members, 2 * self.padded, dtype=torch.float64, device=self.device)
      self.max_priority = torch.ones(self.members, dtype=torch.float64, device=self.device)
    self._tree = _abi.BleSumTreeGroupedF64(self.members, leaves, self.padded, 2 * self.padded, self.tree.data_ptr(),
                                           self.max_priority.data_ptr())

  def batch_buffers(self, batch_size: int) -> TrainBatch:
    """The prioritized TrainBatch of P * B rows of B rows per member."""
    rows = self.members * int(batch_size)
    return dev.first_use(self._batches, rows, lambda: TrainBatch(rows, self.device, True),
                         f'VecPopulationPrioritizedReplayBuffer: sample once at {batch_size} rows per member before capturing it in a graph')

  def leaf_priorities(self) -> torch.Tensor:
    """The leaves as [members, capacity_steps, rows_per_member] (a view)."""
    t, r = self.capacity, self.rows_per_member
    return self.tree[:, self.padded:self.padded + t * r].view(self.members, t, r)

  @dev.on_own_device
  def add(self, obs, action, reward, terminal, episode_end=None) -> None:
    super().add(obs, action, reward, terminal, episode_end)
    _lib.call('ble_replay_tree_add_grouped_f64', ctypes.byref(self.struct(self.counter)), ctypes.byref(self._tree),
              dev.stream_ptr(self.device))

  @dev.on_own_device
  def sample(self, batch_size: int, seeds: torch.Tensor, counter: Optional[torch.Tensor] = None) -> TrainBatch:
    """B stratified prioritized draws per member (ble_replay_sample_prioritized_grouped_f32) into this buffer's batch of P * B rows;
    batch.priority [P * B] holds each row's leaf (fp32).  seeds and counter as VecPopulationReplayBuffer.sample."""
    assert seeds.dtype == torch.int64 and seeds.is_contiguous() and seeds.numel() == self.members and seeds.device == self.device
    bt = self.batch_buffers(int(batch_size))
    rp = self.struct(self.counter if counter is None else counter)
    _lib.call('ble_replay_sample_prioritized_grouped_f32', ctypes.byref(rp), ctypes.byref(self._tree), seeds.data_ptr(),
              ctypes.byref(bt.struct), bt.priority.data_ptr(), self.err_flags.data_ptr(), dev.stream_ptr(self.device))
    return bt

  @dev.on_own_device
  def set_priority(self, batch: TrainBatch, loss: torch.Tensor) -> torch.Tensor:
    """Member p's leaves of its rows = sqrt(loss + 1e-10) (ble_replay_set_priority_grouped_f32); returns the weighted per-row losses
    [P * B] (a buffer the next call at this size overwrites)."""
    _lib.call('ble_replay_set_priority_grouped_f32', ctypes.byref(self.struct(self.counter)), ctypes.byref(self._tree),
              ctypes.byref(batch.struct), batch.priority.data_ptr(), loss.data_ptr(), batch.weighted_loss.data_ptr(),
              self.err_flags.data_ptr(), dev.stream_ptr(self.device))
    return batch.weighted_loss

  def member_buffer(self, p: int) -> VecPrioritizedReplayBuffer:
    """A copy of member p's R columns as a VecPrioritizedReplayBuffer of its own, with tree p and max_priority[p] copied in."""
    if not 0 <= int(p) < self.members:
      raise IndexError(f'member {p} of a population of {self.members}')
    r = self.rows_per_member
    cols = slice(int(p) * r, (int(p) + 1) * r)
    solo = VecPrioritizedReplayBuffer(r, self.capacity, self.update_horizon, self.gamma, self.device)
    for k in ('obs', 'action', 'reward', 'terminal', 'episode_end'):
      getattr(solo, k).copy_(getattr(self, k)[:, cols])
    solo.tree.copy_(self.tree[int(p)])
    solo.max_priority.copy_(self.max_priority[int(p):int(p) + 1])
    solo.cursor = self.cursor
    solo.count.fill_(self.cursor)
    return solo


def _epsilons(epsilon, members: int) -> np.ndarray:
  """A scalar or a length-P sequence as float32 [P], each in [0, 1] (the entry point cannot see device values)."""
  a = np.asarray(epsilon, np.float64)
  a = np.full(members, float(a)) if a.ndim == 0 else a.reshape(-1)
  if a.shape != (members,):
    raise ValueError(f'epsilon: a scalar or {members} values, not {a.shape[0]}')
  if not ((a >= 0.0) & (a <= 1.0)).all():
    raise ValueError(f'epsilon must lie in [0, 1], not {a.tolist()}')
  return a.astype(np.float32)


def explore_grouped(actions: torch.Tensor, epsilon, seeds: torch.Tensor, step: int) -> torch.Tensor:
  """epsilon-greedy in place on the uint8 device actions of a population, P = len(seeds) members of actions.numel() / P rows each
  (ble_qnet_explore_grouped_u8): row p R + r is keyed by (seeds[p], r, step) and explores at epsilon[p] -- member p's own explore() on
  its rows.  epsilon: a scalar or a length-P sequence (validated, then uploaded), or a float32 device tensor [P] the caller keeps in
  [0, 1] (no upload, no host synchronisation); seeds: device int64 [P] (member_seeds)."""
  if actions.dtype != torch.uint8 or not actions.is_contiguous():
    raise ValueError('explore_grouped: actions must be a contiguous uint8 tensor (the kernel writes numel() bytes from data_ptr())')
  members = int(seeds.numel())
  if seeds.dtype != torch.int64 or not seeds.is_contiguous() or seeds.device != actions.device or members < 1 or actions.numel() % members:
    raise ValueError('explore_grouped: seeds is a contiguous int64 [P] tensor on the actions\' device, P dividing the number of actions')
  if not isinstance(epsilon, torch.Tensor):
    epsilon = torch.from_numpy(_epsilons(epsilon, members)).to(actions.device)
  if epsilon.dtype != torch.float32 or not epsilon.is_contiguous() or epsilon.numel() != members or epsilon.device != actions.device:
    raise ValueError('explore_grouped: epsilon is a scalar, P values, or a contiguous float32 [P] tensor on the actions\' device')
  ex = _abi.BleExploreGroupedF32(actions.numel(), members, 0, epsilon.data_ptr(), seeds.data_ptr(), int(step) & (2 ** 64 - 1))
  _lib.call('ble_qnet_explore_grouped_u8', ctypes.byref(ex), actions.data_ptr(), dev.stream_ptr(actions.device))
  return actions
