"""On-policy training on the device: an actor-critic with PPO and generalised advantage estimation (csrc/ble_actor.h).

An actor-critic is a `QNetwork` with num_atoms == 2 read differently: of its six outputs z[a * 2 + j], z[0], z[2], z[4] are the
policy logits of the three actions and z[1] is the state value; z[3] and z[5] are not read and receive a zero gradient.  Packing,
the Dense stack, the backward pass, Adam, save_npz and state_dict are therefore the replay learners' own.

`VecActorCriticAgent` acts (greedy, or sampled from the Philox stream of (seed, environment, step)); `VecRolloutBuffer` holds T steps
of N environments, computes advantages over the block and hands out shuffled minibatches; `PPOTrainer` takes one clipped-PPO update
per minibatch (`ble_qnet_ppo_step_f32`), capturable as one graph.  train_lib.run_ppo_loop_vec is the loop.  No floating-point atomics
and every reduction in an order fixed by the shapes: a run is a pure function of (initial parameters, environment seeds, seeds).
"""
import ctypes
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import qnet_train

ROW_FLOATS = qnet_train.ROW_FLOATS
NUM_ATOMS = 2
POLICY_COLUMNS = (0, 2, 4)
VALUE_COLUMN = 1


def init_params(kind: str = 'actor_critic', seed: int = 0, num_layers: int = 3, hidden_units: int = 256) -> dict:
  """Parameters of an actor-critic: qnet.init_params('mlp')'s Glorot-uniform on every layer (six outputs) with zero biases, then the
  last layer's three policy columns scaled by 0.01, so that the initial policy is near uniform."""
  if kind != 'actor_critic':
    raise ValueError(f"kind is 'actor_critic', not {kind!r}")
  if num_layers < 1:
    raise ValueError('num_layers >= 1')
  rng = np.random.default_rng(seed)
  dims = [_lib.OBS_DIM] + [hidden_units] * (num_layers - 1) + [qnet.NUM_ACTIONS * NUM_ATOMS]
  tree = {}
  for i in range(num_layers):
    fan_in, fan_out = dims[i], dims[i + 1]
    limit = np.sqrt(6.0 / (fan_in + fan_out))
    tree[f'Dense_{i}'] = {'kernel': rng.uniform(-limit, limit, (fan_in, fan_out)).astype(np.float32), 'bias': np.zeros(fan_out, np.float32)}
  tree[f'Dense_{num_layers - 1}']['kernel'][:, list(POLICY_COLUMNS)] *= np.float32(0.01)
  return {'params': tree}


def _require_actor_critic(network: qnet.QNetwork, who: str) -> None:
  if network.num_atoms != NUM_ATOMS:
    raise ValueError(f'{who} needs a two-atom network (policy logits and a value), not {network.num_atoms} atoms')


class ActorForward:
  """ble_ac_act_f32 on a network descriptor whose image is on the device, with the buffers it needs: scratch, logp and value of a
  batch size are allocated on the first call at that size, which must not be inside a graph capture (qnet.Forward's contract)."""

  def __init__(self, struct: _abi.BleQnetF32, device: torch.device, owner: str):
    self.struct, self.device, self.owner = struct, device, owner
    self._buffers: Dict[int, tuple] = {}

  def _allocate(self, n: int) -> tuple:
    floats = ctypes.c_int64()
    _lib.call('ble_qnet_workspace_f32', ctypes.byref(self.struct), n, None, ctypes.byref(floats))
    return (torch.empty(max(floats.value, 1), dtype=torch.float32, device=self.device),
            torch.empty(n, dtype=torch.float32, device=self.device), torch.empty(n, dtype=torch.float32, device=self.device))

  def __call__(self, obs: torch.Tensor, out: Optional[torch.Tensor], logp: Optional[torch.Tensor], value: Optional[torch.Tensor],
               probs: Optional[torch.Tensor], sample: Optional[_abi.BleAcSample]) -> torch.Tensor:
    assert obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] >= _lib.OBS_DIM and obs.stride(1) == 1, (obs.dtype, obs.shape)
    assert obs.device == self.device
    n = obs.shape[0]
    if out is None:
      out = torch.empty(n, dtype=torch.uint8, device=self.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n
    for t, numel in ((logp, n), (value, n), (probs, n * qnet.NUM_ACTIONS)):
      assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel)
    if n == 0:
      return out
    scratch, own_logp, own_value = dev.first_use(self._buffers, n, lambda: self._allocate(n),
                                                 f'{self.owner}: call act once at batch size {n} before capturing it in a graph')
    stride = obs.stride(0) if n > 1 else max(obs.stride(0), _lib.OBS_DIM)      # (torch gives a one-row tensor any stride)
    rows = _abi.BleAcRowsF32(n, stride, obs.data_ptr(), out.data_ptr(), (own_logp if logp is None else logp).data_ptr(),
                             (own_value if value is None else value).data_ptr(), dev.ptr(probs))
    _lib.call('ble_ac_act_f32', ctypes.byref(self.struct), ctypes.byref(rows), scratch.data_ptr(),
              ctypes.byref(sample) if sample is not None else None, dev.stream_ptr(self.device))
    return out


class _Sampler:
  """The sampled head's stream: a seed, the first environment's index and the device step counter, which advances after each act
  (a device add: part of the captured work)."""

  def __init__(self, seed: int, device: torch.device, env_offset: int = 0):
    self.seed, self.env_offset = int(seed), int(env_offset)
    self.step = torch.zeros(1, dtype=torch.int64, device=device)      # (read as uint64 by the kernel)

  def struct(self) -> _abi.BleAcSample:
    return _abi.BleAcSample(self.seed & (2 ** 64 - 1), self.env_offset, self.step.data_ptr(), 0)


class VecActorCriticAgent:
  """An actor-critic policy for N environments at once: act(obs [N, >= 1099] float32 device) -> uint8 [N] device.  deterministic:
  the greedy action (the first largest policy logit); otherwise a draw from the policy, keyed by (seed, environment, step), the device
  step counter advancing after each act."""

  def __init__(self, network: qnet.QNetwork, deterministic: bool = True, seed: int = 0, env_offset: int = 0):
    """env_offset: the index of row 0's environment in the stream's keying (a shard of a larger batch draws what the whole draws)."""
    _require_actor_critic(network, 'VecActorCriticAgent')
    self.network = network.to_device()
    self.device = network.device
    self.deterministic = bool(deterministic)
    self._forward = ActorForward(network._struct, self.device, 'VecActorCriticAgent')
    self._sampler = None if self.deterministic else _Sampler(seed, self.device, env_offset)
    self.step = None if self.deterministic else self._sampler.step      # int64 [1] on the device: the draws' step counter

  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None,
          value: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """obs rows may be padded (stride(0) >= 1099, stride(1) == 1); only the first 1099 columns are read.  out: optional uint8 [N];
    logp, value: optional float32 [N]; probs: optional float32 [N, 3]."""
    if self._sampler is None:
      return self._forward(obs, out, logp, value, probs, None)
    out = self._forward(obs, out, logp, value, probs, self._sampler.struct())
    if obs.shape[0]:
      self._sampler.step.add_(1)
    return out

  __call__ = act

  def get_name(self) -> str:
    return 'ActorCriticAgent'


class PPOBatch(qnet_train.TrainBatch):
  """One minibatch of B on-policy rows (static device buffers): TrainBatch's state, ret (the return R) and action; old_logp and
  advantage; no next_state, discount or index."""

  def __init__(self, batch_size: int, device):      # pylint: disable=super-init-not-called
    b = int(batch_size)
    self.batch_size = b
    self.state = torch.zeros(b, ROW_FLOATS, dtype=torch.float32, device=device)
    self.ret = torch.zeros(b, dtype=torch.float32, device=device)
    self.action = torch.zeros(b, dtype=torch.uint8, device=device)
    self.old_logp = torch.zeros(b, dtype=torch.float32, device=device)
    self.advantage = torch.zeros(b, dtype=torch.float32, device=device)
    self.next_state = self.discount = self.index = self.priority = self.weighted_loss = None
    self.struct = _abi.BleTrainBatchF32(b, ROW_FLOATS, self.state.data_ptr(), None, self.ret.data_ptr(), None, self.action.data_ptr(), None)

  @classmethod
  def from_tensors(cls, state, ret, action, old_logp, advantage, device) -> 'PPOBatch':      # pylint: disable=arguments-differ
    """A batch given on the host or device (state rows of 1099 features); for tests and offline data."""
    bt = cls(len(action), device)
    bt.state[:, :_lib.OBS_DIM].copy_(torch.as_tensor(np.asarray(state, np.float32)))
    bt.ret.copy_(torch.as_tensor(np.asarray(ret, np.float32)))
    bt.action.copy_(torch.as_tensor(np.asarray(action, np.uint8)))
    bt.old_logp.copy_(torch.as_tensor(np.asarray(old_logp, np.float32)))
    bt.advantage.copy_(torch.as_tensor(np.asarray(advantage, np.float32)))
    return bt


class VecRolloutBuffer:
  """T steps of N environments stepped in lockstep, on the device: obs [T, N, ROW_FLOATS], action, logp, value, reward, terminal,
  episode_end (each [T, N]), boot_value [N], advantage and ret [T, N].

  add(t, ...) copies one vector step; finish(boot_value, gamma, lam, normalize) runs generalised advantage estimation over the block
  (ble_gae_f32) and, if asked, the advantage normalisation (ble_adv_normalize_f32); minibatches(B, generator) yields PPOBatch buffers
  filled by index_select over a torch.randperm of the T N rows (a trailing partial minibatch is dropped).  No call synchronises with
  the host."""

  _TENSORS = ('obs', 'action', 'logp', 'value', 'reward', 'terminal', 'episode_end', 'boot_value', 'advantage', 'ret')

  def __init__(self, num_envs: int, horizon: int, device='cuda:0'):
    self.device = d = dev.require_gpu(device)
    self.num_envs, self.horizon = int(num_envs), int(horizon)
    if self.num_envs < 1 or self.horizon < 1:
      raise ValueError('num_envs and horizon must be at least 1')
    t, n = self.horizon, self.num_envs
    with torch.cuda.device(d):
      self.obs = torch.zeros(t, n, ROW_FLOATS, dtype=torch.float32, device=d)
      self.action = torch.zeros(t, n, dtype=torch.uint8, device=d)
      self.terminal = torch.zeros(t, n, dtype=torch.uint8, device=d)
      self.episode_end = torch.zeros(t, n, dtype=torch.uint8, device=d)
      self.logp, self.value, self.reward, self.advantage, self.ret = (torch.zeros(t, n, dtype=torch.float32, device=d) for _ in range(5))
      self.boot_value = torch.zeros(n, dtype=torch.float32, device=d)
      self.generator = torch.Generator(device=d)
    self.generator.manual_seed(0)
    self._batches: Dict[int, PPOBatch] = {}

  def _block(self, gamma: float = 0.0, lam: float = 0.0) -> _abi.BleGaeBlockF32:
    return _abi.BleGaeBlockF32(self.horizon, self.num_envs, gamma, lam, self.reward.data_ptr(), self.value.data_ptr(),
                               self.boot_value.data_ptr(), self.terminal.data_ptr(), self.episode_end.data_ptr(),
                               self.advantage.data_ptr(), self.ret.data_ptr())

  @dev.on_own_device
  def add(self, t: int, obs: torch.Tensor, action: torch.Tensor, logp: torch.Tensor, value: torch.Tensor, reward: torch.Tensor,
          terminal: torch.Tensor, episode_end: Optional[torch.Tensor] = None) -> None:
    """Step t of the block: obs is the observation the actions were taken on, logp and value what the policy said there."""
    self.obs[t, :, :_lib.OBS_DIM].copy_(obs[:, :_lib.OBS_DIM])
    self.action[t].copy_(action)
    self.logp[t].copy_(logp)
    self.value[t].copy_(value)
    self.reward[t].copy_(reward)
    self.terminal[t].copy_(terminal)
    self.episode_end[t].copy_(terminal if episode_end is None else episode_end)

  @dev.on_own_device
  def finish(self, boot_value: torch.Tensor, gamma: float, lam: float, normalize: bool = True) -> None:
    """boot_value [N]: the value of the observation after the last step.  Writes advantage and ret."""
    self.boot_value.copy_(boot_value)
    blk = self._block(float(gamma), float(lam))
    _lib.call('ble_gae_f32', ctypes.byref(blk), dev.stream_ptr(self.device))
    if normalize:
      _lib.call('ble_adv_normalize_f32', ctypes.byref(blk), dev.stream_ptr(self.device))

  def batch_buffers(self, batch_size: int) -> PPOBatch:
    return dev.first_use(self._batches, batch_size, lambda: PPOBatch(batch_size, self.device),
                         f'VecRolloutBuffer: draw minibatches once at batch size {batch_size} before capturing an update')

  @dev.on_own_device
  def minibatches(self, batch_size: int, generator: Optional[torch.Generator] = None) -> Iterator[PPOBatch]:
    """One pass over the block in a random order: the same PPOBatch buffers, refilled for every minibatch."""
    b, m = int(batch_size), self.horizon * self.num_envs
    bt = self.batch_buffers(b)
    perm = torch.randperm(m, device=self.device, generator=self.generator if generator is None else generator)
    flat = {'state': self.obs.view(m, ROW_FLOATS), 'ret': self.ret.view(m), 'action': self.action.view(m), 'old_logp': self.logp.view(m),
            'advantage': self.advantage.view(m)}
    for k in range(m // b):
      idx = perm[k * b:(k + 1) * b]
      for name, src in flat.items():
        torch.index_select(src, 0, idx, out=getattr(bt, name))
      yield bt

  def state_dict(self) -> dict:
    return {'num_envs': self.num_envs, 'horizon': self.horizon, 'generator': self.generator.get_state().clone(),
            **{k: getattr(self, k).clone() for k in self._TENSORS}}

  def load_state_dict(self, d: dict) -> None:
    assert (d['num_envs'], d['horizon']) == (self.num_envs, self.horizon)
    for k in self._TENSORS:
      getattr(self, k).copy_(d[k])
    self.generator.set_state(d['generator'])


class VecPopulationRolloutBuffer:
  """VecRolloutBuffer for a population (agents/population.py: PopulationPPOTrainer): T steps of P * R environments, environment rows
  [p R, (p + 1) R) member p's, held member-major -- obs [P, T, R, ROW_FLOATS], the others [P, T, R], boot_value [P, R] -- so each
  member's [T, R] block is contiguous and is what that member's own VecRolloutBuffer(R, T) holds.

  add(t, ...) takes one vector step of all P * R environments; finish runs ble_gae_f32 and (if asked) ble_adv_normalize_f32 once per
  member on its block: each member's advantages are normalised over its own T R rows.  minibatches(B) draws ONE torch.randperm(T R) per
  pass from a generator seeded 0 (VecRolloutBuffer's stream), shared by all members, and yields a PopulationPPOBatch of P * B rows
  whose member-p rows are that member's rows perm[k B:(k + 1) B].  No call synchronises with the host."""

  _TENSORS = VecRolloutBuffer._TENSORS

  def __init__(self, members: int, rows_per_member: int, horizon: int, device='cuda:0'):
    from balloon_learning_environment_amd.agents import population
    self._batch_type = population.PopulationPPOBatch
    self.device = d = dev.require_gpu(device)
    self.members, self.rows_per_member, self.horizon = int(members), int(rows_per_member), int(horizon)
    if self.members < 1 or self.rows_per_member < 1 or self.horizon < 1:
      raise ValueError('members, rows_per_member and horizon must be at least 1')
    self.num_envs = self.members * self.rows_per_member
    p, t, r = self.members, self.horizon, self.rows_per_member
    with torch.cuda.device(d):
      self.obs = torch.zeros(p, t, r, ROW_FLOATS, dtype=torch.float32, device=d)
      self.action = torch.zeros(p, t, r, dtype=torch.uint8, device=d)
      self.terminal = torch.zeros(p, t, r, dtype=torch.uint8, device=d)
      self.episode_end = torch.zeros(p, t, r, dtype=torch.uint8, device=d)
      self.logp, self.value, self.reward, self.advantage, self.ret = (torch.zeros(p, t, r, dtype=torch.float32, device=d) for _ in range(5))
      self.boot_value = torch.zeros(p, r, dtype=torch.float32, device=d)
      self.generator = torch.Generator(device=d)
    self.generator.manual_seed(0)
    self._batches: Dict[int, object] = {}

  @dev.on_own_device
  def add(self, t: int, obs: torch.Tensor, action: torch.Tensor, logp: torch.Tensor, value: torch.Tensor, reward: torch.Tensor,
          terminal: torch.Tensor, episode_end: Optional[torch.Tensor] = None) -> None:
    """Step t of the block, every argument over the P * R environments."""
    p, r = self.members, self.rows_per_member
    self.obs[:, t, :, :_lib.OBS_DIM].copy_(obs[:, :_lib.OBS_DIM].view(p, r, _lib.OBS_DIM))
    for name, src in (('action', action), ('logp', logp), ('value', value), ('reward', reward), ('terminal', terminal),
                      ('episode_end', terminal if episode_end is None else episode_end)):
      getattr(self, name)[:, t].copy_(src.view(p, r))

  @dev.on_own_device
  def finish(self, boot_value: torch.Tensor, gamma: float, lam: float, normalize: bool = True) -> None:
    """boot_value [P * R]: the value of the observation after the last step.  Writes advantage and ret, member by member."""
    self.boot_value.copy_(boot_value.view(self.members, self.rows_per_member))
    stream = dev.stream_ptr(self.device)
    for p in range(self.members):
      blk = _abi.BleGaeBlockF32(self.horizon, self.rows_per_member, float(gamma), float(lam), self.reward[p].data_ptr(),
                                self.value[p].data_ptr(), self.boot_value[p].data_ptr(), self.terminal[p].data_ptr(),
                                self.episode_end[p].data_ptr(), self.advantage[p].data_ptr(), self.ret[p].data_ptr())
      _lib.call('ble_gae_f32', ctypes.byref(blk), stream)
      if normalize:
        _lib.call('ble_adv_normalize_f32', ctypes.byref(blk), stream)

  def batch_buffers(self, batch_size: int):
    return dev.first_use(self._batches, batch_size, lambda: self._batch_type(self.members, batch_size, self.device),
                         f'VecPopulationRolloutBuffer: draw minibatches once at batch size {batch_size} before capturing an update')

  @dev.on_own_device
  def minibatches(self, batch_size: int, generator: Optional[torch.Generator] = None):
    """One pass over the block in a random order, batch_size rows PER MEMBER: the same buffers, refilled for every minibatch."""
    b, m, p = int(batch_size), self.horizon * self.rows_per_member, self.members
    bt = self.batch_buffers(b)
    perm = torch.randperm(m, device=self.device, generator=self.generator if generator is None else generator)
    flat = {'state': self.obs.view(p, m, ROW_FLOATS), 'ret': self.ret.view(p, m), 'action': self.action.view(p, m),
            'old_logp': self.logp.view(p, m), 'advantage': self.advantage.view(p, m)}
    outs = {name: getattr(bt, name).view(p, b, *src.shape[2:]) for name, src in flat.items()}
    for k in range(m // b):
      idx = perm[k * b:(k + 1) * b]
      for name, src in flat.items():
        torch.index_select(src, 1, idx, out=outs[name])
      yield bt

  def state_dict(self) -> dict:
    return {'members': self.members, 'rows_per_member': self.rows_per_member, 'horizon': self.horizon,
            'generator': self.generator.get_state().clone(), **{k: getattr(self, k).clone() for k in self._TENSORS}}

  def load_state_dict(self, d: dict) -> None:
    assert (d['members'], d['rows_per_member'], d['horizon']) == (self.members, self.rows_per_member, self.horizon)
    for k in self._TENSORS:
      getattr(self, k).copy_(d[k])
    self.generator.set_state(d['generator'])


class PPOTrainer(qnet_train.QNetworkLearner):
  """Clipped-PPO training of an actor-critic's parameters on its device.

    trainer = PPOTrainer(qnet.QNetwork.from_params(init_params('actor_critic'), num_atoms=2))
    train_lib.run_ppo_loop_vec(env, trainer, VecRolloutBuffer(env.num_envs, 32), num_iterations=..., batch_size=4096)
    policy = trainer.network()                     # a QNetwork: VecActorCriticAgent, eval_agent_vec, save_npz
  """

  _TENSORS = ('weights', 'adam_m', 'adam_v', 'adam_step', 'act_step')

  def __init__(self, network: qnet.QNetwork, *, lr: float = 3e-4, eps: float = 1e-5, gamma: float = 0.993, lam: float = 0.95,
               clip: float = 0.2, value_coef: float = 0.5, entropy_coef: float = 0.01, normalize_advantage: bool = True, seed: int = 0,
               b1: float = 0.9, b2: float = 0.999, env_offset: int = 0):
    """env_offset: the index of row 0's environment in the sampled head's keying (VecActorCriticAgent's)."""
    _require_actor_critic(network, 'PPOTrainer')
    super().__init__(network)
    self.lr, self.eps, self.b1, self.b2 = float(lr), float(eps), float(b1), float(b2)
    self.gamma, self.lam, self.clip = float(gamma), float(lam), float(clip)
    self.value_coef, self.entropy_coef = float(value_coef), float(entropy_coef)
    self.normalize_advantage, self.seed = bool(normalize_advantage), int(seed)
    d = self.device
    with torch.cuda.device(d):
      self.adam_m = torch.zeros_like(self.weights)
      self.adam_v = torch.zeros_like(self.weights)
      self.adam_step = torch.zeros(1, dtype=torch.int64, device=d)
    self._sampler = _Sampler(self.seed, d, env_offset)
    self.act_step = self._sampler.step
    self._actor = ActorForward(self._net, d, 'PPOTrainer')
    self._ws: Dict[int, tuple] = {}

  workspace = qnet_train.QNetworkTrainer.workspace

  # ---- acting
  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None,
          value: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sampled actions of the live image (VecActorCriticAgent.act's contract); the device step counter advances after each call."""
    self._sampler.seed = self.seed
    out = self._actor(obs, out, logp, value, probs, self._sampler.struct())
    if obs.shape[0]:
      self.act_step.add_(1)
    return out

  @dev.on_own_device
  def act_greedy(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None,
                 value: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Greedy actions of the live image; the step counter stays."""
    return self._actor(obs, out, logp, value, probs, None)

  # ---- the update
  def _ppo(self, batch: PPOBatch) -> _abi.BlePpoF32:
    return _abi.BlePpoF32(self.clip, self.value_coef, self.entropy_coef, 0, batch.old_logp.data_ptr(), batch.advantage.data_ptr())

  @dev.on_own_device
  def train_on_batch(self, batch: PPOBatch, apply_update: bool = True) -> torch.Tensor:
    """One update on a minibatch: the per-row losses [B] (a view of a buffer the next update at this size overwrites)."""
    ws, _, loss = self.workspace(batch.batch_size)
    tr, ppo = self._struct(ws, apply_update), self._ppo(batch)
    _lib.call('ble_qnet_ppo_step_f32', ctypes.byref(tr), ctypes.byref(ppo), ctypes.byref(batch.struct), loss.data_ptr(),
              self.err_flags.data_ptr(), dev.stream_ptr(self.device))
    return loss[:batch.batch_size]

  def train_step(self, batch: PPOBatch) -> torch.Tensor:
    """train_on_batch, by the captured graph of this batch's buffers when there is one (capture())."""
    g = self._graphs.get(batch.batch_size)
    if g is not None and g[1] is batch:
      g[0].replay()
      return g[2]
    return self.train_on_batch(batch)

  def capture(self, batch: PPOBatch) -> torch.Tensor:
    """Records one minibatch update on `batch`'s static buffers into a HIP graph that train_step(batch) replays from then on.  Runs
    one eager update first (the lazy allocations) -- that is a real update; returns its per-row losses."""
    first = self.train_on_batch(batch)
    graph, loss = dev.capture(self.device, lambda: self.train_on_batch(batch))
    self._graphs[batch.batch_size] = (graph, batch, loss)
    return first

  def views(self, batch_size: int) -> dict:
    """The workspace's tensors of the last update at this batch size: 'acts' (every layer's output, [B, ld] each), 'logits' [B, 6],
    'aux' [B, 2] (the batch action's log-probability, the entropy), 'dlogits' [B, ld], 'loss' [B]."""
    ws, lay, loss = self.workspace(batch_size)
    b, ld = batch_size, lay.ld

    def mat(off, cols, width):
      return ws[off:off + b * cols].view(b, cols)[:, :width]
    return {'acts': [mat(lay.acts + l * b * ld, ld, ld) for l in range(self.num_layers)],
            'logits': mat(lay.acts + (self.num_layers - 1) * b * ld, ld, qnet.NUM_ACTIONS * NUM_ATOMS),
            'aux': mat(lay.targets, NUM_ATOMS, NUM_ATOMS), 'dlogits': mat(lay.dlogits, ld, ld), 'loss': loss[:b]}

  # ---- checkpoints
  def _hyper(self) -> tuple:
    return (self.lr, self.eps, self.b1, self.b2, self.gamma, self.lam, self.clip, self.value_coef, self.entropy_coef,
            self.normalize_advantage)

  def state_dict(self) -> dict:
    return {**super().state_dict(), 'hyper': self._hyper()}

  def load_state_dict(self, d: dict) -> None:
    hyper = tuple(d['hyper'])
    if int(d['seed']) != self.seed or hyper != self._hyper():
      self._graphs.clear()                     # (the seed and hyperparameters are arguments of the captured launches)
    (self.lr, self.eps, self.b1, self.b2, self.gamma, self.lam, self.clip, self.value_coef, self.entropy_coef,
     self.normalize_advantage) = hyper
    super().load_state_dict(d)
