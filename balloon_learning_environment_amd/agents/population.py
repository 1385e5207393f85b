"""A population of Q-network policies in one batch.

`QNetworkPopulation` holds P packed images of ONE network shape in a [P, member_stride] device tensor; `VecPopulationAgent` runs them
over a batch of P * R observation rows in one flight -- rows [p R, (p + 1) R) go through image p (`ble_qnet_forward_grouped_f32`).  A row
gets the bits member p's own VecQNetworkAgent (head 'q') or greedy VecActorCriticAgent (head 'actor') gives it: the forward's reduction
order depends on the network's shape alone, so a sweep of checkpoints, the seeds of a study or the members of an evolution strategy fly
the flights they would fly alone, P at a time.

`PopulationPPOTrainer` trains the P images by gradient in one batch: one grouped clipped-PPO update of P * B rows
(`ble_qnet_ppo_step_grouped_f32`) gives member p the bytes its own `PPOTrainer` gives it on its B rows, with its own learning rate, clip
and coefficients; `copy_members` and `scale_hyper` are the exploit and explore steps of population-based training
(train_lib.run_pbt_loop_vec).

`PopulationQTrainer` is the same for the replay learners: one grouped QR-DQN or DQN update
(`ble_qnet_td_step_grouped_f32`) on P * B rows drawn from one `VecPopulationReplayBuffer` gives member p the bytes its own
`QNetworkTrainer` / `DQNTrainer` gives it, with its own learning rate, Huber threshold, replay seed and target image
(train_lib.run_population_training_loop_vec).
"""
import ctypes
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import qnet_train

ROW_FLOATS = qnet_train.ROW_FLOATS
HYPER = ('lr', 'clip', 'value_coef', 'entropy_coef')      # the per-member hyperparameters, device [P] float32 each

HEADS = {'q': _abi.POP_HEAD_Q, 'actor': _abi.POP_HEAD_ACTOR_GREEDY}


def member_stride_for(packed_floats: int) -> int:
  """The smallest legal stride between images: the image's size rounded up to 64 floats (every image 256-byte aligned)."""
  return -(-int(packed_floats) // 64) * 64


class QNetworkPopulation:
  """P networks of one shape on the device: images [P, member_stride] float32, image p the packed image of member p.

  QNetworkPopulation(network, members): P copies of `network`.  member_stride (floats, default the image rounded up to 64) may leave
  room between images; the kernels never read it."""

  def __init__(self, network: qnet.QNetwork, members: int, member_stride: Optional[int] = None):
    self.members = int(members)
    if self.members < 1:
      raise ValueError('a population has at least one member')
    self.device = dev.require_gpu(network.device)
    self.num_layers, self.hidden_units, self.num_atoms = network.shape
    self.packed_floats = int(network.packed_host.size)
    self.member_stride = member_stride_for(self.packed_floats) if member_stride is None else int(member_stride)
    if self.member_stride < self.packed_floats or self.member_stride % 64:
      raise ValueError(f'member_stride must be a multiple of 64 and at least the image ({self.packed_floats} floats)')
    with torch.cuda.device(self.device):
      self.images = torch.zeros(self.members, self.member_stride, dtype=torch.float32, device=self.device)
      self.images[:, :self.packed_floats] = torch.from_numpy(network.packed_host).to(self.device)
    self._net = _abi.BleQnetF32(self.num_layers, _lib.OBS_DIM, self.hidden_units, qnet.NUM_ACTIONS, self.num_atoms, 0,
                                self.images.data_ptr())

  @property
  def shape(self):
    """(num_layers, hidden_units, num_atoms) of every member."""
    return self.num_layers, self.hidden_units, self.num_atoms

  @classmethod
  def from_networks(cls, networks: Sequence[qnet.QNetwork], member_stride: Optional[int] = None) -> 'QNetworkPopulation':
    networks = list(networks)
    if not networks:
      raise ValueError('from_networks: no network')
    if any(n.shape != networks[0].shape for n in networks):
      raise ValueError(f'from_networks: the members differ in shape ({sorted({n.shape for n in networks})})')
    pop = cls(networks[0], len(networks), member_stride)
    for p, n in enumerate(networks[1:], 1):
      pop.set_member(p, n)
    return pop

  def set_member(self, p: int, network: qnet.QNetwork) -> None:
    if network.shape != self.shape:
      raise ValueError(f'set_member: a network of shape {network.shape} in a population of shape {self.shape}')
    self.images[self._index(p), :self.packed_floats] = torch.from_numpy(network.packed_host).to(self.device)

  def member(self, p: int) -> qnet.QNetwork:
    """A copy of member p as a QNetwork (ble_qnet_unpack_f32 of its image)."""
    host = self.images[self._index(p), :self.packed_floats].cpu().numpy()
    return qnet.QNetwork.from_params(qnet_train.unpack(self._net, host), num_atoms=self.num_atoms, device=self.device)

  def _index(self, p: int) -> int:
    if not 0 <= int(p) < self.members:
      raise IndexError(f'member {p} of a population of {self.members}')
    return int(p)


class VecPopulationAgent:
  """P policies over P * R environments at once: act(obs [P * R, 1099] float32 device) -> uint8 [P * R] device; row p R + r is row r
  of member p.  head 'q': q = the mean of each action's atoms, argmax (VecQNetworkAgent's rule); 'actor': a two-atom network read as
  an actor, greedy (VecActorCriticAgent's).  The scratch is allocated on the first call, which must not be inside a graph capture."""

  def __init__(self, population: QNetworkPopulation, rows_per_member: int, head: str = 'q'):
    if head not in HEADS:
      raise ValueError(f"head is 'q' or 'actor', not {head!r}")
    if head == 'actor' and population.num_atoms != 2:
      raise ValueError("head 'actor' reads a two-atom network")
    self.population, self.head = population, head
    self.rows_per_member = int(rows_per_member)
    if self.rows_per_member < 1:
      raise ValueError('rows_per_member >= 1')
    self.device = population.device
    self.n = population.members * self.rows_per_member
    self._scratch: Dict[int, torch.Tensor] = {}

  def _allocate(self) -> torch.Tensor:
    floats = ctypes.c_int64()
    _lib.call('ble_qnet_workspace_f32', ctypes.byref(self.population._net), self.n, None, ctypes.byref(floats))
    return torch.empty(max(floats.value, 1), dtype=torch.float32, device=self.device)

  def logits(self) -> torch.Tensor:
    """The last call's logits [P * R, 3 * num_atoms] (a view of the scratch)."""
    s = self._scratch[self.n]
    ld = s.numel() // (2 * self.n)
    off = ((self.population.num_layers - 1) & 1) * self.n * ld
    return s[off:off + self.n * ld].view(self.n, ld)[:, :qnet.NUM_ACTIONS * self.population.num_atoms]

  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, q_values: Optional[torch.Tensor] = None,
          value: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """obs: [P * R, >= 1099] float32 on the population's device (stride(1) == 1).  out: optional uint8 [P * R]; q_values: optional
    float32 [P * R, 3] (head 'q'); value [P * R] and probs [P * R, 3]: optional float32 (head 'actor')."""
    assert obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] >= _lib.OBS_DIM and obs.stride(1) == 1, (obs.dtype, obs.shape)
    assert obs.device == self.device
    n = self.n
    assert obs.shape[0] == n, f'{obs.shape[0]} rows for {self.population.members} members x {self.rows_per_member} rows'
    if out is None:
      out = torch.empty(n, dtype=torch.uint8, device=self.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n
    for t, width in ((q_values, qnet.NUM_ACTIONS), (value, 1), (probs, qnet.NUM_ACTIONS)):
      assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n * width)
    scratch = dev.first_use(self._scratch, n, self._allocate,
                            f'VecPopulationAgent: call act once at batch size {n} before capturing it in a graph (scratch allocation)')
    stride = obs.stride(0) if n > 1 else max(obs.stride(0), _lib.OBS_DIM)
    pop = self.population
    desc = _abi.BleQnetGroupedF32(pop._net, pop.members, HEADS[self.head], pop.member_stride, self.rows_per_member, stride, obs.data_ptr(),
                                  scratch.data_ptr(), out.data_ptr(), dev.ptr(q_values) or None, dev.ptr(value) or None,
                                  dev.ptr(probs) or None)
    _lib.call('ble_qnet_forward_grouped_f32', ctypes.byref(desc), dev.stream_ptr(self.device))
    return out

  __call__ = act

  def get_name(self) -> str:
    kind = 'ActorCritic' if self.head == 'actor' else ('QuantileAgent' if self.population.num_atoms > 1 else 'DQNAgent')
    return f'Population[{self.population.members} x {kind}]'


class PopulationPPOBatch:
  """One grouped minibatch of P * B on-policy rows (static device buffers), rows [p B, (p + 1) B) member p's: state, ret, action,
  old_logp, advantage (PPOBatch's, P times)."""

  def __init__(self, members: int, rows_per_member: int, device):
    self.members, self.rows_per_member = int(members), int(rows_per_member)
    n = self.batch_size = self.members * self.rows_per_member
    self.state = torch.zeros(n, ROW_FLOATS, dtype=torch.float32, device=device)
    self.ret = torch.zeros(n, dtype=torch.float32, device=device)
    self.action = torch.zeros(n, dtype=torch.uint8, device=device)
    self.old_logp = torch.zeros(n, dtype=torch.float32, device=device)
    self.advantage = torch.zeros(n, dtype=torch.float32, device=device)
    self.struct = _abi.BleTrainBatchF32(n, ROW_FLOATS, self.state.data_ptr(), None, self.ret.data_ptr(), None, self.action.data_ptr(), None)


def _per_member(name: str, value, members: int) -> np.ndarray:
  """A scalar or a length-P sequence as float32 [P]; finite (the entry point cannot see device values)."""
  a = np.asarray(value, np.float64)
  a = np.full(members, float(a)) if a.ndim == 0 else a.reshape(-1)
  if a.shape != (members,):
    raise ValueError(f'{name}: a scalar or {members} values, not {a.shape[0]}')
  a = a.astype(np.float32)
  if not np.isfinite(a).all() or (name == 'clip' and not (a > 0).all()):
    raise ValueError(f'{name} must be finite' + (' and > 0' if name == 'clip' else '') + f', not {a.tolist()}')
  return a


class PopulationPPOTrainer:
  """Clipped-PPO training of a QNetworkPopulation of two-atom networks, all P members in one update.

    pop = QNetworkPopulation(qnet.QNetwork.from_params(actor_critic.init_params('actor_critic'), num_atoms=2), 16)
    trainer = PopulationPPOTrainer(pop, lr=[1e-4 * 1.3 ** p for p in range(16)])
    train_lib.run_pbt_loop_vec(env, trainer, VecPopulationRolloutBuffer(16, env.num_envs // 16, 32), ...)

  lr, clip, value_coef, entropy_coef: scalars or length-P sequences, held as device [P] float32 tensors of those names.  The trainer
  trains population.images in place: a VecPopulationAgent or eval_population_vec on the same population sees the live weights.  It owns
  weights_t, grad, adam_m, adam_v ([P, stride] each), one adam_step and one act_step (the members update and act in lockstep).  Member
  p's images hold the bytes PPOTrainer(member p, lr=lr[p], ..., seed=seed, env_offset=p * R) holds after the same rows."""

  _TENSORS = ('weights_t', 'adam_m', 'adam_v', 'adam_step', 'act_step') + HYPER

  def __init__(self, population: QNetworkPopulation, *, lr: Union[float, Sequence[float]] = 3e-4,
               clip: Union[float, Sequence[float]] = 0.2, value_coef: Union[float, Sequence[float]] = 0.5,
               entropy_coef: Union[float, Sequence[float]] = 0.01, eps: float = 1e-5, b1: float = 0.9, b2: float = 0.999,
               gamma: float = 0.993, lam: float = 0.95, normalize_advantage: bool = True, seed: int = 0):
    if population.num_atoms != 2:
      raise ValueError(f'PopulationPPOTrainer needs two-atom networks (policy logits and a value), not {population.num_atoms} atoms')
    self.population = population
    self.device = d = population.device
    self.members = p = population.members
    self.num_layers, self.hidden_units, self.num_atoms = population.shape
    self.eps, self.b1, self.b2 = float(eps), float(b1), float(b2)
    self.gamma, self.lam = float(gamma), float(lam)
    self.normalize_advantage, self.seed = bool(normalize_advantage), int(seed)
    self._net = population._net
    lay = self._layout(1)
    self.transposed_floats = int(lay.transposed_floats)
    self.transposed_stride = member_stride_for(max(self.transposed_floats, 64))
    with torch.cuda.device(d):
      for name, value in zip(HYPER, (lr, clip, value_coef, entropy_coef)):
        setattr(self, name, torch.from_numpy(_per_member(name, value, p)).to(d))
      self.weights_t = torch.zeros(p, self.transposed_stride, dtype=torch.float32, device=d)
      self.grad = torch.zeros_like(population.images)
      self.adam_m = torch.zeros_like(population.images)
      self.adam_v = torch.zeros_like(population.images)
      self.adam_step = torch.zeros(1, dtype=torch.int64, device=d)
      self.act_step = torch.zeros(1, dtype=torch.int64, device=d)      # (read as uint64 by the kernel)
      self.err_flags = torch.zeros(1, dtype=torch.int32, device=d)
    self._retranspose()
    self._act_buffers: Dict[int, tuple] = {}
    self._ws: Dict[int, tuple] = {}
    self._graphs: dict = {}

  # ---- plumbing
  @property
  def images(self) -> torch.Tensor:
    return self.population.images

  def _struct(self, batch_rows: int, workspace: Optional[torch.Tensor] = None, batch: Optional[PopulationPPOBatch] = None,
              apply_update: bool = True) -> _abi.BlePpoGroupedF32:
    pop = self.population
    tr = _abi.BleQnetTrainF32(pop._net, None, self.weights_t.data_ptr(), self.grad.data_ptr(), self.adam_m.data_ptr(), self.adam_v.data_ptr(),
                              self.adam_step.data_ptr(), dev.ptr(workspace) or None, self.b1, self.b2, 0.0, self.eps, 0.0,
                              1 if apply_update else 0)
    return _abi.BlePpoGroupedF32(tr, self.members, 0, pop.member_stride, self.transposed_stride, int(batch_rows), self.lr.data_ptr(),
                                 self.clip.data_ptr(), self.value_coef.data_ptr(), self.entropy_coef.data_ptr(),
                                 None if batch is None else batch.old_logp.data_ptr(), None if batch is None else batch.advantage.data_ptr())

  def _layout(self, batch_rows: int) -> _abi.BleQnetTrainLayout:
    out = _abi.BleQnetTrainLayout()
    g = _abi.BlePpoGroupedF32(_abi.BleQnetTrainF32(self._net), self.members, 0, 0, 0, int(batch_rows))
    _lib.call('ble_qnet_ppo_grouped_workspace_f32', ctypes.byref(g), ctypes.byref(out))
    return out

  def _retranspose(self) -> None:
    """weights_t of every member from its image (host transposes; at construction and after a load)."""
    pop = self.population
    host = pop.images[:, :pop.packed_floats].cpu().numpy()
    host_t = np.zeros((self.members, self.transposed_stride), np.float32)
    for p in range(self.members):
      w = np.ascontiguousarray(host[p])
      _lib.call('ble_qnet_transpose_f32', ctypes.byref(self._net), w.ctypes.data, host_t[p].ctypes.data)
    self.weights_t.copy_(torch.from_numpy(host_t))

  def workspace(self, batch_rows: int):
    """(workspace tensor, layout, loss [P * B]) of B rows per member (allocated on first use, which must not be inside a capture)."""
    def make():
      lay = self._layout(batch_rows)
      with torch.cuda.device(self.device):
        return (torch.zeros(max(lay.total, 64), dtype=torch.float32, device=self.device), lay,
                torch.zeros(self.members * batch_rows, dtype=torch.float32, device=self.device))
    return dev.first_use(self._ws, int(batch_rows), make,
                         f'PopulationPPOTrainer: run one update at {batch_rows} rows per member before capturing it')

  def check_errors(self) -> None:
    qnet_train._check_flags(self.err_flags)

  # ---- acting
  def _act(self, obs: torch.Tensor, out, logp, value, probs, sampled: bool) -> torch.Tensor:
    assert obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] >= _lib.OBS_DIM and obs.stride(1) == 1, (obs.dtype, obs.shape)
    assert obs.device == self.device
    n = obs.shape[0]
    assert n >= self.members and n % self.members == 0, f'{n} rows for {self.members} members'

    def make():
      floats = ctypes.c_int64()
      _lib.call('ble_qnet_workspace_f32', ctypes.byref(self._net), n, None, ctypes.byref(floats))
      return (torch.empty(max(floats.value, 1), dtype=torch.float32, device=self.device),
              torch.empty(n, dtype=torch.float32, device=self.device))
    scratch, own_logp = dev.first_use(self._act_buffers, n, make,
                                      f'PopulationPPOTrainer: call act once at batch size {n} before capturing it in a graph')
    if out is None:
      out = torch.empty(n, dtype=torch.uint8, device=self.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n
    for t, numel in ((logp, n), (value, n), (probs, n * qnet.NUM_ACTIONS)):
      assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel)
    stride = obs.stride(0) if n > 1 else max(obs.stride(0), _lib.OBS_DIM)
    pop = self.population
    desc = _abi.BleQnetGroupedF32(pop._net, pop.members, _abi.POP_HEAD_ACTOR_GREEDY, pop.member_stride, n // pop.members, stride,
                                  obs.data_ptr(), scratch.data_ptr(), out.data_ptr(), None, dev.ptr(value) or None, dev.ptr(probs) or None)
    sample = _abi.BleAcSample(self.seed & (2 ** 64 - 1), 0, self.act_step.data_ptr(), 0) if sampled else None
    _lib.call('ble_ac_act_grouped_f32', ctypes.byref(desc), ctypes.byref(sample) if sampled else None,
              (own_logp if logp is None else logp).data_ptr(), dev.stream_ptr(self.device))
    return out

  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None,
          value: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sampled actions of the live images over P * R rows (rows [p R, (p + 1) R) member p's): what PPOTrainer.act of member p with
    env_offset = p R gives; the device step counter advances after each call."""
    out = self._act(obs, out, logp, value, probs, True)
    self.act_step.add_(1)
    return out

  @dev.on_own_device
  def act_greedy(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None,
                 value: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Greedy actions of the live images; the step counter stays."""
    return self._act(obs, out, logp, value, probs, False)

  # ---- the update
  @dev.on_own_device
  def train_on_batch(self, batch: PopulationPPOBatch, apply_update: bool = True) -> torch.Tensor:
    """One grouped update: the per-row losses [P * B] (a view of a buffer the next update at this size overwrites)."""
    assert batch.members == self.members
    ws, _, loss = self.workspace(batch.rows_per_member)
    g = self._struct(batch.rows_per_member, ws, batch, apply_update)
    _lib.call('ble_qnet_ppo_step_grouped_f32', ctypes.byref(g), ctypes.byref(batch.struct), loss.data_ptr(), self.err_flags.data_ptr(),
              dev.stream_ptr(self.device))
    return loss

  def train_step(self, batch: PopulationPPOBatch) -> torch.Tensor:
    """train_on_batch, by the captured graph of this batch's buffers when there is one (capture())."""
    g = self._graphs.get(batch.rows_per_member)
    if g is not None and g[1] is batch:
      g[0].replay()
      return g[2]
    return self.train_on_batch(batch)

  def capture(self, batch: PopulationPPOBatch) -> torch.Tensor:
    """Records one grouped update on `batch`'s static buffers into a HIP graph that train_step(batch) replays from then on (the
    hyperparameters are device arrays: a replay reads their current values).  Runs one eager update first -- a real update; returns
    its per-row losses."""
    first = self.train_on_batch(batch)
    graph, loss = dev.capture(self.device, lambda: self.train_on_batch(batch))
    self._graphs[batch.rows_per_member] = (graph, batch, loss)
    return first

  def views(self, batch_rows: int) -> dict:
    """The workspace's tensors of the last update at B rows per member, member-major: 'acts' (every layer's output, [P, B, ld] each),
    'logits' [P, B, 6], 'aux' [P, B, 2], 'dlogits' [P, B, ld], 'loss' [P, B]."""
    ws, lay, loss = self.workspace(batch_rows)
    p, b, ld = self.members, int(batch_rows), lay.ld
    n = p * b

    def mat(off, cols, width):
      return ws[off:off + n * cols].view(p, b, cols)[:, :, :width]
    return {'acts': [mat(lay.acts + l * n * ld, ld, ld) for l in range(self.num_layers)],
            'logits': mat(lay.acts + (self.num_layers - 1) * n * ld, ld, qnet.NUM_ACTIONS * 2),
            'aux': mat(lay.targets, 2, 2), 'dlogits': mat(lay.dlogits, ld, ld), 'loss': loss.view(p, b)}

  # ---- population-based training
  @dev.on_own_device
  def copy_members(self, src: torch.Tensor, dst: torch.Tensor) -> None:
    """Rows dst of the images, weights_t, adam_m, adam_v and the four hyperparameter tensors become rows src (device int64 index
    tensors of one length, dst without repeats).  No host synchronisation."""
    assert src.shape == dst.shape and src.dim() == 1 and src.dtype == dst.dtype == torch.int64
    for t in (self.population.images, self.weights_t, self.adam_m, self.adam_v) + tuple(getattr(self, k) for k in HYPER):
      t.index_copy_(0, dst, t.index_select(0, src))

  @dev.on_own_device
  def scale_hyper(self, name: str, dst: torch.Tensor, factor) -> None:
    """hyper[name][dst] *= factor (a float, or a float32 device tensor of dst's length): a float32 product on the device."""
    if name not in HYPER:
      raise ValueError(f'scale_hyper: {name!r} is not one of {HYPER}')
    t = getattr(self, name)
    f = factor if isinstance(factor, torch.Tensor) else torch.full((dst.numel(),), float(factor), dtype=torch.float32, device=self.device)
    assert f.dtype == torch.float32 and f.shape == dst.shape
    t.index_copy_(0, dst, t.index_select(0, dst) * f)

  # ---- export and checkpoints
  def member(self, p: int) -> qnet.QNetwork:
    """A copy of member p's live parameters as a QNetwork."""
    return self.population.member(p)

  def member_trainer_state(self, p: int) -> dict:
    """Member p's part as a PPOTrainer.state_dict(): PPOTrainer(...).load_state_dict of it continues member p alone."""
    p = self.population._index(p)
    n = self.population.packed_floats
    h = {k: float(getattr(self, k)[p].item()) for k in HYPER}
    return {'shape': self.population.shape, 'seed': self.seed, 'weights': self.population.images[p, :n].clone(),
            'adam_m': self.adam_m[p, :n].clone(), 'adam_v': self.adam_v[p, :n].clone(), 'adam_step': self.adam_step.clone(),
            'act_step': self.act_step.clone(),
            'hyper': (h['lr'], self.eps, self.b1, self.b2, self.gamma, self.lam, h['clip'], h['value_coef'], h['entropy_coef'],
                      self.normalize_advantage)}

  def state_dict(self) -> dict:
    return {'shape': self.population.shape, 'members': self.members, 'seed': self.seed, 'images': self.population.images.clone(),
            'hyper': (self.eps, self.b1, self.b2, self.gamma, self.lam, self.normalize_advantage),
            **{k: getattr(self, k).clone() for k in self._TENSORS}}

  def load_state_dict(self, d: dict) -> None:
    """Restores in place (every tensor keeps its address: captured graphs stay valid unless a host-side argument changed)."""
    assert tuple(d['shape']) == self.population.shape and int(d['members']) == self.members, 'checkpoint of another population'
    hyper = tuple(d['hyper'])
    if int(d['seed']) != self.seed or hyper != (self.eps, self.b1, self.b2, self.gamma, self.lam, self.normalize_advantage):
      self._graphs.clear()                     # (Adam's constants are arguments of the captured launches)
    self.seed = int(d['seed'])
    self.eps, self.b1, self.b2, self.gamma, self.lam, self.normalize_advantage = hyper
    self.population.images.copy_(d['images'])
    for k in self._TENSORS:
      getattr(self, k).copy_(d[k])


Q_KINDS = {'quantile': _abi.TD_GROUPED_QUANTILE, 'dqn_mse': _abi.TD_DQN_MSE + 1, 'dqn_huber': _abi.TD_DQN_HUBER + 1}
Q_HYPER = ('lr', 'kappa')                                 # the replay learners' per-member hyperparameters, device [P] float32 each


def _per_member_q(name: str, value, members: int) -> np.ndarray:
  """_per_member for Q_HYPER: finite, and a Huber threshold > 0."""
  a = _per_member(name, value, members)
  if name == 'kappa' and not (a > 0).all():
    raise ValueError(f'kappa must be > 0, not {a.tolist()}')
  return a


class PopulationQTrainer:
  """QR-DQN / DQN training of a QNetworkPopulation, all P members in one update.

    pop = QNetworkPopulation(qnet.QNetwork.from_params(qnet.init_params('quantile')), 16)
    trainer = PopulationQTrainer(pop, kind='quantile', lr=[2e-6 * 1.5 ** p for p in range(16)], seed=0)
    replay = qnet_train.VecPopulationReplayBuffer(16, env.num_envs // 16, 1024)
    train_lib.run_population_training_loop_vec(env, trainer, replay, num_iterations=..., steps_per_iteration=..., epsilon=[...])

  kind: 'quantile' (QNetworkTrainer's update), 'dqn_mse' or 'dqn_huber' (DQNTrainer's, one-atom networks).  lr, kappa: scalars or
  length-P sequences, held as device [P] float32 tensors of those names (kappa is read by the quantile loss alone).  seed: a scalar
  (member p draws its replay batches and explores with seed + p) or a length-P sequence, held as `seeds`, device int64 [P] read as
  uint64.  The trainer trains population.images in place; it owns target, weights_t, grad, adam_m, adam_v ([P, stride] each), one
  adam_step and one replay counter (the members update in lockstep).  Member p's images hold the bytes a QNetworkTrainer / DQNTrainer
  of member p with lr[p], kappa[p] and seed seeds[p] holds after the same rows (member_trainer_state(p) is that trainer's state_dict)."""

  _TENSORS = ('target', 'weights_t', 'adam_m', 'adam_v', 'adam_step', 'counter', 'seeds') + Q_HYPER

  def __init__(self, population: QNetworkPopulation, *, kind: str = 'quantile', lr: Union[float, Sequence[float]] = 2e-6,
               kappa: Union[float, Sequence[float]] = 1.0, eps: float = 2e-5, gamma: float = 0.993, update_horizon: int = 5,
               seed: Union[int, Sequence[int]] = 0, b1: float = 0.9, b2: float = 0.999):
    if kind not in Q_KINDS:
      raise ValueError(f'kind is one of {sorted(Q_KINDS)}, not {kind!r}')
    if kind != 'quantile' and population.num_atoms != 1:
      raise ValueError(f'{kind!r} trains one-atom networks, not {population.num_atoms} atoms')
    self.population, self.kind = population, kind
    self.device = d = population.device
    self.members = p = population.members
    self.num_layers, self.hidden_units, self.num_atoms = population.shape
    self.eps, self.b1, self.b2 = float(eps), float(b1), float(b2)
    self.gamma, self.update_horizon = float(gamma), int(update_horizon)
    self._net = population._net
    lay = self._layout(1)
    self.transposed_floats = int(lay.transposed_floats)
    self.transposed_stride = member_stride_for(max(self.transposed_floats, 64))
    with torch.cuda.device(d):
      for name, value in zip(Q_HYPER, (lr, kappa)):
        setattr(self, name, torch.from_numpy(_per_member_q(name, value, p)).to(d))
      self.seeds = qnet_train.member_seeds(seed, p, d)
      self.target = population.images.clone()
      self.weights_t = torch.zeros(p, self.transposed_stride, dtype=torch.float32, device=d)
      self.grad = torch.zeros_like(population.images)
      self.adam_m = torch.zeros_like(population.images)
      self.adam_v = torch.zeros_like(population.images)
      self.adam_step = torch.zeros(1, dtype=torch.int64, device=d)
      self.counter = torch.zeros(1, dtype=torch.int64, device=d)       # the update counter every member's replay draw is keyed by
      self.err_flags = torch.zeros(1, dtype=torch.int32, device=d)
    self._retranspose()
    self._agents: Dict[int, VecPopulationAgent] = {}
    self._ws: Dict[int, tuple] = {}
    self._graphs: dict = {}

  # ---- plumbing
  @property
  def images(self) -> torch.Tensor:
    return self.population.images

  def _struct(self, batch_rows: int, workspace: Optional[torch.Tensor] = None, apply_update: bool = True) -> _abi.BleTdGroupedF32:
    pop = self.population
    tr = _abi.BleQnetTrainF32(pop._net, self.target.data_ptr(), self.weights_t.data_ptr(), self.grad.data_ptr(), self.adam_m.data_ptr(),
                              self.adam_v.data_ptr(), self.adam_step.data_ptr(), dev.ptr(workspace) or None, self.b1, self.b2, 0.0, self.eps,
                              0.0, 1 if apply_update else 0)
    return _abi.BleTdGroupedF32(tr, self.members, 0, pop.member_stride, self.transposed_stride, int(batch_rows), Q_KINDS[self.kind], 0,
                                self.lr.data_ptr(), self.kappa.data_ptr())

  def _layout(self, batch_rows: int) -> _abi.BleQnetTrainLayout:
    out = _abi.BleQnetTrainLayout()
    g = _abi.BleTdGroupedF32(_abi.BleQnetTrainF32(self._net), self.members, 0, 0, 0, int(batch_rows), Q_KINDS[self.kind])
    _lib.call('ble_qnet_td_grouped_workspace_f32', ctypes.byref(g), ctypes.byref(out))
    return out

  _retranspose = PopulationPPOTrainer._retranspose

  def workspace(self, batch_rows: int):
    """(workspace tensor, layout, loss [P * B]) of B rows per member (allocated on first use, which must not be inside a capture)."""
    def make():
      lay = self._layout(batch_rows)
      with torch.cuda.device(self.device):
        return (torch.zeros(max(lay.total, 64), dtype=torch.float32, device=self.device), lay,
                torch.zeros(self.members * batch_rows, dtype=torch.float32, device=self.device))
    return dev.first_use(self._ws, int(batch_rows), make,
                         f'PopulationQTrainer: run one update at {batch_rows} rows per member before capturing it')

  def check_errors(self) -> None:
    qnet_train._check_flags(self.err_flags)

  # ---- acting
  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The live images' greedy actions over P * R rows, rows [p R, (p + 1) R) member p's (ble_qnet_forward_grouped_f32,
    BLE_POP_HEAD_Q): what member p's own trainer's act gives its rows.  No host synchronisation."""
    n = obs.shape[0]
    assert n >= self.members and n % self.members == 0, f'{n} rows for {self.members} members'
    agent = self._agents.get(n)
    if agent is None:
      agent = self._agents[n] = VecPopulationAgent(self.population, n // self.members, 'q')
    return agent.act(obs, out)

  # ---- the update
  @dev.on_own_device
  def train_on_batch(self, batch: qnet_train.TrainBatch, apply_update: bool = True) -> torch.Tensor:
    """One grouped update on a batch of P * B rows (rows [p B, (p + 1) B) member p's): the per-row losses [P * B] (a view of a buffer
    the next update at this size overwrites)."""
    assert batch.batch_size >= self.members and batch.batch_size % self.members == 0, f'{batch.batch_size} rows for {self.members} members'
    rows = batch.batch_size // self.members
    ws, _, loss = self.workspace(rows)
    g = self._struct(rows, ws, apply_update)
    _lib.call('ble_qnet_td_step_grouped_f32', ctypes.byref(g), ctypes.byref(batch.struct), loss.data_ptr(), self.err_flags.data_ptr(),
              dev.stream_ptr(self.device))
    return loss

  @dev.on_own_device
  def train_step(self, replay: 'qnet_train.VecPopulationReplayBuffer', batch_size: int = 32) -> torch.Tensor:
    """Sample B rows per member (member p keyed by (seeds[p], update counter)) and update: per-row losses [P * B] on the device, no
    host synchronisation.  A captured graph of this batch size (capture()) replays it.  With a VecPopulationPrioritizedReplayBuffer of
    this population's member count the update is followed by the grouped set_priority and the losses returned are the
    importance-weighted ones, each member's normalised by its own largest weight; a plain VecPrioritizedReplayBuffer, or a
    buffer of another member count, is refused."""
    g = self._graphs.get(batch_size)
    if g is not None and g[1] is replay:
      g[0].replay()
      return g[2]
    return self._update(replay, batch_size)

  def _update(self, replay, batch_size: int) -> torch.Tensor:
    if getattr(replay, 'members', None) != self.members:      # (a plain VecPrioritizedReplayBuffer has no members)
      raise ValueError(f'PopulationQTrainer samples a VecPopulationReplayBuffer of its {self.members} members')
    batch = replay.sample(batch_size, self.seeds, self.counter)
    loss = self.train_on_batch(batch)
    if replay.prioritized:                          # sample -> grouped update -> set_priority; the reported loss is the weighted one
      return replay.set_priority(batch, loss)
    return loss

  def capture(self, replay, batch_size: int = 32) -> torch.Tensor:
    """Records one update (grouped sample + grouped train step, + the grouped set_priority with a prioritized population buffer) into
    a HIP graph that train_step(replay, batch_size) replays from then on: the counters, seeds and hyperparameters are device memory, so each replay draws a new batch, takes a new Adam step and reads
    their current values.  Runs one eager update first (the lazy allocations) -- a real update; returns its per-row losses."""
    first = self.train_step(replay, batch_size)
    graph, loss = dev.capture(self.device, lambda: self._update(replay, batch_size))
    self._graphs[batch_size] = (graph, replay, loss)
    return first

  @dev.on_own_device
  def sync_target(self) -> None:
    """Every member's target image = its online image, in one copy."""
    self.target.copy_(self.population.images)

  def views(self, batch_rows: int) -> dict:
    """The workspace's tensors of the last update at B rows per member, member-major: 'acts' (every online layer's output, [P, B, ld]
    each), 'logits' and 'target_logits' [P, B, 3 * atoms], 'targets' [P, B, atoms], 'dlogits' [P, B, ld], 'loss' [P, B]."""
    ws, lay, loss = self.workspace(batch_rows)
    p, b, ld, out = self.members, int(batch_rows), lay.ld, qnet.NUM_ACTIONS * self.num_atoms
    n = p * b

    def mat(off, cols, width):
      return ws[off:off + n * cols].view(p, b, cols)[:, :, :width]
    return {'acts': [mat(lay.acts + l * n * ld, ld, ld) for l in range(self.num_layers)],
            'logits': mat(lay.acts + (self.num_layers - 1) * n * ld, ld, out), 'target_logits': mat(lay.target_logits, ld, out),
            'targets': mat(lay.targets, self.num_atoms, self.num_atoms), 'dlogits': mat(lay.dlogits, ld, ld), 'loss': loss.view(p, b)}

  # ---- population-based training
  @dev.on_own_device
  def copy_members(self, src: torch.Tensor, dst: torch.Tensor) -> None:
    """Rows dst of the images, the target, weights_t, adam_m, adam_v and the hyperparameter tensors become rows src (device int64
    index tensors of one length, dst without repeats).  The seeds stay: a copy draws its own batches and explores its own way.  The
    replay contents stay the columns' own, and with them the priorities of a VecPopulationPrioritizedReplayBuffer (trees and maxima)
    and the state of a VecPopulationMarcoPoloExploration, which belong to the environment rows.  No host synchronisation."""
    assert src.shape == dst.shape and src.dim() == 1 and src.dtype == dst.dtype == torch.int64
    for t in (self.population.images, self.target, self.weights_t, self.adam_m, self.adam_v) + tuple(getattr(self, k) for k in Q_HYPER):
      t.index_copy_(0, dst, t.index_select(0, src))

  @dev.on_own_device
  def scale_hyper(self, name: str, dst: torch.Tensor, factor) -> None:
    """hyper[name][dst] *= factor (a float, or a float32 device tensor of dst's length): a float32 product on the device."""
    if name not in Q_HYPER:
      raise ValueError(f'scale_hyper: {name!r} is not one of {Q_HYPER}')
    t = getattr(self, name)
    f = factor if isinstance(factor, torch.Tensor) else torch.full((dst.numel(),), float(factor), dtype=torch.float32, device=self.device)
    assert f.dtype == torch.float32 and f.shape == dst.shape
    t.index_copy_(0, dst, t.index_select(0, dst) * f)

  # ---- export and checkpoints
  def member(self, p: int) -> qnet.QNetwork:
    """A copy of member p's live parameters as a QNetwork."""
    return self.population.member(p)

  def member_trainer_state(self, p: int) -> dict:
    """Member p's part as the state_dict() of its own trainer -- QNetworkTrainer (kind 'quantile') or DQNTrainer (loss_type 'mse' /
    'huber'): that trainer's load_state_dict of it continues member p alone, on member_buffer(p) of the replay."""
    p = self.population._index(p)
    n = self.population.packed_floats
    seed = int(self.seeds[p].item()) & (2 ** 64 - 1)
    d = {'shape': self.population.shape, 'seed': seed, 'weights': self.population.images[p, :n].clone(), 'target': self.target[p, :n].clone(),
         'adam_m': self.adam_m[p, :n].clone(), 'adam_v': self.adam_v[p, :n].clone(), 'adam_step': self.adam_step.clone(),
         'counter': self.counter.clone(),
         'hyper': (float(self.lr[p].item()), self.eps, self.b1, self.b2, float(self.kappa[p].item()), self.gamma, self.update_horizon)}
    if self.kind != 'quantile':
      d['loss_type'] = self.kind[len('dqn_'):]
    return d

  def state_dict(self) -> dict:
    return {'shape': self.population.shape, 'members': self.members, 'kind': self.kind, 'images': self.population.images.clone(),
            'hyper': (self.eps, self.b1, self.b2, self.gamma, self.update_horizon),
            **{k: getattr(self, k).clone() for k in self._TENSORS}}

  def load_state_dict(self, d: dict) -> None:
    """Restores in place (every tensor keeps its address: captured graphs stay valid unless a host-side argument changed)."""
    assert tuple(d['shape']) == self.population.shape and int(d['members']) == self.members, 'checkpoint of another population'
    assert d['kind'] == self.kind, f"checkpoint of a {d['kind']!r} trainer"
    hyper = tuple(d['hyper'])
    if hyper != (self.eps, self.b1, self.b2, self.gamma, self.update_horizon):
      self._graphs.clear()                     # (Adam's constants are arguments of the captured launches)
    self.eps, self.b1, self.b2, self.gamma, self.update_horizon = hyper
    self.population.images.copy_(d['images'])
    for k in self._TENSORS:
      getattr(self, k).copy_(d[k])
