"""A population of Q-network policies in one batch.

`QNetworkPopulation` holds P packed images of ONE network shape in a [P, member_stride] device tensor; `VecPopulationAgent` runs them
over a batch of P * R observation rows in one flight -- rows [p R, (p + 1) R) go through image p (`ble_qnet_forward_grouped_f32`).  A row
gets the bits member p's own VecQNetworkAgent (head 'q') or greedy VecActorCriticAgent (head 'actor') gives it: the forward's reduction
order depends on the network's shape alone, so a sweep of checkpoints, the seeds of a study or the members of an evolution strategy fly
the flights they would fly alone, P at a time.
"""
import ctypes
from typing import Dict, Optional, Sequence

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import qnet_train

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
