"""An evolution strategy over a Q-network's parameters on the device: OpenAI-ES (Salimans et al. 2017) with antithetic
pairs, centred-rank shaping and Adam.

`ESTrainer` holds the centre theta in a QNetworkTrainer's allocations (the online image, its transposed mirror, Adam's moments), and a
QNetworkPopulation of P perturbed images.  perturb() writes theta +- sigma eps_i into the population (`ble_es_perturb_f32`); the caller
scores the members -- a VecPopulationAgent flies them all in one batch (train_lib.run_es_loop_vec) -- and update(fitness) turns the
scores into a gradient estimate (`ble_es_gradient_f32`, which regenerates the noise from its Philox address instead of storing it) and
takes one Adam step on it (`ble_qnet_apply_grad_f32`).  No backward pass, no host synchronisation; a run is a pure function of (initial
parameters, seed, fitness values).
"""
import ctypes

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import population as population_lib
from balloon_learning_environment_amd.agents import qnet
from balloon_learning_environment_amd.agents import qnet_train

SHAPINGS = ('centered_rank', 'raw')


def centered_ranks(fitness: torch.Tensor) -> torch.Tensor:
  """float32 [P] in [-0.5, 0.5]: rank / (P - 1) - 0.5, rank 0 the smallest fitness, equal values in member order (a stable sort).
  P == 1 gives 0."""
  p = fitness.numel()
  order = torch.argsort(fitness, stable=True)
  rank = torch.empty_like(order)
  rank[order] = torch.arange(p, dtype=order.dtype, device=fitness.device)
  if p == 1:
    return torch.zeros(1, dtype=torch.float32, device=fitness.device)
  return rank.to(torch.float32) / float(p - 1) - 0.5


class ESTrainer(qnet_train.QNetworkTrainer):
  """Evolution-strategy training of a QNetwork's parameters on its device.

    es = ESTrainer(QNetwork.from_params(init_params('mlp', num_layers=3, hidden_units=256)), population_size=256)
    es.perturb()                                   # es.population: theta +- sigma eps_i, 128 antithetic pairs
    es.update(fitness)                             # float32 [256] on the device, larger is better
    policy = es.network()                          # the centre as a QNetwork

  antithetic: members 2i and 2i + 1 share eps_i with opposite signs (population_size even); otherwise member i has its own eps_i.
  shaping: 'centered_rank' (fitness -> its rank in [-0.5, 0.5]) or 'raw' (the fitness itself).  weight_decay: + wd theta on the gradient.
  lr, adam_eps, b1, b2: Adam's.  The noise of generation g is keyed by (seed, g): the generation counter is device memory, advanced by
  update()."""

  _TENSORS = qnet_train.QNetworkTrainer._TENSORS + ('generation',)

  def __init__(self, network: qnet.QNetwork, population_size: int, sigma: float = 0.02, lr: float = 1e-2, seed: int = 0,
               antithetic: bool = True, weight_decay: float = 0.0, shaping: str = 'centered_rank', adam_eps: float = 1e-8,
               b1: float = 0.9, b2: float = 0.999):
    if shaping not in SHAPINGS:
      raise ValueError(f'shaping is one of {SHAPINGS}, not {shaping!r}')
    p = int(population_size)
    if p < 1 or (antithetic and p % 2):
      raise ValueError('population_size >= 1, and even with antithetic pairs')
    if not sigma > 0.0:
      raise ValueError('sigma > 0')
    super().__init__(network, lr=lr, eps=adam_eps, seed=seed, b1=b1, b2=b2)
    self.sigma, self.weight_decay, self.antithetic, self.shaping = float(sigma), float(weight_decay), bool(antithetic), shaping
    self.population = population_lib.QNetworkPopulation(network, p)
    self.streams = p // 2 if self.antithetic else p
    with torch.cuda.device(self.device):
      self.generation = torch.zeros(1, dtype=torch.int64, device=self.device)      # (read as uint64 by the kernels)
      self._apply_ws = torch.zeros(64, dtype=torch.float32, device=self.device)
      self._w = torch.zeros(self.streams, dtype=torch.float32, device=self.device)

  def _es(self) -> _abi.BleEsF32:
    pop = self.population
    return _abi.BleEsF32(self._net, pop.members, 1 if self.antithetic else 0, pop.member_stride, pop.images.data_ptr(), self.sigma,
                         self.weight_decay, self.seed & (2 ** 64 - 1), self.generation.data_ptr())

  @dev.on_own_device
  def perturb(self) -> population_lib.QNetworkPopulation:
    """Fills the population from the centre with this generation's noise."""
    _lib.call('ble_es_perturb_f32', ctypes.byref(self._es()), dev.stream_ptr(self.device))
    return self.population

  def shape_fitness(self, fitness: torch.Tensor) -> torch.Tensor:
    """The weights the gradient call takes: float32 [streams] from the members' fitness [P]."""
    u = centered_ranks(fitness) if self.shaping == 'centered_rank' else fitness
    return (u[0::2] - u[1::2]) * 0.5 if self.antithetic else u

  @dev.on_own_device
  def estimate(self, w: torch.Tensor) -> torch.Tensor:
    """The gradient of -fitness from the shaped weights w (float32 [streams], device) into .grad (packed); advances the generation."""
    assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() == self.streams and w.device == self.device
    _lib.call('ble_es_gradient_f32', ctypes.byref(self._es()), ctypes.byref(self._struct(self._apply_ws)), w.data_ptr(),
              dev.stream_ptr(self.device))
    return self.grad

  @dev.on_own_device
  def apply_grad(self) -> None:
    """One Adam step on what .grad holds (ble_qnet_apply_grad_f32)."""
    _lib.call('ble_qnet_apply_grad_f32', ctypes.byref(self._struct(self._apply_ws)), dev.stream_ptr(self.device))

  @dev.on_own_device
  def update(self, fitness: torch.Tensor) -> None:
    """One generation's update from the members' fitness (float32 [P] on the device, larger is better)."""
    assert fitness.dtype == torch.float32 and fitness.numel() == self.population.members and fitness.device == self.device
    self._w.copy_(self.shape_fitness(fitness.reshape(-1)))
    self.estimate(self._w)
    self.apply_grad()

  def state_dict(self) -> dict:
    return {**super().state_dict(), 'es': (self.population.members, self.sigma, self.antithetic, self.weight_decay, self.shaping)}

  def load_state_dict(self, d: dict) -> None:
    members, sigma, antithetic, weight_decay, shaping = d['es']
    assert int(members) == self.population.members and bool(antithetic) == self.antithetic, 'checkpoint of another population'
    self.sigma, self.weight_decay, self.shaping = float(sigma), float(weight_decay), shaping
    super().load_state_dict(d)
