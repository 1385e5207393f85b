"""What the look-ahead planners share: VecLookaheadAgent, VecBeamSearchAgent, VecScenarioBeamSearchAgent, VecMCTSAgent and
VecScenarioMCTSAgent derive from VecPlanner and differ in their search alone.  The shell owns the critic rule, the shared constructor checks, bind, the wind
of a decision with its buffers, the leaf score and the small methods; a subclass checks its own sizes, allocates its own buffers
(`_allocate`) and searches (`act`).
"""
import ctypes
from typing import Callable, Optional, Tuple, Union

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd import vec_state


class VecPlanner:
  """A planner for N environments at once: act(obs) -> uint8 [N] device actions, planned in the simulator that `bind` attaches."""

  WINDS: Tuple[str, ...] = ()     # the winds the class plans in
  SEEDED = False                  # bind(seeds=) keys something (the plans' or the scenarios' streams): a new tensor is a new binding
  PLANNER = 'planner()'           # the VecBalloonEnv call that returns a bound agent of the class

  def __init__(self, wind: str, gamma: float, action_repeat: int, segment: int, device, substeps: int):
    """The checks every planner makes, after its own: the wind, the discount, the step counts; then the device and the library."""
    name = type(self).__name__
    if wind not in self.WINDS:
      if wind == 'scenarios':
        raise ValueError(f"{name}: wind='scenarios' is VecScenarioBeamSearchAgent's tree (M end states per node); here plan in "
                         "the belief, the forecast or the truth")
      winds = [repr(w) for w in self.WINDS]
      raise ValueError(f"{name}: wind is {', '.join(winds[:-1])} or {winds[-1]}, not {wind!r}")
    if not 0.0 <= float(gamma) <= 1.0:
      raise ValueError(f'{name}: gamma in [0, 1], not {gamma}')
    if int(segment) < 1 or int(action_repeat) < 1:
      raise ValueError(f'{name}: segment >= 1 and action_repeat >= 1, not {segment}, {action_repeat}')
    self.device = dev.require_gpu(device)
    self.lib = _lib.lib()
    self.wind, self.gamma, self.action_repeat, self.segment, self.substeps = wind, float(gamma), int(action_repeat), int(segment), int(substeps)
    self.sim: Optional[vec_state.VecSimulator] = None
    self._seeds: Optional[torch.Tensor] = None
    self._noise_seed: Union[None, int, Callable[[], int]] = None

  def _critic(self, name: str, critic, signature: str) -> Optional[Callable]:
    """The callable of a critic given as the argument `name` (leaf_value, guide): its act_greedy (a trainer: the live weights), else
    its act -- a sampling agent (deterministic=False) refused --, taking `signature`; None for None."""
    if critic is None:
      return None
    if hasattr(critic, 'act_greedy'):
      return critic.act_greedy
    if getattr(critic, 'deterministic', True) is False:
      raise ValueError(f'{type(self).__name__}: {name} is a sampling agent (deterministic=False): its step counter would move with every '
                       'decision; give a deterministic one, or a trainer (act_greedy)')
    if hasattr(critic, 'act'):
      return critic.act
    raise ValueError(f'{type(self).__name__}: {name} needs act_greedy{signature} or act{signature}')

  # ------------------------------------------------------------------ attach a simulator
  @dev.on_own_device
  def bind(self, sim: vec_state.VecSimulator, seeds: Optional[torch.Tensor] = None, noise_seed=None) -> 'VecPlanner':
    """Attaches the simulator whose environments this agent flies.  All buffers are allocated here, once: binding the same simulator
    (and, where the seeds key a stream, the same `seeds` tensor) again allocates nothing, so a captured graph stays valid.
    seeds: int64 / uint64 device tensor [N], a seed per environment (read at every decision): what the agent draws for an environment
    then does not depend on its batch; an agent that draws nothing accepts and ignores them -- except with wind='truth', which is refused
    with a seed per environment (the look-ahead's noise generator takes one seed).  noise_seed: the seed of the environments' wind
    noise, or a callable returning it, for wind='truth' (None there: the truth is the forecast)."""
    name = type(self).__name__
    if sim.has_fleet:
      raise ValueError(f'{name}: a fleet (set_fleet) has no look-ahead kernel; fly one vehicle per batch (set_vehicle)')
    if sim.device != self.device:
      raise ValueError(f'{name} on {self.device} cannot plan for a simulator on {sim.device}')
    if seeds is not None and self.wind == 'truth':
      raise ValueError(f"{name}: wind='truth' with per-environment seeds: the look-ahead's noise generator takes one seed")
    if not self.SEEDED:
      seeds = None
    if seeds is not None:
      assert seeds.dtype in (torch.int64, torch.uint64) and seeds.is_contiguous() and tuple(seeds.shape) == (sim.n,), seeds.shape
      assert seeds.device == self.device
    same = self.sim is sim and self._seeds is seeds
    self.sim, self._seeds, self._noise_seed = sim, seeds, noise_seed
    if not same:
      self._allocate(sim)
    return self

  def _allocate(self, sim: vec_state.VecSimulator) -> None:
    """The subclass's buffers for `sim` (bind, at a new binding): `action` and what its search writes, and through _allocate_wind the
    wind's."""
    raise NotImplementedError

  def _allocate_wind(self) -> None:
    """The buffers that the wind of a decision is fitted into: a WindBelief, WindScenarios (num_scenarios of them, their streams keyed
    by seed or the bound seeds), or neither."""
    n = self.sim.n
    z = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype, device=self.device)
    self._belief = self._scenarios = None
    if self.wind == 'belief':
      self._belief = vec_state.WindBelief(z(torch.float64, n, _lib.GP_BELIEF_DOUBLES), z(torch.int32, n))
    if self.wind == 'scenarios':
      m = self.num_scenarios
      self._scenarios = vec_state.WindScenarios(z(torch.float64, n, _abi.gp_scenario_doubles(m)), z(torch.int32, n), m, self.seed, self._seeds)

  def _allocate_leaf_rows(self, rows: int) -> None:
    """The critic's observation, value and action rows; the critic is called once at that row count, as a graph capture needs
    (ActorForward's contract)."""
    self.leaf_obs = torch.zeros(rows, _lib.OBS_DIM, dtype=torch.float32, device=self.device)
    self.leaf_values = torch.zeros(rows, dtype=torch.float32, device=self.device)
    self.leaf_actions = torch.zeros(rows, dtype=torch.uint8, device=self.device)
    self._leaf_fn(self.leaf_obs, out=self.leaf_actions, value=self.leaf_values)      # the first call at this row count: not in a capture

  def _bound(self) -> vec_state.VecSimulator:
    if self.sim is None:
      raise ValueError(f'{type(self).__name__}.act before bind(sim): the agent plans in a simulator (VecBalloonEnv.{self.PLANNER} binds one)')
    return self.sim

  # ------------------------------------------------------------------ the parts of a decision
  def _flying(self) -> vec_state.VecSimulator:
    """The bound simulator at act: still one vehicle per batch."""
    sim = self._bound()
    if sim.has_fleet:
      raise ValueError(f'{type(self).__name__}: the bound simulator flies a fleet now; a fleet has no look-ahead kernel')
    return sim

  def _wind(self) -> dict:
    """The wind of this decision as the keyword the search takes (rollout_plans, tree_search, mcts_search): belief= or scenarios=,
    fitted now into the agent's own buffers; noise_seed=, the callable resolved now; nothing for the forecast."""
    if self.wind == 'belief':
      return {'belief': self.sim.fit_wind_belief(out=self._belief)}
    if self.wind == 'scenarios':
      return {'scenarios': self.sim.fit_wind_scenarios(self.num_scenarios, seed=self.seed, seeds=self._seeds, out=self._scenarios)}
    if self.wind == 'truth':
      return {'noise_seed': self._noise_seed() if callable(self._noise_seed) else self._noise_seed}
    return {}

  def _leaf_score(self, leaves, returns, steps_flown, score):
    """score = return + gamma^steps_flown * V(leaf) over a leaf arena: observe_leaves -> the critic -> ble_plan_bootstrap_f32.
    `score` may be `returns` (in place).  A leaf that ended in a terminal keeps its return."""
    sim = self.sim
    sim.observe_leaves(leaves, out=self.leaf_obs)
    self._leaf_fn(self.leaf_obs, out=self.leaf_actions, value=self.leaf_values)
    bs = _abi.BlePlanBootstrap(sim.n, leaves.leaves_per_env, 0, self.gamma, returns.data_ptr(), steps_flown.data_ptr(),
                               leaves.state['status'].data_ptr(), self.leaf_values.data_ptr(), score.data_ptr())
    _lib.check(self.lib.ble_plan_bootstrap_f32(ctypes.byref(bs), dev.stream_ptr(self.device)), 'ble_plan_bootstrap_f32')
    return score

  def _checked_out(self, out: torch.Tensor) -> torch.Tensor:
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == self.sim.n and out.device == self.device
    return out

  def _emit(self, out: Optional[torch.Tensor]) -> torch.Tensor:
    """The decision in self.action, copied into `out` if one is given."""
    if out is None:
      return self.action
    self._checked_out(out).view(-1).copy_(self.action)
    return out

  def __call__(self, *args, **kwargs) -> torch.Tensor:
    return self.act(*args, **kwargs)

  # ------------------------------------------------------------------ the last decision, the run
  def plan(self) -> Tuple[torch.Tensor, torch.Tensor]:
    """(best_plan uint8 [horizon, N], best_return float32 [N]) of the last decision: the agent's own buffers, overwritten by the next
    one.  best_return is what the search ordered by: a return, a risk score, with a leaf_value the bootstrapped score."""
    self._bound()
    return self.best_plan, self.best_return

  def action_values(self) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q float32 [N, 3], visits int32 [N, 3]) of the last decision, for an agent built with action_values=True: q[e, a] the best
    return (or score) among the plans -- in a tree, the last level's nodes -- that begin with action a, -Inf when none of them is
    finite; visits[e, a] how many of them (in a tree: non-void) begin with a.  q[e, action[e]] is best_return[e] wherever that is
    finite.  The agent's own buffers, overwritten by the next decision."""
    self._bound()
    if not self.with_action_values:
      raise ValueError(f'{type(self).__name__}.action_values: build the agent with action_values=True')
    return self.q, self.visits

  def state_dict(self) -> dict:
    """Nothing is carried from one decision to the next: every search starts at the state itself."""
    self._bound()
    return {}

  def load_state_dict(self, d: dict) -> None:
    self._bound()

  def check_errors(self) -> None:
    """The agent latches no error of its own: its kernels cannot fail on valid buffers, and the flags of the flights it imagines stay
    in sim.rollout_flags (a plan that leaves the valid range is no error of the flight that really happens)."""

  def get_name(self) -> str:
    return type(self).__name__[len('Vec'):]
