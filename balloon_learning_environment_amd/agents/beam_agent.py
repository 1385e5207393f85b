"""A model-predictive agent that SEARCHES its plans (no counterpart in the reference).

Where VecLookaheadAgent samples K plans and flies each of them from the root, this agent grows a shared-prefix tree of plans level by
level (`VecSimulator.tree_search`: `ble_tree_expand_f32`, `ble_tree_select_f32`, `ble_tree_finish_f32`): every level flies the three
children of the best `beam_width` nodes of the one before for one segment, so a prefix is flown once however many plans share it, and
the search is systematic and deterministic -- there is no random stream and no seed.  With 3^depth <= 3 * beam_width it is the
enumeration of all 3^depth plans.  No host synchronisation anywhere, so a decision is capturable in the same HIP graph as the step.
The agent needs no trained weights; it needs the simulator, which `bind` attaches (eval_lib.VecEvaluator does that for any agent with a
`bind`; `VecBalloonEnv.planner(search='beam')` returns a bound agent).
"""
import ctypes
from typing import Callable, Optional, Tuple, Union

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd import vec_state

WINDS = ('belief', 'forecast', 'truth')


class VecBeamSearchAgent:
  """Beam search over action plans for N environments at once: act(obs) -> uint8 [N] device actions.

  depth D levels of one action each, flown `segment` plan entries x action_repeat agent steps (D * segment * action_repeat <= 960); the
  best beam_width B (<= 256) nodes of a level are expanded into 3 B children.  gamma: the discount of a plan's return.
  wind: 'belief' (default) -- forecast + the mean of the WindGP over the balloon's own measurements, fitted at every decision;
  'forecast' -- the forecast alone; 'truth' -- the wind the environments will fly (bind(noise_seed=)): a simulator-side upper bound.
  Scenario winds are VecScenarioBeamSearchAgent's ('scenarios' is refused here).
  leaf_value: a critic -- an object with act_greedy(obs, value=) or else act(obs, value=), VecLookaheadAgent's rule --
  whose value of every node of the LAST level is added to its return before the final order: score = return + gamma^steps_flown *
  V(node) (`observe_leaves` -> the critic -> `ble_plan_bootstrap_f32`); the inner levels are ordered by their returns alone.  A node
  that ended in a terminal keeps its return.  The [n C, 1099] observation buffer is allocated in bind (C = the last level's children
  per environment), which also calls the critic once at that row count, as a graph capture needs.
  action_values: True also computes the best key among the last level's nodes under each first action (action_values())."""

  def __init__(self, beam_width: int = 27, depth: int = 6, segment: int = 4, action_repeat: int = 1, gamma: float = 0.993,
               wind: str = 'belief', leaf_value=None, action_values: bool = False, device='cuda:0', substeps: int = vec_state.SUBSTEPS):
    if wind == 'scenarios':
      raise ValueError("VecBeamSearchAgent: wind='scenarios' is VecScenarioBeamSearchAgent's tree (M end states per node); here plan in "
                       "the belief, the forecast or the truth")
    if wind not in WINDS:
      raise ValueError(f"VecBeamSearchAgent: wind is 'belief', 'forecast' or 'truth', not {wind!r}")
    if not 1 <= int(beam_width) <= _abi.TREE_MAX_BEAM:
      raise ValueError(f'VecBeamSearchAgent: 1 <= beam_width <= {_abi.TREE_MAX_BEAM}, not {beam_width}')
    if int(depth) < 1 or int(segment) < 1 or int(action_repeat) < 1 or int(depth) * int(segment) * int(action_repeat) > _abi.ROLLOUT_MAX_STEPS:
      raise ValueError(f'VecBeamSearchAgent: depth, segment, action_repeat >= 1 and depth * segment * action_repeat <= '
                       f'{_abi.ROLLOUT_MAX_STEPS}, not {depth} x {segment} x {action_repeat}')
    if not 0.0 <= float(gamma) <= 1.0:
      raise ValueError(f'VecBeamSearchAgent: gamma in [0, 1], not {gamma}')
    self.leaf_value, self._leaf_fn = leaf_value, None
    if leaf_value is not None:
      if hasattr(leaf_value, 'act_greedy'):
        self._leaf_fn = leaf_value.act_greedy
      elif getattr(leaf_value, 'deterministic', True) is False:
        raise ValueError('VecBeamSearchAgent: leaf_value is a sampling agent (deterministic=False): its step counter would move with every '
                         'decision; give a deterministic one, or a trainer (act_greedy)')
      elif hasattr(leaf_value, 'act'):
        self._leaf_fn = leaf_value.act
      else:
        raise ValueError('VecBeamSearchAgent: leaf_value needs act_greedy(obs, value=) or act(obs, value=)')
    self.device = dev.require_gpu(device)
    self.lib = _lib.lib()
    self.beam_width, self.depth, self.segment, self.action_repeat = int(beam_width), int(depth), int(segment), int(action_repeat)
    self.gamma, self.wind, self.substeps, self.with_action_values = float(gamma), wind, int(substeps), bool(action_values)
    self.horizon = self.depth * self.segment
    self.sim: Optional[vec_state.VecSimulator] = None
    self._noise_seed: Union[None, int, Callable[[], int]] = None

  # ------------------------------------------------------------------ attach a simulator
  @dev.on_own_device
  def bind(self, sim: vec_state.VecSimulator, seeds: Optional[torch.Tensor] = None, noise_seed=None) -> 'VecBeamSearchAgent':
    """Attaches the simulator whose environments this agent flies.  All buffers are allocated here, once: binding the same simulator
    again changes nothing, so a captured graph stays valid.  seeds: accepted for VecLookaheadAgent's signature; the search draws
    nothing, so an environment plans the same in any batch with or without them -- except with wind='truth', which is refused with a
    seed per environment (the look-ahead's noise generator takes one seed).  noise_seed: the seed of the environments' wind noise, or a
    callable returning it, for wind='truth' (None there: the truth is the forecast)."""
    if sim.has_fleet:
      raise ValueError('VecBeamSearchAgent: a fleet (set_fleet) has no look-ahead kernel; fly one vehicle per batch (set_vehicle)')
    if sim.device != self.device:
      raise ValueError(f'VecBeamSearchAgent on {self.device} cannot plan for a simulator on {sim.device}')
    if seeds is not None and self.wind == 'truth':
      raise ValueError("VecBeamSearchAgent: wind='truth' with per-environment seeds: the look-ahead's noise generator takes one seed")
    same = self.sim is sim
    self.sim, self._noise_seed = sim, noise_seed
    if not same:
      n = sim.n
      self.buffers = sim.tree_buffers(self.depth, self.beam_width, self.segment, self.with_action_values)
      self.action, self.best_plan, self.best_return = self.buffers.action, self.buffers.best_plan, self.buffers.best_return
      self.q, self.visits = self.buffers.q, self.buffers.visits
      self._belief = None
      if self.wind == 'belief':
        self._belief = vec_state.WindBelief(torch.zeros(n, _lib.GP_BELIEF_DOUBLES, dtype=torch.float64, device=self.device),
                                            torch.zeros(n, dtype=torch.int32, device=self.device))
      if self._leaf_fn is not None:
        leaves = self.buffers.arenas[self.depth & 1]
        self.leaf_obs = torch.zeros(leaves.n, _lib.OBS_DIM, dtype=torch.float32, device=self.device)
        self.leaf_values = torch.zeros(leaves.n, dtype=torch.float32, device=self.device)
        self.leaf_actions = torch.zeros(leaves.n, dtype=torch.uint8, device=self.device)
        self.score = torch.zeros(n, leaves.leaves_per_env, dtype=torch.float32, device=self.device)
        self._leaf_fn(self.leaf_obs, out=self.leaf_actions, value=self.leaf_values)      # the first call at this row count: not in a capture
    return self

  def _bound(self) -> vec_state.VecSimulator:
    if self.sim is None:
      raise ValueError("VecBeamSearchAgent.act before bind(sim): the agent plans in a simulator (VecBalloonEnv.planner(search='beam') binds one)")
    return self.sim

  def _leaf_score(self, leaves, returns, steps_flown):
    """score = return + gamma^steps_flown * V(node) over the last level: VecLookaheadAgent's three calls, into a buffer of its own (the
    returns stay what the flights earned)."""
    sim = self.sim
    sim.observe_leaves(leaves, out=self.leaf_obs)
    self._leaf_fn(self.leaf_obs, out=self.leaf_actions, value=self.leaf_values)
    bs = _abi.BlePlanBootstrap(sim.n, leaves.leaves_per_env, 0, self.gamma, returns.data_ptr(), steps_flown.data_ptr(),
                               leaves.state['status'].data_ptr(), self.leaf_values.data_ptr(), self.score.data_ptr())
    _lib.check(self.lib.ble_plan_bootstrap_f32(ctypes.byref(bs), dev.stream_ptr(self.device)), 'ble_plan_bootstrap_f32')
    return self.score

  # ------------------------------------------------------------------ one decision
  @dev.on_own_device
  def act(self, obs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
          prior_probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decision for every environment of the bound simulator, from the state where it lies: uint8 [N] actions (device).  obs and
    prior_probs are accepted and unused (the search starts at the state itself and takes no prior).  out: optional uint8 [N] for the
    actions.  Nothing of the simulator is written; flags of the imagined flights go to sim.rollout_flags.  Asynchronous, capturable in
    a HIP graph."""
    del obs, prior_probs
    sim = self._bound()
    if sim.has_fleet:
      raise ValueError('VecBeamSearchAgent: the bound simulator flies a fleet now; a fleet has no look-ahead kernel')
    belief, noise_seed = None, None
    if self.wind == 'belief':
      belief = sim.fit_wind_belief(out=self._belief)
    elif self.wind == 'truth':
      noise_seed = self._noise_seed() if callable(self._noise_seed) else self._noise_seed
    self.result = sim.tree_search(self.depth, self.beam_width, self.segment, self.action_repeat, self.gamma, noise_seed=noise_seed,
                                  belief=belief, substeps=self.substeps, action_values=self.with_action_values,
                                  leaf_score=self._leaf_score if self._leaf_fn is not None else None, buffers=self.buffers)
    if out is None:
      return self.action
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == sim.n and out.device == self.device
    out.view(-1).copy_(self.action)
    return out

  __call__ = act

  def plan(self) -> Tuple[torch.Tensor, torch.Tensor]:
    """(best_plan uint8 [depth * segment, N], best_return float32 [N]) of the last decision: the agent's own buffers, overwritten by the
    next one.  With a leaf_value best_return is the bootstrapped score of the best node."""
    self._bound()
    return self.best_plan, self.best_return

  def action_values(self) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q float32 [N, 3], visits int32 [N, 3]) of the last decision, for an agent built with action_values=True: q[e, a] the best
    return (or score) among the last level's nodes whose first action is a, -Inf when none of them is finite; visits[e, a] how many
    non-void nodes of the last level begin with a.  q[e, action[e]] is best_return[e] wherever that is finite."""
    self._bound()
    if not self.with_action_values:
      raise ValueError('VecBeamSearchAgent.action_values: build the agent with action_values=True')
    return self.q, self.visits

  def state_dict(self) -> dict:
    """Nothing is carried from one decision to the next: every search starts at the state itself."""
    self._bound()
    return {}

  def load_state_dict(self, d: dict) -> None:
    self._bound()

  def check_errors(self) -> None:
    """The agent latches no error of its own: the flags of the flights it imagines stay in sim.rollout_flags."""

  def get_name(self) -> str:
    return 'BeamSearchAgent'


class VecScenarioBeamSearchAgent(VecBeamSearchAgent):
  """VecBeamSearchAgent in SAMPLED winds: every edge of the tree is flown in each of num_scenarios (<= 16) winds drawn
  from the WindGP's posterior, fitted at every decision (`fit_wind_scenarios`; the scenarios themselves are fixed over an
  episode, only the conditioning moves), and every level is ordered by the risk score of its groups: the mean of the risk_tail smallest
  scenario returns -- None = all of them, the expectation; 1 = the worst case; between them a CVaR.  The scenario streams are keyed as
  VecLookaheadAgent keys them: by `seed`, or with bind(seeds=) by each environment's own seed -- an environment then plans the same in
  any batch.  beam_width, depth, segment, action_repeat, gamma, action_values: the parent's; n * 3 * beam_width * num_scenarios < 2^31.
  No leaf_value: it would need C * M observations per environment and decision."""

  def __init__(self, beam_width: int = 27, depth: int = 6, segment: int = 4, action_repeat: int = 1, gamma: float = 0.993,
               num_scenarios: int = 8, risk_tail: Optional[int] = None, seed: int = 0, leaf_value=None, action_values: bool = False,
               device='cuda:0', substeps: int = vec_state.SUBSTEPS):
    if leaf_value is not None:
      raise ValueError('VecScenarioBeamSearchAgent: leaf_value has no scenario tree (C * M observations per environment and decision); '
                       'plan in the belief (VecBeamSearchAgent)')
    self.num_scenarios = int(num_scenarios)
    self.risk_tail = self.num_scenarios if risk_tail is None else int(risk_tail)
    if not (1 <= self.num_scenarios <= _abi.SCENARIO_MAX and 1 <= self.risk_tail <= self.num_scenarios):
      raise ValueError(f'VecScenarioBeamSearchAgent: 1 <= num_scenarios <= {_abi.SCENARIO_MAX} and 1 <= risk_tail <= num_scenarios, '
                       f'not {num_scenarios}, {risk_tail}')
    # (the parent checks the shape of the tree and opens the device; of its winds it keeps refusing 'scenarios', so it is given another)
    super().__init__(beam_width, depth, segment, action_repeat, gamma, 'forecast', None, action_values, device, substeps)
    self.wind, self.seed = 'scenarios', int(seed)
    self._seeds: Optional[torch.Tensor] = None

  @dev.on_own_device
  def bind(self, sim: vec_state.VecSimulator, seeds: Optional[torch.Tensor] = None, noise_seed=None) -> 'VecScenarioBeamSearchAgent':
    """Attaches the simulator.  All buffers are allocated here, once: binding the same simulator (and the same `seeds` tensor) again
    changes nothing.  seeds: int64 / uint64 device tensor [N], a seed per environment (read at every decision).  noise_seed: accepted
    for the planners' common signature and unused -- no scenario is the truth."""
    del noise_seed
    if sim.has_fleet:
      raise ValueError('VecScenarioBeamSearchAgent: a fleet (set_fleet) has no look-ahead kernel; fly one vehicle per batch (set_vehicle)')
    if sim.device != self.device:
      raise ValueError(f'VecScenarioBeamSearchAgent on {self.device} cannot plan for a simulator on {sim.device}')
    if seeds is not None:
      assert seeds.dtype in (torch.int64, torch.uint64) and seeds.is_contiguous() and tuple(seeds.shape) == (sim.n,), seeds.shape
      assert seeds.device == self.device
    same = self.sim is sim and self._seeds is seeds
    self.sim, self._seeds = sim, seeds
    if not same:
      n, m = sim.n, self.num_scenarios
      self.buffers = sim.tree_buffers(self.depth, self.beam_width, self.segment, self.with_action_values, m)
      self.action, self.best_plan, self.best_return = self.buffers.action, self.buffers.best_plan, self.buffers.best_return
      self.q, self.visits = self.buffers.q, self.buffers.visits
      self._scenarios = vec_state.WindScenarios(torch.zeros(n, _abi.gp_scenario_doubles(m), dtype=torch.float64, device=self.device),
                                                torch.zeros(n, dtype=torch.int32, device=self.device), m, self.seed, seeds)
    return self

  @dev.on_own_device
  def act(self, obs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
          prior_probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decision for every environment of the bound simulator: the scenarios fitted now, the tree searched in them.  The parent's
    contract: uint8 [N] device actions, nothing of the simulator written, asynchronous, capturable in a HIP graph."""
    del obs, prior_probs
    sim = self._bound()
    if sim.has_fleet:
      raise ValueError('VecScenarioBeamSearchAgent: the bound simulator flies a fleet now; a fleet has no look-ahead kernel')
    scenarios = sim.fit_wind_scenarios(self.num_scenarios, seed=self.seed, seeds=self._seeds, out=self._scenarios)
    self.result = sim.tree_search(self.depth, self.beam_width, self.segment, self.action_repeat, self.gamma, substeps=self.substeps,
                                  action_values=self.with_action_values, buffers=self.buffers, scenarios=scenarios,
                                  risk_tail=self.risk_tail)
    if out is None:
      return self.action
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == sim.n and out.device == self.device
    out.view(-1).copy_(self.action)
    return out

  __call__ = act

  def state_dict(self) -> dict:
    """Nothing moves from one decision to the next -- the scenarios are refitted from the simulator's own history and their streams are
    keyed by the environments' episode counters -- so a resume needs what keys the streams and shapes the score, to hold the resumed
    agent to them."""
    self._bound()
    return {'seed': self.seed, 'num_scenarios': self.num_scenarios, 'risk_tail': self.risk_tail}

  def load_state_dict(self, d: dict) -> None:
    self._bound()
    mine = self.state_dict()
    if any(k in d and int(d[k]) != mine[k] for k in mine):
      raise ValueError(f'VecScenarioBeamSearchAgent: a checkpoint of another agent ({ {k: d[k] for k in mine if k in d} }, this one {mine})')

  def get_name(self) -> str:
    return 'ScenarioBeamSearchAgent'
