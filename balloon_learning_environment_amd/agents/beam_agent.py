"""A model-predictive agent that SEARCHES its plans (no counterpart in the reference).

Where VecLookaheadAgent samples K plans and flies each of them from the root, this agent grows a shared-prefix tree of plans level by
level (`VecSimulator.tree_search`: `ble_tree_expand_f32`, `ble_tree_select_f32`, `ble_tree_finish_f32`): every level flies the three
children of the best `beam_width` nodes of the one before for one segment, so a prefix is flown once however many plans share it, and
the search is systematic and deterministic -- there is no random stream and no seed.  With 3^depth <= 3 * beam_width it is the
enumeration of all 3^depth plans.  No host synchronisation anywhere, so a decision is capturable in the same HIP graph as the step.
The agent needs no trained weights; it needs the simulator, which `bind` attaches (eval_lib.VecEvaluator does that for any agent with a
`bind`; `VecBalloonEnv.planner(search='beam')` returns a bound agent).
"""
from typing import Optional

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd import vec_state
from balloon_learning_environment_amd.agents import planner

WINDS = ('belief', 'forecast', 'truth')


class VecBeamSearchAgent(planner.VecPlanner):
  """Beam search over action plans for N environments at once: act(obs) -> uint8 [N] device actions.

  depth D levels of one action each, flown `segment` plan entries x action_repeat agent steps (D * segment * action_repeat <= 960); the
  best beam_width B (<= 256) nodes of a level are expanded into 3 B children.  gamma: the discount of a plan's return.
  wind: 'belief' (default) -- forecast + the mean of the WindGP over the balloon's own measurements, fitted at every decision;
  'forecast' -- the forecast alone; 'truth' -- the wind the environments will fly (bind(noise_seed=)): a simulator-side upper bound.
  Scenario winds are VecScenarioBeamSearchAgent's ('scenarios' is refused here).
  leaf_value: a critic -- an object with act_greedy(obs, value=) or else act(obs, value=), VecLookaheadAgent's rule --
  whose value of every node of the LAST level is added to its return before the final order: score = return + gamma^steps_flown *
  V(node) (`observe_leaves` -> the critic -> `ble_plan_bootstrap_f32`), into a buffer of its own (the returns stay what the flights
  earned); the inner levels are ordered by their returns alone.  A node that ended in a terminal keeps its return.  The [n C, 1099]
  observation buffer is allocated in bind (C = the last level's children per environment), which also calls the critic once at that
  row count, as a graph capture needs.
  action_values: True also computes the best key among the last level's nodes under each first action (action_values()).
  bind(seeds=) is accepted for VecLookaheadAgent's signature: the search draws nothing, so an environment plans the same in any batch
  with or without them."""

  WINDS, PLANNER = WINDS, "planner(search='beam')"
  num_scenarios, risk_tail = 0, None      # (VecScenarioBeamSearchAgent's)

  def __init__(self, beam_width: int = 27, depth: int = 6, segment: int = 4, action_repeat: int = 1, gamma: float = 0.993,
               wind: str = 'belief', leaf_value=None, action_values: bool = False, device='cuda:0', substeps: int = vec_state.SUBSTEPS):
    if not 1 <= int(beam_width) <= _abi.TREE_MAX_BEAM:
      raise ValueError(f'VecBeamSearchAgent: 1 <= beam_width <= {_abi.TREE_MAX_BEAM}, not {beam_width}')
    if int(depth) < 1 or int(depth) * int(segment) * int(action_repeat) > _abi.ROLLOUT_MAX_STEPS:
      raise ValueError(f'VecBeamSearchAgent: depth >= 1 and depth * segment * action_repeat <= {_abi.ROLLOUT_MAX_STEPS}, '
                       f'not {depth} x {segment} x {action_repeat}')
    self.leaf_value, self._leaf_fn = leaf_value, self._critic('leaf_value', leaf_value, '(obs, value=)')
    super().__init__(wind, gamma, action_repeat, segment, device, substeps)
    self.beam_width, self.depth, self.with_action_values = int(beam_width), int(depth), bool(action_values)
    self.horizon = self.depth * self.segment

  def _allocate(self, sim: vec_state.VecSimulator) -> None:
    self.buffers = sim.tree_buffers(self.depth, self.beam_width, self.segment, self.with_action_values, self.num_scenarios)
    self.action, self.best_plan, self.best_return = self.buffers.action, self.buffers.best_plan, self.buffers.best_return
    self.q, self.visits = self.buffers.q, self.buffers.visits
    self._allocate_wind()
    if self._leaf_fn is not None:
      leaves = self.buffers.arenas[self.depth & 1]
      self.score = torch.zeros(sim.n, leaves.leaves_per_env, dtype=torch.float32, device=self.device)
      self._allocate_leaf_rows(leaves.n)

  # ------------------------------------------------------------------ one decision
  @dev.on_own_device
  def act(self, obs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
          prior_probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decision for every environment of the bound simulator, from the state where it lies: uint8 [N] actions (device).  obs and
    prior_probs are accepted and unused (the search starts at the state itself and takes no prior).  out: optional uint8 [N] for the
    actions.  Nothing of the simulator is written; flags of the imagined flights go to sim.rollout_flags.  Asynchronous, capturable in
    a HIP graph."""
    del obs, prior_probs
    sim = self._flying()
    leaf_score = None
    if self._leaf_fn is not None:
      leaf_score = lambda leaves, returns, steps_flown: self._leaf_score(leaves, returns, steps_flown, self.score)
    self.result = sim.tree_search(self.depth, self.beam_width, self.segment, self.action_repeat, self.gamma, substeps=self.substeps,
                                  action_values=self.with_action_values, leaf_score=leaf_score, buffers=self.buffers,
                                  risk_tail=self.risk_tail, **self._wind())
    return self._emit(out)


class VecScenarioBeamSearchAgent(VecBeamSearchAgent):
  """VecBeamSearchAgent in SAMPLED winds: every edge of the tree is flown in each of num_scenarios (<= 16) winds drawn
  from the WindGP's posterior, fitted at every decision (`fit_wind_scenarios`; the scenarios themselves are fixed over an
  episode, only the conditioning moves), and every level is ordered by the risk score of its groups: the mean of the risk_tail smallest
  scenario returns -- None = all of them, the expectation; 1 = the worst case; between them a CVaR.  The scenario streams are keyed as
  VecLookaheadAgent keys them: by `seed`, or with bind(seeds=) by each environment's own seed -- an environment then plans the same in
  any batch.  beam_width, depth, segment, action_repeat, gamma, action_values: the parent's; n * 3 * beam_width * num_scenarios < 2^31.
  No leaf_value: it would need C * M observations per environment and decision.  bind(noise_seed=) is accepted for the planners' common
  signature and unused -- no scenario is the truth."""

  WINDS, SEEDED = ('scenarios',), True

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
    super().__init__(beam_width, depth, segment, action_repeat, gamma, 'scenarios', None, action_values, device, substeps)
    self.seed = int(seed)

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
