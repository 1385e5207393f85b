"""A model-predictive agent that grows its tree where a prior and a value point (no counterpart in the reference).

Where VecBeamSearchAgent spends 3 * beam_width edges on every level whatever it has learnt, this agent keeps a pool of nodes per
environment and, round by round, descends from the root by PUCT -- the mean value of a subtree plus an exploration term weighted by the
guide's prior -- to leaves_per_round leaves, flies their three children for one segment each, asks the guide ONCE about every new node
(its value and its prior), and backs the value up along the path (`VecSimulator.mcts_search`: `ble_mcts_select_f32`,
`ble_mcts_expand_f32`, `ble_mcts_backup_f32`, `ble_mcts_finish_f32`).  The answer is the root's visit counts.  Deterministic: there is
no random stream and no seed.  No host synchronisation anywhere, so a decision is capturable in the same HIP graph as the step.
Without a guide the search needs no trained weights (V = 0, uniform priors: the returns alone steer it); with guide=trainer an expert
iteration's learner steers its own expert.  `bind` attaches the simulator (`VecBalloonEnv.planner(search='mcts', num_rounds=, leaves_per_round=, max_depth=)` returns a bound
agent).  VecScenarioMCTSAgent is the same search in sampled winds: a node is a group of M scenario nodes.
"""
from typing import Optional, Tuple

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd import vec_state
from balloon_learning_environment_amd.agents import planner

WINDS = ('belief', 'forecast', 'truth')


class VecMCTSAgent(planner.VecPlanner):
  """Guided tree search for N environments at once: act(obs) -> uint8 [N] device actions.

  num_rounds R rounds of leaves_per_round L descents (L * R <= 256): at most 3 L R edges flown per environment and decision, each one
  action for `segment` plan entries x action_repeat agent steps, to at most max_depth edges from the root (max_depth * segment *
  action_repeat <= 960).  The three have no default: the budget of a search is the caller's decision (3 L R edges and, with a
  guide, 3 L R observations and forward rows per environment and decision).  gamma: the discount of a return.  c_puct >= 0: the
  weight of the exploration term (0: by value alone).
  wind: 'belief' (default) -- forecast + the mean of the WindGP over the balloon's own measurements, fitted at every decision;
  'forecast'; 'truth' -- the wind the environments will fly (bind(noise_seed=)).  'scenarios' is refused: a node is one state (VecScenarioMCTSAgent's is a group).
  guide: an actor-critic -- an object with act_greedy(obs, out=, value=, probs=) or else act(obs, out=, value=, probs=), a sampling agent
  refused (VecBeamSearchAgent's rule) -- whose value of every new node enters its G = return + gamma^steps * V(node) (a node that ended
  in a terminal keeps its return) and whose probabilities are the node's prior over its children; on act's own observation they are the
  root's prior unless act is given prior_probs.  None: no observation and no forward at all.
  plan() is the principal variation -- the most visited child followed down, padded with STAY -- and the mean value of its first node."""

  WINDS, PLANNER = WINDS, "planner(search='mcts')"
  num_scenarios, risk_tail = 0, None      # (VecScenarioMCTSAgent's)

  def __init__(self, num_rounds: int, leaves_per_round: int, max_depth: int, segment: int = 4, action_repeat: int = 1,
               gamma: float = 0.993, c_puct: float = 1.25, wind: str = 'belief', guide=None, device='cuda:0',
               substeps: int = vec_state.SUBSTEPS):
    if int(num_rounds) < 1 or int(leaves_per_round) < 1 or int(num_rounds) * int(leaves_per_round) > _abi.MCTS_MAX_LEAVES:
      raise ValueError(f'VecMCTSAgent: num_rounds >= 1, leaves_per_round >= 1 and their product <= {_abi.MCTS_MAX_LEAVES}, '
                       f'not {num_rounds} x {leaves_per_round}')
    if int(max_depth) < 1 or int(max_depth) * int(segment) * int(action_repeat) > _abi.ROLLOUT_MAX_STEPS:
      raise ValueError(f'VecMCTSAgent: max_depth >= 1 and max_depth * segment * action_repeat <= {_abi.ROLLOUT_MAX_STEPS}, '
                       f'not {max_depth} x {segment} x {action_repeat}')
    if not 0.0 <= float(c_puct) < float('inf'):
      raise ValueError(f'VecMCTSAgent: c_puct finite and >= 0, not {c_puct}')
    self.guide, self._guide_fn = guide, self._critic('guide', guide, '(obs, out=, value=, probs=)')
    super().__init__(wind, gamma, action_repeat, segment, device, substeps)
    self.num_rounds, self.leaves_per_round, self.max_depth, self.c_puct = int(num_rounds), int(leaves_per_round), int(max_depth), float(c_puct)
    self.horizon = self.max_depth * self.segment

  def _allocate(self, sim: vec_state.VecSimulator) -> None:
    """With a guide it is called once at each of its two row counts (n 3L, in scenario winds n 3L M: a round's nodes; n: the root), as a
    graph capture needs."""
    n = sim.n
    self.buffers = sim.mcts_buffers(self.num_rounds, self.leaves_per_round, self.max_depth, self.segment, self._guide_fn is not None,
                                    self.num_scenarios)
    bf = self.buffers
    self.action, self.best_plan, self.best_return, self.q, self.visits = bf.action, bf.best_plan, bf.best_return, bf.q, bf.root_visits
    self._allocate_wind()
    self._root_probs = self._root_action = self._root_obs = None
    if self._guide_fn is not None:
      self._root_probs = torch.zeros(n, 3, dtype=torch.float32, device=self.device)
      self._root_action = torch.zeros(n, dtype=torch.uint8, device=self.device)
      self._guide_fn(bf.obs, out=bf.guide_action, value=bf.value, probs=bf.probs)      # the first calls at these row counts: not in a capture
      self._guide_fn(torch.zeros(n, _lib.OBS_DIM, dtype=torch.float32, device=self.device), out=self._root_action, probs=self._root_probs)

  # ------------------------------------------------------------------ one decision
  @dev.on_own_device
  def act(self, obs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
          prior_probs: Optional[torch.Tensor] = None, trace: Optional[list] = None) -> torch.Tensor:
    """One decision for every environment of the bound simulator, from the state where it lies: uint8 [N] actions (device).  The root's
    prior: prior_probs (float32 [N, 3]) if given; else the guide's probabilities on obs; else uniform.  out: optional uint8 [N] for the
    actions.  trace: mcts_search's (tests).  Nothing of the simulator is written; flags of the imagined flights go to sim.rollout_flags.
    Asynchronous, capturable in a HIP graph."""
    sim = self._flying()
    wind = self._wind()
    root_prior = prior_probs
    if root_prior is None and self._guide_fn is not None and obs is not None:
      self._guide_fn(obs, out=self._root_action, probs=self._root_probs)
      root_prior = self._root_probs
    self.result = sim.mcts_search(self.num_rounds, self.leaves_per_round, self.max_depth, self.segment, self.action_repeat, self.gamma,
                                  self.c_puct, substeps=self.substeps, guide_fn=self._guide_fn, root_prior=root_prior,
                                  buffers=self.buffers, trace=trace, risk_tail=self.risk_tail, **wind)
    return self._emit(out)

  def action_values(self) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q float32 [N, 3], visits int32 [N, 3]) of the last decision: the mean value of the root's child under each action (-Inf: a void
    child, or a source that is not OK) and its visit count.  q[e, action[e]] is best_return[e] wherever the root has a visited child."""
    self._bound()
    return self.q, self.visits

  def visit_probs(self) -> torch.Tensor:
    """float32 [N, 3]: the root's visit counts as a distribution (all zero where no child was visited) -- the search's policy target."""
    self._bound()
    visits = self.visits.to(torch.float32)
    return visits / visits.sum(1, keepdim=True).clamp_min(1.0)


class VecScenarioMCTSAgent(VecMCTSAgent):
  """VecMCTSAgent in SAMPLED winds: a node of the pool is a GROUP of num_scenarios (<= 16) scenario nodes, every edge is
  flown in each of that many winds drawn from the WindGP's posterior, fitted at every decision (`fit_wind_scenarios`; the
  scenarios themselves are fixed over an episode, only the conditioning moves), and a group backs up ONE value: the mean of the
  risk_tail smallest of its M values G_m = return_m + gamma^steps_m * V(node m) -- None = all of them, the expectation; 1 = the worst
  case; between them a CVaR.  A scenario node that stopped is carried on unchanged under every action; a group whose nodes all stopped is
  never expanded again.  With a guide every one of the M nodes of a group is observed and evaluated; the group's prior is the mean of
  the probability rows of its nodes that are OK.  The scenario streams are keyed as VecScenarioBeamSearchAgent keys them: by `seed`, or
  with bind(seeds=) by each environment's own seed -- an environment then plans the same in any batch.
  num_rounds, leaves_per_round, max_depth and num_scenarios have no default: the budget of a search is the caller's decision.
  Memory: the pool is 3 * leaves_per_round * num_rounds * num_scenarios nodes per environment (about 150 B each); with a guide, 3 *
  leaves_per_round * num_scenarios observation rows of 4.4 KB per environment on top.  n * 3 * leaves_per_round * num_scenarios < 2^31.
  act, plan, action_values and visit_probs: the parent's; q and best_return are means of group values, that is, risk scores.
  bind(noise_seed=) is accepted for the planners' common signature and unused -- no scenario is the truth."""

  WINDS, SEEDED = ('scenarios',), True

  def __init__(self, num_rounds: int, leaves_per_round: int, max_depth: int, num_scenarios: int, risk_tail: Optional[int] = None,
               seed: int = 0, segment: int = 4, action_repeat: int = 1, gamma: float = 0.993, c_puct: float = 1.25, guide=None,
               device='cuda:0', substeps: int = vec_state.SUBSTEPS):
    self.num_scenarios = int(num_scenarios)
    self.risk_tail = self.num_scenarios if risk_tail is None else int(risk_tail)
    if not (1 <= self.num_scenarios <= _abi.SCENARIO_MAX and 1 <= self.risk_tail <= self.num_scenarios):
      raise ValueError(f'VecScenarioMCTSAgent: 1 <= num_scenarios <= {_abi.SCENARIO_MAX} and 1 <= risk_tail <= num_scenarios, '
                       f'not {num_scenarios}, {risk_tail}')
    super().__init__(num_rounds, leaves_per_round, max_depth, segment, action_repeat, gamma, c_puct, 'scenarios', guide, device, substeps)
    self.seed = int(seed)

  def state_dict(self) -> dict:
    """Nothing moves from one decision to the next; a resume needs what keys the scenario streams and shapes the score."""
    self._bound()
    return {'seed': self.seed, 'num_scenarios': self.num_scenarios, 'risk_tail': self.risk_tail}

  def load_state_dict(self, d: dict) -> None:
    self._bound()
    mine = self.state_dict()
    if any(k in d and int(d[k]) != mine[k] for k in mine):
      raise ValueError(f'VecScenarioMCTSAgent: a checkpoint of another agent ({ {k: d[k] for k in mine if k in d} }, this one {mine})')
