"""A model-predictive agent that plans entirely on the device (no counterpart in the reference).

Per decision: sample K piecewise-constant action plans per environment (`ble_plan_sample_u8`), fly them from the state where each
balloon lies with the look-ahead kernels (`VecSimulator.rollout_plans`: `ble_rollout_f32` / `ble_rollout_belief_f32` /
`ble_rollout_scenarios_f32`, the last followed by `ble_plan_risk_f32`), pick the best (`ble_plan_select_f32`) -- optionally refined by cross-entropy iterations: the next iteration samples around the elite plans of
this one -- and emit the plan's first action.  No host synchronisation anywhere, so a decision is capturable in the same HIP graph
as the step.  The agent needs no trained weights; it needs the simulator, which `bind` attaches (eval_lib.VecEvaluator does that for
any agent with a `bind`; `VecBalloonEnv.planner()` returns a bound agent).
"""
import ctypes
from typing import Optional

import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd import vec_state
from balloon_learning_environment_amd.agents import planner

WINDS = ('belief', 'forecast', 'truth', 'scenarios')
STAY = 1


class VecLookaheadAgent(planner.VecPlanner):
  """Look-ahead planning for N environments at once: act(obs) -> uint8 [N] device actions.

  num_plans K (<= 1024) plans per environment of `horizon` H entries, every entry flown action_repeat agent steps
  (H * action_repeat <= 960); a plan is constant over `segment` entries.  gamma: the discount of a plan's return.
  wind: 'belief' (default) -- forecast + the mean of the WindGP over the balloon's own measurements, fitted at every decision: all an
  agent may legitimately know; 'forecast' -- the forecast alone; 'truth' -- the wind the environments will fly (bind(noise_seed=)):
  a simulator-side upper bound; 'scenarios' -- forecast + each of num_scenarios (<= 16) winds sampled from the WindGP's posterior (a draw
  of the noise field conditioned on the measurements), fitted at every decision; the scenarios themselves are fixed over an
  episode (common random numbers: only the conditioning moves).  A plan's score is then the mean of its risk_tail smallest scenario
  returns: None = all of them, the expectation; 1 = the worst case; between them a CVaR.  The scenario streams are keyed by `seed`, or
  with bind(seeds=) by each environment's own seed.  iterations (<= 16): 1 picks the best of K; more refine by cross-entropy, each iteration drawing
  every segment's action with probability (c_a + 1) / (E + 3) from the counts c_a of the E = min(elite, K) best plans of the one
  before, the best plan so far always kept.  Iteration 0 always holds all-STAY, all-DOWN, all-UP and the previous decision's best
  plan shifted by one entry (as far as K reaches).  seed: the plans' Philox streams are keyed by (seed, environment, decision
  counter, iteration, k), or with bind(seeds=) by (that environment's seed, decision counter, iteration, k): then an environment
  plans the same in any batch.
  prior_strength (0 .. 65 535): with a value above 0 and act(prior_probs=) given, iteration 0 draws its free plans around a
  policy prior instead of from uniform thirds: segment s draws action a with probability (c_a + 1) / (c_0 + c_1 + c_2 + 3),
  c_a = trunc(p_a * (prior_strength >> s)) -- the prior's weight halves per segment.  0, or no prior_probs: today's calls.
  action_values: True computes, after every selection of a decision, the best return among the plans that begin with each action
  (action_values()); False (the default) adds no launch.
  leaf_value: a critic -- an object with act_greedy(obs, value=) (PPOTrainer, BCTrainer, SoftBCTrainer: their live weights)
  or else act(obs, value=) (a deterministic VecActorCriticAgent) -- whose value of every plan's END state is added to the plan's return:
  score = return + gamma^steps_flown * V(leaf), so a plan of H steps is judged by what follows it as well.  Every iteration of a
  decision then runs sample -> rollout_plans(leaves=) -> observe_leaves -> the critic over the n K leaf observations ->
  ble_plan_bootstrap_f32 into `returns` -> select (and the action values, if on): best_return, q and the elite counts are all taken
  from the bootstrapped scores.  A plan that ends in a terminal keeps its return (no value after the end).  The leaf arena, the
  [n K, 1099] observation buffer and the values are allocated in bind: 4.4 KB per leaf for the observations (288 MB at n = 4 096,
  K = 16) plus about 230 B per leaf of state; bind also calls the critic once at that row count, as a graph capture needs
  (ActorForward's contract).  A sampling VecActorCriticAgent (deterministic=False) is refused -- its step counter would move with
  every decision -- and so is wind='scenarios' (M end states per plan).  The same network may serve as the prior of a
  VecPriorPlannerAgent and as leaf_value.  None (the default): today's calls and today's bits."""

  WINDS, SEEDED = WINDS, True

  def __init__(self, num_plans: int = 64, horizon: int = 24, action_repeat: int = 1, segment: int = 4, gamma: float = 0.993,
               wind: str = 'belief', iterations: int = 1, elite: int = 8, seed: int = 0, device='cuda:0',
               substeps: int = vec_state.SUBSTEPS, num_scenarios: int = 8, risk_tail: Optional[int] = None, prior_strength: int = 0,
               action_values: bool = False, leaf_value=None):
    self.num_scenarios = int(num_scenarios) if wind == 'scenarios' else 0
    self.risk_tail = self.num_scenarios if risk_tail is None else int(risk_tail)
    if wind == 'scenarios' and not (1 <= self.num_scenarios <= _abi.SCENARIO_MAX and 1 <= self.risk_tail <= self.num_scenarios):
      raise ValueError(f'VecLookaheadAgent: 1 <= num_scenarios <= {_abi.SCENARIO_MAX} and 1 <= risk_tail <= num_scenarios, '
                       f'not {num_scenarios}, {risk_tail}')
    if not 1 <= int(num_plans) <= _abi.PLAN_MAX_PLANS:
      raise ValueError(f'VecLookaheadAgent: 1 <= num_plans <= {_abi.PLAN_MAX_PLANS}, not {num_plans}')
    if int(horizon) < 1 or int(horizon) * int(action_repeat) > _abi.ROLLOUT_MAX_STEPS:
      raise ValueError(f'VecLookaheadAgent: horizon >= 1 and horizon * action_repeat <= {_abi.ROLLOUT_MAX_STEPS}, '
                       f'not {horizon} x {action_repeat}')
    if not 1 <= int(iterations) <= _abi.PLAN_MAX_ITERATIONS or int(elite) < 1:
      raise ValueError(f'VecLookaheadAgent: 1 <= iterations <= {_abi.PLAN_MAX_ITERATIONS} and elite >= 1, not {iterations}, {elite}')
    if not 0 <= int(prior_strength) <= 65535:
      raise ValueError(f'VecLookaheadAgent: 0 <= prior_strength <= 65535, not {prior_strength}')
    if leaf_value is not None and wind == 'scenarios':
      raise ValueError("VecLookaheadAgent: leaf_value with wind='scenarios': a plan has M end states there; plan in the belief or the forecast")
    self.prior_strength, self.with_action_values = int(prior_strength), bool(action_values)
    self.leaf_value, self._leaf_fn = leaf_value, self._critic('leaf_value', leaf_value, '(obs, value=)')
    super().__init__(wind, gamma, action_repeat, segment, device, substeps)
    self.num_plans, self.horizon, self.iterations, self.seed = int(num_plans), int(horizon), int(iterations), int(seed)
    self.elite = min(int(elite), self.num_plans)
    self.segments = -(-self.horizon // self.segment)

  # ------------------------------------------------------------------ attach a simulator
  def bind(self, sim: vec_state.VecSimulator, seeds: Optional[torch.Tensor] = None, noise_seed=None) -> 'VecLookaheadAgent':
    """VecPlanner.bind, and a new run of decisions (counter 0, previous best plan all STAY): binding the same simulator and the same
    `seeds` tensor again only restarts the run.  With seeds, the plans of an environment do not depend on its batch."""
    if sim.n * self.num_plans * max(self.num_scenarios, 1) >= 2 ** 31:
      raise ValueError(f'VecLookaheadAgent: n * num_plans * num_scenarios < 2^31, not {sim.n} x {self.num_plans} x {max(self.num_scenarios, 1)}')
    super().bind(sim, seeds, noise_seed)
    self.counter.zero_()
    self.best_plan.fill_(STAY)
    self.best_return.zero_()
    self.best_k.fill_(-1)
    return self

  def _allocate(self, sim: vec_state.VecSimulator) -> None:
    n, k, h = sim.n, self.num_plans, self.horizon
    z = lambda dtype, *shape: torch.zeros(*shape, dtype=dtype, device=self.device)
    self.counter = z(torch.int64, 1)                       # the decision counter: device memory, advanced by the last selection
    self.plans = z(torch.uint8, h, n, k)
    self.returns, self.steps_flown = z(torch.float32, n, k), z(torch.int32, n, k)
    self.best_return, self.best_k = z(torch.float32, n), z(torch.int32, n)
    self.best_plan = z(torch.uint8, h, n)
    self.elite_counts = z(torch.int16, n, self.segments, 3)
    self.action = z(torch.uint8, n)
    self.prior_counts = z(torch.int16, n, self.segments, 3) if self.prior_strength > 0 else None
    self.q, self.q_k, self.visits = ((z(torch.float32, n, 3), z(torch.int32, n, 3), z(torch.int32, n, 3)) if self.with_action_values
                                     else (None, None, None))
    self._allocate_wind()
    if self.wind == 'scenarios':
      m = self.num_scenarios
      self.scenario_returns, self.scenario_steps = z(torch.float32, n, k, m), z(torch.int32, n, k, m)
    self.leaves = None
    if self._leaf_fn is not None:
      self.leaves = sim.leaf_arena(k)
      self._allocate_leaf_rows(n * k)

  # ------------------------------------------------------------------ one decision
  @dev.on_own_device
  def act(self, obs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
          prior_probs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One decision for every environment of the bound simulator, from the state where it lies: uint8 [N] actions (device).  obs is
    accepted and unused (the plans are flown from the state itself).  out: optional uint8 [N] for the actions.  prior_probs: optional
    float32 [N, 3] device tensor, a policy's probabilities of the three actions (an actor-critic's probs, a softmax of Q-values): read
    by iteration 0 of an agent built with prior_strength > 0, ignored otherwise.  Nothing of the simulator is written; flags of the
    imagined flights go to sim.rollout_flags.  Asynchronous, capturable in a HIP graph."""
    del obs
    sim = self._flying()
    n = sim.n
    out = self.action if out is None else self._checked_out(out)
    stream = dev.stream_ptr(self.device)
    with_prior = self.prior_strength > 0 and prior_probs is not None
    if with_prior:
      assert prior_probs.dtype == torch.float32 and prior_probs.is_contiguous() and tuple(prior_probs.shape) == (n, 3), prior_probs.shape
      assert prior_probs.device == self.device
      pr = _abi.BlePlanPrior(n, self.segments, self.prior_strength, prior_probs.data_ptr(), self.prior_counts.data_ptr())
      _lib.check(self.lib.ble_plan_prior_u16(ctypes.byref(pr), stream), 'ble_plan_prior_u16')
    wind = self._wind()
    in_scenarios = self.wind == 'scenarios'
    rollout_out = (self.scenario_returns, self.scenario_steps, None, None) if in_scenarios else (self.returns, self.steps_flown, None, None)
    for it in range(self.iterations):
      last = it + 1 == self.iterations
      ps = _abi.BlePlanSample(n, self.num_plans, self.horizon, self.segment, it, self.seed & (2 ** 64 - 1), dev.ptr(self._seeds),
                              0 if self._seeds is not None else sim.env_offset, self.counter.data_ptr(), self.elite_counts.data_ptr(),
                              self.best_plan.data_ptr(), self.plans.data_ptr())
      if with_prior and it == 0:
        pp = _abi.BlePlanSamplePrior(*(getattr(ps, name) for name, _ in _abi.BlePlanSample._fields_), self.prior_counts.data_ptr())
        _lib.check(self.lib.ble_plan_sample_prior_u8(ctypes.byref(pp), stream), 'ble_plan_sample_prior_u8')
      else:
        _lib.check(self.lib.ble_plan_sample_u8(ctypes.byref(ps), stream), 'ble_plan_sample_u8')
      sim.rollout_plans(self.plans, self.gamma, self.action_repeat, substeps=self.substeps, out=rollout_out, leaves=self.leaves, **wind)
      if in_scenarios:      # every plan was flown in every scenario wind; one score per plan: the selection below runs on the scores
        sim.plan_risk(self.scenario_returns, self.risk_tail, out=self.returns)
      if self.leaves is not None:    # in place: everything below reads the scores
        self._leaf_score(self.leaves, self.returns, self.steps_flown, self.returns)
      # (the elite counts are the next iteration's: the last selection writes none, and moves the decision counter on)
      sel = _abi.BlePlanSelect(n, self.num_plans, self.horizon, self.segment, it, 0 if last else self.elite, 0, self.returns.data_ptr(),
                               self.plans.data_ptr(), self.best_return.data_ptr(), self.best_k.data_ptr(), self.best_plan.data_ptr(),
                               out.data_ptr(), self.elite_counts.data_ptr(), self.counter.data_ptr() if last else None)
      _lib.check(self.lib.ble_plan_select_f32(ctypes.byref(sel), stream), 'ble_plan_select_f32')
      if self.with_action_values:      # (plans[0] is [n][K]: the plans' first entries)
        av = _abi.BlePlanActionValues(n, self.num_plans, 1 if it > 0 else 0, self.returns.data_ptr(), self.plans.data_ptr(),
                                      self.q.data_ptr(), self.q_k.data_ptr(), self.visits.data_ptr())
        _lib.check(self.lib.ble_plan_action_values_f32(ctypes.byref(av), stream), 'ble_plan_action_values_f32')
    return out

  def state_dict(self) -> dict:
    """What a run of decisions carries from one to the next: the decision counter and the best plan (the warm start)."""
    self._bound()
    return {'counter': self.counter.clone(), 'best_plan': self.best_plan.clone()}

  def load_state_dict(self, d: dict) -> None:
    self._bound()
    self.counter.copy_(d['counter'])
    self.best_plan.copy_(d['best_plan'])
