"""BalloonEnv (env/balloon_env.py:106-300): the gym-style RL surface over the HIP arena."""
import datetime as dt
import math
import time
from typing import Any, Callable, Dict, Mapping, Optional, Tuple, Union

import numpy as np
import torch

from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.env import balloon_arena
from balloon_learning_environment_amd.env import features
from balloon_learning_environment_amd.env import grid_based_wind_field
from balloon_learning_environment_amd.env import grid_wind_field_sampler
from balloon_learning_environment_amd.env import simulator_data
from balloon_learning_environment_amd.env.balloon import balloon
from balloon_learning_environment_amd.env.balloon import control
from balloon_learning_environment_amd.utils import units


def perciatelli_reward_function(simulator_state: simulator_data.SimulatorState, *, station_keeping_radius_km: float = 50.0,
                                reward_dropoff: float = 0.4, reward_halflife: float = 100.0) -> float:
  """Host restatement of env/balloon_env.py:44-102 for callers that pass their own
  reward_function / non-default parameters; the default path uses the kernel's reward."""
  b = simulator_state.balloon_state
  radius = units.Distance(km=station_keeping_radius_km)
  distance = units.relative_distance(b.x, b.y)
  if distance <= radius:
    reward = 1.0
  else:
    reward = reward_dropoff * math.exp(-0.69314718056 / reward_halflife * (distance - radius).kilometers)
  if b.last_command == control.AltitudeControlCommand.DOWN and not b.excess_energy:
    scale = min(max((b.acs_power.watts - 100.0) / (300.0 - 100.0), 0.0), 1.0)
    reward *= 0.95 - 0.3 * scale
  return reward


def generative_wind_field_factory(device='cuda:0'):
  """GridBasedWindField over the VAE sampler, as in the reference (env/generative_wind_field.py:35-37).
  The decoder runs on the device with synthetic weights (the trained blob is not in the checkout)."""
  from balloon_learning_environment_amd.env import generative_wind_field
  return grid_based_wind_field.GridBasedWindField(generative_wind_field.GenerativeWindFieldSampler(device=device), device)


def gaussian_wind_field_factory(device='cuda:0'):
  """White-noise grid (tests, worst case for the interpolation)."""
  return grid_based_wind_field.GridBasedWindField(grid_wind_field_sampler.GaussianFieldSampler(), device)


class BalloonEnv:
  """Old-gym (0.21) 4-tuple API like the reference."""
  metadata: Dict[str, Any] = {'render.modes': []}

  def __init__(self, *, station_keeping_radius_km: float = 50.0,
               arena: Optional[balloon_arena.BalloonArenaInterface] = None,
               reward_function: Callable[[simulator_data.SimulatorState], float] = perciatelli_reward_function,
               feature_constructor_factory: Callable = features.perciatelli_feature_constructor,
               wind_field_factory: Callable = generative_wind_field_factory, seed: Optional[int] = None,
               renderer=None):
    self.radius = units.Distance(km=station_keeping_radius_km)
    self._reward_fn = reward_function
    self._use_kernel_reward = (reward_function is perciatelli_reward_function and station_keeping_radius_km == 50.0)
    self._global_iteration = 0
    self.arena = arena if arena is not None else balloon_arena.BalloonArena(feature_constructor_factory, wind_field_factory())
    self._renderer = renderer
    if renderer is not None:
      self.metadata = {'render.modes': renderer.render_modes}       # env/balloon_env.py:150-152
    self.reset(seed=seed if seed is not None else int(time.time() * 1e6) % (2 ** 31))

  def step(self, action: int) -> Tuple[np.ndarray, float, bool, Mapping[str, Any]]:
    command = control.AltitudeControlCommand(action)
    observation = self.arena.step(command)
    assert isinstance(observation, np.ndarray)
    kernel_reward = getattr(self.arena, 'last_reward', None)
    row = getattr(self.arena, '_row', None)
    if row is not None and self._renderer is None and self._use_kernel_reward and kernel_reward is not None:
      # the step brought the balloon's row back with the observation (BalloonArena._step_fast): status and clock straight from it;
      # the BalloonState object is built when somebody asks for it (get_simulator_state)
      reward, status = kernel_reward, int(row['status'])
      info = {'out_of_power': status == balloon.BalloonStatus.OUT_OF_POWER.value, 'envelope_burst': status == balloon.BalloonStatus.BURST.value,
              'zeropressure': status == balloon.BalloonStatus.ZEROPRESSURE.value, 'time_elapsed': dt.timedelta(seconds=int(row['time_elapsed_s']))}
    else:
      simulator_state = self.arena.get_simulator_state()
      if self._renderer is not None:
        self._renderer.step(simulator_state)
      reward = kernel_reward if (self._use_kernel_reward and kernel_reward is not None) else self._reward_fn(simulator_state)
      info = self._get_info(simulator_state.balloon_state)
    is_terminal = info['out_of_power'] or info['envelope_burst'] or info['zeropressure']
    self._global_iteration += 1
    return observation, reward, is_terminal, info

  def reset(self, *, seed: Optional[int] = None, return_info: bool = False):
    if seed is not None:
      self.seed(seed)
    self._rng = np.random.Generator(np.random.Philox(self._rng.integers(0, 2 ** 31)))
    observation = self.arena.reset(int(self._rng.integers(0, 2 ** 31)))
    if self._renderer is not None:                                  # env/balloon_env.py:216-218
      self._renderer.reset()
      self._renderer.step(self.arena.get_simulator_state())
    if return_info:
      return observation, self._get_info(self.get_simulator_state().balloon_state)
    return observation

  def render(self, mode: str = 'human'):
    return None if self._renderer is None else self._renderer.render(mode)

  def close(self) -> None:
    pass

  def seed(self, seed: int) -> None:
    self._rng = np.random.Generator(np.random.Philox(int(seed)))

  @property
  def unwrapped(self): return self

  @property
  def action_space(self): return features.Discrete(3)

  @property
  def observation_space(self): return self.arena.feature_constructor.observation_space

  @property
  def reward_range(self): return (0.0, 1.0)

  def get_simulator_state(self) -> simulator_data.SimulatorState:
    return self.arena.get_simulator_state()

  def _get_info(self, balloon_state: balloon.BalloonState) -> Dict[str, Any]:
    return {'out_of_power': balloon_state.status == balloon.BalloonStatus.OUT_OF_POWER,
            'envelope_burst': balloon_state.status == balloon.BalloonStatus.BURST,
            'zeropressure': balloon_state.status == balloon.BalloonStatus.ZEROPRESSURE,
            'time_elapsed': balloon_state.time_elapsed}

  def __str__(self): return 'BalloonEnv'
  def __enter__(self): return self

  def __exit__(self, *args):
    self.close()
    return False


class VecBalloonEnv:
  """N BalloonEnvs advanced together on one GPU (no reference counterpart: the reference steps one
  environment per Python call).  Same semantics per environment as BalloonEnv -- Perciatelli
  observation, perciatelli_reward_function, terminal on out-of-power / burst / zero-pressure --
  with device tensors in and out and optional auto-reset of terminated environments.

    env = VecBalloonEnv(65536, seed=0)
    obs = env.reset()                                  # [N, 1099] float32 (device)
    obs, reward, terminal = env.step(actions_u8)       # device tensors
  """

  def __init__(self, num_envs: int, *, seed: int = 0, wind_field=None, wind_noise: bool = True,
               auto_reset: bool = True, per_env_fields: bool = False, field_refresh_every: int = 32, device='cuda:0',
               vehicles=None, vehicle_index=None, sample_vehicles: bool = False):
    """wind_noise=True (default, as the reference): ground truth = forecast + SimplexWindNoise, so the WindGP
    has an error signal to model; False is the opt-out (forecast == truth, every GP error exactly 0).
    Wind fields: see VecBalloonArena (default: generative sampler, one shared field per reset();
    per_env_fields=True: one decoded field per environment and per episode).
    vehicles / vehicle_index / sample_vehicles: a fleet of up to 16 vehicles in the batch, each environment's entry given or (sample_vehicles)
    drawn at every reset, auto-resets included -- under capture_graph() replay too, the index being device memory.  The palette is read
    when a call is made: a graph captured before a palette change keeps the old palette, so capture again (VecBalloonArena)."""
    self.arena = balloon_arena.VecBalloonArena(num_envs, wind_field, seed=seed, device=device, per_env_fields=per_env_fields,
                                               vehicles=vehicles, vehicle_index=vehicle_index, sample_vehicles=sample_vehicles)
    self.num_envs, self.device = self.arena.num_envs, self.arena.device
    self._seed, self._wind_noise, self._auto_reset = int(seed), bool(wind_noise), bool(auto_reset)
    self._field_refresh_every, self._steps_since_refresh = int(field_refresh_every), 0
    self._noise = None
    self._graph = None
    self._belief = None                      # lookahead(wind='belief')'s fitted WindGP: one slab, reused from call to call
    self._scenarios = None                   # lookahead(wind='scenarios')'s scenario winds, reused while their number stays
    self._reseed = True               # the first reset() replays the constructor's seed

  def _noise_now(self):
    if not self._wind_noise:
      return None
    self._noise = self.arena.sim.wind_noise(self.arena._seed, out=self._noise)
    return self._noise

  def seed(self, seed: int) -> None:
    self._seed = int(seed)
    self._reseed = True

  def reset(self, seed: Optional[int] = None):
    """reset(seed) / seed(s); reset(): reproducible new episodes and wind field(s).  reset() without a
    seed: the next episodes of the current seed (new initial conditions, new wind field(s))."""
    if seed is not None:
      self.seed(seed)
    if getattr(self, '_reseed', False):
      self.arena.reset(self._seed); self._reseed = False
    else:
      self.arena.reset()
    self.check_errors()
    self._graph = None
    self._steps_since_refresh = 0
    return self.arena.observe(self._noise_now())

  def state_dict(self) -> dict:
    """Checkpoint of the whole batch (balloons, episode counters, wind field(s), WindGP histories, seeds): a run restored
    with load_state_dict() continues bit for bit -- same observations, rewards, terminals, auto-resets."""
    return {'arena': self.arena.state_dict(), 'seed': self._seed, 'reseed': bool(getattr(self, '_reseed', False)),
            'steps_since_refresh': self._steps_since_refresh,
            'noise': None if self._noise is None else self._noise.clone()}

  def load_state_dict(self, d: dict) -> None:
    self.arena.load_state_dict(d['arena'])
    self._seed, self._reseed, self._steps_since_refresh = int(d['seed']), bool(d['reseed']), int(d['steps_since_refresh'])
    self._noise = None if d['noise'] is None else d['noise'].clone()
    self._graph = None                       # a captured graph holds the old buffers: capture again after a resume

  def check_errors(self) -> None:
    """Synchronises and raises what the reference would have raised inside step / observe since the last
    call (non-finite state, pressure out of range, WindGP window overflow, failed pressure-range search...)."""
    self.arena.sim.check_errors()

  def query_wind(self, xyp, time_s=None, add_forecast: bool = True, out=None):
    """The WindGP posterior of every environment at the caller's points -- "what wind, with what confidence, at these (x, y, p), at
    that time?": xyp [N, q, 3] float32 device tensor -> (mean_uv [N, q, 2], deviation [N, q]); VecSimulator.query_wind."""
    return self.arena.sim.query_wind(xyp, time_s, add_forecast, out)

  def lookahead(self, plans, gamma: float = 0.993, action_repeat: int = 1, wind: str = 'truth', want_rewards: bool = False,
                want_final: bool = False, out=None, num_scenarios: int = 8, risk_tail: Optional[int] = None, want_leaves: bool = False):
    """"From where each balloon is now, what happens under these K action sequences?": plans uint8 device tensor [H, N, K] ->
    Rollout(returns [N, K], steps_flown [N, K], rewards or None, final or None), nothing of the environments changed
    (VecSimulator.rollout_plans; no auto-reset inside a plan: a plan that goes terminal stops there).
    wind='truth': the wind the environments themselves will fly -- forecast + this env's wind noise with wind_noise=True, the forecast
    alone otherwise; what a simulator-side planner or a return estimator wants.  wind='forecast': the forecast alone, which ignores
    what the balloon has measured.  wind='belief': forecast + the mean of the WindGP over the balloon's own measurements -- the wind
    the observation is built on, all an agent may legitimately know; fitted now (arena.fit_wind_belief) and flown
    (rollout_plans(belief=)): two launches, no host synchronisation, capturable in a HIP graph.
    wind='scenarios': forecast + each of num_scenarios (<= 16) winds SAMPLED from the WindGP's posterior -- draws of the noise field
    conditioned on the balloon's measurements, from streams of their own keyed by this env's seed (never the truth's draw): fitted now
    (arena.fit_wind_scenarios), flown (rollout_plans(scenarios=)) and scored (arena.plan_risk).  Returns (Rollout with returns
    [N, K, M], steps_flown [N, K, M], ..., score [N, K]): score is the mean of the risk_tail smallest scenario returns of every plan
    (None: all M, the expectation; 1: the worst case).
    want_leaves: every plan's end state as a full state, Rollout.leaves: a VecSimulator of N K environments (environment e K + k is
    plan k of environment e; kept and reused per K), which arena.sim.observe_leaves() observes against these environments' histories.
    Not with wind='scenarios' (ValueError).
    Flags of the imagined flights go to arena.sim.rollout_flags, never to check_errors()."""
    if wind not in ('truth', 'forecast', 'belief', 'scenarios'):
      raise ValueError(f"lookahead: wind is 'truth', 'forecast', 'belief' or 'scenarios', not {wind!r}")
    leaves = None
    if want_leaves:
      if wind == 'scenarios':
        raise ValueError("lookahead: wind='scenarios' hands back no leaves (M end states per plan)")
      k = int(plans.shape[2])
      if getattr(self, '_leaf_arena', None) is None or self._leaf_arena.leaves_per_env != k:
        self._leaf_arena = self.arena.sim.leaf_arena(k)
      leaves = self._leaf_arena
    if wind == 'scenarios':
      reuse = self._scenarios if (self._scenarios is not None and self._scenarios.num == int(num_scenarios)) else None
      self._scenarios = self.arena.fit_wind_scenarios(num_scenarios, seed=self.arena._seed, out=reuse)
      ro = self.arena.lookahead(plans, gamma, action_repeat, None, want_rewards, want_final, out, scenarios=self._scenarios)
      return ro, self.arena.plan_risk(ro.returns, risk_tail)
    if wind == 'belief':
      self._belief = self.arena.fit_wind_belief(out=self._belief)
      return self.arena.lookahead(plans, gamma, action_repeat, None, want_rewards, want_final, out, belief=self._belief, leaves=leaves)
    noise_seed = self.arena._seed if (wind == 'truth' and self._wind_noise) else None
    return self.arena.lookahead(plans, gamma, action_repeat, noise_seed, want_rewards, want_final, out, leaves=leaves)

  def tree_search(self, depth: int, beam_width: int, segment: int = 4, action_repeat: int = 1, gamma: float = 0.993, wind: str = 'truth',
                  **kw):
    """Plan by beam search from where each balloon is now, nothing of the environments changed: depth levels of one action flown
    segment * action_repeat agent steps, the best beam_width nodes kept per environment and level -> TreeSearch(action, best_plan,
    best_return, q, visits, returns, steps_flown, leaves) (VecSimulator.tree_search; action_values=, leaf_score=, buffers= go through).
    wind: lookahead's 'truth', 'forecast' or 'belief' (fitted now), or 'scenarios': num_scenarios (<= 16) winds sampled from the
    WindGP's posterior, fitted now from streams keyed by this env's seed (arena.fit_wind_scenarios), every edge flown in each of them
    and every level ordered by the mean of the risk_tail smallest scenario returns of a node (None: all of them); TreeSearch.returns is
    then [N, C, M] and TreeSearch.score [N, C]."""
    if wind not in ('truth', 'forecast', 'belief', 'scenarios'):
      raise ValueError(f"tree_search: wind is 'truth', 'forecast', 'belief' or 'scenarios', not {wind!r}")
    if wind == 'scenarios':
      num_scenarios, risk_tail = kw.pop('num_scenarios', 8), kw.pop('risk_tail', None)
      reuse = self._scenarios if (self._scenarios is not None and self._scenarios.num == int(num_scenarios)) else None
      self._scenarios = self.arena.fit_wind_scenarios(num_scenarios, seed=self.arena._seed, out=reuse)
      return self.arena.tree_search(depth, beam_width, segment, action_repeat, gamma, scenarios=self._scenarios, risk_tail=risk_tail, **kw)
    if wind == 'belief':
      self._belief = self.arena.fit_wind_belief(out=self._belief)
      return self.arena.tree_search(depth, beam_width, segment, action_repeat, gamma, belief=self._belief, **kw)
    noise_seed = self.arena._seed if (wind == 'truth' and self._wind_noise) else None
    return self.arena.tree_search(depth, beam_width, segment, action_repeat, gamma, noise_seed=noise_seed, **kw)

  def mcts_search(self, num_rounds: int, leaves_per_round: int, max_depth: int, segment: int = 4, action_repeat: int = 1,
                  gamma: float = 0.993, c_puct: float = 1.25, wind: str = 'truth', **kw):
    """Guided tree search from where each balloon is now, nothing of the environments changed -> MCTSSearch(action, q,
    visits, best_return, best_plan, pv_length, pool) (VecSimulator.mcts_search; guide_fn=, root_prior=, buffers=, trace= go through).
    wind: lookahead's 'truth', 'forecast' or 'belief' (fitted now), or 'scenarios' with num_scenarios=M (required: the budget of a
    search is the caller's decision) and risk_tail (None: M): M winds sampled from the WindGP's posterior, fitted now from streams keyed
    by this env's seed (arena.fit_wind_scenarios) into a kept WindScenarios; a node is a group of M scenario nodes, backed up by the mean
    of the risk_tail smallest of its M values.  The pool is 3 L R M nodes per environment; with a guide, 3 L M observation
    rows of 4.4 KB per environment on top."""
    if wind == 'scenarios':
      if 'num_scenarios' not in kw:
        raise ValueError("mcts_search: wind='scenarios' needs num_scenarios (the pool holds M nodes per group: the budget of a search has no "
                         "default); or search in the belief, the forecast or the truth")
      num_scenarios, risk_tail = kw.pop('num_scenarios'), kw.pop('risk_tail', None)
      reuse = self._scenarios if (self._scenarios is not None and self._scenarios.num == int(num_scenarios)) else None
      self._scenarios = self.arena.fit_wind_scenarios(num_scenarios, seed=self.arena._seed, out=reuse)
      return self.arena.mcts_search(num_rounds, leaves_per_round, max_depth, segment, action_repeat, gamma, c_puct, scenarios=self._scenarios,
                                    risk_tail=risk_tail, **kw)
    if wind not in ('truth', 'forecast', 'belief'):
      raise ValueError(f"mcts_search: wind is 'truth', 'forecast', 'belief' or 'scenarios', not {wind!r}")
    if wind == 'belief':
      self._belief = self.arena.fit_wind_belief(out=self._belief)
      return self.arena.mcts_search(num_rounds, leaves_per_round, max_depth, segment, action_repeat, gamma, c_puct, belief=self._belief, **kw)
    noise_seed = self.arena._seed if (wind == 'truth' and self._wind_noise) else None
    return self.arena.mcts_search(num_rounds, leaves_per_round, max_depth, segment, action_repeat, gamma, c_puct, noise_seed=noise_seed, **kw)

  def planner(self, search: str = 'sample', **kw):
    """A look-ahead agent bound to these environments.  search='sample' (the default): agents.lookahead_agent.VecLookaheadAgent(**kw)
    -- num_plans, horizon, action_repeat, segment, gamma, wind ('belief' by default; 'scenarios' with num_scenarios, risk_tail), iterations, elite, seed,
    leaf_value (a critic whose value of every plan's end state is added to its return) -- planning in this batch's simulator.
    search='beam': agents.beam_agent.VecBeamSearchAgent(**kw) -- beam_width, depth, segment, action_repeat, gamma, wind ('belief' by
    default, 'forecast' or 'truth'), leaf_value, action_values: a systematic, deterministic search of a shared-prefix tree of plans;
    with wind='scenarios' agents.beam_agent.VecScenarioBeamSearchAgent -- the same tree flown in num_scenarios sampled winds and ordered
    by risk_tail's score (seed keys the scenario streams; no leaf_value).
    search='mcts': agents.mcts_agent.VecMCTSAgent(**kw) -- num_rounds, leaves_per_round, max_depth (all three required), segment, action_repeat, gamma, c_puct,
    wind ('belief' by default, 'forecast' or 'truth'), guide (a device agent or trainer whose prior and value steer the search): PUCT over
    a node pool, the root's visit counts as the answer; with wind='scenarios' agents.mcts_agent.VecScenarioMCTSAgent -- the
    same search over groups of num_scenarios (required) scenario nodes, a group backed up by risk_tail's score (seed keys the scenario
    streams).
    wind='truth' flies the plans in the wind these environments fly, this env's wind noise included (with wind_noise=False the truth
    is the forecast).  actions = agent.act(obs); obs, reward, terminal = env.step(actions): no host synchronisation in either."""
    if search not in ('sample', 'beam', 'mcts'):
      raise ValueError(f"planner: search is 'sample', 'beam' or 'mcts', not {search!r}")
    kw.setdefault('device', self.device)
    if search == 'mcts':
      from balloon_learning_environment_amd.agents import mcts_agent
      missing = [k for k in ('num_rounds', 'leaves_per_round', 'max_depth') if k not in kw]
      if missing:                  # (VecMCTSAgent's three arguments without a default)
        raise ValueError(f"planner: search='mcts' needs {', '.join(missing)}: the budget of a guided tree search has no default")
      if kw.get('wind') == 'scenarios':
        if 'num_scenarios' not in kw:
          raise ValueError("planner: search='mcts' with wind='scenarios' needs num_scenarios: the budget of a guided tree search has no default")
        agent = mcts_agent.VecScenarioMCTSAgent(**{k: v for k, v in kw.items() if k != 'wind'})
      else:
        agent = mcts_agent.VecMCTSAgent(**kw)
    elif search == 'beam':
      from balloon_learning_environment_amd.agents import beam_agent
      if kw.get('wind') == 'scenarios':
        agent = beam_agent.VecScenarioBeamSearchAgent(**{k: v for k, v in kw.items() if k != 'wind'})
      else:
        agent = beam_agent.VecBeamSearchAgent(**kw)
    else:
      from balloon_learning_environment_amd.agents import lookahead_agent
      agent = lookahead_agent.VecLookaheadAgent(**kw)
    return agent.bind(self.arena.sim, noise_seed=(lambda: self.arena._seed) if self._wind_noise else None)

  def _step_eager(self, actions, obs_out=None, end_mask=None):
    noise = None
    if self._wind_noise:
      noise = self._noise if self._noise is not None else self._noise_now()     # step() before reset()
    reward, terminal = self.arena.step(actions, noise)
    if self._auto_reset:
      self._terminal_buf.copy_(terminal)
      if end_mask is not None:
        self._terminal_buf.bitwise_or_(end_mask)
      self.arena.reset_lanes(self._terminal_buf)
    return self.arena.observe(self._noise_now(), out=obs_out), reward, terminal

  def step(self, actions, end_mask=None):
    """actions: uint8 device tensor [N] in {0, 1, 2}.  Returns (obs [N, 1099], reward [N], terminal [N] u8);
    `terminal` refers to the transition just made; with auto_reset the returned observation of a
    terminated environment is the first one of its next episode.  With `capture_graph()` the three
    tensors are static buffers that the next step overwrites.  Error conditions are latched on the device:
    call check_errors() (reset() does) to have them raised.
    end_mask: optional uint8 device [N] (auto_reset, no captured graph): these environments' episodes end after this step
    without a terminal (a time limit) and restart as a terminated one does."""
    if not hasattr(self, '_terminal_buf'):
      self._terminal_buf = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
    if end_mask is not None:
      if not self._auto_reset or self._graph is not None:
        raise ValueError('step(end_mask=...) needs auto_reset and eager steps (no captured graph)')
      assert end_mask.dtype == torch.uint8 and end_mask.numel() == self.num_envs
      obs, reward, terminal = self._step_eager(actions, end_mask=end_mask)
      out = obs, reward.clone(), terminal.clone()
    elif self._graph is not None:
      self._g_actions.copy_(actions)
      self._graph.replay()
      out = self._g_obs, self._g_reward, self._g_terminal
    else:
      obs, reward, terminal = self._step_eager(actions)
      out = obs, reward.clone(), terminal.clone()
    if self.arena.per_env_fields and self._auto_reset:
      self._steps_since_refresh += 1
      if self._steps_since_refresh >= self._field_refresh_every:
        self._steps_since_refresh = 0
        self.arena.refresh_fields()
    return out

  def capture_graph(self):
    """Records one step (wind noise, transition, masked reset, observation: four kernels plus a few
    fills) into a HIP graph and replays it from then on -- for small batches the loop is launch-bound.
    Call after reset() and at least one step() (lazy allocations must have happened)."""
    n, dev_ = self.num_envs, self.device
    self._g_actions = torch.ones(n, dtype=torch.uint8, device=dev_)
    self._g_obs = torch.empty(n, 1099, dtype=torch.float32, device=dev_)
    if not hasattr(self, '_terminal_buf'):
      self._terminal_buf = torch.zeros(n, dtype=torch.uint8, device=dev_)

    def body():
      _, reward, terminal = self._step_eager(self._g_actions, obs_out=self._g_obs)
      return reward.clone(), terminal.clone()
    self._graph, (self._g_reward, self._g_terminal) = dev.capture(dev_, body)

  @property
  def observation_space(self):
    return features.Box(np.concatenate([[0, 0, 0, -1, -1, -1, -1], np.zeros(8), [1.0], np.zeros(1083)]).astype(np.float32),
                        np.concatenate([np.ones(15), [np.inf], np.ones(1083)]).astype(np.float32))

  @property
  def action_space(self):
    return features.Discrete(3)
