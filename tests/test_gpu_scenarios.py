"""Scenario winds on the device: ble_gp_fit_scenarios_f32 / ble_gp_scenario_wind_f32 / ble_rollout_scenarios_f32 /
ble_plan_risk_f32 through VecSimulator.fit_wind_scenarios, scenario_wind, rollout_plans(scenarios=), plan_risk and
VecLookaheadAgent(wind='scenarios').

References.  (a) The prior f_m: the noise oracle (oracle/noise_oracle.py, float32) over the harmonics of the twin's scenario stream
(tests/scenario_host.py), to the bar tests/test_gpu_noise.py holds ble_wind_noise_f32 to (1e-5 against the float32 oracle), and the
pointwise noise kernel fed the same 50 words through its harmonic cache, bit for bit.  (b) The fit: alpha^m = cho_solve(K + 0.05 I,
y - f_m(X)) with the DEVICE's own prior_only values at the ring's points as f_m(X) (the float32 rounding of the noise would otherwise
be amplified by up to 1 / 0.05), the scenario wind = float32(prior) + float32(k* alpha^m) within the project's 1e-5 m/s.
(c) The rollout: a copy of the source stepped with scenario_wind at the copy's state as ble_step_f32's noise_uv -- rewards,
steps_flown and the final state bit for bit, the return within one float32 ulp of the float64 host sum (tests/test_gpu_belief.py's
contract).  (d) The risk score and the planner: the twin, bit for bit."""
import dataclasses

import numpy as np
import pytest
import torch

import helpers
import noise_oracle
import plan_host
import scenario_host as sh
from helpers import observations as _observations, ring_back as _ring_back, write_ring as _write_ring
from balloon_learning_environment_amd import _abi, _lib, device as dev, vec_state
from balloon_learning_environment_amd.agents import lookahead_agent
from balloon_learning_environment_amd.env import balloon_env
from balloon_learning_environment_amd.eval import eval_lib, suites

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
TOL = 1e-5
FINAL_FIELDS = ('x', 'y', 'pressure', 'battery_charge')
OFFSETS = (0, 3600, 6 * 3600, 12 * 3600)


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)
  return t if dtype is None else t.to(dtype)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flags(sim, clear=True):
  word = int(sim.err_flags.item())
  if clear:
    sim.err_flags.zero_()
  return word


def _wind(sim, scn, m, pts, t, prior_only=False):
  """scenario_wind at one point per environment: pts [n, 3] float32, t [n] -> [n, 2] float32 (host)."""
  out = sim.scenario_wind(scn, m, _dev(pts[:, 0]), _dev(pts[:, 1]), _dev(pts[:, 2]), _dev(np.asarray(t, np.int32)), prior_only=prior_only)
  torch.cuda.synchronize()
  return out.cpu().numpy()


def _points(rng, n):
  return np.concatenate([rng.uniform(-2.5e5, 2.5e5, (n, 2)), rng.uniform(4000.0, 15000.0, (n, 1))], -1).astype(np.float32)


def _empty_scn(sim, num, seed=0, seeds=None):
  return vec_state.WindScenarios(torch.zeros(sim.n, _abi.gp_scenario_doubles(num), dtype=torch.float64, device=sim.device),
                                 torch.zeros(sim.n, dtype=torch.int32, device=sim.device), num, seed, seeds)


# ---------------------------------------------------------------------------------------------- 1. the prior
def _noise_kernel(words_seeds, words_offsets, x, y, p, t, seed, episode):
  """ble_wind_noise_f32 over GIVEN harmonics (through its harmonic cache, keyed for (seed, episode)): [q, 2] float32."""
  q = len(x)
  cache = _dev(helpers.noise_cache_from_draws(words_seeds, words_offsets, q, seed=seed, episode=episode).view(np.int32))
  ep = torch.full((q,), episode, dtype=torch.int32, device=DEVICE)
  out = torch.empty(q, 2, device=DEVICE)
  d = [_dev(a) for a in (x, y, p, t)]
  assert _lib.lib().ble_wind_noise_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), seed, ep.data_ptr(), 0, cache.data_ptr(),
                                       out.data_ptr(), q, 0) == 0
  torch.cuda.synchronize()
  return out.cpu().numpy()


def test_prior_against_the_oracle_and_the_noise_kernel():
  rng = np.random.default_rng(60)
  # (a) a seed per environment: two seeds x three scenarios x two episodes, 50 points each -- groups share one stream
  groups = [(s, m, ep) for s in (77, 2 ** 40 + 5) for m in (0, 7, 15) for ep in (0, 3)]
  per = 50
  n = per * len(groups)
  sim = vec_state.VecSimulator(n, DEVICE)
  seeds = np.repeat([g[0] for g in groups], per).astype(np.int64)
  index = np.repeat([g[1] for g in groups], per).astype(np.int32)
  sim.episode.copy_(_dev(np.repeat([g[2] for g in groups], per).astype(np.int32)))
  pts = _points(rng, n)
  t = rng.integers(0, 48 * 3600, n).astype(np.int32)
  scn = _empty_scn(sim, 16, seeds=_dev(seeds))
  got = _wind(sim, scn, _dev(index), pts, t, prior_only=True)
  worst = 0.0
  for g, (s, m, ep) in enumerate(groups):
    rows = slice(per * g, per * (g + 1))
    hs, ho = sh.harmonics(s, 0, ep, m)
    x, y, p = pts[rows, 0], pts[rows, 1], pts[rows, 2]
    o32 = sh.prior(hs, ho, x, y, p, t[rows])
    err = np.abs(got[rows] - o32).max()
    worst = max(worst, err)
    assert err < TOL, (s, m, ep, err)
    assert np.array_equal(_bits(got[rows]), _bits(_noise_kernel(hs, ho, x, y, p, t[rows], s, ep))), (s, m, ep)
  print(f'prior vs the float32 oracle over {len(groups)} streams: max |diff| {worst:.2e}')
  assert 0.6 < got.var() < 1.5
  # (b) a batch seed: environment e's stream is keyed env_offset + e
  n2, offset = 24, 5
  sim2 = vec_state.VecSimulator(n2, DEVICE, env_offset=offset)
  sim2.episode.copy_(_dev((np.arange(n2) % 3).astype(np.int32)))
  pts2, t2 = _points(rng, n2), rng.integers(0, 48 * 3600, n2).astype(np.int32)
  index2 = (np.arange(n2) % 3).astype(np.int32)
  got2 = _wind(sim2, _empty_scn(sim2, 3, seed=91), _dev(index2), pts2, t2, prior_only=True)
  for e in range(n2):
    hs, ho = sh.harmonics(91, offset + e, e % 3, index2[e])
    o32 = sh.prior(hs, ho, pts2[e:e + 1, 0], pts2[e:e + 1, 1], pts2[e:e + 1, 2], t2[e:e + 1])
    assert np.abs(got2[e] - o32[0]).max() < TOL, e
  # with n_obs = 0 (the zero slab above) the scenario IS its prior, by value; an index outside 0 .. M - 1 is NaN
  full = _wind(sim2, _empty_scn(sim2, 3, seed=91), _dev(index2), pts2, t2)
  assert np.array_equal(full, got2 + np.float32(0.0))
  bad = index2.copy(); bad[1] = 3; bad[2] = -1
  out = _wind(sim2, _empty_scn(sim2, 3, seed=91), _dev(bad), pts2, t2)
  assert np.isnan(out[1:3]).all() and np.array_equal(_bits(out[3:]), _bits(full[3:])) and np.array_equal(_bits(out[0]), _bits(full[0]))


# ---------------------------------------------------------------------------------------------- 2, 3. the fit and its laws
SIZES = (0, 1, 3, 17, 120)          # environments 0 .. 4; 5: more than 120 inside 6 h (the flag); 6: the NaN case
FIT_SEED = 19


def _fit_sim():
  rng = np.random.default_rng(61)
  n = len(SIZES) + 2
  sim = vec_state.VecSimulator(n, DEVICE)
  sim._allocate_history(False)
  for e, m in enumerate(SIZES):
    _write_ring(sim, e, _observations(rng, m, 180))
  _write_ring(sim, 5, _observations(rng, 125, 60))
  _write_ring(sim, 6, _observations(rng, 300, 180))
  anchor = np.array([180 * max(m - 1, 0) for m in SIZES] + [60 * 124, 180 * 299 - 3600], np.int32)
  sim.state['time_elapsed_s'].copy_(_dev(anchor))
  sim.episode.copy_(_dev(np.array([0, 1, 0, 2, 0, 0, 0], np.int32)))
  return sim, anchor, rng


@pytest.fixture(scope='module')
def fits():
  """The fit at M = 1, 3, 16 on one simulator, the device's own prior at the ring's points and the twin's windows: computed once."""
  sim, anchor, rng = _fit_sim()
  rings = [_ring_back(sim, e) for e in range(sim.n)]
  windows = [sh.Window(rings[e], anchor[e]) for e in range(sim.n)]
  out = {'sim': sim, 'anchor': anchor, 'windows': windows, 'rng': rng}
  belief = sim.fit_wind_belief()
  torch.cuda.synchronize()
  out['belief'] = belief
  out['belief_flags'] = _flags(sim)
  for num in (1, 3, 16):
    scn = sim.fit_wind_scenarios(num, seed=FIT_SEED)
    torch.cuda.synchronize()
    out[num] = (scn, _flags(sim))
  # f_m(X) as the device gives it, for the 16 scenarios: [n][m] -> [n_obs, 2]; one launch per (m, row of the longest window)
  scn16 = out[16][0]
  rows = max(w.n_obs for w in windows[:6])
  prior = np.zeros((16, rows, sim.n, 2), np.float32)
  pts, ts = np.zeros((rows, sim.n, 3), np.float32), np.zeros((rows, sim.n), np.int32)
  for e, w in enumerate(windows[:6]):
    pts[:w.n_obs, e], ts[:w.n_obs, e] = w.xyp.astype(np.float32), w.t.astype(np.int32)
  dp = [[_dev(pts[i, :, k]) for k in range(3)] + [_dev(ts[i])] for i in range(rows)]
  for m in range(16):
    index = torch.full((sim.n,), m, dtype=torch.int32, device=DEVICE)
    res = [sim.scenario_wind(scn16, index, *dp[i], prior_only=True) for i in range(rows)]
    prior[m] = torch.stack(res).cpu().numpy()
  out['prior_at_x'] = prior
  out['pts_at_x'], out['t_at_x'] = pts, ts
  return out


@pytest.mark.parametrize('num', [1, 3, 16])
def test_fit_against_the_twin(fits, num):
  sim, anchor, windows, rng = fits['sim'], fits['anchor'], fits['windows'], np.random.default_rng(62 + num)
  scn, flags = fits[num]
  belief = fits['belief']
  assert flags == _lib.FLAG_GP_WINDOW == fits['belief_flags']          # environments 5 and 6
  assert scn.slab.shape == (sim.n, 480 + 240 * num) and scn.num == num
  n_obs = scn.n_obs.cpu().numpy().tolist()
  assert n_obs == list(SIZES) + [120, -1] == belief.n_obs.cpu().numpy().tolist()
  assert [w.n_obs for w in windows[:6]] == n_obs[:6]
  slab = scn.slab.cpu().numpy()
  # the window: ble_gp_fit_f32's, bit for bit; zero beyond it, in loc and in every scenario's weights
  assert np.array_equal(slab[:, :480].view(np.uint64), belief.slab.cpu().numpy()[:, :480].view(np.uint64))
  for e, m in enumerate(n_obs):
    m = max(m, 0)
    assert not slab[e, 4 * m:480].any(), e
    alpha = slab[e, 480:].reshape(num, 120, 2)
    assert not alpha[:, m:].any(), e
    assert m == 0 or alpha[:, :m].all(), e
  assert not slab[6].any() and not slab[0].any()
  # alpha^m against the twin's solve of the device's own right-hand side, then the wind at random points and times
  q = 3
  worst = 0.0
  for m in sorted({0, num // 2, num - 1}):
    hs = [sh.harmonics(FIT_SEED, e, int(sim.episode[e].item()), m) for e in range(sim.n)]
    alphas = [windows[e].alpha(fits['prior_at_x'][m, :windows[e].n_obs, e]) for e in range(6)]
    for e in range(1, 6):
      got_alpha = slab[e, 480 + 240 * m:480 + 240 * (m + 1)].reshape(120, 2)[:windows[e].n_obs]
      assert np.abs(got_alpha - alphas[e]).max() <= 1e-9 * max(1.0, np.abs(alphas[e]).max()), (e, m)
    for offset in OFFSETS:
      for _ in range(q):
        pts = _points(rng, sim.n)
        t = anchor + offset
        got = _wind(sim, scn, m, pts, t)
        assert np.isnan(got[6]).all()
        for e in range(6):
          f = sh.prior(*hs[e], pts[e:e + 1, 0], pts[e:e + 1, 1], pts[e:e + 1, 2], t[e:e + 1])
          want = sh.scenario_wind(f, windows[e].correction(alphas[e], pts[e:e + 1], t[e:e + 1]))[0]
          err = np.abs(got[e].astype(np.float64) - want.astype(np.float64)).max()
          worst = max(worst, err)
          assert np.isfinite(got[e]).all() and err <= TOL, (num, m, e, offset, err)
  print(f'M={num}: scenario wind vs the twin, max |device - host| = {worst:.3e}')


def test_laws_on_the_device(fits):
  sim, anchor, windows = fits['sim'], fits['anchor'], fits['windows']
  scn, _ = fits[16]
  slab = scn.slab.cpu().numpy()
  pts, ts, prior = fits['pts_at_x'], fits['t_at_x'], fits['prior_at_x']
  rows = pts.shape[0]
  dp = [[_dev(pts[i, :, k]) for k in range(3)] + [_dev(ts[i])] for i in range(rows)]
  worst = 0.0
  for m in (0, 5, 15):
    index = torch.full((sim.n,), m, dtype=torch.int32, device=DEVICE)
    at_x = torch.stack([sim.scenario_wind(scn, index, *dp[i]) for i in range(rows)]).cpu().numpy()          # [rows, n, 2]
    for e in range(1, 6):
      w = windows[e]
      alpha = slab[e, 480 + 240 * m:480 + 240 * (m + 1)].reshape(120, 2)[:w.n_obs]
      # interpolation: the scenario passes through the measurements up to the observation noise's share
      err = np.abs(at_x[:w.n_obs, e].astype(np.float64) - (w.y - 0.05 * alpha)).max()
      worst = max(worst, err)
      assert err <= TOL, (m, e, err)
      # linearity: alpha^m + (K + 0.05 I)^-1 f_m(X) = the belief's alpha (fit_wind_belief's slab)
      belief_alpha = fits['belief'].slab[e, 480:].cpu().numpy().reshape(120, 2)[:w.n_obs]
      lin = np.abs(alpha + w.solve(prior[m, :w.n_obs, e]) - belief_alpha).max()
      assert lin <= 1e-9 * max(1.0, np.abs(belief_alpha).max()), (m, e, lin)
    # n_obs = 0: the scenario is its prior, by value; the NaN case: NaN
    assert np.array_equal(at_x[:, 0], prior[m, :, 0] + np.float32(0.0))
    assert np.isnan(at_x[:, 6]).all()
  print(f'interpolation on the device: max |error_m(X_i) - (y_i - 0.05 alpha_i)| = {worst:.3e}')
  # scenarios differ from each other and from the belief's mean away from the measurements
  far = _points(np.random.default_rng(5), sim.n)
  a, b = _wind(sim, scn, 0, far, anchor + 6 * 3600), _wind(sim, scn, 1, far, anchor + 6 * 3600)
  assert np.abs(a[:6] - b[:6]).min() > 1e-3


def test_window_flags_one_by_one():
  sim, anchor, _ = _fit_sim()

  def fit(envs):
    count = sim._gp['count'].clone()
    mask = torch.ones(sim.n, dtype=torch.bool, device=sim.device)
    mask[envs] = False
    sim._gp['count'][mask] = 0
    scn = sim.fit_wind_scenarios(3, seed=1)
    torch.cuda.synchronize()
    sim._gp['count'].copy_(count)
    return scn

  assert fit([1, 2, 3, 4]).n_obs.cpu().numpy().tolist() == [0, 1, 3, 17, 120, 0, 0] and _flags(sim) == 0
  assert fit([5]).n_obs.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 120, 0] and _flags(sim) == _lib.FLAG_GP_WINDOW
  scn = fit([6])
  assert scn.n_obs.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 0, -1] and _flags(sim) == _lib.FLAG_GP_WINDOW
  assert not scn.slab.cpu().numpy().any()
  sim.reset_observation_history(torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.uint8, device=sim.device))
  assert fit([3, 4]).n_obs.cpu().numpy().tolist() == [0, 0, 0, 0, 120, 0, 0] and _flags(sim) == 0
  # before any observe(): no history is allocated, every scenario is its prior
  fresh = vec_state.VecSimulator(3, DEVICE)
  scn = fresh.fit_wind_scenarios(2, seed=4)
  torch.cuda.synchronize()
  assert fresh._gp is None and not scn.slab.cpu().numpy().any() and scn.n_obs.cpu().numpy().tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------- 4. rollout == stepping a copy
def _source(n, seed, window_sizes, vehicle=None, warm=4, env_offset=0):
  """A simulator `warm` random agent steps into its episodes whose rings hold window_sizes[e] observations 180 s apart ending now."""
  rng = np.random.default_rng(seed)
  sim = vec_state.VecSimulator(n, DEVICE, env_offset=env_offset)
  sim.set_grid(rng.uniform(-12.0, 12.0, vec_state.GRID_SHAPE).astype(np.float32))
  if vehicle:
    sim.set_vehicle(**vehicle)
  sim.reset_device(seed)
  a = _dev(rng.integers(0, 3, (warm, n)).astype(np.uint8))
  sim.step_n(a, torch.zeros(a.shape, dtype=torch.float32, device=sim.device), torch.zeros(a.shape, dtype=torch.uint8, device=sim.device))
  sim.check_errors()
  sim._allocate_history(False)
  now = sim.state['time_elapsed_s'].cpu().numpy()
  xy = np.stack([sim.state['x'].cpu().numpy(), sim.state['y'].cpu().numpy()], -1)
  for e, m in enumerate(window_sizes):
    xyp, t, err = _observations(rng, m, 180, end=int(now[e]))
    xyp[:, :2] = (0.2 * xyp[:, :2] + xy[e]).astype(np.float32)          # measurements within 40 km of the balloon
    _write_ring(sim, e, (xyp, t, err))
  return sim, rng


def _reference(src, scn, plans, action_repeat, substeps):
  """scenario_wind + ble_step_f32 on a copy of the source, plan by plan and scenario by scenario:
  (rewards [T, n, K, M], steps_flown [n, K, M], final [4, n, K, M])."""
  h, n, k_plans = plans.shape
  num, steps = scn.num, h * action_repeat
  sd = src.state_dict()
  ok = (sd['state']['status'] == 0).cpu().numpy()
  ref = vec_state.VecSimulator(n, DEVICE, env_offset=src.env_offset)
  rewards = torch.zeros(steps, n, k_plans, num, dtype=torch.float32, device=src.device)
  term = torch.zeros(steps, n, k_plans, num, dtype=torch.uint8, device=src.device)
  final = np.zeros((4, n, k_plans, num), np.float32)
  actions = _dev(np.repeat(plans, action_repeat, axis=0))
  uv = torch.zeros(n, 2, dtype=torch.float32, device=src.device)
  for m in range(num):
    index = torch.full((n,), m, dtype=torch.int32, device=src.device)
    for k in range(k_plans):
      ref.load_state_dict(sd)
      for t in range(steps):
        ref.scenario_wind(scn, index, out=uv)
        r, tm = ref.step(actions[t, :, k].contiguous(), uv, substeps=substeps)
        rewards[t, :, k, m] = r; term[t, :, k, m] = tm
      final[:, :, k, m] = np.stack([ref.state[f].cpu().numpy() for f in FINAL_FIELDS])
  term = term.cpu().numpy() != 0
  flown = np.where(ok[:, None, None], np.where(term.any(0), term.argmax(0) + 1, steps), 0).astype(np.int32)
  return rewards.cpu().numpy(), flown, final


def _host_returns(rewards, gamma):
  acc, disc = np.zeros(rewards.shape[1:], np.float64), 1.0
  for t in range(rewards.shape[0]):
    term = disc * rewards[t].astype(np.float64)
    acc += term
    disc *= gamma
  return acc.astype(np.float32)


# name: (n, K, M, H, action_repeat, substeps, window sizes, vehicle)
CASES = {
    'n5_k5_m3_a_wave_spans_environments': (5, 5, 3, 3, 1, 18, (0, 1, 3, 17, 120), None),
    'n5_k7_m8_280_lanes_repeat_2': (5, 7, 8, 3, 2, 18, (120, 0, 17, 3, 1), None),
    'n3_k5_m16_substeps_7_runtime_vehicle': (3, 5, 16, 3, 1, 7, (17, 120, 0), {'payload_mass': 95.0, 'battery_capacity_wh': 2800.0}),
    'n3_k5_m1': (3, 5, 1, 3, 1, 18, (3, 120, 17), None),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_rollout_equals_scenario_wind_and_step_on_a_copy(case):
  n, k, num, h, repeat, substeps, sizes, vehicle = CASES[case]
  gamma = 0.993
  src, rng = _source(n, 300 + sorted(CASES).index(case), sizes, vehicle=vehicle)
  if n == 5:
    src.state['status'][1] = 1                       # a source that is not OK flies nothing
    src.state['mols_air'][2] += 30000.0              # far above the superpressure limit: every plan bursts in its first step
  src.wind_noise(7)                                  # (allocates the harmonic cache: it must stay as it is)
  scn = src.fit_wind_scenarios(num, seed=33)
  torch.cuda.synchronize()
  assert scn.n_obs.cpu().numpy().tolist() == list(sizes) and _flags(src) == 0
  plans = rng.integers(0, 3, (h, n, k)).astype(np.uint8)
  before = {name: t.clone() for name, t in src.state.items()}
  before.update(episode_cache=src.episode_cache.clone(), noise_cache=src._noise_cache.clone(), slab=scn.slab.clone(), n_obs=scn.n_obs.clone(),
                episode=src.episode.clone(), **{'gp_' + key: t.clone() for key, t in src._gp.items()})
  out = src.rollout_plans(_dev(plans), gamma=gamma, action_repeat=repeat, substeps=substeps, want_rewards=True, want_final=True,
                          scenarios=scn)
  torch.cuda.synchronize()
  after = dict(src.state, episode_cache=src.episode_cache, noise_cache=src._noise_cache, slab=scn.slab, n_obs=scn.n_obs,
               episode=src.episode, **{'gp_' + key: t for key, t in src._gp.items()})
  for name, t in before.items():                     # the source, its caches and the slab: byte for byte
    assert torch.equal(t.view(torch.uint8), after[name].view(torch.uint8)), (case, name)
  assert _flags(src) == 0
  rewards, flown, final = _reference(src, scn, plans, repeat, substeps)
  assert out.returns.shape == (n, k, num) and out.steps_flown.shape == (n, k, num) and out.rewards.shape == (h * repeat, n, k, num)
  assert np.array_equal(out.steps_flown.cpu().numpy(), flown), case
  bad = np.argwhere(_bits(out.rewards.cpu().numpy()) != _bits(rewards))
  assert bad.size == 0, (case, 'rewards', bad[:4].tolist())
  bad = np.argwhere(_bits(out.final.cpu().numpy()) != _bits(final))
  assert bad.size == 0, (case, 'final', bad[:4].tolist())
  want, got = _host_returns(rewards, gamma), out.returns.cpu().numpy()
  err = np.abs(got.astype(np.float64) - want.astype(np.float64))
  ulp = np.spacing(np.abs(want)).astype(np.float64)
  print(f'{case}: returns max |diff| {err.max():.3e} = {np.max(err / ulp):.2f} ulp, exact in {np.mean(got == want):.3f}')
  assert np.all(err <= ulp), (case, 'returns', float(np.max(err / ulp)))
  # the scenarios are really flown: they end elsewhere than each other (M > 1) and than the forecast's flight
  calm = src.rollout_plans(_dev(plans), gamma=gamma, action_repeat=repeat, substeps=substeps, want_final=True)
  torch.cuda.synchronize()
  live = flown[:, 0, 0] > 0
  assert (np.abs(final[0][live] - calm.final.cpu().numpy()[0][live][..., None]) > 0).all(), case
  if num > 1:
    assert (final[0][live][..., 0] != final[0][live][..., 1]).all(), case
  if n == 5:
    assert (flown[1] == 0).all() and (flown[2] < h * repeat).all()


# ---------------------------------------------------------------------------------------------- 5. batch invariance
def _clone_env(src, e, offset=None, seeds=None):
  """Environment e of `src` as a simulator of one environment: at env_offset + e under a batch seed, anywhere under its own seed."""
  one = vec_state.VecSimulator(1, DEVICE, env_offset=(src.env_offset + e) if offset is None else offset)
  one.set_grid(src.grid.clone())
  for name, t in src.state.items():
    one.state[name].copy_(t[e:e + 1])
  one.episode.copy_(src.episode[e:e + 1])
  one.episode_cache.copy_(src.episode_cache[:, e:e + 1])
  one._allocate_history(False)
  for key, t in src._gp.items():
    one._gp[key].copy_(t[e:e + 1])
  return one


def test_batch_invariance():
  n, k, h, e = 4, 5, 3, 2
  src, rng = _source(n, 340, (17, 3, 120, 1), env_offset=3)
  src.episode[e] += 2                                 # (a later episode: the stream's episode word is the environment's own)
  plans = rng.integers(0, 3, (h, n, k)).astype(np.uint8)
  kw = dict(gamma=0.993, want_final=True)

  def fly(sim, p, **fit):
    scn = sim.fit_wind_scenarios(fit.pop('num', 3), **fit)
    out = sim.rollout_plans(_dev(p), scenarios=scn, **kw)
    torch.cuda.synchronize()
    return scn.slab.cpu().numpy(), out.returns.cpu().numpy(), out.final.cpu().numpy()

  slab, ret, final = fly(src, plans, seed=9)
  # alone, at the position env_offset says
  one = _clone_env(src, e)
  slab1, ret1, final1 = fly(one, plans[:, e:e + 1], seed=9)
  assert np.array_equal(slab1[0].view(np.uint64), slab[e].view(np.uint64))
  assert np.array_equal(_bits(ret1[0]), _bits(ret[e])) and np.array_equal(_bits(final1[:, 0]), _bits(final[:, e]))
  # ... and not the same at another position (the key is the global index)
  moved = _clone_env(src, e, offset=0)
  assert not np.array_equal(fly(moved, plans[:, e:e + 1], seed=9)[0][0, 480:], slab[e, 480:])
  # a seed per environment: the same bits in the batch, alone at any offset, and at another position of another batch
  seeds = np.array([101, 102, 103, 104], np.int64)
  slab_s, ret_s, final_s = fly(src, plans, seeds=_dev(seeds))
  for where in (moved, one):
    slab2, ret2, final2 = fly(where, plans[:, e:e + 1], seeds=_dev(seeds[e:e + 1]))
    assert np.array_equal(slab2[0].view(np.uint64), slab_s[e].view(np.uint64))
    assert np.array_equal(_bits(ret2[0]), _bits(ret_s[e])) and np.array_equal(_bits(final2[:, 0]), _bits(final_s[:, e]))
  assert not np.array_equal(slab_s[e, 480:], slab[e, 480:])
  perm = np.array([2, 0, 3, 1])                       # environment 2 flies at position 0 of a permuted seed tensor: its own seed decides
  other = _clone_env(src, e, offset=0)
  assert np.array_equal(fly(other, plans[:, e:e + 1], seeds=_dev(seeds[perm][:1]))[1][0].view(np.uint32), _bits(ret_s[e]))
  # another K: the first plans' returns do not move
  _, ret_k, _ = fly(src, np.ascontiguousarray(plans[:, :, :3]), seed=9)
  assert np.array_equal(_bits(ret_k), _bits(ret[:, :3]))
  # another M: scenario m is the same scenario
  slab16, ret16, final16 = fly(src, plans, seed=9, num=16)
  assert np.array_equal(slab16[:, :480 + 240 * 3].view(np.uint64), slab.view(np.uint64))
  assert np.array_equal(_bits(ret16[..., :3]), _bits(ret)) and np.array_equal(_bits(final16[..., :3]), _bits(final))
  assert len({ret16[0, 0, m].tobytes() + final16[0, 0, 0, m].tobytes() for m in range(16)}) == 16


# ---------------------------------------------------------------------------------------------- 6. the risk score
@pytest.mark.parametrize('num', [1, 3, 16])
def test_risk_against_the_twin(num):
  rng = np.random.default_rng(70 + num)
  n, k = 7, 41                                        # 287 lanes: a workgroup and a ragged tail
  sim = vec_state.VecSimulator(n, DEVICE)
  ret = rng.normal(0.0, 3.0, (n, k, num)).astype(np.float32)
  ret[0] = np.round(ret[0])                           # ties
  ret[1, :, :] = 1.5                                  # all equal
  ret[2] = np.where(rng.random((k, num)) < 0.5, np.float32(0.0), np.float32(-0.0))          # signed zeros only
  ret[3] = np.where(rng.random((k, num)) < 0.3, np.float32(-0.0), np.round(ret[3]))
  ret[4, 0, 0] = np.nan; ret[4, 1, num - 1] = np.inf; ret[4, 2, num // 2] = -np.inf
  ret[5] = (20.0 + 1e-3 * ret[5]).astype(np.float32)  # nearly equal: the order of the fp64 sum shows
  for tail in sorted({1, min(2, num), num}):
    got = sim.plan_risk(_dev(ret), tail)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = sh.risk_scores(ret, tail)
    assert np.isnan(got[4, :3]).all() and np.isnan(want[4, :3]).all() and np.isfinite(got[4, 3:]).all()
    assert np.array_equal(_bits(got), _bits(want)), (num, tail, np.argwhere(_bits(got) != _bits(want))[:4].tolist())
  assert np.array_equal(_bits(sim.plan_risk(_dev(ret)).cpu().numpy()), _bits(sh.risk_scores(ret, num)))          # None: the expectation
  with pytest.raises(ValueError, match='tail'):
    sim.plan_risk(_dev(ret), num + 1)


# ---------------------------------------------------------------------------------------------- 7. the planner
def _env(n, seed=3, steps=3):
  env = balloon_env.VecBalloonEnv(n, seed=seed, wind_noise=True, auto_reset=False)
  env.reset()
  rng = np.random.default_rng(seed)
  for a in rng.integers(0, 3, (steps, n)).astype(np.uint8):
    env.step(_dev(a))
  return env


def _compose(env, agent, decision, prev_plan):
  """One decision as the twin's composition: sample -> scenario returns (from the device) -> risk -> select."""
  sim = env.arena.sim
  n, K, H = env.num_envs, agent.num_plans, agent.horizon
  best_return, best_plan, counts = None, None, None
  scn = sim.fit_wind_scenarios(agent.num_scenarios, seed=agent.seed)
  for it in range(agent.iterations):
    plans = plan_host.sample(n, K, H, agent.segment, it, decision, seed=agent.seed, counts=counts, best_plan=prev_plan)
    ret = sim.rollout_plans(_dev(plans), agent.gamma, agent.action_repeat, scenarios=scn).returns
    torch.cuda.synchronize()
    score = sh.risk_scores(ret.cpu().numpy(), agent.risk_tail)
    last = it + 1 == agent.iterations
    best_return, best_k, best_plan, action, counts = plan_host.select(score, plans, it, 0 if last else agent.elite, agent.segment,
                                                                      best_return=best_return, best_plan=best_plan)
  return best_return, best_k, best_plan, action


def test_act_equals_the_composition():
  n = 9
  env = _env(n)
  env.arena.sim.state['status'][2] = 2                       # one environment is not OK: it flies nothing and gets STAY
  agent = env.planner(num_plans=5, horizon=3, segment=2, action_repeat=2, wind='scenarios', num_scenarios=3, risk_tail=2, iterations=2,
                      elite=2, seed=5)
  prev = np.full((3, n), 1, np.uint8)
  rng = np.random.default_rng(1)
  for decision in range(3):
    action = agent.act(None).clone()
    torch.cuda.synchronize()
    got = (agent.best_return.cpu().numpy(), agent.best_k.cpu().numpy(), agent.best_plan.cpu().numpy(), action.cpu().numpy())
    want = _compose(env, agent, decision, prev)
    assert np.array_equal(_bits(got[0]), _bits(want[0])), decision
    for g, w, name in zip(got[1:], want[1:], ('best_k', 'best_plan', 'action')):
      assert np.array_equal(g, w), (decision, name)
    assert int(agent.counter.item()) == decision + 1 and got[3][2] == 1 and np.isfinite(got[0]).all()
    prev = got[2]
    env.step(_dev(np.where(rng.random(n) < 0.5, got[3], 1).astype(np.uint8)))
  env.check_errors()
  # env.lookahead(wind='scenarios'): the per-scenario returns and the score
  plans = _dev(rng.integers(0, 3, (3, n, 4)).astype(np.uint8))
  ro, score = env.lookahead(plans, wind='scenarios', num_scenarios=3, risk_tail=1)
  torch.cuda.synchronize()
  assert ro.returns.shape == (n, 4, 3) and score.shape == (n, 4)
  assert np.array_equal(_bits(score.cpu().numpy()), _bits(sh.risk_scores(ro.returns.cpu().numpy(), 1)))


def test_one_scenario_scores_its_return():
  env = _env(5, seed=4)
  agent = env.planner(num_plans=5, horizon=3, wind='scenarios', num_scenarios=1, risk_tail=None, seed=2)
  agent.act(None)
  torch.cuda.synchronize()
  assert agent.risk_tail == 1
  assert np.array_equal(_bits(agent.returns.cpu().numpy()), _bits(agent.scenario_returns.cpu().numpy()[..., 0] + np.float32(0.0)))
  assert np.array_equal(_bits(agent.best_return.cpu().numpy()), _bits(agent.returns.cpu().numpy().max(1)))


def test_graph_equals_eager_and_resume():
  n, decisions = 9, 3
  runs = {}
  for mode in ('eager', 'graph', 'resume'):
    env = _env(n, seed=9)
    agent = env.planner(num_plans=5, horizon=3, segment=2, iterations=2, elite=2, seed=2, wind='scenarios', num_scenarios=3, risk_tail=2)
    actions = torch.ones(n, dtype=torch.uint8, device=DEVICE)
    obs = torch.empty(n, 1099, dtype=torch.float32, device=DEVICE)

    def body():
      agent.act(None, out=actions)
      env._step_eager(actions, obs_out=obs)
    body()                                               # (lazy allocations happen here, in every mode)
    graph = dev.capture(env.device, body)[0] if mode == 'graph' else None
    log = []
    for d in range(decisions):
      if mode == 'resume' and d == 1:                    # a new agent picks the run up from the old one's state_dict
        saved = agent.state_dict()
        agent = env.planner(num_plans=5, horizon=3, segment=2, iterations=2, elite=2, seed=2, wind='scenarios', num_scenarios=3, risk_tail=2)
        agent.load_state_dict(saved)
      graph.replay() if graph is not None else body()
      torch.cuda.synchronize()
      log.append((actions.cpu().numpy().copy(), _bits(agent.best_return.cpu().numpy()).copy(), int(agent.counter.item()), obs.cpu().numpy().copy()))
    runs[mode] = log
    env.check_errors()
  for mode in ('graph', 'resume'):
    for d, (a, b) in enumerate(zip(runs['eager'], runs[mode])):
      assert a[2] == b[2] == d + 2, (mode, d)
      assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]), (mode, d)


def test_evaluator_flies_the_agent_seed_by_seed():
  suite = suites.EvaluationSuite(list(suites.get_eval_suite('small_eval').seeds[:4]), 4)
  make = lambda: lookahead_agent.VecLookaheadAgent(num_plans=5, horizon=3, wind='scenarios', num_scenarios=3, risk_tail=2)
  batch = eval_lib.eval_agent_vec(make(), suite)
  alone = eval_lib.eval_agent_vec(make(), suite, batch_size=1)
  for a, b in zip(batch, alone):
    assert dataclasses.asdict(a) == dataclasses.asdict(b), (a, b)
  assert [r.seed for r in batch] == [0, 1, 2, 3]


def test_refusals():
  with pytest.raises(ValueError, match='num_scenarios'):
    lookahead_agent.VecLookaheadAgent(wind='scenarios', num_scenarios=17)
  with pytest.raises(ValueError, match='risk_tail'):
    lookahead_agent.VecLookaheadAgent(wind='scenarios', num_scenarios=4, risk_tail=5)
  sim = vec_state.VecSimulator(3, DEVICE)
  with pytest.raises(ValueError, match='num_scenarios'):
    sim.fit_wind_scenarios(0)
  sim.set_grid(torch.zeros(*vec_state.GRID_SHAPE, device=DEVICE))
  scn = sim.fit_wind_scenarios(2)
  plans = torch.ones(2, 3, 4, dtype=torch.uint8, device=DEVICE)
  with pytest.raises(ValueError, match='three winds'):
    sim.rollout_plans(plans, scenarios=scn, noise_seed=1)
  fleet = balloon_env.VecBalloonEnv(3, seed=1, vehicles=[{}, {'envelope_mass': 75.0}], vehicle_index=[0, 1, 0], auto_reset=False)
  with pytest.raises(ValueError, match='fleet'):
    fleet.planner(wind='scenarios')
  with pytest.raises(ValueError, match='fleet'):
    fleet.arena.sim.rollout_plans(plans, scenarios=scn)
