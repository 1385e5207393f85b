"""Scenario winds on the host, no GPU: the NumPy twin (tests/scenario_host.py) against the host build of the lane functions
(tests/emul/scenario_emul.cpp) -- bit for bit where integers or one fixed fp64 order make that possible: the stream's words, the ranks,
the score -- the twin's own laws, the entry points' argument checks, and a stand-alone program over the same lane functions under
-fsanitize=address,undefined, run as a child process."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import scenario_host as sh
from descriptors_host import E_INVALID_ARG, _FAKE
from emul import belief_emul, scenario_emul
from balloon_learning_environment_amd import _abi, _lib
from helpers import observations

HERE = os.path.dirname(os.path.abspath(__file__))
STREAMS = [(0, 0, 0), (1, 0, 0), (77, 3, 2), (2 ** 64 - 1, 2 ** 33 + 5, 2 ** 32 - 1), (0x5EEDF00D ^ sh.SCENARIO_KEY, 9, 1)]


# ---------------------------------------------------------------------------------------------- the stream
@pytest.mark.parametrize('seed,key,episode', STREAMS)
def test_stream_twin_equals_emulation(seed, key, episode):
  for m in (0, 1, 7, 15):
    seeds, offsets = sh.harmonics(seed, key, episode, m)
    want = sh.words_of_harmonics(seeds, offsets)
    got = scenario_emul.draws(seed, key, episode, m)
    assert np.array_equal(got, want), (m, np.argwhere(got != want)[:4])
    for k in (0, 3, 9):          # the fit's own way to harmonic k
      assert np.array_equal(scenario_emul.harmonic(seed, key, episode, m, k), want[k]), (m, k)
    assert (np.abs(offsets) <= 1.0).all()
  # the twin's Philox and word order are the existing generator's: the truth's harmonics through the same functions
  assert np.array_equal(scenario_emul.truth_draws(seed, key, episode), sh.words_of_harmonics(*sh.truth_harmonics(seed, key, episode)))


def test_every_stream_is_distinct_from_the_truth_and_from_each_other():
  for seed, key, episode in STREAMS:
    truth = sh.words_of_harmonics(*sh.truth_harmonics(seed, key, episode)).reshape(-1)
    rows = [sh.words_of_harmonics(*sh.harmonics(seed, key, episode, m)).reshape(-1) for m in range(16)]
    for m, r in enumerate(rows):
      assert (r == truth).sum() <= 1, m                      # (50 words of 32 bits: one chance collision in 1e8 at most)
      for other in rows[:m]:
        assert (r == other).sum() <= 1, m
  # a seed whose XOR with the scenario constant is another seed's XOR with the truth's: the block counters still differ
  assert sh.SCENARIO_KEY != sh.TRUTH_KEY
  a = sh.stream_words(5 ^ sh.SCENARIO_KEY ^ sh.TRUTH_KEY, 1, 0, 0, 23)            # scenario 0 keyed like seed 5's truth
  assert np.array_equal(a, sh.stream_words(5, 1, 0, 0, 23, sh.TRUTH_KEY))          # (the one aliasing there is: another SEED's truth)
  assert not np.array_equal(sh.stream_words(5, 1, 0, 0, 23), sh.stream_words(5, 1, 0, 0, 23, sh.TRUTH_KEY))


def test_stream_depends_on_seed_key_episode_and_m_alone():
  """No argument for n, K, M or a position exists; what does exist moves the stream, and the two seed sources meet where they must."""
  assert list(inspect.signature(sh.harmonics).parameters) == ['seed', 'key', 'episode', 'm']
  base = sh.words_of_harmonics(*sh.harmonics(11, 4, 2, 3))
  for other in ((12, 4, 2, 3), (11, 5, 2, 3), (11, 4, 3, 3), (11, 4, 2, 4)):
    assert not np.array_equal(base, sh.words_of_harmonics(*sh.harmonics(*other))), other
  # environment e = 4 of a batch at offset 0 == environment 1 of a shard at offset 3 (key = env_offset + e)
  assert np.array_equal(base, scenario_emul.draws(11, 3 + 1, 2, 3))
  # scenario m is the same whatever M: its blocks are 32 m .. 32 m + 22, never another scenario's
  assert 23 <= sh.BLOCKS_PER_SCENARIO
  w = sh.stream_words(11, 4, 2, 0, 32 * 16)
  assert np.array_equal(w[4 * 32 * 3:4 * 32 * 3 + 90], sh.stream_words(11, 4, 2, 32 * 3, 23)[:90])


# ---------------------------------------------------------------------------------------------- the prior on the host build
def test_prior_component_by_component_and_against_the_oracle():
  rng = np.random.default_rng(3)
  q = 4000
  x, y = rng.uniform(-2e5, 2e5, q).astype(np.float32), rng.uniform(-2e5, 2e5, q).astype(np.float32)
  p, t = rng.uniform(5000, 14000, q).astype(np.float32), rng.integers(0, 48 * 3600, q).astype(np.int32)
  seeds, offsets = sh.harmonics(77, 1, 0, 5)
  uv, by = scenario_emul.prior(sh.words_of_harmonics(seeds, offsets), x, y, p, t)
  assert np.array_equal(uv.view(np.uint32), by.view(np.uint32))          # the fit's per-component form: the same bits
  want = sh.prior(seeds, offsets, x, y, p, t)
  assert np.abs(uv - want).max() < 2e-5                                  # tests/test_gpu_noise.py's bar for the host build
  assert 0.5 < uv.var() < 1.6


# ---------------------------------------------------------------------------------------------- the twin's laws
def _window(rng, m, seed=0, m_scn=3):
  ring = observations(rng, m, 180)
  w = sh.Window(tuple(np.asarray(a, np.float64) for a in ring), 180 * (m - 1))
  hs = [sh.harmonics(seed, 0, 0, k) for k in range(m_scn)]
  f = [sh.prior(s, o, w.xyp[:, 0], w.xyp[:, 1], w.xyp[:, 2], w.t.astype(np.int32)) for s, o in hs]
  return w, hs, f


@pytest.mark.parametrize('m', [1, 3, 17, 120])
def test_interpolation_and_linearity(m):
  rng = np.random.default_rng(m)
  w, hs, f = _window(rng, m)
  assert w.n_obs == m
  belief = w.belief_alpha()
  for (seeds, offsets), f_m in zip(hs, f):
    alpha = w.alpha(f_m)
    # interpolation: error_m(X_i) = y_i - 0.05 alpha^m_i
    at_x = f_m + w.correction(alpha, w.xyp, w.t)
    assert np.abs(at_x - (w.y - sh.NOISE2 * alpha)).max() < 1e-9
    # linearity: alpha^m + (K + 0.05 I)^-1 f_m(X) = alpha of the belief
    assert np.abs(alpha + w.solve(f_m) - belief).max() < 1e-9 * max(1.0, np.abs(belief).max())
  # an empty window: the correction is zero, a scenario is its prior
  empty = sh.Window((np.zeros((0, 3)), np.zeros(0), np.zeros((0, 2))), 0)
  assert empty.n_obs == 0 and not empty.correction(empty.alpha(np.zeros((0, 2))), np.zeros((4, 3)), np.zeros(4)).any()
  one = sh.scenario_wind(np.float32([[1.5, -0.0]]), np.zeros((1, 2)))
  assert one[0, 0] == np.float32(1.5) and one.dtype == np.float32


def test_correction_lane_function_equals_the_belief_mean():
  """gp_scenario_correction on scenario m of a scenario slab == gp_belief_mean on a belief slab holding the same alpha, bit for bit (one
  host build, the same loop), and both follow the twin's correction to the belief's host bar."""
  rng = np.random.default_rng(8)
  w, hs, f = _window(rng, 17)
  num = 3
  alphas = [w.alpha(f_m) for f_m in f]
  loc = np.column_stack([w.xyp, w.t])
  slab = np.zeros(480 + 240 * num)
  q = 64
  x, y = rng.uniform(-2e5, 2e5, q).astype(np.float32), rng.uniform(-2e5, 2e5, q).astype(np.float32)
  p, t = rng.uniform(5000, 14000, q).astype(np.float32), (180 * 16 + rng.integers(0, 6 * 3600, q)).astype(np.int32)
  for m, alpha in enumerate(alphas):
    belief = belief_emul.pack(loc, alpha)
    slab[:480] = belief[:480]
    slab[480 + 240 * m:480 + 240 * (m + 1)] = belief[480:720]
  for m, alpha in enumerate(alphas):
    got = scenario_emul.correction(slab, num, m, 17, x, y, p, t)
    want = belief_emul.mean(belief_emul.pack(loc, alpha), 17, np.column_stack([x, y, p]), t)
    assert np.array_equal(got.view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), m
    assert np.abs(got - w.correction(alpha, np.column_stack([x, y, p]), t)).max() < 1e-5
  assert not scenario_emul.correction(slab, num, 1, 0, x, y, p, t).view(np.uint32).any()          # n_obs 0: exactly +0.0f
  assert np.isnan(scenario_emul.correction(slab, num, 1, -1, x, y, p, t)).all()


# ---------------------------------------------------------------------------------------------- the risk score
def _rows(rng):
  yield np.float32([0.5])
  yield np.float32([1.0, 1.0, 1.0])                                       # ties: m ascending
  yield np.float32([0.0, -0.0, 0.0, -0.0, -1.0])                          # -0 == +0
  yield np.float32([3.0, -2.0, 3.0, -2.0, 0.25, 7.5, -2.0])
  for num in (2, 5, 8, 16):
    yield rng.normal(0, 3, num).astype(np.float32)
    yield np.round(rng.normal(0, 1, num)).astype(np.float32)               # many ties
    yield (rng.normal(0, 1, num) * 1e-3 + 20.0).astype(np.float32)          # nearly equal: the order of the fp64 sum shows


def test_risk_twin_equals_emulation_bit_for_bit():
  rng = np.random.default_rng(5)
  for ret in _rows(rng):
    order = sh.risk_order(ret)
    ranks = scenario_emul.risk_ranks(ret)
    assert np.array_equal(np.argsort(ranks, kind='stable'), order) and sorted(ranks) == list(range(len(ret))), ret
    for tail in range(1, len(ret) + 1):
      got, want = scenario_emul.risk_score(ret, tail), sh.risk_score(ret, tail)
      assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), (ret, tail, got, want)


def test_risk_laws():
  rng = np.random.default_rng(6)
  ret = rng.normal(0, 3, 16).astype(np.float32)
  # tail = M: the plain mean in the stated order
  total = 0.0
  for v in np.sort(ret.astype(np.float64), kind='stable'):
    total += v
  assert sh.risk_score(ret, 16) == np.float32(total / 16.0)
  assert sh.risk_score(ret, 1) == ret.min()                                 # tail = 1: the worst case
  scores = [sh.risk_score(ret, tail) for tail in range(1, 17)]
  assert all(a <= b for a, b in zip(scores, scores[1:]))                    # a longer tail never scores lower
  # ties break by m: the first of two equal returns has the smaller rank, and -0 ties with +0
  assert sh.risk_order(np.float32([2.0, 1.0, 1.0, -0.0, 0.0])).tolist() == [3, 4, 1, 2, 0]
  assert scenario_emul.risk_ranks(np.float32([2.0, 1.0, 1.0, -0.0, 0.0])).tolist() == [4, 2, 3, 0, 1]
  # a NaN or an Inf anywhere -- inside the tail or not -- gives NaN, in the twin and in the lane function
  for bad in (np.nan, np.inf, -np.inf):
    row = ret.copy(); row[int(np.argmax(ret))] = bad                        # the largest return: outside every tail < M
    for tail in (1, 2, 16):
      assert np.isnan(sh.risk_score(row, tail)) and np.isnan(scenario_emul.risk_score(row, tail)), (bad, tail)
  # M = 1: the score is the single scenario's return, bit for bit
  for v in np.float32([0.0, -0.0, 1.25, -3e-7, 700.0]):
    assert scenario_emul.risk_score(np.float32([v]), 1).view(np.uint32) == (np.float32(v) + np.float32(0.0)).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the stand-alone program
def test_lane_functions_under_the_sanitizers(tmp_path):
  exe = str(tmp_path / 'scenario_lanes')
  subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                         '-include', os.path.join(HERE, 'emul', 'ble_intrinsics.h'), '-o', exe, os.path.join(HERE, 'scenario_lanes_main.cpp')])
  run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
  assert run.returncode == 0 and run.stdout.startswith('ok ') and not run.stderr, (run.returncode, run.stdout[-400:], run.stderr[-2000:])


# ---------------------------------------------------------------------------------------------- the entry points' argument checks
def _scn(n, num=3, **kw):
  d = dict(slab=_FAKE, stride=_abi.gp_scenario_doubles(num), n_obs=_FAKE, n=n, num=num, reserved_=0)
  d.update(kw)
  return _abi.BleGpScenarios(**d)


def _gen(**kw):
  d = dict(seed=1, env_seed=None, episode=None, env_offset=0)
  d.update(kw)
  return _abi.BleScenarioGen(**d)


def _hist(null=None):
  h = _abi.BleGpHistoryF32()
  for name, ct in (('xyp', ctypes.c_float), ('elapsed_s', ctypes.c_int32), ('err_uv', ctypes.c_float), ('count', ctypes.c_int32)):
    setattr(h, name, ctypes.cast(ctypes.c_void_p(None if name == null else _FAKE), ctypes.POINTER(ct)))
  return h


def _state(null=None):
  return _abi.state_struct({name: 0 if name == null else _FAKE for name in _abi.FIELD_NAMES}, 0, None)


def _ro(n, **kw):
  d = dict(n=n, n_plans=5, n_plan_steps=3, action_repeat=1, substeps=18, gamma=0.99, plans=_FAKE, wind_grid=_FAKE, grid_env_stride=0,
           ret=_FAKE, steps_flown=_FAKE, reward=None, final_state=None)
  d.update(kw)
  return _abi.BleRolloutF32(**d)


def _risk(n, **kw):
  d = dict(n=n, n_plans=5, num=3, tail=2, reserved_=0, ret=_FAKE, score=_FAKE)
  d.update(kw)
  return _abi.BlePlanRisk(**d)


def _fit(n, hist=None, time_s=_FAKE, scn=None, gen=None, null_scn=False, null_gen=False):
  return _lib.lib().ble_gp_fit_scenarios_f32(ctypes.byref(hist or _hist()), None, time_s, None if null_scn else ctypes.byref(scn or _scn(n)),
                                             None if null_gen else ctypes.byref(gen or _gen()), None, None)


def _wind(n, scn=None, gen=None, index=_FAKE, x=_FAKE, uv=_FAKE, prior_only=0):
  return _lib.lib().ble_gp_scenario_wind_f32(ctypes.byref(scn or _scn(n)), ctypes.byref(gen or _gen()), index, x, _FAKE, _FAKE, _FAKE, prior_only,
                                             uv, None)


def _rollout(n, st=None, ro=None, scn=None, gen=None):
  return _lib.lib().ble_rollout_scenarios_f32(ctypes.byref(st or _state()), ctypes.byref(ro or _ro(n)), ctypes.byref(scn or _scn(n)),
                                              ctypes.byref(gen or _gen()), None, None)


def _score(n, **kw):
  return _lib.lib().ble_plan_risk_f32(ctypes.byref(_risk(n, **kw)), None)


_BAD_SCN = {'null_slab': dict(slab=None), 'null_n_obs': dict(n_obs=None), 'num_0': dict(num=0, stride=2000), 'num_17': dict(num=17, stride=8000),
            'stride_short': dict(stride=_abi.gp_scenario_doubles(3) - 2), 'stride_odd': dict(stride=_abi.gp_scenario_doubles(3) + 1),
            'stride_of_a_smaller_num': dict(num=4, stride=_abi.gp_scenario_doubles(3)), 'misaligned_slab': dict(slab=_FAKE + 8)}
_CASES = {
    **{f'fit_{k}': (lambda n, v=v: _fit(n, scn=_scn(n, **v))) for k, v in _BAD_SCN.items()},
    **{f'wind_{k}': (lambda n, v=v: _wind(n, scn=_scn(n, **v))) for k, v in _BAD_SCN.items()},
    **{f'rollout_{k}': (lambda n, v=v: _rollout(n, scn=_scn(n, **v))) for k, v in _BAD_SCN.items()},
    **{f'fit_null_hist_{f}': (lambda n, f=f: _fit(n, hist=_hist(null=f))) for f in ('xyp', 'elapsed_s', 'err_uv', 'count')},
    'fit_null_time_s': lambda n: _fit(n, time_s=None),
    'fit_null_scn': lambda n: _fit(n, null_scn=True),
    'fit_null_gen': lambda n: _fit(n, null_gen=True),
    'fit_negative_env_offset': lambda n: _fit(n, gen=_gen(env_offset=-1)),
    'wind_negative_env_offset': lambda n: _wind(n, gen=_gen(env_offset=-1)),
    'wind_null_index': lambda n: _wind(n, index=None),
    'wind_null_x': lambda n: _wind(n, x=None),
    'wind_null_uv': lambda n: _wind(n, uv=None),
    'wind_prior_only_2': lambda n: _wind(n, prior_only=2),
    'rollout_null_state_field': lambda n: _rollout(n, st=_state(null='pressure')),
    'rollout_null_plans': lambda n: _rollout(n, ro=_ro(n, plans=None)),
    'rollout_null_ret': lambda n: _rollout(n, ro=_ro(n, ret=None)),
    'rollout_null_steps_flown': lambda n: _rollout(n, ro=_ro(n, steps_flown=None)),
    'rollout_null_grid': lambda n: _rollout(n, ro=_ro(n, wind_grid=None)),
    'rollout_plans_0': lambda n: _rollout(n, ro=_ro(n, n_plans=0)),
    'rollout_too_many_steps': lambda n: _rollout(n, ro=_ro(n, n_plan_steps=481, action_repeat=2)),
    'rollout_substeps_0': lambda n: _rollout(n, ro=_ro(n, substeps=0)),
    'rollout_gamma_nan': lambda n: _rollout(n, ro=_ro(n, gamma=float('nan'))),
    'rollout_negative_stride': lambda n: _rollout(n, ro=_ro(n, grid_env_stride=-1)),
    'rollout_scenarios_of_another_batch': lambda n: _rollout(n, scn=_scn(n + 1)),
    'rollout_negative_env_offset': lambda n: _rollout(n, gen=_gen(env_offset=-1)),
    'rollout_lanes_past_int32': lambda n: _rollout(2 ** 20, ro=_ro(2 ** 20, n_plans=1024), scn=_scn(2 ** 20, num=3)),
    'risk_null_ret': lambda n: _score(n, ret=None),
    'risk_null_score': lambda n: _score(n, score=None),
    'risk_plans_0': lambda n: _score(n, n_plans=0),
    'risk_plans_1025': lambda n: _score(n, n_plans=1025),
    'risk_num_0': lambda n: _score(n, num=0, tail=0),
    'risk_num_17': lambda n: _score(n, num=17),
    'risk_tail_0': lambda n: _score(n, tail=0),
    'risk_tail_above_num': lambda n: _score(n, tail=4),
    'risk_lanes_past_int32': lambda n: _score(2 ** 20, n_plans=1024, num=3),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  assert _CASES[case](n) == E_INVALID_ARG


def test_valid_arguments_and_no_environments():
  assert _fit(0) == 0 and _wind(0) == 0 and _wind(0, prior_only=1) == 0 and _rollout(0) == 0 and _score(0) == 0
  assert _fit(0, gen=_gen(env_seed=_FAKE)) == 0
  for entry in (_fit, _wind, _rollout, _score):
    assert entry(-1) == E_INVALID_ARG
  assert _lib.lib().ble_plan_risk_f32(None, None) == E_INVALID_ARG
  assert _abi.gp_scenario_doubles(16) == 4320 and _abi.SCENARIO_MAX == 16
  for name in ('ble_gp_fit_scenarios_f32', 'ble_gp_scenario_wind_f32', 'ble_rollout_scenarios_f32', 'ble_plan_risk_f32'):
    assert name in _lib.EXPORTS and name in _lib.ADDITIVE_EXPORTS


def test_python_signatures():
  from balloon_learning_environment_amd import vec_state
  from balloon_learning_environment_amd.agents import lookahead_agent
  from balloon_learning_environment_amd.env import balloon_arena, balloon_env
  assert vec_state.WindScenarios._fields[:3] == ('slab', 'n_obs', 'num')
  p = inspect.signature(vec_state.VecSimulator.fit_wind_scenarios).parameters
  assert list(p) == ['self', 'num_scenarios', 'seed', 'seeds', 'time_s', 'out']
  p = inspect.signature(vec_state.VecSimulator.scenario_wind).parameters
  assert list(p)[:8] == ['self', 'scn', 'm', 'x', 'y', 'pressure', 'elapsed_s', 'prior_only'] and p['prior_only'].default is False
  assert inspect.signature(vec_state.VecSimulator.rollout_plans).parameters['scenarios'].default is None
  for name in ('fit_wind_scenarios', 'scenario_wind', 'plan_risk'):
    assert callable(getattr(balloon_arena.VecBalloonArena, name))
  p = inspect.signature(balloon_env.VecBalloonEnv.lookahead).parameters
  assert p['num_scenarios'].default == 8 and p['risk_tail'].default is None
  p = inspect.signature(lookahead_agent.VecLookaheadAgent.__init__).parameters
  assert p['num_scenarios'].default == 8 and p['risk_tail'].default is None and 'scenarios' in lookahead_agent.WINDS
