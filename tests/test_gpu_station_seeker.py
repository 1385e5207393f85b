"""ble_station_seeker_f32 (csrc/ble_agent.h) and the agents/ mirror against the reference's StationSeeker.

F13 holds the reference agent's chosen level and action for the 960 observations it flew; oracle/station_seeker_oracle.py restates
its scores (pinned to those 960 decisions by tests/test_oracle_golden.py).  The kernel is checked against both, on a randomised batch
with invalid masks, a sweep of the distance feature and constructed exact ties, and on its error and batch-shape edges.
"""
import numpy as np
import pytest
import torch

import helpers
import station_seeker_oracle as sso

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ssa():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd.agents import station_seeker_agent
  return station_seeker_agent


def _run(ssa, feats, stride=None, err_flags=None):
  """(actions, levels, scores) of the kernel on host float32 rows; `stride`: rows padded to that many floats (padding NaN)."""
  feats = np.ascontiguousarray(feats, np.float32)
  n = feats.shape[0]
  if stride is None:
    obs = torch.from_numpy(feats).cuda()
  else:
    buf = torch.full((n, stride), float('nan'), dtype=torch.float32, device='cuda')
    buf[:, :1099] = torch.from_numpy(feats).cuda()
    obs = buf[:, :1099]
  agent = ssa.VecStationSeekerAgent(err_flags=err_flags)
  level = torch.empty(n, dtype=torch.int32, device='cuda')
  scores = torch.empty(n, 361, dtype=torch.float64, device='cuda')
  action = agent.act(obs, level=level, scores=scores)
  return action.cpu().numpy(), level.cpu().numpy(), scores.cpu().numpy(), agent


def _invalid(f):
  w = f[16:].reshape(361, 3)
  return (w[:, 0] == 0) & (w[:, 1] == 1) & (w[:, 2] == 1)


def test_f13_levels_actions_and_scores(ssa):
  g = helpers.golden('f13_station_seeker')
  n = int(g['n_flown'])
  feats = g['features'][0, :n]
  action, level, scores, agent = _run(ssa, feats)
  agent.check_errors()
  np.testing.assert_array_equal(level, g['levels'][:n])
  np.testing.assert_array_equal(action, g['actions'][0])
  worst = 0.0
  for i in range(n):
    want = sso.scores(feats[i])
    inv = _invalid(feats[i])
    assert (scores[i][inv] == 0.0).all(), i
    rel = np.abs(scores[i][~inv] - want[~inv]) / np.abs(want[~inv])
    worst = max(worst, float(rel.max()))
  assert worst <= 1e-13, worst
  print(f'F13: 960/960 levels and actions equal; worst score rel err {worst:.2e}')


def _random_batch(n, seed):
  """Observations built from F11 / F13 vectors: random invalid masks, the distance feature swept over the bearing ramp, and
  constructed exact ties (levels 180 - k and 180 + k identical and best).  Returns (features, tie rows)."""
  rng = np.random.default_rng(seed)
  pool = np.concatenate([helpers.golden('f13_station_seeker')['features'][0],
                         helpers.golden('f11_features')['features'].reshape(-1, 1099)]).astype(np.float32)
  f = pool[rng.integers(0, len(pool), n)].copy()
  w = f[:, 16:].reshape(n, 361, 3)
  for i in np.nonzero(rng.random(n) < 0.5)[0]:                # random invalid masks, sparse to almost all
    m = rng.random(361) < rng.choice([0.05, 0.5, 0.97])
    w[i, m] = (0.0, 1.0, 1.0)
    w[i, int(rng.integers(0, 361))] = (0.3, 0.3, 0.3)           # (at least one valid level)
  dist_km = rng.uniform(0.0, 650.0, n)                        # through the 250 .. 500 km ramp of the bearing weight
  dist_km[rng.random(n) < 0.1] = 0.0
  f[:, 7] = (dist_km / (250.0 + dist_km)).astype(np.float32)
  ties = np.nonzero(rng.random(n) < 0.05)[0]
  for i in ties:
    k = int(rng.integers(1, 181))
    w[i, :, :] = (0.2, 0.6, 0.7)                               # every other level clearly worse
    w[i, 180 - k] = w[i, 180 + k] = (0.0, 0.05, 0.1)
  f[:, 16:] = w.reshape(n, -1)
  return f, ties


def test_randomised_batch(ssa):
  n = 4097
  f, ties = _random_batch(n, 11)
  action, level, _, agent = _run(ssa, f)
  agent.check_errors()
  excluded = 0
  for i in range(n):
    s = sso.scores(f[i])
    best = sso.best_level(f[i])
    top = np.sort(s)[::-1]
    margin = top[0] - top[1]
    if i in ties:
      assert margin == 0.0 and best < 180, i
    if 0.0 < margin <= 1e-12 * top[0]:
      assert i not in ties
      excluded += 1
      continue
    assert level[i] == best, (i, level[i], best)
    assert action[i] == (2 if best < 180 else (0 if best > 180 else 1)), i
  assert excluded < n // 100
  print(f'randomised batch of {n}: {len(ties)} constructed exact ties, {excluded} near-ties excluded')


def test_no_valid_level_and_nonfinite_raise(ssa):
  from balloon_learning_environment_amd import vec_state
  g = helpers.golden('f13_station_seeker')
  f = np.repeat(g['features'][0, :1], 4, axis=0).astype(np.float32)
  f[1, 16:] = np.tile([0.0, 1.0, 1.0], 361)                    # no valid level
  f[2, 16 + 3 * 200] = np.nan                                  # a non-finite feature
  f[3, 7] = np.inf
  sim = vec_state.VecSimulator(1)
  action, level, _, _ = _run(ssa, f, err_flags=sim.err_flags)
  assert list(level[1:]) == [-1, -1, -1] and list(action[1:]) == [1, 1, 1]
  assert level[0] == g['levels'][0]
  with pytest.raises(AssertionError):
    sim.check_errors()
  sim.check_errors()                                           # cleared
  action, level, _, _ = _run(ssa, f[2:3], err_flags=sim.err_flags)
  assert level[0] == -1 and action[0] == 1
  with pytest.raises(AssertionError):
    sim.check_errors()


def test_batch_shapes_and_padded_rows(ssa):
  f, _ = _random_batch(4097, 12)
  want = _run(ssa, f)
  for n in (1, 63, 64, 65, 4097):
    for stride in (None, 1104):
      got = _run(ssa, f[:n], stride=stride)
      for a, b in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(a, b[:n], err_msg=f'n={n} stride={stride}')


def test_mirror_reference_cases(ssa):
  """agents/station_seeker_agent_test.py of the reference, restated, and find_best_pressure_level on F13."""
  from balloon_learning_environment_amd.env import features
  agent = ssa.StationSeekerAgent(3, (3, 4))
  assert agent.get_name() == 'StationSeekerAgent'
  mock_observation = np.zeros(1099)
  for _ in range(10):
    assert agent.begin_episode(mock_observation) == 1
    for _ in range(20):
      assert agent.step(0.0, mock_observation) == 1
  agent.end_episode(0.0, True)
  g = helpers.golden('f13_station_seeker')
  for i in range(0, 960, 7):
    level, scores = agent.find_best_pressure_level(features.NamedPerciatelliFeatures(g['features'][0, i]))
    assert level == g['levels'][i], i
    assert scores.shape == (361,)
    assert agent.pick_action(g['features'][0, i]) == g['actions'][0, i]
  f = np.tile([0.0, 1.0, 1.0], 361)
  with pytest.raises(AssertionError):
    agent.pick_action(np.concatenate([np.zeros(16), f]))
