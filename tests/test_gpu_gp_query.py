"""ble_gp_query_f32 / VecSimulator.query_wind against the host twin (tests/wind_gp_host.py), fed the ring's own float32 values read
back from the device.

Tolerance: the project's bar, 1e-5 absolute on the mean [m/s] and on the deviation.  The outputs are float32: a mean of a
few m/s rounds by 2.4e-7, a mean + forecast of up to 34 m/s by 1.9e-6, a deviation <= 1 by 6e-8 -- all well inside the bar; the fp64
algebra at cond(K) ~ 3e4 contributes ~1e-11.  The forecast grid is synthetic with |u|, |v| <= 30 m/s.

The rings are written directly into the simulator's ring tensors (random positions, pressures and errors, regular spacing), so that
every window size around the 16-row MFMA tile and the 64-lane wave comes up in ONE launch; the host reference of a ring is computed
once per module and shared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import wind_gp_host
from helpers import observations as _observations, ring_back as _ring_back, write_ring as _write_ring
from balloon_learning_environment_amd import _lib, device as dev, vec_state
from balloon_learning_environment_amd.env import balloon_env
from balloon_learning_environment_amd.env import wind_field
from balloon_learning_environment_amd.utils import units

pytestmark = pytest.mark.gpu

TOL = 1e-5
CAP = 128
SIZES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 119, 120)
Q_MAX = 181
N_COLUMNS = 8          # the query points of an environment stand in 8 columns (x, y): the host twin answers one column per call


class _NoForecast(wind_field.WindField):
  def __init__(self):
    pass

  def reset_forecast(self, key, date_time):
    pass

  def get_forecast(self, x, y, pressure, elapsed_time):
    return wind_field.WindVector(units.Velocity(mps=0.0), units.Velocity(mps=0.0))


def _host(ring, points, tq, newest=None):
  """The host twin's posterior at `points` [q, 3] (float32 values) and time tq from a ring read back from the device: (mean [q, 2],
  deviation [q], observations in the window).  newest: keep only that many newest observations of the window."""
  xyp, t, err = ring
  keep = np.flatnonzero(np.abs(t - float(tq)) < 6 * 3600)
  if newest is not None:
    keep = keep[-newest:]
  gp = wind_gp_host.WindGP(_NoForecast())
  gp.measurement_locations = [np.array([xyp[i, 0], xyp[i, 1], xyp[i, 2], t[i]]) for i in keep]
  gp.error_values = [err[i].copy() for i in keep]
  points = np.asarray(points, np.float64)
  mean, dev_ = np.zeros((len(points), 2)), np.zeros(len(points))
  columns = {}
  for j, p in enumerate(points):
    columns.setdefault((p[0], p[1]), []).append(j)
  for (x, y), idx in columns.items():
    loc = np.column_stack([np.full(len(idx), x), np.full(len(idx), y), points[idx, 2], np.full(len(idx), float(tq))])
    mean[idx], dev_[idx] = gp.query_batch(loc)
  return mean, dev_, len(keep)


def _points(rng, n, q):
  """[n, q, 3] float32 query points in N_COLUMNS columns per environment."""
  cols = rng.uniform(-2.5e5, 2.5e5, (n, N_COLUMNS, 2))
  pick = rng.integers(0, N_COLUMNS, (n, q))
  xy = np.take_along_axis(cols, pick[..., None].repeat(2, -1), 1)
  return np.concatenate([xy, rng.uniform(4000.0, 15000.0, (n, q, 1))], -1).astype(np.float32)


def _sim(n, grid=None, per_env=False):
  sim = vec_state.VecSimulator(n, 'cuda:0')
  if grid is not None:
    sim.set_grid(grid, per_env=per_env)
  sim._allocate_history(False)
  return sim


def _query(sim, pts, time_s=None, add_forecast=False):
  xyp = torch.from_numpy(np.ascontiguousarray(pts)).to(sim.device)
  t = None if time_s is None else torch.tensor(np.asarray(time_s, np.int32), dtype=torch.int32, device=sim.device)
  mean, dev_ = sim.query_wind(xyp, t, add_forecast=add_forecast)
  torch.cuda.synchronize()
  return mean.cpu().numpy().astype(np.float64), dev_.cpu().numpy().astype(np.float64)


def _flags(sim, clear=True):
  word = int(sim.err_flags.item())
  if clear:
    sim.err_flags.zero_()
  return word


def _close(got, want, what):
  err = float(np.max(np.abs(got - want))) if got.size else 0.0
  print(f'{what}: max |device - host| = {err:.3e}')
  assert np.isfinite(got).all(), what
  assert err <= TOL, (what, err)


# ---------------------------------------------------------------------------------------------- window sizes
@functools.lru_cache(maxsize=None)
def _sizes_case():
  """11 environments whose rings hold SIZES observations at 180 s spacing, queried now at 181 points: the simulator, the points, the
  times and the host posterior (once for the module)."""
  rng = np.random.default_rng(20)
  sim = _sim(len(SIZES))
  for e, m in enumerate(SIZES):
    _write_ring(sim, e, _observations(rng, m, 180))
  pts = _points(rng, len(SIZES), Q_MAX)
  now = np.array([180 * max(m - 1, 0) for m in SIZES], np.int32)
  host = [_host(_ring_back(sim, e), pts[e], now[e]) for e in range(len(SIZES))]
  assert [h[2] for h in host] == list(SIZES)
  return sim, pts, now, host


@pytest.mark.parametrize('q', [1, 15, 16, 17, 33, 181])
def test_window_sizes_across_tile_and_wave_edges(q):
  sim, pts, now, host = _sizes_case()
  mean, dev_ = _query(sim, pts[:, :q], now)
  assert _flags(sim) == 0
  for e, m in enumerate(SIZES):
    _close(mean[e], host[e][0][:q], f'm={m} q={q} mean')
    _close(dev_[e], host[e][1][:q], f'm={m} q={q} deviation')
  assert (mean[0] == 0).all() and (dev_[0] == 0).all()            # the empty model: zero error, zero deviation


def test_ring_wrap_around():
  """count = 200: observations 72 .. 199 sit in slots 72 .. 127, 0 .. 71; the window of the newest 120 straddles slot 0, and the oldest
  ring entry (22 860 s old) is outside it."""
  rng = np.random.default_rng(21)
  sim = _sim(2)
  _write_ring(sim, 0, _observations(rng, 200, 180))
  _write_ring(sim, 1, _observations(rng, 40, 180))
  pts = _points(rng, 2, 33)
  now = [180 * 199, 180 * 39]
  mean, dev_ = _query(sim, pts, now)
  assert _flags(sim) == 0
  for e, want_m in ((0, 120), (1, 40)):
    hm, hd, m = _host(_ring_back(sim, e), pts[e], now[e])
    assert m == want_m
    _close(mean[e], hm, f'wrap env {e} mean')
    _close(dev_[e], hd, f'wrap env {e} deviation')


@pytest.mark.parametrize('offset,want_m', [(0, 100), (7200, 80), (-1200, 100)], ids=['now', 'plus_2h', 'minus_20min'])
def test_query_times(offset, want_m):
  """100 observations at 180 s: now and 20 min ago see all of them, two hours ahead only those younger than 6 h then."""
  rng = np.random.default_rng(22)
  sim = _sim(2)
  _write_ring(sim, 0, _observations(rng, 100, 180))
  _write_ring(sim, 1, _observations(rng, 30, 180))
  pts = _points(rng, 2, 17)
  tq = [180 * 99 + offset, 180 * 29]
  mean, dev_ = _query(sim, pts, tq)
  assert _flags(sim) == 0
  hm, hd, m = _host(_ring_back(sim, 0), pts[0], tq[0])
  assert m == want_m
  _close(mean[0], hm, f'offset {offset} mean')
  _close(dev_[0], hd, f'offset {offset} deviation')


def test_time_defaults_to_each_environments_clock():
  rng = np.random.default_rng(23)
  sim = _sim(2)
  _write_ring(sim, 0, _observations(rng, 20, 180))
  _write_ring(sim, 1, _observations(rng, 64, 180))
  sim.state['time_elapsed_s'].copy_(torch.tensor([180 * 19, 180 * 63], dtype=torch.int32))
  pts = _points(rng, 2, 5)
  a = _query(sim, pts)
  b = _query(sim, pts, [180 * 19, 180 * 63])
  assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and _flags(sim) == 0


# ---------------------------------------------------------------------------------------------- forecast
def _forecast(sim, pts, time_s):
  """ble_forecast_f32 at the query points: [n, q, 2] float64 (one grid for all, or -- q == 1 -- a grid per environment)."""
  n, q = pts.shape[:2]
  assert sim.grid_env_stride == 0 or q == 1
  flat = torch.from_numpy(np.ascontiguousarray(pts.reshape(n * q, 3).T)).to(sim.device).contiguous()
  t = torch.from_numpy(np.repeat(np.asarray(time_s, np.int32), q)).to(sim.device)
  u = torch.empty(n * q, dtype=torch.float32, device=sim.device)
  v = torch.empty(n * q, dtype=torch.float32, device=sim.device)
  _lib.check(sim.lib.ble_forecast_f32(sim.grid.data_ptr(), sim.grid_env_stride, flat[0].data_ptr(), flat[1].data_ptr(), flat[2].data_ptr(),
                                      t.data_ptr(), u.data_ptr(), v.data_ptr(), n * q, dev.stream_ptr(sim.device)), 'ble_forecast_f32')
  torch.cuda.synchronize()
  return np.stack([u.cpu().numpy(), v.cpu().numpy()], -1).astype(np.float64).reshape(n, q, 2)


@pytest.mark.parametrize('per_env,q', [(False, 33), (True, 1)], ids=['shared_grid', 'per_env_grids'])
def test_forecast_is_added(per_env, q):
  rng = np.random.default_rng(24)
  n = 3
  shape = ((n,) if per_env else ()) + vec_state.GRID_SHAPE
  sim = _sim(n, rng.uniform(-30.0, 30.0, shape).astype(np.float32), per_env)
  for e, m in enumerate((50, 0, 120)):
    _write_ring(sim, e, _observations(rng, m, 180))
  pts = _points(rng, n, q)
  pts[..., 0:2] *= 0.5                      # inside the grid's +-500 km
  tq = [180 * 49 + 600, 3600, 180 * 119]
  plain = _query(sim, pts, tq, add_forecast=False)
  with_fc = _query(sim, pts, tq, add_forecast=True)
  fc = _forecast(sim, pts, tq)
  assert _flags(sim) == 0 and np.abs(fc).max() > 1.0
  _close(with_fc[0], plain[0] + fc, 'mean + forecast')
  assert (with_fc[1] == plain[1]).all()
  _close(with_fc[0][1], fc[1], 'empty history: the forecast alone')
  assert (with_fc[1][1] == 0).all()


# ---------------------------------------------------------------------------------------------- flags
def test_more_than_120_in_the_window_keeps_the_newest_120():
  rng = np.random.default_rng(25)
  sim = _sim(3)
  _write_ring(sim, 0, _observations(rng, 50, 180))
  _write_ring(sim, 1, _observations(rng, 130, 60))
  _write_ring(sim, 2, _observations(rng, 120, 180))
  pts = _points(rng, 3, 17)
  now = [180 * 49, 60 * 129, 180 * 119]
  mean, dev_ = _query(sim, pts, now)
  assert _flags(sim) == _lib.FLAG_GP_WINDOW
  for e in range(3):
    hm, hd, m = _host(_ring_back(sim, e), pts[e], now[e], newest=120)
    assert m == (50, 120, 120)[e]
    _close(mean[e], hm, f'env {e} mean')
    _close(dev_[e], hd, f'env {e} deviation')
  assert _flags(sim) == 0                    # zeroed above, and nothing sets it again without a launch
  sim.err_flags.fill_(_lib.FLAG_GP_WINDOW)
  with pytest.raises(OverflowError):
    sim.check_errors()
  assert _flags(sim) == 0


def test_evicted_observations_in_the_window_answer_nan():
  """count = 300 at 180 s, asked about an hour ago: the window reaches back past the oldest ring entry, to observations the ring has
  evicted -- NaN for that environment alone, and the flag."""
  rng = np.random.default_rng(26)
  sim = _sim(3)
  _write_ring(sim, 0, _observations(rng, 60, 180))
  _write_ring(sim, 1, _observations(rng, 300, 180))
  _write_ring(sim, 2, _observations(rng, 100, 180))
  pts = _points(rng, 3, 33)
  tq = [180 * 59 - 3600, 180 * 299 - 3600, 180 * 99 - 3600]
  mean, dev_ = _query(sim, pts, tq)
  assert _flags(sim) == _lib.FLAG_GP_WINDOW
  assert np.isnan(mean[1]).all() and np.isnan(dev_[1]).all()
  for e in (0, 2):
    hm, hd, _ = _host(_ring_back(sim, e), pts[e], tq[e])
    _close(mean[e], hm, f'env {e} mean')
    _close(dev_[e], hd, f'env {e} deviation')
  assert _flags(sim) == 0


# ---------------------------------------------------------------------------------------------- pending reset
def test_pending_history_restart():
  rng = np.random.default_rng(27)
  n = 4
  sim = _sim(n, rng.uniform(-30.0, 30.0, vec_state.GRID_SHAPE).astype(np.float32))
  for e in range(n):
    _write_ring(sim, e, _observations(rng, 30 + 10 * e, 180))
  pts = _points(rng, n, 17)
  pts[..., 0:2] *= 0.5
  now = [180 * (29 + 10 * e) for e in range(n)]
  before = _query(sim, pts, now, add_forecast=True)
  sim.reset_observation_history(torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device=sim.device))
  after = _query(sim, pts, now, add_forecast=True)
  fc = _forecast(sim, pts, now)
  assert _flags(sim) == 0
  for e in (0, 2):
    assert (after[0][e] == before[0][e]).all() and (after[1][e] == before[1][e]).all()
    assert (before[1][e] > 0).all()
  for e in (1, 3):
    _close(after[0][e], fc[e], f'env {e}: the forecast alone')
    assert (after[1][e] == 0).all()


def test_before_any_observe_allocates_no_history():
  rng = np.random.default_rng(28)
  sim = vec_state.VecSimulator(3, 'cuda:0')
  sim.set_grid(rng.uniform(-30.0, 30.0, vec_state.GRID_SHAPE).astype(np.float32))
  pts = _points(rng, 3, 5)
  pts[..., 0:2] *= 0.5
  mean, dev_ = _query(sim, pts, [0, 600, 7200], add_forecast=True)
  assert sim._gp is None and _flags(sim) == 0
  _close(mean, _forecast(sim, pts, [0, 600, 7200]), 'no history: the forecast alone')
  assert (dev_ == 0).all()


# ---------------------------------------------------------------------------------------------- read-only, no cross-talk
def _gp_bits(env):
  gp = env.arena.sim.state_dict()['gp']
  return {k: t.cpu() for k, t in gp.items()}


def test_read_only_and_no_cross_talk():
  n, steps, more = 4, 12, 5
  rng = np.random.default_rng(29)
  actions = torch.from_numpy(rng.integers(0, 3, (steps + more, n)).astype(np.uint8)).cuda()
  envs = [balloon_env.VecBalloonEnv(n, seed=11, wind_noise=True) for _ in range(2)]
  for env in envs:
    env.reset()
    for k in range(steps):
      env.step(actions[k])
  sim = envs[0].arena.sim
  pts = _points(rng, n, 33)
  pts[..., 0:2] *= 0.2
  pts[..., 0:2] += np.stack([sim.state['x'].cpu().numpy(), sim.state['y'].cpu().numpy()], -1)[:, None, :]
  xyp = torch.from_numpy(pts).cuda()
  before = _gp_bits(envs[0])
  mean, dev_ = envs[0].query_wind(xyp, add_forecast=False)
  envs[0].arena.query_wind(xyp)
  torch.cuda.synchronize()
  after = _gp_bits(envs[0])
  assert sorted(before) == sorted(after) and 'chol' in before
  for k in before:
    assert torch.equal(before[k], after[k]), k
  # against the host twin rebuilt from the ring
  now = sim.state['time_elapsed_s'].cpu().numpy()
  mean, dev_ = mean.cpu().numpy().astype(np.float64), dev_.cpu().numpy().astype(np.float64)
  for e in range(n):
    hm, hd, m = _host(_ring_back(sim, e), pts[e], now[e])
    assert m == min(int(sim._gp['count'][e].item()), steps + 1) and m >= 1
    _close(mean[e], hm, f'rollout env {e} mean')
    _close(dev_[e], hd, f'rollout env {e} deviation')
  # the rollout goes on bit for bit, with queries between the steps or without
  for k in range(steps, steps + more):
    a = envs[0].step(actions[k])
    envs[0].query_wind(xyp)
    b = envs[1].step(actions[k])
    for x, y in zip(a, b):
      assert torch.equal(x, y), k
  envs[0].check_errors(); envs[1].check_errors()


def test_graph_capture_replays_the_eager_result():
  rng = np.random.default_rng(30)
  n, q = 5, 33
  sim = _sim(n, rng.uniform(-30.0, 30.0, vec_state.GRID_SHAPE).astype(np.float32))
  for e, m in enumerate((0, 7, 64, 100, 120)):
    _write_ring(sim, e, _observations(rng, m, 180))
  sim.state['time_elapsed_s'].copy_(torch.tensor([0, 180 * 6, 180 * 63, 180 * 99, 180 * 119], dtype=torch.int32))
  pts = _points(rng, n, q)
  pts[..., 0:2] *= 0.5
  xyp = torch.from_numpy(pts).cuda()
  eager = sim.query_wind(xyp)
  torch.cuda.synchronize()
  out = (torch.zeros_like(eager[0]), torch.zeros_like(eager[1]))
  graph, _ = dev.capture(sim.device, lambda: sim.query_wind(xyp, out=out))
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]) and _flags(sim) == 0
  # the graph reads the tensors it was recorded with: new points, same launch
  xyp.copy_(torch.from_numpy(_points(rng, n, q) * np.float32(0.5)))
  graph.replay()
  again = sim.query_wind(xyp)
  torch.cuda.synchronize()
  assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1])
