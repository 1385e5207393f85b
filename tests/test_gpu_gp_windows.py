"""The three kernels that call the WindGP window of ble_gp_factor.h -- ble_gp_query_kernel (ble_gp_query.h), ble_gp_fit_kernel
(ble_gp_belief.h) and ble_gp_fit_scenarios_kernel (ble_scenarios.h): ballot pair, `drop`, the evicted-entries rule, popcount compaction
in one copy, the exits and what is kept of an entry per kernel -- held to ONE table of rings and anchors (tests/gp_window_cases.py; the table itself is checked by
tests/test_gp_window_cases_host.py).  One environment per case on one simulator.

References.  n_obs and BLE_FLAG_GP_WINDOW: include/ble_abi.h's rule restated over the held entries (gp_window_cases.expected).  The
posterior: gp_window_cases.Twin (tests/wind_gp_host.py's kernel, cho_solve) over the ring's own float32 values read back from the
device.  The scenario fit's right-hand side is y - f_m(X) with the DEVICE's own prior_only values as f_m(X), as in
tests/test_gpu_scenarios.py (the prior has its own test there).

Bars.  Outputs: the project's 1e-5 m/s absolute (float32 outputs of a few m/s round by 2.4e-7, the fp64 algebra at cond(K)
<= 208 contributes ~1e-12).  alpha: 1e-9 max(1, |alpha|max), tests/test_gpu_scenarios.py's.  The window's content: loc divided back by
the length scales against the twin's kept entries at rtol 1e-12 -- one fp64 multiply by one fp64 constant (2 ulp = 4.4e-16) against
entries whose times differ by >= 60 s in <= 7e4 s, so a wrong or permuted entry is off by >= 1e-3 relative.  A window shifted by one
entry at either end moves the mean at the case's boundary points by >= 0.069 m/s (the host test), 6 900 x the output bar."""
import numpy as np
import pytest
import torch

import gp_window_cases as wc
import helpers
from balloon_learning_environment_amd import _lib, vec_state

pytestmark = pytest.mark.gpu

DEVICE = 'cuda:0'
TOL = 1e-5
NUM = 2                    # scenarios
FIT_SEED = 23
N, Q = len(wc.CASES), wc.Q
FLAGGED = tuple(i for i, c in enumerate(wc.CASES) if c.flag)
UNFLAGGED = tuple(i for i, c in enumerate(wc.CASES) if not c.flag)
NAN_ROWS = tuple(i for i, c in enumerate(wc.CASES) if c.n_obs < 0)
FINITE = tuple(i for i, c in enumerate(wc.CASES) if c.n_obs > 0)
EMPTY = tuple(i for i, c in enumerate(wc.CASES) if c.n_obs == 0)
TABLE_N_OBS = [c.n_obs for c in wc.CASES]
AHEAD_S = 3600
# the slab's loc is in units of ln2 / 32 length scales (ble_gp_belief.h: kBeliefKappa = 32 / ln 2)
SCALES = 46.16624130844683 / np.array([357000.0, 357000.0, 326.0, 34560.0])


def _dev(a, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)
  return t if dtype is None else t.to(dtype)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flags(sim):
  word = int(sim.err_flags.item())
  sim.err_flags.zero_()
  return word


def _fit_all(sim, anchor, xyp):
  """query_wind, fit_wind_belief and fit_wind_scenarios at the anchors, one launch each, the flag word read after each."""
  t = _dev(anchor)
  mean, dev_ = sim.query_wind(xyp, t, add_forecast=False)
  torch.cuda.synchronize()
  fq = _flags(sim)
  belief = sim.fit_wind_belief(t)
  torch.cuda.synchronize()
  fb = _flags(sim)
  scn = sim.fit_wind_scenarios(NUM, seed=FIT_SEED, time_s=t)
  torch.cuda.synchronize()
  fs = _flags(sim)
  return dict(mean=mean.cpu().numpy(), dev=dev_.cpu().numpy(), belief=belief, scn=scn, flags=(fq, fb, fs),
              bslab=belief.slab.cpu().numpy(), bn=belief.n_obs.cpu().numpy(), sslab=scn.slab.cpu().numpy(), sn=scn.n_obs.cpu().numpy())


def _winds(sim, belief, scn, pts, anchor):
  """belief_wind at the anchor and scenario_wind (m = 0 .. NUM - 1, with and without the correction) at the anchor and AHEAD_S later,
  at pts [n, Q, 3]: (belief [n, Q, 2], scenario [2, NUM, n, Q, 2], prior [2, NUM, n, Q, 2]) float32."""
  n = pts.shape[0]
  bw = np.zeros((n, Q, 2), np.float32)
  sw, pw = np.zeros((2, NUM, n, Q, 2), np.float32), np.zeros((2, NUM, n, Q, 2), np.float32)
  times = [_dev(anchor), _dev(anchor + AHEAD_S)]
  for j in range(Q):
    x, y, p = (_dev(pts[:, j, k]) for k in range(3))
    bw[:, j] = sim.belief_wind(belief, x, y, p, times[0]).cpu().numpy()
    for o in range(2):
      for m in range(NUM):
        sw[o, m, :, j] = sim.scenario_wind(scn, m, x, y, p, times[o]).cpu().numpy()
        pw[o, m, :, j] = sim.scenario_wind(scn, m, x, y, p, times[o], prior_only=True).cpu().numpy()
  return bw, sw, pw


@pytest.fixture(scope='module')
def win():
  """The rings on one simulator, their read-back twins, the launches (the unflagged cases together, every flagged case alone, all of
  them at once) and the device's own prior at the window's points: computed once."""
  sim = vec_state.VecSimulator(N, DEVICE)
  sim._allocate_history(False)
  built = [wc.build(i) for i in range(N)]
  for i, (obs, _) in enumerate(built):
    helpers.write_ring(sim, i, obs)
  anchor = np.array([a for _, a in built], np.int32)
  sim.reset_observation_history(_dev(np.array([c.reset for c in wc.CASES], np.uint8)))
  rings = helpers.rings_back(sim)
  for i, (obs, _) in enumerate(built):          # the device holds what the host test looked at
    for a, b in zip(rings[i], wc.held(obs)):
      assert np.array_equal(a, b), wc.NAMES[i]
  keeps = [wc.kept(rings[i][1], anchor[i]) if wc.CASES[i].n_obs > 0 else np.zeros(0, np.int64) for i in range(N)]
  twins = [wc.Twin(rings[i], keeps[i]) for i in range(N)]
  pts_and_boundary = [wc.points(i, rings[i], keeps[i]) for i in range(N)]
  pts = np.stack([p for p, _ in pts_and_boundary])
  xyp = _dev(pts)
  count = sim._gp['count'].clone()

  def launch(envs):
    """The three kernels with only `envs` holding a history (the others' counts zeroed for the call)."""
    mask = torch.ones(N, dtype=torch.bool, device=sim.device)
    mask[list(envs)] = False
    sim._gp['count'][mask] = 0
    out = _fit_all(sim, anchor, xyp)
    sim._gp['count'].copy_(count)
    return out

  out = dict(sim=sim, built=built, anchor=anchor, rings=rings, twins=twins, pts=pts, boundary=[b for _, b in pts_and_boundary])
  out['group'] = launch(UNFLAGGED)
  out['alone'] = {i: launch([i]) for i in FLAGGED}
  out['all'] = launch(range(N))
  # every case's own result: the unflagged from their one launch, the flagged from the launch each had to itself
  src = [out['alone'][i] if i in FLAGGED else out['group'] for i in range(N)]
  for key in ('mean', 'dev', 'bslab', 'bn', 'sslab', 'sn'):
    out[key] = np.stack([src[i][key][i] for i in range(N)])
  belief = vec_state.WindBelief(_dev(out['bslab']), _dev(out['bn']))
  scn = vec_state.WindScenarios(_dev(out['sslab']), _dev(out['sn']), NUM, FIT_SEED, None)
  out['belief_wind'], out['scenario_wind'], out['prior'] = _winds(sim, belief, scn, pts, anchor)
  # f_m(X) as the device gives it: [NUM, rows, N, 2], one launch per (m, row of the longest window)
  rows = max(t.n_obs for t in twins)
  at_x, t_x = np.zeros((rows, N, 3), np.float32), np.zeros((rows, N), np.int32)
  for i, t in enumerate(twins):
    at_x[:t.n_obs, i], t_x[:t.n_obs, i] = t.xyp.astype(np.float32), t.t.astype(np.int32)
  prior = np.zeros((NUM, rows, N, 2), np.float32)
  for r in range(rows):
    args = [_dev(at_x[r, :, k]) for k in range(3)] + [_dev(t_x[r])]
    for m in range(NUM):
      prior[m, r] = sim.scenario_wind(scn, m, *args, prior_only=True).cpu().numpy()
  out['prior_at_x'] = prior
  return out


# ---------------------------------------------------------------------------------------------- n_obs and the flag
def test_unflagged_cases_in_one_launch(win):
  group = win['group']
  assert group['flags'] == (0, 0, 0)          # after the query, the belief's fit and the scenario fit
  want = [c.n_obs if i in UNFLAGGED else 0 for i, c in enumerate(wc.CASES)]
  assert group['bn'].tolist() == want and group['sn'].tolist() == want
  assert np.isfinite(group['mean']).all() and np.isfinite(group['dev']).all()
  for i in UNFLAGGED:
    assert wc.expected(wc.CASES[i].count, win['rings'][i][1], win['anchor'][i], wc.CASES[i].reset)[1:] == (want[i], 0)


@pytest.mark.parametrize('name', [wc.NAMES[i] for i in FLAGGED])
def test_flagged_cases_one_at_a_time(win, name):
  i = wc.index(name)
  case, alone = wc.CASES[i], win['alone'][i]
  assert wc.expected(case.count, win['rings'][i][1], win['anchor'][i])[1:] == (case.n_obs, 1)
  assert alone['flags'] == (_lib.FLAG_GP_WINDOW,) * 3, name
  want = [case.n_obs if e == i else 0 for e in range(N)]
  assert alone['bn'].tolist() == want and alone['sn'].tolist() == want, name
  others = [e for e in range(N) if e != i]
  assert not alone['bslab'][others].any() and not alone['sslab'][others].any()
  assert not alone['mean'][others].view(np.uint32).any() and not alone['dev'][others].view(np.uint32).any()
  if case.n_obs < 0:
    assert np.isnan(alone['mean'][i]).all() and np.isnan(alone['dev'][i]).all(), name
    assert not alone['bslab'][i].any() and not alone['sslab'][i].any(), name
  else:
    assert np.isfinite(alone['mean'][i]).all() and np.isfinite(alone['dev'][i]).all(), name


def test_all_cases_in_one_launch(win):
  every = win['all']
  assert every['flags'] == (_lib.FLAG_GP_WINDOW,) * 3
  assert every['bn'].tolist() == TABLE_N_OBS == every['sn'].tolist()
  # a case gives the same bits whatever shares its launch
  for key in ('mean', 'dev', 'bslab', 'sslab'):
    a, b = every[key], win[key]
    assert np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(np.uint32 if b.dtype == np.float32 else np.uint64)), key


# ---------------------------------------------------------------------------------------------- the window's content
def test_window_content(win):
  bslab, sslab = win['bslab'], win['sslab']
  assert bslab.shape == (N, 720) and sslab.shape == (N, 480 + 240 * NUM)
  assert win['bn'].tolist() == TABLE_N_OBS == win['sn'].tolist()
  # the scenario fit's window: the belief's, bit for bit
  assert np.array_equal(sslab[:, :480].view(np.uint64), bslab[:, :480].view(np.uint64))
  for i, case in enumerate(wc.CASES):
    m = max(case.n_obs, 0)
    twin = win['twins'][i]
    assert twin.n_obs == m, case.name
    for what, slab in (('belief', bslab[i]), ('scenarios', sslab[i])):
      loc = slab[:480].reshape(120, 4)
      # the twin's kept entries, chronological
      np.testing.assert_allclose(loc[:m] / SCALES, twin.loc, rtol=1e-12, atol=0.0, err_msg=f'{case.name} {what}')
      assert not loc[m:].any(), (case.name, what)
      alpha = slab[480:].reshape(-1, 120, 2)
      assert not alpha[:, m:].any(), (case.name, what)
      assert m == 0 or alpha[:, :m].all(), (case.name, what)


# ---------------------------------------------------------------------------------------------- alpha
def test_alpha_against_cho_solve(win):
  print()
  for i in FINITE:
    twin, name = win['twins'][i], wc.NAMES[i]
    m = twin.n_obs
    got = win['bslab'][i, 480:].reshape(120, 2)[:m]
    err_b = np.abs(got - twin.alpha).max()
    assert err_b <= 1e-9 * max(1.0, np.abs(twin.alpha).max()), (name, 'belief', err_b)
    err_s = 0.0
    for s in range(NUM):
      want = twin.solve(twin.y - win['prior_at_x'][s, :m, i].astype(np.float64))
      got = win['sslab'][i, 480 + 240 * s:480 + 240 * (s + 1)].reshape(120, 2)[:m]
      err = np.abs(got - want).max()
      err_s = max(err_s, err)
      assert err <= 1e-9 * max(1.0, np.abs(want).max()), (name, 'scenario', s, err)
    print(f'{name:30s} alpha: belief fit max |device - twin| {err_b:.3e}, scenario fit {err_s:.3e}  (|alpha|max {np.abs(twin.alpha).max():.1f})')


# ---------------------------------------------------------------------------------------------- the outputs
def test_outputs_against_the_twin(win):
  anchor, pts = win['anchor'], win['pts']
  print()
  for i in FINITE:
    twin, name = win['twins'][i], wc.NAMES[i]
    mean, dev_ = twin.mean(pts[i], anchor[i]), twin.deviation(pts[i], anchor[i])
    got_mean, got_dev, got_belief = (win[k][i].astype(np.float64) for k in ('mean', 'dev', 'belief_wind'))
    assert np.isfinite(got_mean).all() and np.isfinite(got_dev).all() and np.isfinite(got_belief).all(), name
    e_mean, e_dev, e_belief = np.abs(got_mean - mean).max(), np.abs(got_dev - dev_).max(), np.abs(got_belief - mean).max()
    e_both = np.abs(got_belief - got_mean).max()
    e_scn = 0.0
    for s in range(NUM):
      alpha = twin.solve(twin.y - win['prior_at_x'][s, :twin.n_obs, i].astype(np.float64))
      for o, t in enumerate((anchor[i], anchor[i] + AHEAD_S)):
        want = win['prior'][o, s, i] + twin.mean(pts[i], t, alpha).astype(np.float32)          # ONE float32 addition of two float32 values
        got = win['scenario_wind'][o, s, i]
        assert np.isfinite(got).all(), (name, s, o)
        e_scn = max(e_scn, np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f'{name:30s} max |device - twin|: query mean {e_mean:.3e} deviation {e_dev:.3e}, belief mean {e_belief:.3e} '
          f'(vs the query {e_both:.3e}), scenario wind {e_scn:.3e}')
    assert e_mean <= TOL and e_dev <= TOL, (name, 'query', e_mean, e_dev)
    assert e_belief <= TOL and e_both <= TOL, (name, 'belief', e_belief, e_both)
    assert e_scn <= TOL, (name, 'scenarios', e_scn)
    # the window really shapes these numbers: at the boundary points the correction is not small
    assert np.abs(mean[win['boundary'][i]]).max() > 1e-2, name


def test_empty_windows_are_exact(win):
  assert EMPTY == (wc.index('empty_far_ahead'), wc.index('pending_restart'))
  for i in EMPTY:
    name = wc.NAMES[i]
    assert not win['bslab'][i].any() and not win['sslab'][i].any(), name
    assert not win['mean'][i].view(np.uint32).any() and not win['dev'][i].view(np.uint32).any(), name          # exactly +0.0
    assert not win['belief_wind'][i].view(np.uint32).any(), name
    # the scenario is its prior: f_m + 0.0f, the kernel's one addition
    assert np.array_equal(_bits(win['scenario_wind'][:, :, i]), _bits(win['prior'][:, :, i] + np.float32(0.0))), name
    assert np.abs(win['prior'][:, :, i]).min() > 0.0
  # the restart stays pending: the three kernels only read
  assert win['sim']._obs_reset.cpu().numpy().tolist() == [int(c.reset) for c in wc.CASES]


# ---------------------------------------------------------------------------------------------- consumers of a NaN belief
def test_nan_rows_and_their_neighbours(win):
  """belief_wind and scenario_wind over ALL cases in one launch: the -1 rows are NaN, the rows next to them -- lanes of the same wave,
  one loop to the largest trip count (belief_wave_trip) -- are finite and bit for bit what the same ring gives on a simulator of its
  own."""
  sim, anchor, pts, every = win['sim'], win['anchor'], win['pts'], win['all']
  assert NAN_ROWS == (wc.index('prefix_wrapped'), wc.index('overfull_wrapped_one_back'))
  bw, sw, _ = _winds(sim, every['belief'], every['scn'], pts, anchor)
  for i in NAN_ROWS:
    assert np.isnan(bw[i]).all() and np.isnan(sw[:, :, i]).all(), wc.NAMES[i]
  rest = [i for i in range(N) if i not in NAN_ROWS]
  assert np.isfinite(bw[rest]).all() and np.isfinite(sw[:, :, rest]).all()
  assert np.array_equal(_bits(bw[rest]), _bits(win['belief_wind'][rest]))
  assert np.array_equal(_bits(sw[:, :, rest]), _bits(win['scenario_wind'][:, :, rest]))
  for i in sorted({e for r in NAN_ROWS for e in (r - 1, r + 1)}):
    assert wc.CASES[i].n_obs > 0
    one = vec_state.VecSimulator(1, DEVICE, env_offset=i)          # (the scenario stream is keyed by the global index)
    one._allocate_history(False)
    helpers.write_ring(one, 0, win['built'][i][0])
    alone = _fit_all(one, anchor[i:i + 1], _dev(pts[i:i + 1]))
    assert alone['bn'].tolist() == [wc.CASES[i].n_obs] == alone['sn'].tolist()
    assert alone['flags'] == ((_lib.FLAG_GP_WINDOW,) * 3 if wc.CASES[i].flag else (0, 0, 0))
    assert np.array_equal(alone['bslab'][0].view(np.uint64), every['bslab'][i].view(np.uint64)), wc.NAMES[i]
    assert np.array_equal(alone['sslab'][0].view(np.uint64), every['sslab'][i].view(np.uint64)), wc.NAMES[i]
    bw1, sw1, _ = _winds(one, alone['belief'], alone['scn'], pts[i:i + 1], anchor[i:i + 1])
    assert np.array_equal(_bits(bw1[0]), _bits(bw[i])), wc.NAMES[i]
    assert np.array_equal(_bits(sw1[:, :, 0]), _bits(sw[:, :, i])), wc.NAMES[i]
