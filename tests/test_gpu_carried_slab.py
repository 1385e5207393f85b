"""The carried WindGP factor slab of ble_observe_f32, word by word ("The carried slab").

An environment whose call ends with n_chol = m owns, of its chol_stride doubles: the packed triangle [0, tri(m)), the drop vector
[7260, 7260 + m - 1), zeta_u / d and zeta_v / d [7380, 7380 + m) and [7500, 7500 + m).  The kernel writes NO other word: not the pad
word after an odd triangle (tri(m) is odd for m % 4 in {1, 2}), nothing beyond 7620 of a wider stride, nothing of an environment
that live_only leaves out.  Every test pre-fills the slab with one finite sentinel double and compares bit patterns: a word the kernel
must not write still holds what it held before the call.

Reference (tests/test_gpu_observe.py::test_carried_factor_equals_fresh_factorisation): fp64 NumPy cholesky of K + 0.05 I rebuilt from
the ring as read back from the device; K + 0.05 I = Lt D Lt^T, p = -(Lt^-1 e_0)[1:], zeta / d = (Lt^-1 y) / d.  Bars, the project's
(same test): the triangle 1e-11, zeta 1e-10, and p zeta's 1e-10 (the same kind of quantity: a unit-lower solve against the same Lt) --
max |device - host| over an environment's region relative to the region's largest reference entry.  cond(K + 0.05 I) <= 3.2e4 for any
window of 120, so the reference's own error is ~ 3e4 x 1.1e-16 = 4e-12 at the worst and typically far below.

Histories are flight-shaped: a random walk that ends at the balloon (3 km and 60 Pa per 180 s), neighbouring observations strongly
correlated -- the windows a flight builds, not the nearly diagonal K of scattered points.  The times of the slide at a partial window
come from helpers.slide_times, shown on the host to drop exactly the oldest observation (tests/test_carried_slab_host.py)."""
import ctypes

import numpy as np
import pytest
import scipy.linalg
import torch

import helpers
from balloon_learning_environment_amd import _lib, device as dev, vec_state

SENTINEL = 0x4D5A17C0DEC0FFEE          # a FINITE double (2.9e64) no kernel computes: a scan for non-finite words stays meaningful
SENTINEL_I32 = 0x5EA7BEEF              # the same idea for int32 / float32 tensors (1.588e9; 6.05e18 as a float32)
TRI, ROWS, STRIDE, OBS_DIM = 7260, 120, 7620, 1099
LENGTH_SCALE = np.array([357000.0, 357000.0, 326.0, 34560.0])
BAR = {'triangle': 1e-11, 'p': 1e-10, 'zeta': 1e-10}
SLIDE_SIZES = (2, 3, 5, 63, 64, 65, 118, 119)
FORCED = ((2, 2), (5, 2), (64, 3), (65, 2))          # (m after the call, observations that age out at once)
RESTART = (40, 7)                                     # windows before the pending restart


def _tri(m):
  return m * (m + 1) // 2


def _valid(m, stride=STRIDE):
  """The words of one environment's slab that a call ending with n_chol = m owns."""
  v = np.zeros(stride, bool)
  v[:_tri(m)] = True
  v[TRI:TRI + max(m - 1, 0)] = True
  v[TRI + ROWS:TRI + ROWS + m] = True
  v[TRI + 2 * ROWS:TRI + 2 * ROWS + m] = True
  return v


def _reference(ring, now):
  """(m, packed triangle [tri(m)], p [m - 1], zeta / d [m, 2]) of the window at `now`, fp64 on the host."""
  xyp, t, err = ring
  keep = helpers.gp_window(t, now)
  m = len(keep)
  if m == 0:
    return 0, np.zeros(0), np.zeros(0), np.zeros((0, 2))
  x = np.column_stack([xyp[keep], t[keep]])
  d = (x[:, None, :] - x[None, :, :]) / LENGTH_SCALE
  k = 3.6 ** 2 * np.exp(-np.sqrt((d * d).sum(-1))) + 0.05 * np.eye(m)
  chol = np.linalg.cholesky(k)
  dd = np.diag(chol) ** 2
  unit = np.tril(chol / np.diag(chol)[None, :], -1) + np.eye(m)
  packed = (np.tril(unit, -1) + np.diag(dd))[np.tril_indices(m)]          # row by row: the kernel's packing
  p = -scipy.linalg.solve_triangular(unit, np.eye(m)[:, 0], lower=True, unit_diagonal=True)[1:]
  zeta = scipy.linalg.solve_triangular(unit, err[keep], lower=True, unit_diagonal=True) / dd[:, None]
  return m, packed, p, zeta


def _rel(got, want):
  return float(np.max(np.abs(got - want)) / np.max(np.abs(want))) if want.size else 0.0


def _dev(a, sim, dtype=None):
  t = torch.from_numpy(np.ascontiguousarray(a)).to(sim.device)
  return t if dtype is None else t.to(dtype)


def _bits(t):
  t = t.contiguous()
  return t.view(torch.int64 if t.element_size() == 8 else torch.int32).cpu().numpy().copy()


def _sim(n, seed, warm=4):
  """A simulator `warm` agent steps into its episodes with an empty history and a sentinel-filled carried slab."""
  rng = np.random.default_rng(seed)
  sim = vec_state.VecSimulator(n, 'cuda:0')
  sim.set_grid(rng.uniform(-12.0, 12.0, vec_state.GRID_SHAPE).astype(np.float32))
  sim.reset_device(seed)
  a = _dev(rng.integers(0, 3, (warm, n)).astype(np.uint8), sim)
  sim.step_n(a, torch.zeros(a.shape, dtype=torch.float32, device=sim.device), torch.zeros(a.shape, dtype=torch.uint8, device=sim.device))
  sim.check_errors()
  sim._allocate_history(True)
  sim._gp['chol'].view(torch.int64).fill_(SENTINEL)
  return sim, rng


def _now(sim):
  return sim.state['time_elapsed_s'].cpu().numpy().astype(np.int64)


def _here(sim):
  return np.stack([sim.state[f].cpu().numpy().astype(np.float64) for f in ('x', 'y', 'pressure')], -1)


def _history(rng, sim, env, times, here, now):
  """Writes observations at `times` (chronological, all before `now`) into env's ring: a random walk back from the balloon."""
  times = np.asarray(times, np.int64)
  if not len(times):
    return
  gaps = np.diff(np.concatenate([times, [now]]))[::-1]                   # walking back from now
  steps = rng.normal(0.0, 1.0, (len(times), 3)) * np.array([3000.0, 3000.0, 60.0]) * np.sqrt(np.maximum(gaps, 1) / 180.0)[:, None]
  xyp = (here + np.cumsum(steps, 0))[::-1].copy()
  xyp[:, 2] = np.clip(xyp[:, 2], 5000.0, 14000.0)
  helpers.write_ring(sim, env, (xyp.astype(np.float32), times.astype(np.int32), rng.normal(0.0, 2.0, (len(times), 2)).astype(np.float32)))


def _spaced(now, count):
  """`count` observation times 180 s apart, the newest 180 s before `now`."""
  return now - 180 * np.arange(count, 0, -1)


def _refill(slab, n_chol):
  """Puts the sentinel back into every word outside the valid regions (nothing to do after a correct kernel) and returns the slab's
  bits: what the next call must leave outside ITS valid regions."""
  bits = _bits(slab)
  for e, m in enumerate(n_chol):
    bits[e][~_valid(int(m), bits.shape[1])] = SENTINEL
  slab.view(torch.int64).copy_(torch.from_numpy(bits).to(slab.device))
  return bits


class _Snap:
  """The carried state after a call, on the host, next to the slab's bits from before the call."""

  def __init__(self, sim, before, slab=None, n_chol=None, obs=None):
    torch.cuda.synchronize()
    slab = sim._gp['chol'] if slab is None else slab
    n_chol = sim._gp['n_chol'] if n_chol is None else n_chol
    self.before, self.bits, self.slab = before, _bits(slab), slab.cpu().numpy()
    self.n_chol = n_chol.cpu().numpy()
    self.count = sim._gp['count'].cpu().numpy()
    self.now, self.rings = _now(sim), helpers.rings_back(sim)
    self.clones_equal = torch.equal(slab.clone(), slab.clone())          # the symptom: two clones differ only over a NaN
    self.finite = bool(torch.isfinite(slab).all())
    self.obs = None if obs is None else obs.cpu().numpy()
    self.flags = int(sim.err_flags.item())


def _check(snap, what, sizes, envs=None):
  """Every environment of `envs` (default: all of `sizes`): n_chol, the three regions against the host, every other word as before
  the call.  sizes: {env: m} or a sequence.  Returns the worst relative errors."""
  sizes = dict(enumerate(sizes)) if not isinstance(sizes, dict) else sizes
  envs = sorted(sizes) if envs is None else envs
  stride = snap.bits.shape[1]
  worst = {'triangle': 0.0, 'p': 0.0, 'zeta': 0.0}
  touched, wrong_size = [], []
  for e in envs:
    m, packed, p, zeta = _reference(snap.rings[e], snap.now[e])
    if not (m == sizes[e] == int(snap.n_chol[e])):
      wrong_size.append((e, sizes[e], m, int(snap.n_chol[e])))
      continue
    row = snap.slab[e]
    worst['triangle'] = max(worst['triangle'], _rel(row[:_tri(m)], packed))
    worst['p'] = max(worst['p'], _rel(row[TRI:TRI + m - 1], p))
    got_z = np.stack([row[TRI + ROWS:TRI + ROWS + m], row[TRI + 2 * ROWS:TRI + 2 * ROWS + m]], 1)
    worst['zeta'] = max(worst['zeta'], _rel(got_z, zeta))
    outside = np.flatnonzero(~_valid(m, stride))
    changed = outside[snap.bits[e][outside] != snap.before[e][outside]]
    if changed.size:
      touched.append((m, changed[:3].tolist()))
  print(f'{what}: {len(envs)} environments, m = {min(sizes[e] for e in envs)} .. {max(sizes[e] for e in envs)}: worst relative error '
        f'triangle {worst["triangle"]:.3e}, p {worst["p"]:.3e}, zeta {worst["zeta"]:.3e}; flags {snap.flags}')
  assert not wrong_size, (what, '(env, planned m, host window, n_chol)', wrong_size)
  assert not touched, f'{what}: words outside the valid region written at m = {[m for m, _ in touched]} (first words: {touched[:6]})'
  assert snap.finite, (what, 'a non-finite word in the slab')
  assert snap.clones_equal, (what, 'two clones of the slab differ')
  for region, bar in BAR.items():
    assert worst[region] <= bar, (what, region, worst[region])
  assert snap.flags == 0, (what, snap.flags)
  return worst


# ---------------------------------------------------------------------------------------------- 1. every size: refit, border, full slide
@pytest.fixture(scope='module')
def every_size():
  """Environment e ends the first call with m = e + 1 (refit: n_chol = 0), the second, one agent step later, with m + 1 (one row
  bordered) -- but the last, whose window of 120 slides."""
  n = ROWS
  sim, rng = _sim(n, 50)
  now, here = _now(sim), _here(sim)
  for e in range(n):
    _history(rng, sim, e, _spaced(now[e], e), here[e], now[e])
  before = _bits(sim._gp['chol'])
  assert np.all(before == SENTINEL)
  sim.observe(_dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), sim))
  refit = _Snap(sim, before)
  before = _refill(sim._gp['chol'], refit.n_chol)
  sim.step(_dev(rng.integers(0, 3, n).astype(np.uint8), sim))
  assert np.array_equal(_now(sim), now + 180)
  sim.observe(_dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), sim))
  return {'refit': refit, 'second': _Snap(sim, before)}


@pytest.mark.gpu
def test_refit_at_every_size(every_size):
  _check(every_size['refit'], 'refit', range(1, ROWS + 1))


@pytest.mark.gpu
def test_border_one_row_added_at_every_size(every_size):
  _check(every_size['second'], 'border', {e: e + 2 for e in range(ROWS - 1)})


@pytest.mark.gpu
def test_slide_at_the_full_window(every_size):
  snap = every_size['second']
  assert int(snap.count[ROWS - 1]) == ROWS + 1            # 121 observations in the ring, the oldest exactly 6 h old: outside
  _check(snap, 'slide at 120', {ROWS - 1: ROWS})


# ---------------------------------------------------------------------------------------------- 2. slide at a partial window, forced refit, restart
@pytest.fixture(scope='module')
def paths():
  plan = [(m, 1) for m in SLIDE_SIZES] + list(FORCED)
  n = len(plan) + len(RESTART)
  sim, rng = _sim(n, 51)
  now, here = _now(sim), _here(sim)
  for e, (m, leaving) in enumerate(plan):
    _history(rng, sim, e, helpers.slide_times(m, int(now[e]), leaving), here[e], now[e])
  for e, m in enumerate(RESTART, len(plan)):
    _history(rng, sim, e, _spaced(now[e], m - 1), here[e], now[e])
  first_sizes = [m - 1 + leaving for m, leaving in plan] + list(RESTART)
  noise = lambda: _dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), sim)
  before = _bits(sim._gp['chol'])
  sim.observe(noise())
  first = _Snap(sim, before)
  before = _refill(sim._gp['chol'], first.n_chol)
  sim.step(_dev(rng.integers(0, 3, n).astype(np.uint8), sim))
  assert np.array_equal(_now(sim), now + 180)
  mask = np.zeros(n, np.uint8)
  mask[len(plan):] = 1
  sim.reset_observation_history(_dev(mask, sim))
  sim.observe(noise())
  second = _Snap(sim, before)
  before = _refill(sim._gp['chol'], second.n_chol)
  sim.observe(noise(), append=False)
  third = _Snap(sim, before)
  return {'plan': plan, 'first': first, 'first_sizes': first_sizes, 'second': second, 'third': third,
          'second_sizes': [m for m, _ in plan] + [1] * len(RESTART)}


@pytest.mark.gpu
def test_slide_at_a_partial_window(paths):
  _check(paths['first'], 'the refit before the slides', paths['first_sizes'])
  envs = list(range(len(SLIDE_SIZES)))
  assert [int(paths['second'].count[e]) for e in envs] == [m + 1 for m in SLIDE_SIZES]          # m + 1 in the ring, m in the window
  _check(paths['second'], 'slide at a partial window', paths['second_sizes'], envs)


@pytest.mark.gpu
def test_forced_refit_when_two_or_more_age_out_at_once(paths):
  envs = list(range(len(SLIDE_SIZES), len(paths['plan'])))
  _check(paths['second'], 'forced refit', paths['second_sizes'], envs)


@pytest.mark.gpu
def test_pending_history_restart_gives_one_row(paths):
  envs = list(range(len(paths['plan']), len(paths['second_sizes'])))
  assert [int(paths['second'].count[e]) for e in envs] == [1] * len(envs)
  _check(paths['second'], 'history restart', paths['second_sizes'], envs)


@pytest.mark.gpu
def test_append_false_leaves_m_unchanged(paths):
  second, third = paths['second'], paths['third']
  assert np.array_equal(second.n_chol, third.n_chol) and np.array_equal(second.count, third.count)
  _check(third, 'append=False', paths['second_sizes'])


# ---------------------------------------------------------------------------------------------- 3. live_only
@pytest.mark.gpu
def test_live_only_leaves_a_terminated_environment_alone():
  sizes = (1, 6, 62, 31, 120, 3)
  dead = (1, 3)
  n = len(sizes)
  sim, rng = _sim(n, 52)
  now, here = _now(sim), _here(sim)
  for e, m in enumerate(sizes):
    _history(rng, sim, e, _spaced(now[e], m - 1), here[e], now[e])
  for e in dead:                      # everything the kernel could touch of a terminated environment holds a sentinel
    sim.state['status'][e] = 1
    for name in ('xyp', 'elapsed_s', 'err_uv', 'count', 'n_chol'):
      sim._gp[name][e:e + 1].view(torch.int32).fill_(SENTINEL_I32)
  sim._obs_reset[3] = 1
  out = torch.full((n, OBS_DIM), SENTINEL_I32, dtype=torch.int32, device=sim.device).view(torch.float32)
  gp_before = {k: _bits(v) for k, v in sim._gp.items()}
  sim.observe(_dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), sim), out=out, live_only=True)
  snap = _Snap(sim, gp_before['chol'], obs=out)
  for e in dead:
    for k, v in sim._gp.items():
      assert np.array_equal(_bits(v)[e], gp_before[k][e]), (e, k)
    assert np.all(snap.bits[e] == SENTINEL) and int(snap.n_chol[e]) == SENTINEL_I32
    assert np.all(_bits(out)[e] == SENTINEL_I32), e
  assert sim._obs_reset.cpu().numpy().tolist() == [0, 0, 0, 1, 0, 0]          # a terminated environment's restart stays pending
  live = [e for e in range(n) if e not in dead]
  _check(snap, 'live_only', dict(enumerate(sizes)), live)
  assert np.isfinite(snap.obs[live]).all() and not np.any(_bits(out)[live] == SENTINEL_I32)


# ---------------------------------------------------------------------------------------------- 4. a strided slab through the C entry point
def _observe_f32(sim, hist, noise, out, append=1):
  """ble_observe_f32 through the ctypes binding, over the caller's struct ble_gp_history_f32."""
  code = _lib.lib().ble_observe_f32(ctypes.byref(sim._struct), sim.grid.data_ptr(), sim.grid_env_stride, dev.ptr(noise),
                                    sim._obs_reset.data_ptr(), ctypes.byref(hist), append, out.data_ptr(), sim.err_flags.data_ptr(), sim.n,
                                    dev.stream_ptr(sim.device))
  assert code == _lib.BLE_OK, code


@pytest.mark.gpu
def test_a_strided_slab():
  stride = 7700
  first_sizes = (1, 2, 3, 4, 61, 62, 63, 64, 117, 118, 119, 120)          # every residue mod 4, small, middle and at the top
  n = len(first_sizes)
  sim, rng = _sim(n, 53)
  now, here = _now(sim), _here(sim)
  for e, m in enumerate(first_sizes):
    _history(rng, sim, e, _spaced(now[e], m - 1), here[e], now[e])
  # one row more than environments: the word after the last environment's gap is "the next environment's first word"
  slab = torch.full((n + 1, stride), SENTINEL, dtype=torch.int64, device=sim.device).view(torch.float64)
  n_chol = torch.zeros(n + 1, dtype=torch.int32, device=sim.device)
  n_chol[n] = SENTINEL_I32
  assert slab.data_ptr() % 16 == 0
  hist = vec_state.gp_history_struct(dict(sim._gp, chol=slab, n_chol=n_chol))
  hist.chol_stride = stride
  ours = _bits(sim._gp['chol'])
  out = torch.full((n, OBS_DIM), float('nan'), dtype=torch.float32, device=sim.device)

  def check(what, sizes, before):
    snap = _Snap(sim, before, slab=slab, n_chol=n_chol, obs=out)
    assert snap.bits.shape == (n + 1, stride)
    _check(snap, what, sizes)
    gap = snap.bits[:n, STRIDE:]
    assert gap.shape == (n, stride - STRIDE) and np.all(gap == SENTINEL), np.argwhere(gap != SENTINEL)[:4].tolist()
    assert np.all(snap.bits[n] == SENTINEL) and int(snap.n_chol[n]) == SENTINEL_I32
    assert np.isfinite(snap.obs).all()
    assert np.array_equal(_bits(sim._gp['chol']), ours)          # the simulator's own slab is not the one the struct names
    return snap

  _observe_f32(sim, hist, _dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), sim), out)
  snap = check('stride 7700, refit', first_sizes, _bits(slab))
  before = _refill(slab[:n], snap.n_chol[:n])
  sim.step(_dev(rng.integers(0, 3, n).astype(np.uint8), sim))
  assert np.array_equal(_now(sim), now + 180)
  out.fill_(float('nan'))
  _observe_f32(sim, hist, _dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), sim), out)          # the carried factor is READ at the stride too
  check('stride 7700, border and slide', [min(m + 1, ROWS) for m in first_sizes], np.concatenate([before, _bits(slab[n:])]))


# ---------------------------------------------------------------------------------------------- 5. the symptom: carried state is a function of the inputs alone
@pytest.mark.gpu
def test_carried_state_does_not_depend_on_what_ran_before():
  sizes = (1, 2, 5, 6, 9, 61, 62, 3, 4, 64, 117, 118, 119, 120, 1, 1)
  n = len(sizes)

  def fly():
    sim, rng = _sim(n, 54)
    now, here = _now(sim), _here(sim)
    for e, m in enumerate(sizes):
      _history(rng, sim, e, _spaced(now[e], m - 1), here[e], now[e])
    noise = [_dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), sim) for _ in range(2)]
    action = _dev(rng.integers(0, 3, n).astype(np.uint8), sim)
    return sim, noise, action

  def observe_twice(sim, noise, action):
    rows = [torch.full((n, OBS_DIM), float('nan'), dtype=torch.float32, device=sim.device) for _ in range(2)]
    sim.observe(noise[0], out=rows[0])
    sim.step(action)
    sim.observe(noise[1], out=rows[1])
    torch.cuda.synchronize()
    return rows

  a, noise_a, action_a = fly()
  b, noise_b, action_b = fly()
  rows_a = observe_twice(a, noise_a, action_a)
  # another kernel's data in the LDS of every CU: a belief fit over 1024 environments with full windows (69 KB of LDS per workgroup)
  other = vec_state.VecSimulator(1024, 'cuda:0')
  other._allocate_history(False)
  rng = np.random.default_rng(55)
  other._gp['xyp'].copy_(_dev(np.concatenate([rng.uniform(-2e5, 2e5, (1024, 128, 2)), rng.uniform(5000.0, 14000.0, (1024, 128, 1))], -1)
                              .astype(np.float32), other))
  other._gp['elapsed_s'].copy_(_dev(np.tile(180 * np.arange(128, dtype=np.int32), (1024, 1)), other))
  other._gp['err_uv'].copy_(_dev(rng.normal(0.0, 2.0, (1024, 128, 2)).astype(np.float32), other))
  other._gp['count'].fill_(120)
  other.state['time_elapsed_s'].fill_(180 * 119)
  belief = other.fit_wind_belief()
  torch.cuda.synchronize()
  assert belief.n_obs.cpu().numpy().tolist() == [120] * 1024
  rows_b = observe_twice(b, noise_b, action_b)
  for call, (ra, rb) in enumerate(zip(rows_a, rows_b)):
    assert np.array_equal(_bits(ra), _bits(rb)), f'observation rows of call {call}'
  for k in a._gp:
    assert np.array_equal(_bits(a._gp[k]), _bits(b._gp[k])), k
  for sim in (a, b):
    slab = sim._gp['chol']
    assert torch.equal(slab.clone(), slab.clone()) and bool(torch.isfinite(slab).all())
    bits, n_chol = _bits(slab), sim._gp['n_chol'].cpu().numpy()
    assert n_chol.tolist() == [min(m + 1, ROWS) for m in sizes]
    for e, m in enumerate(n_chol):
      assert np.all(bits[e][~_valid(int(m))] == SENTINEL), (e, int(m))


# ---------------------------------------------------------------------------------------------- 6. checkpoint
@pytest.mark.gpu
def test_a_checkpoint_resumes_bit_for_bit_into_a_sentinel_filled_slab():
  sizes = (117, 118, 119, 60, 5, 0)          # windows before the first observe(): the first three reach 120 and slide on the way
  n, calls_before, calls_after = len(sizes), 2, 3
  a, rng = _sim(n, 57)
  now, here = _now(a), _here(a)
  for e, m in enumerate(sizes):
    _history(rng, a, e, _spaced(now[e], m), here[e], now[e])
  noise = [_dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), a) for _ in range(calls_before + calls_after)]
  actions = [_dev(rng.integers(0, 3, n).astype(np.uint8), a) for _ in range(calls_before + calls_after)]
  for i in range(calls_before):
    a.observe(noise[i])
    a.step(actions[i])
  sd = a.state_dict()
  b = vec_state.VecSimulator(n, 'cuda:0')
  b._allocate_history(True)
  b._gp['chol'].view(torch.int64).fill_(SENTINEL)
  b.load_state_dict(sd)
  assert np.array_equal(_bits(b._gp['chol']), _bits(sd['gp']['chol']))
  for i in range(calls_before, calls_before + calls_after):
    rows = [sim.observe(noise[i]).clone() for sim in (a, b)]
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rows[0]), _bits(rows[1])), f'observation rows of call {i}'
    sa, sb = a.state_dict(), b.state_dict()
    assert sorted(sa['gp']) == sorted(sb['gp']) == ['chol', 'count', 'elapsed_s', 'err_uv', 'n_chol', 'xyp']
    for k in sa['gp']:
      assert np.array_equal(_bits(sa['gp'][k]), _bits(sb['gp'][k])), (i, k)
      assert torch.equal(sa['gp'][k], sb['gp'][k]), (i, k)          # state_dict() equality as a user writes it: no NaN in the way
    assert torch.equal(sa['obs_reset'], sb['obs_reset'])
    for sim in (a, b):
      sim.step(actions[i])
  n_chol = a._gp['n_chol'].cpu().numpy()
  assert n_chol.tolist() == [120, 120, 120, 60 + 5, 5 + 5, 0 + 5] and a._gp['count'].cpu().numpy().tolist() == [m + 5 for m in sizes]
  bits = _bits(a._gp['chol'])
  for e, m in enumerate(n_chol):
    assert np.all(bits[e][~_valid(int(m))] == SENTINEL), (e, int(m))
  assert bool(torch.isfinite(a._gp['chol']).all())
  a.check_errors(); b.check_errors()


# ---------------------------------------------------------------------------------------------- 7. every word of the observation row
@pytest.mark.gpu
@pytest.mark.parametrize('append', (False, True))
@pytest.mark.parametrize('entry', ('ble_observe_f32', 'forecast_levels'))
def test_every_word_of_the_row_is_written(entry, append):
  windows = (1, 2, 3, 64, 120) if append else (0, 1, 2, 64, 120)          # after the call
  pressures = (5030.0, 13970.0)          # both ends of the 181 levels: pad_above 179 and 1, the reachable levels at either end
  n = len(windows) * len(pressures)
  sim, rng = _sim(n, 58)
  for e in range(n):
    sim.state['pressure'][e] = pressures[e % 2]
  now, here = _now(sim), _here(sim)
  sizes = [windows[e // 2] for e in range(n)]
  for e, m in enumerate(sizes):
    # append: m - 1 older observations and this call's; not: m observations, the newest made now
    _history(rng, sim, e, _spaced(now[e], m - 1) if append else _spaced(now[e] + 180, m), here[e], now[e])
  noise = _dev(rng.normal(0.0, 2.0, (n, 2)).astype(np.float32), sim)
  out = torch.full((n, OBS_DIM), float('nan'), dtype=torch.float32, device=sim.device)
  if entry == 'ble_observe_f32':
    _observe_f32(sim, sim._gp_struct, noise, out, append=1 if append else 0)
  else:
    levels = _dev(rng.uniform(-15.0, 15.0, (n, 181, 2)).astype(np.float32), sim)
    sim.observe(noise, append=append, out=out, forecast_levels=levels)
  torch.cuda.synchronize()
  rows = out.cpu().numpy()
  flags = int(sim.err_flags.item())
  unreachable = (rows[:, 16::3] == 0) & (rows[:, 17::3] == 1) & (rows[:, 18::3] == 1)
  first = [int(np.flatnonzero(~u)[0]) if (~u).any() else -1 for u in unreachable]
  last = [int(np.flatnonzero(~u)[-1]) if (~u).any() else -1 for u in unreachable]
  print(f'{entry} append={append}: flags {flags}, n_chol {sim._gp["n_chol"].cpu().numpy().tolist()}, reachable columns first {first} last {last}')
  assert sim._gp['n_chol'].cpu().numpy().tolist() == sizes
  bad = np.argwhere(~np.isfinite(rows))
  assert bad.size == 0, bad[:8].tolist()
  # the two pressures really put the reachable levels at the two ends of the 361 columns
  assert all(first[e] >= 0 for e in range(n))
  assert min(first[0::2]) > max(first[1::2]) and min(last[0::2]) > max(last[1::2]), (first, last)
  assert bool(torch.isfinite(sim._gp['chol']).all())
