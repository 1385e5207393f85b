"""The one-lane transition with a helper wave (csrc/ble_step_helper.h, _lib.STEP_FORM_HELPER) against the plain one-lane kernel
(_lib.step_form(1)) from the same state: every state array, reward, terminal, effective action, err_flags and active_count BIT FOR BIT.
The two forms call the same lane functions; what this guards is the hand-over between the main and the helper wave -- the record ring
and its wrap, the per-step publication, lanes and whole waves that are frozen, the reward's record of a lane whose episode ends inside
a step, the solar `near` path on the helper.  Every launch is awaited under a time limit of its own: a hand-over that never completes
shows as that limit, once -- the kernel is then still on the device, so the whole pytest process ends there (status 124) without
launching anything more and without waiting for the device at teardown.  Needs a real MI355X:  pytest -m gpu."""
import os
import sys
import time

import numpy as np
import pytest

from balloon_learning_environment_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

LIMIT_S = 20.0          # per launch; the largest one here takes milliseconds


def _await(what):
  ev = torch.cuda.Event()
  ev.record()
  deadline = time.monotonic() + LIMIT_S
  while not ev.query():
    if time.monotonic() > deadline:
      # a hung kernel cannot be taken off the device from here: no later test of this session may launch onto it, and the
      # interpreter's teardown would block on it -- end the process now, with the status of a time limit
      sys.stderr.write(f'\nFAILED {what}: not finished after {LIMIT_S} s -- the hand-over between the two waves did not complete; '
                       f'ending the test session\n')
      sys.stderr.flush()
      os._exit(124)


def _field(seed=6, scale=5.0):
  return (np.random.default_rng(seed).standard_normal((21, 21, 10, 9, 2)) * scale).astype(np.float32)


def _fly(form, init, acts_h, field, substeps=18, single=False):
  """acts_h [k, n] through one step_n launch (or, `single`, k step launches: they report the effective action too)."""
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd import vec_state as ble
  k, n = acts_h.shape
  acts = torch.from_numpy(acts_h).cuda()
  with _lib.step_form(form):
    sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(field)
    out = {}
    if single:
      rews, terms, effs = [], [], []
      for j in range(k):
        r, t = sim.step(acts[j], substeps=substeps)
        _await(f'form {form}, step launch {j}')
        rews.append(r.cpu().numpy().copy()); terms.append(t.cpu().numpy().copy()); effs.append(sim.effective_action.cpu().numpy().copy())
      out['reward'] = np.stack(rews); out['terminal'] = np.stack(terms); out['effective_action'] = np.stack(effs)
      out['active_count'] = sim.active_slots.cpu().numpy().copy()
    else:
      rew = torch.zeros((k, n), dtype=torch.float32).cuda(); term = torch.zeros((k, n), dtype=torch.uint8).cuda()
      cnt = torch.zeros((k, ble.COUNT_SLOTS), dtype=torch.int64).cuda()
      sim.step_n(acts, rew, term, cnt, substeps=substeps)
      _await(f'form {form}, {k}-step launch of {n} environments')
      out['reward'] = rew.cpu().numpy(); out['terminal'] = term.cpu().numpy(); out['active_count'] = cnt.cpu().numpy()
    out['err_flags'] = int(sim.err_flags.item())
    out['state'] = sim.get_state()
  return out


def _assert_same(a, b):
  for name in a['state']:
    np.testing.assert_array_equal(a['state'][name], b['state'][name], err_msg=name)
  np.testing.assert_array_equal(a['reward'].view(np.uint32), b['reward'].view(np.uint32), err_msg='reward')
  for name in ('terminal', 'active_count', 'effective_action'):
    if name in a:
      np.testing.assert_array_equal(a[name], b[name], err_msg=name)
  assert a['err_flags'] == b['err_flags']


def _both(init, acts, field, **kw):
  one = _fly(1, init, acts, field, **kw)
  helper = _fly(_lib.STEP_FORM_HELPER, init, acts, field, **kw)
  _assert_same(one, helper)
  return one


@pytest.mark.parametrize('n_steps', [1, 5, 32])
def test_199_environments(n_steps):
  """Three full waves and a 7-lane one; 19 records per step through a 16-record ring."""
  import reset_host
  n = 199
  init = reset_host.sample_initial_state(n, seed=31)
  acts = np.random.default_rng(32).integers(0, 3, (n_steps, n)).astype(np.uint8)
  _both(init, acts, _field())
  if n_steps == 1:
    _both(init, acts, _field(), single=True)          # ble_step_f32: the effective action too


@pytest.mark.parametrize('substeps', [1, 2, 3])
def test_short_steps(substeps):
  """The odd-stride tail, a step of two records, the reward's sun at k = substeps."""
  import reset_host
  n = 199
  init = reset_host.sample_initial_state(n, seed=33)
  acts = np.random.default_rng(34).integers(0, 3, (3, n)).astype(np.uint8)
  acts[:, :64] = 0                                    # DOWN: the reward reads the end-of-step record
  _both(init, acts, _field(), substeps=substeps)


def test_f18_failure_cases_tiled():
  """F18's transition cases (episodes that end at later strides, range flags) tiled to 130 environments, three steps: parking, the parked
  reward record, frozen lanes in later steps and the publication of a wave whose lanes are all frozen."""
  from helpers import f18_state, f18_step_cases, golden
  d = golden('f18_failures')
  cases = f18_step_cases(d)
  rows = np.arange(130) % cases
  ost = f18_state(d, rows)
  init = {k: v for k, v in ost.items() if k not in ('sunrise_h', 'sunset')}
  init['sunrise_h_rel'] = ost['sunrise_h'] - ost['start_unix']
  init['sunset_rel'] = ost['sunset'] - ost['start_unix']
  acts = np.repeat(d['actions'][rows][None], 3, 0).astype(np.uint8)
  one = _both(init, acts, _field(7, 3.0))
  assert (one['state']['status'] != 0).sum() >= 1, 'no episode of the batch ended'
  assert (one['terminal'][0] != 0).sum() < 130, 'every episode ended in the first step'


def _threshold_batch(substeps, seed):
  """256 environments, 64 per solar threshold (day / night, the two panel shadows, the 5 deg refraction branch), each placed so that one
  stride of its first step lands on the threshold: no wind, the start time chosen to the second with the oracle's fp64 solar calculator,
  then x moved (east: the hour angle) by bisection until that stride's elevation is on the threshold.  Returns the state and, per
  environment, the distance |sin(el) - sin(threshold)| of that stride in fp64."""
  import oracle
  import reset_host
  n = 256
  init = reset_host.sample_initial_state(n, seed=seed)
  rng = np.random.default_rng(seed)
  # corrected elevations of the four thresholds [deg] (csrc/ble_physics.h: kOmsDay ...; 5 deg uncorrected lies at the jump between the two
  # refraction formulas, 5.159618 | 5.160090 corrected: the middle of the jump separates the sides)
  thr = np.repeat(np.array([-4.242, 37.738149050524044, 34.39486500086289, 5.159854]), 64)
  lat0 = np.radians(init['center_lat_deg'].astype(np.float64)); lng0 = np.radians(init['center_lng_deg'].astype(np.float64))
  start = init['start_unix'].astype(np.int64)
  y = init['y'].astype(np.float64)
  kstar = rng.integers(0, substeps, n)

  def el_at(x, t):
    lat, lng = oracle.latlng_from_offset(lat0, lng0, x, y)
    return oracle.solar_calculator(lat, lng, t)[0]

  # the second of the day (next 24 h, 60 s grid first) at which the elevation passes the threshold
  x0 = init['x'].astype(np.float64)
  grid = np.arange(0, 86400, 60)
  els = np.stack([el_at(x0, start + g) for g in grid], 1) - thr[:, None]
  ok = np.zeros(n, bool); t_cross = np.zeros(n, np.int64)
  for i in range(n):
    sign = np.flatnonzero(np.signbit(els[i, :-1]) != np.signbit(els[i, 1:]))
    if sign.size:
      ok[i] = True; t_cross[i] = grid[sign[0]]
  lo_t, hi_t = t_cross.copy(), t_cross + 60
  for _ in range(7):                                   # to the second
    mid = (lo_t + hi_t) // 2
    same = np.signbit(el_at(x0, start + mid) - thr) == np.signbit(el_at(x0, start + lo_t) - thr)
    lo_t = np.where(same, mid, lo_t); hi_t = np.where(same, hi_t, mid)
  t_star = lo_t
  elapsed = np.maximum(t_star - 10 * kstar, 0)
  kstar = (t_star - elapsed) // 10
  t_eval = start + elapsed + 10 * kstar
  # x: +-3 km brackets one second of hour angle at every latitude of the sampler
  lo_x, hi_x = x0 - 3000.0, x0 + 3000.0
  f_lo = el_at(lo_x, t_eval) - thr
  for _ in range(60):
    mid = 0.5 * (lo_x + hi_x)
    same = np.signbit(el_at(mid, t_eval) - thr) == np.signbit(f_lo)
    lo_x = np.where(same, mid, lo_x); hi_x = np.where(same, hi_x, mid)
  x = (0.5 * (lo_x + hi_x)).astype(np.float32)
  bracketed = np.signbit(el_at(x0 - 3000.0, t_eval) - thr) != np.signbit(el_at(x0 + 3000.0, t_eval) - thr)
  init['x'] = x
  init['time_elapsed_s'] = elapsed.astype(init['time_elapsed_s'].dtype)
  el = el_at(x.astype(np.float64), t_eval)
  dist = np.abs(np.sin(np.radians(el)) - np.sin(np.radians(thr)))
  # the refraction branch point is a jump of the corrected elevation (5.159618 below, 5.160090 above an uncorrected 5 deg): the distance of
  # the uncorrected elevation to 5 deg is the corrected one's to its side of the jump over the formula's slope there (0.97; 0.9 bounds
  # it from below, i.e. the distance from above)
  side = np.where(el[192:] < 5.159854, 5.159618, 5.160090)
  dist[192:] = np.abs(np.radians(el[192:] - side)) * np.cos(np.radians(5.0)) / 0.9
  dist[~(ok & bracketed)] = np.inf
  return init, dist


@pytest.mark.parametrize('substeps', [18, 60])
def test_environments_on_the_solar_thresholds(substeps):
  """The helper's `near` path (sun_exact behind its vote).  The band formula on the host: a stride is re-decided in fp64 when its distance to
  a threshold in 1 - sin(el) is below sun_band(substeps) = 6e-8 (substeps / 18)^3; an environment counts when the host's fp64 distance is
  below a quarter of it (the rest covers the quadratic's 1.8e-8 (substeps / 18)^3 and the refraction's slope at the horizon)."""
  init, dist = _threshold_batch(substeps, seed=640 + substeps)
  band = 6.0e-8 * max(1.0, (substeps / 18.0) ** 3)
  for j, name in enumerate(('day / night', 'shadow 3.3 m', 'shadow 2.7 m', 'refraction 5 deg')):
    assert (dist[64 * j: 64 * j + 64] < 0.25 * band).sum() >= 1, f'no environment within the band of the {name} threshold'
  acts = np.random.default_rng(41).integers(0, 3, (2, 256)).astype(np.uint8)
  _both(init, acts, np.zeros((21, 21, 10, 9, 2), np.float32), substeps=substeps)


def test_mixed_status_bytes_and_dead_waves():
  """700 environments, every status byte among them, two whole waves frozen from the start, 32 steps."""
  import reset_host
  n = 700
  init = reset_host.sample_initial_state(n, seed=35)
  status = np.zeros(n, np.uint8)
  status[64:128] = 1; status[320:384] = 3              # two whole waves
  status[400:700:7] = np.arange(len(range(400, 700, 7)), dtype=np.uint8) % 4
  init['status'] = status
  init['battery_charge'][130:160] = np.linspace(0.05, 20.0, 30).astype(np.float32)     # out of power inside the rollout
  acts = np.random.default_rng(36).integers(0, 3, (32, n)).astype(np.uint8)
  one = _both(init, acts, _field())
  assert (one['state']['status'][130:160] != 0).sum() >= 1


def _frozen_lane0_batch(lane0_dead_at_launch):
  """199 environments; in the first group lane 0 is out of the game before the others -- frozen at launch, or out of power in the first
  step -- while every other lane of the group runs out of power within the first few of 32 steps: the group's later publications are made
  by a wave without a live lane, after steps that lane 0 took no part in."""
  import reset_host
  n = 199
  init = reset_host.sample_initial_state(n, seed=51)
  init['time_elapsed_s'][:64] = (init['sunset_rel'][:64] + 3600).astype(init['time_elapsed_s'].dtype)      # an hour into each one's own night
  init['battery_charge'][:64] = np.linspace(2.0, 30.0, 64).astype(np.float32)      # (183.7 W at night: 0.5 Wh per stride, 9 Wh per step)
  if lane0_dead_at_launch:
    init['status'][0] = 2
  else:
    init['battery_charge'][0] = np.float32(0.05)       # lane 0 first, in the first strides; lane 1 (2.2 Wh) and the rest later
  return init


@pytest.mark.parametrize('lane0_dead_at_launch', [True, False], ids=['lane0_frozen_at_launch', 'lane0_dies_first'])
def test_group_dies_out_after_its_lane_0(lane0_dead_at_launch):
  init = _frozen_lane0_batch(lane0_dead_at_launch)
  acts = np.random.default_rng(52).integers(0, 3, (32, 199)).astype(np.uint8)
  one = _both(init, acts, _field())
  ended_at = np.where(one['terminal'][:, :64] != 0, np.arange(32)[:, None], 32).min(0)      # first step each lane reports terminal
  assert ended_at.max() < 31, 'a lane of the first group was still live in the last step'
  assert ended_at[0] == 0 and ended_at[1:].max() > ended_at[0], 'lane 0 was not the first of its group to stop'


def _last_form(n, form=0, noise_seed=None):
  """One one-step launch of n environments under `form`; what the library says it launched."""
  import reset_host
  from balloon_learning_environment_amd import vec_state as ble
  init = reset_host.sample_initial_state(n, seed=53)
  acts = torch.zeros((1, n), dtype=torch.uint8).cuda()
  with _lib.step_form(form):
    sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(_field())
    rew = torch.zeros((1, n), dtype=torch.float32).cuda(); term = torch.zeros((1, n), dtype=torch.uint8).cuda()
    sim.step_n(acts, rew, term, noise_seed=noise_seed)
    _await(f'form {form}, one step of {n} environments')
    return _lib.lib().ble_last_step_form()


def test_form_query():
  """ble_last_step_form after real launches.  The automatic choice is the helper form exactly while every group of 64 environments has
  a second wave slot on its SIMD (256 x the device's compute units) and there is no wind-noise generator."""
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  full = 256 * torch.cuda.get_device_properties(0).multi_processor_count
  assert _last_form(full) == _lib.STEP_FORM_HELPER
  assert _last_form(32768 + 1) == _lib.STEP_FORM_HELPER
  assert _last_form(full + 64) == 1 and _last_form(full + 1) == 1
  assert _last_form(full, noise_seed=5) == 1                     # a wind-noise generator: the one-lane form
  assert _last_form(32768) == 4 and _last_form(199) == 4 and _last_form(199, noise_seed=5) == 4
  assert _last_form(199, form=_lib.STEP_FORM_HELPER) == _lib.STEP_FORM_HELPER
  assert _last_form(199, form=_lib.STEP_FORM_HELPER, noise_seed=5) == 1
  assert _last_form(full, form=1) == 1


def test_full_size_automatic_choice():
  """65 536 environments, two steps: the automatic choice launches the helper form there (ble_last_step_form right after the launch), and
  what it launches equals the forced one-lane form; the forced helper form equals it too."""
  import reset_host
  n = 65536
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  assert torch.cuda.get_device_properties(0).multi_processor_count >= 256, 'not an MI355X: 65 536 environments need 256 compute units'
  init = reset_host.sample_initial_state(n, seed=37)
  acts = np.random.default_rng(38).integers(0, 3, (2, n)).astype(np.uint8)
  field = _field()
  one = _both(init, acts, field)
  auto = _fly(0, init, acts, field)
  assert _lib.lib().ble_last_step_form() == _lib.STEP_FORM_HELPER, 'the automatic choice did not launch ble_step_helper_kernel at 65 536'
  _assert_same(one, auto)
