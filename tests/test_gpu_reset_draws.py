"""The sampled device reset (ble_reset_kernel's sampling branch through ble_reset_at_f32, ble_reset_seeded_f32 and
ble_reset_fleet_at_f32) against its NumPy twin (tests/reset_draws_host.py, written from DESIGN 3e), draw by draw, and against the
analytic laws of its eight fields.  Needs a real MI355X:  pytest -m gpu.

Draw by draw: alpha, start_unix, the episode counters and a fleet's vehicle index are exact.  x, y, pressure, centre latitude /
longitude and IR go through the device's fast fp64 log / exp / pow / sincos, whose error is orders below half a float32 step: the
stored value may round the other way, never further -- at most ONE float32 step from the twin's (x and y also 1e-6 m absolute, for
angles at a zero of cos or sin), and per field at least 99.9 % bitwise equal.  An environment with unrelated values is a flipped
accept / reject (its whole stream shifts): a failure, not a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import oracle  # noqa: E402
import reset_draws_host as rd  # noqa: E402

SEEDS = (0, 17, 2 ** 32, 0x9E3779B97F4A7C15, 2 ** 64 - 1)
OFFSETS = (0, 5, 2 ** 32 - 3)          # the last: the key carries into the fourth counter word inside the batch
EXACT = ('alpha', 'start_unix')
MIN_BITWISE = 0.999
IC = EXACT + rd.FLOAT_FIELDS


@pytest.fixture(scope='module')
def ble():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd import _lib, vec_state
  _lib.lib()     # raises loudly when libble_hip.so is missing -- no fallback
  return vec_state


def _state(sim):
  torch.cuda.synchronize(); sim.check_errors()
  return sim.get_state()


def _episodes(sim):
  return sim.episode.cpu().numpy().view(np.uint32)


def assert_draws(got, twin, rows=None, label=''):
  """The device's initial conditions on `rows` (all if None) against the twin's.  -> {field: (bitwise share, worst step)}."""
  rows = slice(None) if rows is None else rows
  out = {}
  for k in EXACT:
    np.testing.assert_array_equal(got[k][rows], twin[k][rows], err_msg=f'{label} {k}')
  for k in rd.FLOAT_FIELDS:
    a, b = got[k][rows], twin[k][rows]
    steps = rd.f32_steps(a, b)
    near = steps <= 1
    if k in ('x', 'y'):
      near |= np.abs(a.astype(np.float64) - b.astype(np.float64)) <= 1e-6
    share = float(np.mean(steps == 0))
    out[k] = (share, int(steps.max()))
    if share < 1.0:
      print(f'{label} {k}: {share:.5f} bitwise equal, worst {steps.max()} step(s)')
    bad = np.flatnonzero(~near)
    assert bad.size == 0, f'{label} {k}: {bad.size} values off the twin, first at {bad[0]}: {a[bad[0]]!r} vs {b[bad[0]]!r} ({steps[bad[0]]} steps)'
    assert share >= MIN_BITWISE, f'{label} {k}: {share:.5f} bitwise equal'
  return out


# ----------------------------------------------------------------------- scalar seed
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1000])
def test_scalar_seed_draw_by_draw(ble, n):
  """Either side of a wave and of the 256-lane workgroup; five seeds (both key words, all bits set); three batch offsets."""
  for off in OFFSETS:
    sim = ble.VecSimulator(n, env_offset=off)
    for e, seed in enumerate(SEEDS):                       # (successive resets of one simulator: episodes 0 .. 4)
      sim.reset_device(seed=seed)
      got = _state(sim)
      assert_draws(got, rd.sample(seed, off + np.arange(n, dtype=np.uint64), e), label=f'n={n} seed={seed:#x} offset={off} episode={e}')
      assert (_episodes(sim) == e + 1).all()


def test_scalar_seed_first_episode_of_every_seed(ble):
  """Episode 0 of each seed (the loop above meets a seed at one episode only), n = 257 at the carrying offset."""
  n, off = 257, OFFSETS[2]
  for seed in SEEDS:
    sim = ble.VecSimulator(n, env_offset=off)
    sim.reset_device(seed=seed)
    assert_draws(_state(sim), rd.sample(seed, off + np.arange(n, dtype=np.uint64), 0), label=f'seed={seed:#x}')


# ----------------------------------------------------------------------- episode counters, masks
def test_episode_counters_key_the_draws_and_wrap(ble):
  """Counters 0, 1, 7 and 2^32 - 1 across lanes: the draws use the counter before the increment; the last wraps to 0."""
  n = 257
  ep = np.array([0, 1, 7, 2 ** 32 - 1], np.uint32)[np.arange(n) % 4]
  sim = ble.VecSimulator(n, env_offset=5)
  sim.episode.copy_(torch.from_numpy(ep.view(np.int32)))
  sim.reset_device(seed=17)
  assert_draws(_state(sim), rd.sample(17, 5 + np.arange(n), ep), label='counters')
  after = _episodes(sim)
  np.testing.assert_array_equal(after, ep + np.uint32(1))
  assert (after[ep == 2 ** 32 - 1] == 0).all()


def test_masked_reset_redraws_only_masked_lanes(ble):
  n = 257
  rng = np.random.default_rng(2)
  sim = ble.VecSimulator(n)
  sim.reset_device(seed=17)
  ep = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
  ep[:8] = [0, 1, 7, 2 ** 32 - 1, 0, 1, 7, 2 ** 32 - 1]
  sim.episode.copy_(torch.from_numpy(ep.view(np.int32)))
  mask = (rng.random(n) < 0.4).astype(np.uint8)
  mask[:8] = [1, 1, 1, 1, 0, 0, 0, 0]; mask[-1] = 1
  sim.state['time_elapsed_s'].fill_(540); sim.state['status'].fill_(1)          # (a flown, ended batch)
  before = _state(sim)
  sim.reset_device(seed=2 ** 32, mask=torch.from_numpy(mask).cuda())
  after = _state(sim)
  m = mask != 0
  assert_draws(after, rd.sample(2 ** 32, np.arange(n), ep), rows=m, label='masked')
  for k in after:
    np.testing.assert_array_equal(after[k][~m], before[k][~m], err_msg=k)
  assert (after['status'][m] == 0).all() and (after['time_elapsed_s'][m] == 0).all()
  np.testing.assert_array_equal(_episodes(sim), ep + m.astype(np.uint32))


# ----------------------------------------------------------------------- seed per environment
def test_seeded_reset_draw_by_draw(ble):
  """reset_device_seeded: lane i is the twin at (seed[i], key 0), wherever it stands in the batch."""
  n = 257
  seeds = np.array(SEEDS, np.uint64)[np.arange(n) % len(SEEDS)]
  sim = ble.VecSimulator(n, env_offset=5)                     # (the offset plays no part)
  dev_seeds = torch.from_numpy(seeds.view(np.int64).copy()).cuda()
  for e in range(2):
    sim.reset_device_seeded(dev_seeds)
    assert_draws(_state(sim), rd.sample(seeds, 0, e), label=f'seeded episode={e}')
  assert (_episodes(sim) == 2).all()


# ----------------------------------------------------------------------- fleets
@pytest.mark.parametrize('n_vehicles', [1, 2, 3, 16])
def test_fleet_draws_its_vehicle_from_its_own_stream(ble, n_vehicles):
  """sample_per_episode: every index is the first word of stream(seed ^ 0xF1EE7C0DE, key, episode) scaled to the palette; the
  initial conditions are the plain twin's."""
  n, off, seed = 257, 5, 0x9E3779B97F4A7C15
  vehicles = [{} if j == 0 else {'payload_mass': 92.5 + 0.5 * j} for j in range(n_vehicles)]
  sim = ble.VecSimulator(n, env_offset=off)
  sim.set_fleet(vehicles, sample_per_episode=True)
  for e in range(2):
    sim.reset_device(seed=seed)
    got = _state(sim)
    want = rd.vehicle_index(seed, off + np.arange(n), e, n_vehicles)
    np.testing.assert_array_equal(sim.vehicle_index.cpu().numpy(), want)
    if n_vehicles > 1:
      assert len(set(want.tolist())) == n_vehicles
    assert_draws(got, rd.sample(seed, off + np.arange(n), e), label=f'fleet of {n_vehicles}, episode {e}')


# ----------------------------------------------------------------------- one large reset: the laws, the derived state
N_LAW = 65536


@pytest.fixture(scope='module')
def law_reset(ble):
  sim = ble.VecSimulator(N_LAW)
  for k, v in (('status', 2), ('time_elapsed_s', 999), ('last_command', 0), ('alt_fsm', 2), ('env_fsm', 3), ('power_paused', 1)):
    sim.state[k].fill_(v)                                         # everything the reset must overwrite
  for k in ('battery_charge', 'acs_power', 'acs_mass_flow', 'solar_charging', 'power_load', 'sunrise_h_rel', 'sunset_rel'):
    sim.state[k].fill_(7)
  sim.reset_device(seed=17)
  return _state(sim), rd.sample(17, np.arange(N_LAW), 0)


def test_large_reset_draw_by_draw_and_laws(law_reset):
  """65 536 environments at seed 17: draw by draw, then the CPU test's law checks on the DEVICE's values with the same bounds."""
  got, twin = law_reset
  shares = assert_draws(got, twin, label='65536')
  print('bitwise share, worst step: ' + ', '.join(f'{k} {s:.5f} {w}' for k, (s, w) in shares.items()))
  rd.assert_laws(got, 'device')
  # the try count is not part of the state.  The values above are those of the twin's accepted try in every environment (another
  # try gives an unrelated value below 315, and a longer or shorter loop at 315.0 an unrelated stream position for nothing after it),
  # so the rate is checked on the tries of the stream the device has just been held to
  rd.assert_acceptance(twin['tries'])
  assert twin['words'].max() > 64


def test_derived_state_after_sampled_reset(law_reset):
  """Every lane, every derived field: oracle.stable_init on the device's own sampled inputs, sunrise and sunset exact, fresh
  status / clocks / FSMs / battery."""
  got, _ = law_reset
  f = {k: got[k].astype(np.float64) for k in ('alpha', 'x', 'y', 'pressure', 'center_lat_deg', 'center_lng_deg', 'upwelling_infrared')}
  ref, err = oracle.stable_init(f['pressure'], f['center_lat_deg'], f['center_lng_deg'], f['x'], f['y'], got['start_unix'],
                                f['upwelling_infrared'], f['alpha'])
  assert err == 0
  for k, v in ref.items():
    np.testing.assert_allclose(got[k], v, rtol=2e-7, atol=1e-6, err_msg=k)      # fp32 storage of an fp64 result
  la, lo = oracle.latlng_from_offset(np.radians(f['center_lat_deg']), np.radians(f['center_lng_deg']), f['x'], f['y'])
  sr, ss = oracle.next_sunrise_sunset(la, lo, got['start_unix'])
  np.testing.assert_array_equal(got['start_unix'] + got['sunrise_h_rel'], sr + 1800)
  np.testing.assert_array_equal(got['start_unix'] + got['sunset_rel'], ss)
  assert (got['status'] == 0).all() and (got['time_elapsed_s'] == 0).all() and (got['last_command'] == 1).all()
  assert (got['alt_fsm'] == 0).all() and (got['env_fsm'] == 0).all() and (got['power_paused'] == 0).all()
  assert (got['battery_charge'] == np.float32(2905.6)).all()
  for k in ('acs_power', 'acs_mass_flow', 'solar_charging', 'power_load'):
    assert (got[k] == 0).all(), k
