"""Shared test helpers (golden loading, state conversion, tolerances)."""
import datetime as dt
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def golden(name):
  return np.load(os.path.join(GOLDEN, name + '.npz'))


def known_answers():
  with open(os.path.join(GOLDEN, 'reference_known_answers.json')) as f:
    return json.load(f)


def unix(iso):
  return int(dt.datetime.fromisoformat(iso).replace(tzinfo=dt.timezone.utc).timestamp())


STATE_FLOATS = ('x', 'y', 'pressure', 'ambient_temperature', 'internal_temperature', 'envelope_volume',
                'superpressure', 'mols_air', 'battery_charge', 'acs_power', 'acs_mass_flow',
                'solar_charging', 'power_load')
STATE_INTS = ('time_elapsed_s', 'sunrise_h', 'sunset')
STATE_U8 = ('status', 'last_command', 'alt_fsm', 'env_fsm', 'power_paused')
CONSTS = ('center_lat_deg', 'center_lng_deg', 'upwelling_infrared', 'alpha')

# Absolute floors that turn "1e-5 relative" into a usable bound for fields that pass
# through zero (position, ACS outputs, ...).  |a-b| <= rtol * max(|b|, floor).
FLOORS = dict(x=1000.0, y=1000.0, pressure=1.0, ambient_temperature=1.0, internal_temperature=1.0,
              envelope_volume=1.0, superpressure=100.0, mols_air=100.0, battery_charge=100.0,
              acs_power=10.0, acs_mass_flow=1e-3, solar_charging=10.0, power_load=10.0)


def rel_err(a, b, floor):
  a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
  return np.abs(a - b) / np.maximum(np.abs(b), floor)


def traj_state_at(d, step, rows=None):
  """Oracle-typed state dict from a trajectory fixture (f8/f9) at `step`."""
  import oracle
  n = d['x'].shape[0]
  rows = np.arange(n) if rows is None else rows
  st = oracle.new_state(len(rows))
  for k in STATE_FLOATS:
    st[k][:] = d[k][rows, step]
  for k in STATE_INTS:
    st[k][:] = d[k][rows, step]
  for k in STATE_U8:
    st[k][:] = d[k][rows, step]
  for k in CONSTS:
    st[k][:] = d[k][rows]
  st['start_unix'][:] = d['start_unix'][rows]
  return st


def feature_row(g, j, i):
  """Row dict (fields of ble_state_f32, float64) of env j at step i of a features fixture (F11/F12)."""
  row = {k: float(g[k][j, i]) for k in STATE_FLOATS}
  for k in ('status', 'last_command', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
    row[k] = int(g[k][j, i])
  for k in ('center_lat_deg', 'center_lng_deg', 'upwelling_infrared', 'alpha'):
    row[k] = float(g[k][j])
  row['start_unix'] = int(g['start_unix'][j])
  row['sunrise_h_rel'] = int(g['sunrise_h'][j, i] - g['start_unix'][j])
  row['sunset_rel'] = int(g['sunset'][j, i] - g['start_unix'][j])
  return row


def fixture_field(g):
  import numpy as np
  return (np.random.default_rng(int(g['field_seed'])).standard_normal((21, 21, 10, 9, 2)) * float(g['field_scale'])).astype(np.float32)


def wide_domain_states(n, seed):
  """ABI-typed initial states far outside the flight envelope the samplers draw (tests of the transition's robustness):
  pressures 1 200 .. 40 000 Pa (above the 21 km window and below the troposphere's top), stations up to 85 deg of latitude
  (polar day and night),
  balloons up to 850 km from the station (beyond the wind grid), up to 110 h into the episode (the boomeranged part of the
  forecast, later table segments of everything time-based), any temperatures / infrared / battery, safety layers in any
  state.  The envelope is consistent: a superpressure drawn in 20 .. 2 300 Pa fixes volume and air content."""
  import reset_host
  rng = np.random.default_rng(seed)
  init = reset_host.sample_initial_state(n, seed=seed)
  init['pressure'][:] = np.exp(rng.uniform(np.log(1200.0), np.log(40000.0), n))
  init['x'][:] = rng.uniform(-600e3, 600e3, n); init['y'][:] = rng.uniform(-600e3, 600e3, n)
  init['center_lat_deg'][:] = rng.uniform(-85, 85, n); init['center_lng_deg'][:] = rng.uniform(-180, 180, n)
  init['time_elapsed_s'][:] = rng.integers(0, 2200, n) * 180
  init['upwelling_infrared'][:] = rng.uniform(150, 400, n)
  init['battery_charge'][:] = rng.uniform(5, 3058, n)
  init['internal_temperature'][:] = rng.uniform(180, 300, n); init['ambient_temperature'][:] = rng.uniform(180, 280, n)
  sp = rng.uniform(20, 2300, n); vol = 1804.0 + 0.0199 * sp
  p = init['pressure'].astype(np.float64); t_int = init['internal_temperature'].astype(np.float64)
  init['mols_air'][:] = np.maximum((p + sp) * vol / (8.3144621 * t_int) - 6830.0, 0.0)
  init['envelope_volume'][:] = vol; init['superpressure'][:] = sp
  init['alt_fsm'][:] = rng.integers(0, 3, n); init['env_fsm'][:] = rng.integers(0, 5, n); init['power_paused'][:] = rng.integers(0, 2, n)
  return init


def hashed_decoder_params(seed=0, hidden=1000, output_gain=30.0):
  """Synthetic weights of the wind-field VAE decoder (generative/vae.py:140-148: 64 -> hidden x 3 -> 4410, ReLU) for
  fixture F15: [(kernel [in, out] float32, bias [out] float32)] x 4.  A pure integer hash of (layer, row, column, seed)
  -> uniform(-1, 1) scaled like LeCun initialisation, NON-zero biases -- no dependence on any library's random streams,
  so the generator (build container) and the test (GPU box) always rebuild the same numbers."""
  dims = [64, hidden, hidden, hidden, 7 * 7 * 90]
  out = []
  for layer, (a, b) in enumerate(zip(dims, dims[1:])):
    def unit(rows, cols, salt):
      with np.errstate(over='ignore'):
        h = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15) +
             np.arange(cols, dtype=np.uint64)[None, :] * np.uint64(0xC2B2AE3D27D4EB4F) +
             np.uint64((seed * 1000003 + layer * 7919 + salt) & 0xFFFFFFFF))
        h ^= h >> np.uint64(29); h *= np.uint64(0xBF58476D1CE4E5B9); h ^= h >> np.uint64(32)
        h *= np.uint64(0x94D049BB133111EB); h ^= h >> np.uint64(29)
      return (h >> np.uint64(11)).astype(np.float64) * (2.0 / (1 << 53)) - 1.0      # uniform [-1, 1)
    gain = output_gain if layer == 3 else np.sqrt(2.0)
    kernel = (unit(a, b, 1) * np.sqrt(3.0 / a) * gain).astype(np.float32)
    bias = (unit(1, b, 2)[0] * (0.5 if layer == 3 else 0.05)).astype(np.float32)
    out.append((kernel, bias))
  return out


def noise_cache_from_draws(seeds, offsets, n, seed, episode=0):
  """The `harmonic_cache` of ble_wind_noise_f32 / ble_noise_gen ([53][n] 32-bit words) holding GIVEN generator seeds
  [2][5] and offsets [2][5][4] for all n environments -- as if they had been drawn for (seed, episode): rows 5 k .. 5 k + 4 =
  (seed, ox, oy, op, ot) of harmonic k = 5 comp + h, rows 50 .. 52 the key (episode + 1, seed lo, seed hi)."""
  c = np.zeros((53, n), np.uint32)
  for comp in range(2):
    for h in range(5):
      k = 5 * comp + h
      c[5 * k] = np.uint32(int(seeds[comp][h]) & 0xFFFFFFFF)
      c[5 * k + 1:5 * k + 5] = np.asarray(offsets[comp][h], np.float32).view(np.uint32)[:, None]
  c[50] = np.uint32(episode + 1); c[51] = np.uint32(seed & 0xFFFFFFFF); c[52] = np.uint32((seed >> 32) & 0xFFFFFFFF)
  return c


def fixture_vehicle(d, vi):
  """Vehicle `vi` of the F16 fixture as a dict of the fields that DIFFER from the reference's defaults (the keyword form of
  oracle.step(vehicle=...) and VecSimulator.set_vehicle(...)); {} for the default vehicle."""
  import oracle
  names = [str(k) for k in d['vehicle_fields']]
  out = {}
  for k, v in zip(names, d['vehicles'][vi]):
    v = int(v) if k == 'power_safety_layer_enabled' else float(v)
    if v != oracle.VEHICLE_DEFAULTS[k]:
      out[k] = v
  return out


# F18 (tests/golden/f18_failures.npz): the reference's exceptions, case by case.  exc: 0 none, 1 AssertionError, 2 ValueError.
F18_CLASSES = (None, AssertionError, ValueError)


def f18_step_cases(d):
  return int(d['exc'].size)


def f18_state(d, rows):
  """Oracle-typed state dict of the transition cases `rows` of F18 (their pre-step states)."""
  import oracle
  rows = np.atleast_1d(rows)
  st = oracle.new_state(len(rows))
  for k in STATE_FLOATS + STATE_INTS + STATE_U8 + CONSTS:
    st[k][:] = d[k][rows]
  st['start_unix'][:] = d['start_unix'][rows]
  return st


def f18_oracle_class(first):
  """The exception class the reference raises for the oracle's first failing bits (oracle.step(..., per_env=True)['first']):
  its stride evaluates the pressure asserts before anything that raises ValueError; power_table's range check is an assert too."""
  import oracle
  if first & (oracle.ERR_PRESSURE_RANGE | oracle.ERR_TERMINAL_STEP | oracle.ERR_POWER_TABLE):
    return 1
  return 2 if first else 0


# Where the device's flag word deliberately differs from the oracle's per-environment bits (errors):
#  - a step of an episode that is already over: the reference asserts (balloon.py:288-290), a vectorised environment freezes
#    the lane and reports nothing;
#  - within 1 Pa below the atmosphere's first transition pressure the reference's finite-difference probe at p + 1 Pa asserts
#    (balloon.py:437-441); the device has no probe there and reports what the same stride also raises, SOLAR_RANGE.
F18_DEVICE_WORD = {'terminal_on_entry': 0, 'p_atm_in_down': 4, 'p_atm_in_stay': 4}
F18_DEVICE_BITS = 1 | 2 | 4 | 16      # the BLE_FLAG_* bits the oracle also reports (ERR_TERMINAL_STEP = 8 has no device bit)


def f18_device_word(d, j, oracle_env):
  """The flag word a launch of F18 step case j alone must report: the oracle's per-environment bits, but for F18_DEVICE_WORD."""
  return F18_DEVICE_WORD.get(str(d['names'][j]), int(oracle_env) & F18_DEVICE_BITS)


def f18_reference_class(d, j):
  return F18_CLASSES[int(d['exc'][j])]


# WindGP history rings written straight into a simulator's ring tensors (tests/test_gpu_belief.py, test_gpu_gp_query.py,
# test_gpu_carried_slab.py) -- random positions, pressures and errors instead of a flight.
GP_CAPACITY = 128
GP_HORIZON_S = 6 * 3600
GP_ROWS = 120


def observations(rng, count, spacing, end=None):
  """`count` observations in chronological order, the last at time `end` (default: spacing * (count - 1)):
  (xyp [count, 3] f32, t [count] i32, err [count, 2] f32)."""
  xyp = np.column_stack([rng.uniform(-2.0e5, 2.0e5, count), rng.uniform(-2.0e5, 2.0e5, count),
                         rng.uniform(5000.0, 14000.0, count)]).astype(np.float32)
  t = spacing * np.arange(count)
  if end is not None:
    t = t + (end - spacing * (count - 1))
  return xyp, t.astype(np.int32), rng.normal(0.0, 2.0, (count, 2)).astype(np.float32)


def write_ring(sim, env, obs):
  """Appends the observations the way ble_observe_f32 does: observation i in slot i % 128, count = their number."""
  import torch
  xyp, t, err = obs
  count = len(t)
  first = max(0, count - GP_CAPACITY)
  slots = torch.from_numpy(np.arange(first, count) % GP_CAPACITY).to(sim.device)
  sim._gp['xyp'][env, slots] = torch.from_numpy(xyp[first:]).to(sim.device)
  sim._gp['elapsed_s'][env, slots] = torch.from_numpy(t[first:]).to(sim.device)
  sim._gp['err_uv'][env, slots] = torch.from_numpy(err[first:]).to(sim.device)
  sim._gp['count'][env] = count


def ring_back(sim, env):
  """The ring of `env` as the device holds it, chronological: (xyp [m, 3], t [m], err [m, 2]) float64, m = min(count, 128)."""
  count = int(sim._gp['count'][env].item())
  m = min(count, GP_CAPACITY)
  slots = (np.arange(count - m, count) % GP_CAPACITY)
  g = {k: sim._gp[k][env].cpu().numpy() for k in ('xyp', 'elapsed_s', 'err_uv')}
  return g['xyp'][slots].astype(np.float64), g['elapsed_s'][slots].astype(np.float64), g['err_uv'][slots].astype(np.float64)


def gp_window(t, now):
  """WindGP's window at time `now` over observation times `t` (chronological): the indices with |t - now| < 6 h (strict,
  wind_gp.py:183), the newest 120 of them."""
  return np.flatnonzero(np.abs(np.asarray(t, np.float64) - float(now)) < GP_HORIZON_S)[-GP_ROWS:]


def slide_times(m, now, leaving=1, step=180):
  """Times of the m - 1 + (leaving - 1) observations to write BEFORE an observe() at `now` so that the call ends with a window of
  m - 1 + leaving rows, all inside 6 h, and the observe() one agent step later (now + step) finds exactly `leaving` of them -- the
  oldest ones -- outside the strict window while one row is appended: a window of m rows again for leaving = 1 (a slide at a
  partial window), of m rows after `leaving` >= 2 left at once (a refit).  The leaving ones stand between now + step - 6 h
  (excluded at now + step: age == 6 h is outside) and now - 6 h (still inside at now); the others 180 s apart up to now - 180."""
  assert 2 <= m <= GP_ROWS and 1 <= leaving <= 8
  stay = now - step * np.arange(m - 2, 0, -1)                  # m - 2 observations that stay: now - 180 (m - 2) .. now - 180
  leave = now + step - GP_HORIZON_S - 10 * np.arange(leaving - 1, -1, -1)
  return np.concatenate([leave, stay]).astype(np.int32)


def rings_back(sim):
  """ring_back of every environment from ONE copy of the ring tensors: a list of (xyp [m, 3], t [m], err [m, 2]) float64."""
  g = {k: sim._gp[k].cpu().numpy() for k in ('xyp', 'elapsed_s', 'err_uv', 'count')}
  out = []
  for env in range(sim.n):
    count = int(g['count'][env])
    m = max(0, min(count, GP_CAPACITY))
    slots = (np.arange(count - m, count) % GP_CAPACITY)
    out.append((g['xyp'][env][slots].astype(np.float64), g['elapsed_s'][env][slots].astype(np.float64),
                g['err_uv'][env][slots].astype(np.float64)))
  return out
