"""Numerics of the kernel's lane functions compiled ON THE HOST (tests/emul) against the oracle.

The HIP kernel (balloon_learning_environment_amd/csrc/*.h) is plain C++ with a thin
intrinsic layer, so the same source builds with g++.  This covers the arithmetic design
(mixed fp32/fp64 chain, atmosphere window, quadratic solar interpolation, safety layers)
on machines without a GPU.  It is not the product path -- the -m gpu tests exercise the
real library through the C ABI -- and libm here stands in for v_exp/v_log/v_rcp/v_sqrt.
"""
import os

import numpy as np
import pytest

import oracle
from helpers import FLOORS, STATE_FLOATS, golden, rel_err, traj_state_at

def _load_emul():
  from emul import emul as e     # tests/emul/emul.py (builds libble_emul.so with g++ on first use)
  return e


def _compare(st, o2, ctx):
  for k in ('status', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
    np.testing.assert_array_equal(st[k], o2[k], err_msg=f'{ctx} {k}')
  for k in STATE_FLOATS:
    e = rel_err(st[k], o2[k], FLOORS[k])
    assert e.max() <= 1e-5, f'{ctx} {k}: {e.max():.3g} at {e.argmax()}'


@pytest.mark.parametrize('name,use_field', [('f8_trajectories', False), ('f9_arena', True)])
def test_golden_trajectories_teacher_forced(name, use_field):
  e = _load_emul()
  d = golden(name)
  n, steps = d['actions'].shape
  valid = d['valid'] if 'valid' in d.files else np.ones((n, steps), np.uint8)
  field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5).astype(np.float32) if use_field else None
  for s in range(steps):
    rows = np.nonzero(valid[:, s])[0]
    st = e.state_from_oracle(traj_state_at(d, s, rows))
    o2 = e.oracle_from_state(st)
    w = None if use_field else d['wind_uv'][rows, s].astype(np.float32)
    r, t, eff, fl = e.step(st, d['actions'][rows, s], wind_uv=w, field=field)
    ro, to, eo, err = oracle.step(o2, d['actions'][rows, s], wind_uv=None if w is None else w.astype(np.float64), field=field)
    assert fl == 0 and err == 0
    _compare(st, o2, f'{name} step {s}')
    np.testing.assert_array_equal(eff, eo)
    np.testing.assert_allclose(r, ro, rtol=1e-5, atol=1e-5)


def test_random_states_and_layer_transition_chatter():
  """2 048 sampled initial states, 6 free-running steps each (teacher-forced per step), plus
  balloons parked within +-30 Pa of the 17 km lapse-rate transition, where the pressure
  chatters across the layer boundary every substep."""
  e = _load_emul()
  import reset_host
  n = 2048
  init = reset_host.sample_initial_state(n, seed=11)
  # park a quarter of the balloons at the transition pressure of their own atmosphere
  atm = reset_host.AtmosphereTables(init['alpha'])
  k = n // 4
  rng = np.random.default_rng(5)
  init['pressure'][:k] = np.float32(atm.pres[:k, 1] + rng.uniform(-30, 30, k))
  ost = oracle.new_state(n)
  for f in oracle.FLOAT_FIELDS:
    ost[f][:] = np.asarray(init[f], np.float64)
  for f in oracle.U8_FIELDS:
    ost[f][:] = init[f]
  ost['start_unix'][:] = init['start_unix']
  ost['sunrise_h'][:] = init['start_unix'] + init['sunrise_h_rel']; ost['sunset'][:] = init['start_unix'] + init['sunset_rel']
  field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5).astype(np.float32)
  st = e.state_from_oracle(ost)
  crossings = 0
  for s in range(6):
    live = st['status'] == 0
    o2 = e.oracle_from_state(st)
    act = rng.integers(0, 3, n).astype(np.uint8)
    p_before = st['pressure'].copy()
    r, t, eff, fl = e.step(st, act, field=field)
    ro, to, eo, err = oracle.step(o2, act, field=field)
    assert fl == 0 and (err & ~oracle.ERR_TERMINAL_STEP) == 0
    _compare({k_: v[live] for k_, v in st.items()}, {k_: v[live] for k_, v in o2.items()}, f'random step {s}')
    np.testing.assert_array_equal(eff[live], eo[live])
    np.testing.assert_allclose(r[live], ro[live], rtol=1e-5, atol=1e-5)
    p1 = atm.pres[:, 1]
    crossings += int(((p_before[:k] - p1[:k]) * (st['pressure'][:k] - p1[:k]) < 0).sum())
  assert crossings > 50   # the transition really is being crossed


def test_reset_path_host_build_matches_oracle():
  """ble_reset.h (device reset: full-fp64 solar, Newton cold start, sunrise search) built with
  g++ against the reference's golden F10 and the oracle on 512 sampled states."""
  import ctypes
  e = _load_emul()
  lib = e.lib()
  lib.emul_asin.restype = ctypes.c_double
  for x in np.linspace(-1, 1, 2001):
    assert abs(lib.emul_asin(ctypes.c_double(x)) - np.arcsin(x)) < 4e-16
  import reset_host
  d = golden('f10_reset')
  init = reset_host.sample_initial_state(512, seed=21)
  cases = [dict(alpha=d['alpha'], x=d['x'], y=d['y'], pressure=d['pressure'], lat=d['center_lat_deg'], lng=d['center_lng_deg'],
                ir=d['upwelling_infrared'], start=d['unix_s']),
           dict(alpha=init['alpha'], x=init['x'], y=init['y'], pressure=init['pressure'], lat=init['center_lat_deg'],
                lng=init['center_lng_deg'], ir=init['upwelling_infrared'], start=init['start_unix'])]
  for c in cases:
    f32 = {k: np.ascontiguousarray(v, np.float32) for k, v in c.items() if k != 'start'}
    start = np.ascontiguousarray(c['start'], np.int64)
    n = start.size
    outs = [np.empty(n) for _ in range(5)]; sr = np.empty(n, np.int64); ss = np.empty(n, np.int64); el = np.empty(n)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib.emul_reset_derive(ctypes.c_int64(n), P(f32['alpha']), P(f32['x']), P(f32['y']), P(f32['pressure']), P(f32['lat']),
                          P(f32['lng']), P(f32['ir']), P(start), *[P(o) for o in outs], P(sr), P(ss), P(el))
    as64 = {k: v.astype(np.float64) for k, v in f32.items()}
    ref, err = oracle.stable_init(as64['pressure'], as64['lat'], as64['lng'], as64['x'], as64['y'], start, as64['ir'], as64['alpha'])
    assert err == 0
    for o, k in zip(outs, ('ambient_temperature', 'internal_temperature', 'mols_air', 'envelope_volume', 'superpressure')):
      np.testing.assert_allclose(o, ref[k], rtol=1e-9, atol=1e-7, err_msg=k)
    la, lo = oracle.latlng_from_offset(np.radians(as64['lat']), np.radians(as64['lng']), as64['x'], as64['y'])
    eo, _, _, _ = oracle.solar_calculator(la, lo, start)
    assert np.abs(el - eo).max() < 1e-9
    sro, sso = oracle.next_sunrise_sunset(la, lo, start)
    np.testing.assert_array_equal(sr, sro); np.testing.assert_array_equal(ss, sso)


def test_philox_streams_host_build():
  import ctypes
  e = _load_emul()
  lib = e.lib()
  n = 20000
  u = np.empty(n); z = np.empty(n); g = np.empty(n)
  P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  lib.emul_philox(ctypes.c_uint64(7), ctypes.c_uint64(3), ctypes.c_uint32(0), ctypes.c_int64(n), P(u), P(z), P(g))
  assert 0 <= u.min() and u.max() < 1 and abs(u.mean() - 0.5) < 0.01 and abs(u.var() - 1 / 12) < 0.005
  assert abs(z.mean()) < 0.03 and abs(z.std() - 1) < 0.03
  assert abs(g.mean() - 1.2) < 0.04 and abs(g.var() - 1.2) < 0.1        # Gamma(1.2, 1)
  u2 = np.empty(n); z2 = np.empty(n); g2 = np.empty(n)
  lib.emul_philox(ctypes.c_uint64(7), ctypes.c_uint64(4), ctypes.c_uint32(0), ctypes.c_int64(n), P(u2), P(z2), P(g2))
  assert abs(np.corrcoef(u, u2)[0, 1]) < 0.03                           # env streams are independent
  # Philox4x32-10 known answer (Random123 kat_vectors: counter 0, key 0)
  lib.emul_philox(ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_int64(2), P(u[:2]), P(z[:2]), P(g[:2]))
  words = [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]               # out[0..3]; the stream pops from out[3]
  hi, lo = words[3], words[2]
  assert u[0] == (((hi << 32) | lo) >> 11) / 2.0 ** 53


def test_sampled_batch_every_env_within_1e_5_host_build():
  """The sample of the full-size GPU test (65 536 sampled states x 3 free-running steps), host
  build of the lane functions vs the oracle: EVERY environment within 1e-5 on every field.
  With fp32 thermal / ACS increments 13 of these 196 608 env-steps were beyond it (worst
  4.5e-5), and a solar threshold (day/night, panel shadow) flipped a stride early about twice
  per 10^6 env-steps; see DESIGN.md section 5 and tests/test_reference_conditioning.py."""
  e = _load_emul()
  import reset_host
  n = 65536
  init = reset_host.sample_initial_state(n, seed=43)
  ost = oracle.new_state(n)
  for f in oracle.FLOAT_FIELDS:
    ost[f][:] = np.asarray(init[f], np.float64)
  for f in oracle.U8_FIELDS:
    ost[f][:] = init[f]
  ost['start_unix'][:] = init['start_unix']
  ost['sunrise_h'][:] = init['start_unix'] + init['sunrise_h_rel']; ost['sunset'][:] = init['start_unix'] + init['sunset_rel']
  field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5).astype(np.float32)
  st = e.state_from_oracle(ost)
  rng = np.random.default_rng(44)
  worst = 0.0
  for s in range(3):
    live = st['status'] == 0
    o2 = e.oracle_from_state(st)
    act = rng.integers(0, 3, n).astype(np.uint8)
    r, t, eff, fl = e.step(st, act, field=field)
    ro, to, eo, err = oracle.step(o2, act, field=field, threads=8)
    assert fl == 0 and (err & ~oracle.ERR_TERMINAL_STEP) == 0
    for k in ('status', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
      np.testing.assert_array_equal(st[k][live], o2[k][live], err_msg=f'step {s} {k}')
    for k in STATE_FLOATS:
      err_k = rel_err(st[k], o2[k], FLOORS[k]); err_k[~live] = 0.0
      worst = max(worst, float(err_k.max()))
      assert err_k.max() <= 1e-5, f'step {s} {k}: {err_k.max():.3g} at env {err_k.argmax()}'
  print(f'host build, {n} envs x 3 steps: worst relative error {worst:.2e}')


def test_wide_domain_states_host_build():
  """helpers.wide_domain_states through the host build of the lane functions: the transition's arithmetic far outside the
  flight envelope (above the 21 km atmosphere window, beyond the wind grid, later segments of the forecast's boomerang, any
  safety-layer state) against the oracle, three steps, every environment."""
  from helpers import wide_domain_states
  e = _load_emul()
  n = 2048
  init = wide_domain_states(n, 3)
  ost = oracle.new_state(n)
  for f in oracle.FLOAT_FIELDS:
    ost[f][:] = np.asarray(init[f], np.float64)
  for f in oracle.U8_FIELDS:
    ost[f][:] = init[f]
  ost['start_unix'][:] = init['start_unix']; ost['time_elapsed_s'][:] = init['time_elapsed_s']
  ost['sunrise_h'][:] = init['start_unix'] + init['sunrise_h_rel']; ost['sunset'][:] = init['start_unix'] + init['sunset_rel']
  field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5).astype(np.float32)
  st = e.state_from_oracle(ost)
  rng = np.random.default_rng(9)
  stepped = 0
  for s in range(3):
    live = st['status'] == 0
    o2 = e.oracle_from_state(st)
    act = rng.integers(0, 3, n).astype(np.uint8)
    r, t, eff, fl = e.step(st, act, field=field)
    ro, to, eo, err = oracle.step(o2, act, field=field)
    assert fl == 0 and (err & ~oracle.ERR_TERMINAL_STEP) == 0
    for k in ('status', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
      np.testing.assert_array_equal(st[k][live], o2[k][live], err_msg=f'wide step {s} {k}')
    for k in STATE_FLOATS:
      err_k = rel_err(st[k], o2[k], FLOORS[k])[live]
      if k == 'acs_mass_flow':
        # venting: flow ~ sqrt(sp), so the superpressure's own tolerance (1e-5 x 100 Pa) is worth flow / (2 sp) x 1e-3 Pa of it
        ref = np.abs(o2[k][live])
        err_k = err_k - np.where(eo[live] == 2, ref / np.maximum(ref, FLOORS[k]) * 0.5 * 1e-3 / np.maximum(o2['superpressure'][live], 1e-30), 0.0)
      assert err_k.max() <= 1e-5, f'wide step {s} {k}: {err_k.max():.3g}'
    np.testing.assert_array_equal(eff[live], eo[live]); np.testing.assert_array_equal(t, to)
    stepped += int(live.sum())
  assert stepped > 3000 and (st['status'] != 0).mean() > 0.3


def test_dates_outside_the_samplers_range_and_the_reference_julian_day_quirk():
  """The transition turns unix seconds into the Julian date by the exact identity JD = 2440587.5 + unix / 86400 (32-bit
  fast path for 1970 .. 2106, 64-bit otherwise); the reference goes through year / month / day (solar.py:70-76).  Episodes
  starting in 1931 .. 1969 (negative unix time) and in 2101 .. 2199 (beyond 32 bits): every environment within 1e-5.
  The one place the two differ is a quirk of the reference's formula -- its `(month - 9.0) / 7.0` is not truncated, so the
  century correction of the non-leap years 2100, 2200, 2300 arrives in September instead of March: from March to August of
  those years the reference's Julian day is one day late (the oracle, pinned to it, reproduces that; shown below)."""
  import datetime as dt
  import reset_host
  e = _load_emul()
  n = 1024
  field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5).astype(np.float32)
  unix = lambda *a: int(dt.datetime(*a, tzinfo=dt.timezone.utc).timestamp())
  for lo, hi in ((unix(1931, 1, 1), unix(1969, 12, 30)), (unix(2101, 1, 1), unix(2199, 12, 30))):
    rng = np.random.default_rng(5)
    init = reset_host.sample_initial_state(n, seed=9)
    init['start_unix'][:] = rng.integers(lo, hi, n)
    lat, lng = reset_host.latlng_from_offset(np.radians(init['center_lat_deg'].astype(np.float64)), np.radians(init['center_lng_deg'].astype(np.float64)),
                                             init['x'].astype(np.float64), init['y'].astype(np.float64))
    sunrise, sunset = oracle.next_sunrise_sunset(lat, lng, init['start_unix'])
    ost = oracle.new_state(n)
    for f in oracle.FLOAT_FIELDS:
      ost[f][:] = np.asarray(init[f], np.float64)
    for f in oracle.U8_FIELDS:
      ost[f][:] = init[f]
    ost['start_unix'][:] = init['start_unix']; ost['time_elapsed_s'][:] = 0
    ost['sunrise_h'][:] = sunrise + 1800; ost['sunset'][:] = sunset
    st = e.state_from_oracle(ost)
    for s in range(3):
      live = st['status'] == 0
      o2 = e.oracle_from_state(st)
      act = rng.integers(0, 3, n).astype(np.uint8)
      r, t, eff, fl = e.step(st, act, field=field)
      ro, to, eo, err = oracle.step(o2, act, field=field)
      assert fl == 0
      _compare({k: v[live] for k, v in st.items()}, {k: v[live] for k, v in o2.items()}, f'dates {lo} .. {hi}, step {s}')
  # the quirk: noon of 2200-05-01 and of 2200-10-01 at (0, 0); the declination the reference sees in May is that of May 2nd
  zero = np.zeros(1)
  for when, off_by_a_day in ((unix(2200, 5, 1, 12), True), (unix(2200, 10, 1, 12), False), (unix(2100, 2, 20, 12), False), (unix(2100, 3, 2, 12), True)):
    el_ref = oracle.solar_calculator(zero, zero, np.array([when], np.int64))[0][0]
    el_next_day = oracle.solar_calculator(zero, zero, np.array([when + 86400], np.int64))[0][0]
    # the device's elevation (exact Julian date) through the host build of its solar probe
    import ctypes
    t = np.array([when], np.int64); f32 = lambda v: np.array([v], np.float32)
    el = np.empty(1, np.float32); fx = np.empty(1, np.float32)
    args = [f32(0), f32(0), f32(0), f32(0), t, el, fx]
    e.lib().emul_solar(ctypes.c_int64(1), *[a.ctypes.data_as(ctypes.c_void_p) for a in args])
    day_shift = abs(el_next_day - el_ref)                       # what one day of declination is worth at this date
    assert (abs(float(el[0]) - el_ref) > 0.3 * day_shift) == off_by_a_day, (when, el[0], el_ref, day_shift)


def test_battery_excess_threshold_is_the_reference_division():
  """BalloonState.excess_energy compares battery_charge / battery_capacity > 0.99 in float64 (balloon.py:231-238); the kernels
  compare the float32 charge with 3027.9746 instead (csrc/ble_step_core.h::battery_above_99_percent).  A correctly rounded
  division is monotone in its numerator, so the two agree on EVERY float32 iff they agree at the threshold and its neighbours."""
  thr = np.float32(3027.9746)
  assert float(thr).hex() == '0x1.7a7f300000000p+11'
  nb = [thr]
  for _ in range(4):
    nb.append(np.nextafter(nb[-1], np.float32(np.inf)))
  lo = thr
  for _ in range(4):
    lo = np.nextafter(lo, np.float32(-np.inf)); nb.append(lo)
  for b in nb + [np.float32(0.0), np.float32(3058.56), np.float32(2905.6), np.float32(3027.0), np.float32(3028.5)]:
    assert (np.float64(b) / 3058.56 > 0.99) == bool(b >= thr), b
  rng = np.random.default_rng(0)
  b = rng.uniform(3020.0, 3035.0, 200000).astype(np.float32)
  assert np.array_equal(b.astype(np.float64) / 3058.56 > 0.99, b >= thr)


def test_power_safety_thresholds_are_the_reference_divisions():
  """PowerSafetyLayer (power_safety.py:94-115) tests battery_charge / battery_capacity < 0.05 and
  (battery_charge - floating_charge) / battery_capacity < 0.025 in float64; the kernels compare the numerators with
  152.92801f and 76.464 (csrc/ble_physics.h::power_safety) when the capacity is the vehicle's 3058.56 Wh.  Monotonicity of the
  correctly rounded division makes that exact iff it holds at the thresholds and their neighbours."""
  cap = 3058.56
  t1 = np.float32(152.92801)
  assert float(t1).hex() == '0x1.31db240000000p+7'
  b = np.float32(t1)
  for _ in range(6):
    b = np.nextafter(b, np.float32(-np.inf))
  for _ in range(12):
    assert (np.float64(b) / cap < 0.05) == bool(b < t1), b
    b = np.nextafter(b, np.float32(np.inf))
  t2 = float.fromhex('0x1.31db22d0e5604p+6')
  assert t2 == 76.464
  d = t2
  for _ in range(6):
    d = np.nextafter(d, -np.inf)
  for _ in range(12):
    assert (d / cap < 0.025) == bool(d < t2), d
    d = np.nextafter(d, np.inf)
  rng = np.random.default_rng(1)
  x = rng.uniform(152.0, 154.0, 200000).astype(np.float32)
  assert np.array_equal(x.astype(np.float64) / cap < 0.05, x < t1)
  y = rng.uniform(76.0, 77.0, 200000)
  assert np.array_equal(y / cap < 0.025, y < t2)


def test_constant_divisions_are_correctly_rounded():
  """f_div_const / d_div_const (csrc/ble_physics.h: product with the rounded reciprocal + one fma-exact remainder correction) give
  the bits of the division they replace on every input the transition can hand them: all float32 positions from 2^-100 m to 600 km
  and zero (the forecast clips at 500 km; below 2^-100 m the quotient is subnormal), every whole second of the forecast's 48 hours, every whole second of a night."""
  import ctypes
  lib = _load_emul().lib()
  lib.emul_check_constant_divisions.restype = ctypes.c_longlong
  assert lib.emul_check_constant_divisions() == 0


# ----------------------------------------------------------------------------- err_flags against the reference (F18)
def _class_of(word):
  from balloon_learning_environment_amd import vec_state
  try:
    vec_state.raise_for_flags(int(word))
  except Exception as exc:      # noqa: BLE001 -- the class is what is compared
    return type(exc)
  return None


def test_absorptivity_thresholds_are_the_reference_predicate():
  """kAbsTLo / kAbsTHi (csrc/ble_physics.h) are the smallest and the largest double T the reference's
  total_absorptivity(absorptivity_ir(T), 0.0291) accepts, in its own float64 arithmetic (thermal.py:65-147)."""
  import re
  src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'balloon_learning_environment_amd', 'csrc',
                          'ble_physics.h')).read()
  lo = float.fromhex(re.search(r'kAbsTLo = (0x[0-9a-fp.+-]+);', src).group(1))
  hi = float.fromhex(re.search(r'kAbsTHi = (0x[0-9a-fp.+-]+);', src).group(1))

  def raises(t):
    a = 0.04587 + 0.000232 * (t - 210)
    f = a * (1.0 + (1.0 - a - 0.0291) / (1.0 - 0.0291))
    return f < 0.0 or f > 1.0
  assert not raises(lo) and raises(np.nextafter(lo, 0.0))
  assert not raises(hi) and raises(np.nextafter(hi, np.inf))
  assert not any(raises(t) for t in np.linspace(lo, hi, 100001))
  assert raises(12.28) and not raises(12.29) and raises(8400.0) and not raises(8000.0)


def test_f18_error_flags_host_build():
  """Every F18 transition case through the host build of agent_step, one environment per call: the flag word is the oracle's
  bits of that environment (helpers.F18_DEVICE_WORD: the deliberate differences), raise_for_flags raises the reference's
  class, and a clean case's next state is the reference's.  The 12.29 K case failed with the former T_int < 12.3 K predicate."""
  from helpers import f18_device_word, f18_reference_class, f18_state, f18_step_cases
  e = _load_emul()
  d = golden('f18_failures')
  for j in range(f18_step_cases(d)):
    name = str(d['names'][j])
    ost = f18_state(d, j)
    st = e.state_from_oracle(ost)
    sub = int(d['substeps'][j])
    _, _, _, env = e.step(st, d['actions'][j:j + 1], wind_uv=d['wind_uv'][j:j + 1], substeps=sub, per_env=True)
    _, _, _, err = oracle.step(ost, d['actions'][j:j + 1], wind_uv=d['wind_uv'][j:j + 1], substeps=sub, per_env=True)
    want = f18_device_word(d, j, err['env'][0])
    assert int(env[0]) == want, (name, int(env[0]), want)
    if name not in ('terminal_on_entry', 'p_atm_in_down', 'p_atm_in_stay'):
      assert _class_of(env[0]) is f18_reference_class(d, j), name
    if d['exc'][j] == 0:
      assert st['status'][0] == d['next_status'][j] and st['time_elapsed_s'][0] == d['next_time_elapsed_s'][j], name
      for k in STATE_FLOATS:
        assert rel_err(st[k], d['next_' + k][j], FLOORS[k]).max() <= 1e-5, (name, k)


def test_f18_reset_flags_host_build():
  """The reset's range checks (ble_reset.h) on F18's reset cases: the Earth-IR absorptivity and the pressure range raise at the
  reset, as in the reference; a station at |lat| >= 60 deg is computed."""
  import ctypes
  e = _load_emul()
  d = golden('f18_failures')
  n0 = int(d['exc'].size)
  names = [str(s) for s in d['names'][n0:]]
  m = len(names)
  f32 = {k: np.ascontiguousarray(d['reset_' + k], np.float32) for k in ('alpha', 'x', 'y', 'pressure', 'center_lat_deg',
                                                                         'center_lng_deg', 'upwelling_infrared')}
  start = np.ascontiguousarray(d['reset_unix_s'], np.int64)
  outs = [np.empty(m) for _ in range(5)]; sr = np.empty(m, np.int64); ss = np.empty(m, np.int64); el = np.empty(m)
  flags = np.zeros(m, np.uint32)
  P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  e.lib().emul_reset_derive_flags(ctypes.c_int64(m), P(f32['alpha']), P(f32['x']), P(f32['y']), P(f32['pressure']),
                                  P(f32['center_lat_deg']), P(f32['center_lng_deg']), P(f32['upwelling_infrared']), P(start),
                                  *[P(o) for o in outs], P(sr), P(ss), P(el), P(flags))
  for j, name in enumerate(names):
    want = None if name in ('reset_lat_60', 'reset_lat_m75') else (None, AssertionError, ValueError)[int(d['reset_exc'][j])]
    assert _class_of(flags[j]) is want, (name, int(flags[j]))
    if d['reset_exc'][j] == 0:
      assert abs(outs[1][j] - d['reset_out_internal_temperature'][j]) <= 1e-6 * d['reset_out_internal_temperature'][j], name


def test_nonfinite_state_flags_host_build():
  """A NaN in the state (no reference analogue) is reported as BLE_FLAG_NONFINITE, and only that: the absorptivity check
  lets NaN pass as the reference's comparisons do.  NaN inputs are kept off the GPU; this is their test."""
  from helpers import f18_state
  e = _load_emul()
  d = golden('f18_failures')
  clean = [str(s) for s in d['names']].index('clean')
  for k in ('internal_temperature', 'x'):
    st = e.state_from_oracle(f18_state(d, clean))
    st[k][0] = np.nan
    _, _, _, env = e.step(st, d['actions'][clean:clean + 1], wind_uv=d['wind_uv'][clean:clean + 1], per_env=True)
    assert int(env[0]) == 32, (k, int(env[0]))
    assert _class_of(env[0]) is FloatingPointError
