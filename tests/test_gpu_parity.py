"""GPU parity: the HIP path (through the C ABI of libble_hip.so) against the CPU oracle and
the committed golden vectors.  Needs a real MI355X:  pytest -m gpu.

Parity bar (BASELINE.json north_star): discrete outputs (effective action, safety FSM
states, status / terminal, clocks) bit-exact; float32 state within 1e-5 relative.
"Relative" uses |a-b| <= 1e-5 * max(|ref|, floor) with the per-field floors of
tests/helpers.py (fields such as x, y or acs_power pass through zero).
Identical inputs: the oracle is handed exactly the float32 values the kernel reads.
"""
import ctypes
import os

import numpy as np
import pytest

from balloon_learning_environment_amd import _lib      # (step_form)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

import oracle  # noqa: E402
from helpers import FLOORS, STATE_FLOATS, golden, rel_err, traj_state_at  # noqa: E402

RTOL = 1e-5


@pytest.fixture(scope='module')
def ble():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd import _lib, vec_state
  lib = _lib.lib()     # raises loudly when libble_hip.so is missing -- no fallback
  assert lib.ble_device_count() >= 1
  return vec_state


def _dev(a, dtype):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def abi_state_from_oracle(ost):
  st = {}
  for k, v in ost.items():
    if k == 'sunrise_h':
      st['sunrise_h_rel'] = (v - ost['start_unix']).astype(np.int32)
    elif k == 'sunset':
      st['sunset_rel'] = (v - ost['start_unix']).astype(np.int32)
    else:
      st[k] = v
  return st


def oracle_state_from_abi(st):
  ost = oracle.new_state(st['x'].size)
  for k in oracle.FLOAT_FIELDS:
    ost[k][:] = st[k].astype(np.float64)
  ost['start_unix'][:] = st['start_unix']
  ost['time_elapsed_s'][:] = st['time_elapsed_s']
  ost['sunrise_h'][:] = st['start_unix'] + st['sunrise_h_rel'].astype(np.int64)
  ost['sunset'][:] = st['start_unix'] + st['sunset_rel'].astype(np.int64)
  for k in oracle.U8_FIELDS:
    ost[k][:] = st[k]
  return ost


def compare_states(got, ost, ctx=''):
  """got: ABI state (numpy) after the GPU step; ost: oracle state after the oracle step."""
  for k in ('status', 'last_command', 'alt_fsm', 'env_fsm', 'power_paused'):
    np.testing.assert_array_equal(got[k], ost[k], err_msg=f'{ctx} {k}')
  np.testing.assert_array_equal(got['time_elapsed_s'], ost['time_elapsed_s'], err_msg=f'{ctx} time')
  np.testing.assert_array_equal(got['start_unix'] + got['sunrise_h_rel'], ost['sunrise_h'], err_msg=f'{ctx} sunrise')
  np.testing.assert_array_equal(got['start_unix'] + got['sunset_rel'], ost['sunset'], err_msg=f'{ctx} sunset')
  worst = {}
  for k in STATE_FLOATS:
    e = rel_err(got[k], ost[k], FLOORS[k])
    worst[k] = float(e.max()) if e.size else 0.0
    assert worst[k] <= RTOL, f'{ctx} {k}: rel err {worst[k]:.3g} at {int(e.argmax())}: {got[k][e.argmax()]} vs {ost[k][e.argmax()]}'
  return worst


def _trajectory_check(ble, name, use_field):
  d = golden(name)
  n, steps = d['actions'].shape
  valid = d['valid'] if 'valid' in d.files else np.ones((n, steps), np.uint8)
  field = None
  if use_field:
    field = (np.random.default_rng(int(d['field_seed'])).standard_normal((21, 21, 10, 9, 2)) *
             float(d['field_scale'])).astype(np.float32)
  worst_all = {k: 0.0 for k in STATE_FLOATS}
  worst_direct = {k: 0.0 for k in STATE_FLOATS}; worst_sens = {k: 0.0 for k in STATE_FLOATS}; flipped = [0]
  for s in range(steps):
    rows = np.nonzero(valid[:, s])[0]
    if rows.size == 0:
      continue
    ost = traj_state_at(d, s, rows)              # the reference's own state before step s
    sim = ble.VecSimulator(rows.size)
    sim.set_state(abi_state_from_oracle(ost))    # rounds to the kernel's float32 inputs
    o2 = oracle_state_from_abi(sim.get_state())  # the oracle gets exactly those values
    act = d['actions'][rows, s]
    if use_field:
      sim.set_grid(field)
      reward, terminal = sim.step(_dev(act, np.uint8))
      ro, to, eo, err = oracle.step(o2, act, field=field)
    else:
      # fixed wind per step: a constant grid would lose the (u, v) precision, so the wind is
      # injected through the additive noise input on top of an all-zero grid
      sim.set_grid(np.zeros((21, 21, 10, 9, 2), np.float32))
      w = d['wind_uv'][rows, s].astype(np.float32)
      reward, terminal = sim.step(_dev(act, np.uint8), noise_uv=_dev(w, np.float32))
      ro, to, eo, err = oracle.step(o2, act, wind_uv=w.astype(np.float64))
    torch.cuda.synchronize()
    sim.check_errors()
    assert err == 0
    got = sim.get_state()
    worst = compare_states(got, o2, ctx=f'{name} step {s}')
    for k, v in worst.items():
      worst_all[k] = max(worst_all[k], v)
    # DIRECTLY against the reference's stored next state (no transitivity through the oracle): the fixture flew from
    # float64 states, the device from their float32 roundings, and the reference's map amplifies that rounding
    # (tests/test_reference_conditioning.py) -- so the bound per entry is 1e-5 + what the rounding does to the reference
    # arithmetic itself, |oracle(float32 inputs) - fixture|, computed here.
    nxt = traj_state_at(d, s + 1, rows)
    for k in STATE_FLOATS:
      direct = rel_err(got[k], nxt[k], FLOORS[k]); sens = rel_err(o2[k], nxt[k], FLOORS[k])
      assert (direct - sens).max() <= RTOL, f'{name} step {s} {k}: {direct.max():.3g} vs the fixture (input-rounding sensitivity {sens.max():.3g})'
      worst_direct[k] = max(worst_direct[k], float(direct.max())); worst_sens[k] = max(worst_sens[k], float(sens.max()))
    for k in ('status', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
      same = o2[k] == nxt[k]                 # (where the rounding of the inputs flipped nothing in the reference arithmetic)
      np.testing.assert_array_equal(got[k][same], nxt[k][same], err_msg=f'{name} step {s} {k} vs the fixture')
      flipped[0] += int((~same).sum())
    np.testing.assert_array_equal(sim.effective_action.cpu().numpy(), eo, err_msg=f'{name} step {s} effective action')
    np.testing.assert_array_equal(terminal.cpu().numpy(), to)
    np.testing.assert_allclose(reward.cpu().numpy(), ro, rtol=RTOL, atol=RTOL)
  print(f'{name} vs the fixture directly: worst', {k: f'{v:.2g}' for k, v in worst_direct.items() if v > 1e-6},
        '; reference sensitivity to the float32 input rounding:', {k: f'{v:.2g}' for k, v in worst_sens.items() if v > 1e-6},
        f'; discrete fields flipped by that rounding: {flipped[0]}')
  return worst_all


def test_f8_trajectories_teacher_forced(ble):
  worst = _trajectory_check(ble, 'f8_trajectories', use_field=False)
  print('worst relative errors (f8):', {k: f'{v:.2g}' for k, v in worst.items()})


def test_f9_arena_steps_with_grid_wind(ble):
  worst = _trajectory_check(ble, 'f9_arena', use_field=True)
  print('worst relative errors (f9):', {k: f'{v:.2g}' for k, v in worst.items()})


def test_terminated_envs_are_frozen(ble):
  d = golden('f8_trajectories')
  rows = np.arange(d['actions'].shape[0])
  ost = traj_state_at(d, 40, rows)   # final states: some terminal
  assert (ost['status'] != 0).any()
  sim = ble.VecSimulator(rows.size)
  sim.set_state(abi_state_from_oracle(ost))
  before = sim.get_state()
  sim.set_grid(np.zeros((21, 21, 10, 9, 2), np.float32))
  reward, terminal = sim.step(_dev(np.full(rows.size, 2), np.uint8))
  torch.cuda.synchronize()
  after = sim.get_state()
  dead = before['status'] != 0
  for k in before:
    np.testing.assert_array_equal(before[k][dead], after[k][dead], err_msg=k)
  assert (terminal.cpu().numpy()[dead] == 1).all() and (reward.cpu().numpy()[dead] == 0).all()
  assert int(sim.active_count.item()) == int((~dead).sum())


# ---------------------------------------------------------------- function-level probes
def _call(lib, name, *args):
  """Calls a C-ABI entry point; torch tensors are passed as device pointers and are kept
  alive (referenced by `args`) until the call has been enqueued and synchronised."""
  raw = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
  code = getattr(lib, name)(*raw)
  assert code == 0, (name, code)
  torch.cuda.synchronize()


def test_probe_atmosphere_f1(ble):
  from balloon_learning_environment_amd import _lib
  lib = _lib.lib()
  d = golden('f1_atmosphere')
  for i, a in enumerate(d['alphas']):
    keep = d['pressures'] > 1.0
    p = _dev(d['pressures'][keep], np.float32); al = _dev(np.full(p.numel(), a), np.float32)
    h = torch.empty_like(p); t = torch.empty_like(p); fl = torch.zeros(1, dtype=torch.int32).cuda()
    _call(lib, 'ble_probe_atmosphere_f32', al, p, h, t, fl,
          p.numel(), None)
    ho, to, _, _ = oracle.at_pressure(float(np.float32(a)), p.cpu().numpy().astype(np.float64))
    assert int(fl.item()) == 0
    np.testing.assert_allclose(h.cpu().numpy(), ho, rtol=2e-7, atol=2e-3)
    np.testing.assert_allclose(t.cpu().numpy(), to, rtol=2e-7)
  # out-of-range pressures raise in the reference -> flag
  p = _dev([0.2, 110000.0], np.float32); al = _dev([0.5, 0.5], np.float32)
  h = torch.empty_like(p); t = torch.empty_like(p); fl = torch.zeros(1, dtype=torch.int32).cuda()
  _call(lib, 'ble_probe_atmosphere_f32', al, p, h, t, fl, 2, None)
  assert int(fl.item()) & _lib.FLAG_PRESSURE_RANGE


def test_probe_solar_f2(ble):
  from balloon_learning_environment_amd import _lib
  lib = _lib.lib()
  rng = np.random.default_rng(22)
  n = 20000
  lat0 = rng.uniform(-12, 12, n).astype(np.float32); lng0 = rng.uniform(-175, 175, n).astype(np.float32)
  x = rng.uniform(-4e5, 4e5, n).astype(np.float32); y = rng.uniform(-4e5, 4e5, n).astype(np.float32)
  t = rng.integers(1293840000, 1420000000, n).astype(np.int64)
  el = torch.empty(n, dtype=torch.float32).cuda(); fl = torch.empty_like(el)
  _call(lib, 'ble_probe_solar_f32', _dev(lat0, np.float32), _dev(lng0, np.float32),
        _dev(x, np.float32), _dev(y, np.float32), _dev(t, np.int64), el,
        fl, n, None)
  la, lo = oracle.latlng_from_offset(np.radians(lat0.astype(np.float64)), np.radians(lng0.astype(np.float64)),
                                     x.astype(np.float64), y.astype(np.float64))
  eo, _, fo, _ = oracle.solar_calculator(la, lo, t)
  el = el.cpu().numpy()
  # elevation: the kernel carries (sin, cos) of the elevation to ~1e-7; in degrees that is
  # <= 2e-5 deg away from the zenith/nadir, where asin amplifies
  mid = np.abs(eo) < 80
  assert np.abs(el - eo)[mid].max() < 3e-5
  assert np.abs(np.sin(np.radians(el.astype(np.float64))) - np.sin(np.radians(eo))).max() < 5e-7
  np.testing.assert_allclose(fl.cpu().numpy(), fo, rtol=1e-6)
  # golden spot checks through the same probe (reference values, fp64)
  d = golden('f2_solar')
  m = np.abs(np.degrees(d['lat_rad'])) < 60
  lat_deg = np.degrees(d['lat_rad'][m]).astype(np.float32); lng_deg = np.degrees(d['lng_rad'][m]).astype(np.float32)
  z = np.zeros(m.sum(), np.float32)
  el2 = torch.empty(int(m.sum()), dtype=torch.float32).cuda(); fl2 = torch.empty_like(el2)
  _call(lib, 'ble_probe_solar_f32', _dev(lat_deg, np.float32), _dev(lng_deg, np.float32),
        _dev(z, np.float32), _dev(z, np.float32), _dev(d['unix_s'][m], np.int64),
        el2, fl2, int(m.sum()), None)
  e2, _, f2, _ = oracle.solar_calculator(np.radians(lat_deg.astype(np.float64)), np.radians(lng_deg.astype(np.float64)),
                                         d['unix_s'][m])
  ok = np.abs(e2) < 80
  assert np.abs(el2.cpu().numpy() - e2)[ok].max() < 3e-5


def test_probe_solar_power_thermal_volume_acs(ble):
  from balloon_learning_environment_amd import _lib
  lib = _lib.lib()
  d = golden('f2_solar')
  el = d['att_el'].ravel().astype(np.float32); p = d['att_p'].ravel().astype(np.float32)
  keep = np.abs(np.abs(el) - 4.242) > 1e-3   # the day/night threshold itself is a discrete flip
  el, p = el[keep], p[keep]
  att = torch.empty(el.size, dtype=torch.float32).cuda(); pw = torch.empty_like(att)
  _call(lib, 'ble_probe_solar_power_f32', _dev(el, np.float32), _dev(p, np.float32),
        att, pw, el.size, None)
  ao, _ = oracle.solar_attenuation(el.astype(np.float64), p.astype(np.float64))
  po, _ = oracle.solar_power(el.astype(np.float64), p.astype(np.float64))
  np.testing.assert_allclose(att.cpu().numpy(), ao, rtol=3e-6, atol=1e-9)
  np.testing.assert_allclose(pw.cpu().numpy(), po, rtol=3e-6, atol=1e-4)

  d = golden('f3_thermal')
  keys = ('volume', 't_int', 't_amb', 'pressure', 'el', 'flux', 'ir')
  ins = [d[k].astype(np.float32) for k in keys]
  out = torch.empty(ins[0].size, dtype=torch.float32).cuda(); fl = torch.zeros(1, dtype=torch.int32).cuda()
  _call(lib, 'ble_probe_thermal_f32', *[_dev(a, np.float32) for a in ins], out, fl,
        ins[0].size, None)
  ref, _ = oracle.thermal_dtdt(*[a.astype(np.float64) for a in ins])
  np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-6, atol=1e-8)     # fp64 thermal model, fp32 attenuation input

  d = golden('f4_sp_volume')
  ins = [d[k].astype(np.float32) for k in ('mols_air', 't_int', 'pressure')]
  vol = torch.empty(ins[0].size, dtype=torch.float32).cuda(); sp = torch.empty_like(vol)
  _call(lib, 'ble_probe_sp_volume_f32', *[_dev(a, np.float32) for a in ins], vol, sp,
        ins[0].size, None)
  vo, so = oracle.sp_volume(*[a.astype(np.float64) for a in ins])
  np.testing.assert_allclose(vol.cpu().numpy(), vo, rtol=1e-7)
  np.testing.assert_allclose(sp.cpu().numpy(), so, rtol=1e-7, atol=1e-4)

  d = golden('f5_acs_power_table')
  pr = d['pr'].astype(np.float32)
  power = torch.empty(pr.size, dtype=torch.float32).cuda(); eff = torch.empty_like(power); md = torch.empty_like(power)
  _call(lib, 'ble_probe_acs_f32', _dev(pr, np.float32), power, eff, md,
        pr.size, None)
  po, eo, mo = oracle.acs(pr.astype(np.float64))
  np.testing.assert_allclose(power.cpu().numpy(), po, rtol=1e-6)   # fp64 tables on the fp32 input ratio
  np.testing.assert_allclose(eff.cpu().numpy(), eo, rtol=1e-6, atol=1e-7)
  np.testing.assert_allclose(md.cpu().numpy(), mo, rtol=1e-6, atol=1e-9)


def test_safety_layer_probe_matches_oracle_traces(ble):
  """`ble_probe_safety_f32`: each of the three layers on its own, 96 independent flights of 160 calls carried through the FSM
  byte (and, for the power layer, the two clocks it advances), against the oracle's per-layer traces.  Bit-exact."""
  from balloon_learning_environment_amd import _lib
  lib = _lib.lib()
  rng = np.random.default_rng(2024)
  n, T = 96, 160
  actions = rng.integers(0, 3, (T, n)).astype(np.uint8)
  fl = torch.zeros(1, dtype=torch.int32).cuda()

  def flight(layer, values, alpha=None, clocks=None, load=183.7, cap=3058.56):
    fsm = torch.zeros(n, dtype=torch.uint8).cuda(); eff = torch.empty(n, dtype=torch.uint8).cuda()
    out_a, out_f, out_c = [], [], []
    ck = None
    for t in range(T):
      if clocks is not None:
        now = _dev(clocks[0][t], np.int32)
        ck = torch.stack([now, ck[:, 1] if t else _dev(clocks[1], np.int32), ck[:, 2] if t else _dev(clocks[2], np.int32)], 1).contiguous()
      _call(lib, 'ble_probe_safety_f32', layer, _dev(actions[t], np.uint8), _dev(values[t], np.float32),
            None if alpha is None else _dev(alpha, np.float32), ck, load, cap, fsm, eff, fl, n, None)
      out_a.append(eff.cpu().numpy().copy()); out_f.append(fsm.cpu().numpy().copy())
      if ck is not None:
        out_c.append(ck.cpu().numpy().copy())
    assert int(fl.item()) == 0
    return np.array(out_a), np.array(out_f), np.array(out_c)

  # altitude: random walks in height across the three bands, as float32 pressures of each flight's atmosphere
  alpha = rng.uniform(0.05, 0.95, n).astype(np.float32)
  feet = 50500.0 + np.cumsum(rng.normal(0.0, 220.0, (T, n)), 0)
  pressure = np.stack([oracle.at_height(float(alpha[e]), feet[:, e] * 0.3048)[0] for e in range(n)], 1).astype(np.float32)
  ga, gf, _ = flight(0, pressure, alpha=alpha)
  for e in range(n):
    oa, of, err = oracle.altitude_safety_trace(float(alpha[e]), actions[:, e], pressure[:, e].astype(np.float64))
    assert err == 0
    np.testing.assert_array_equal(ga[:, e], oa); np.testing.assert_array_equal(gf[:, e], of)
  assert set(np.unique(gf)) == {0, 1, 2}

  # envelope: random walks over 0 .. 2400 Pa (all five states)
  sp = np.abs(1200.0 + np.cumsum(rng.normal(0.0, 160.0, (T, n)), 0)) % 2400.0
  sp = sp.astype(np.float32)
  ga, gf, _ = flight(1, sp)
  for e in range(n):
    oa, of = oracle.envelope_safety_trace(actions[:, e], sp[:, e].astype(np.float64))
    np.testing.assert_array_equal(ga[:, e], oa); np.testing.assert_array_equal(gf[:, e], of)
  assert set(np.unique(gf)) == {0, 1, 2, 3, 4}

  # power: four days in 36-minute calls, batteries draining at night; two load / capacity pairs (the transition's and the
  # reference test's small battery)
  for load, cap in ((183.7, 3058.56), (1.0, 100.0)):
    now = (np.arange(T)[:, None] * 2160 + rng.integers(0, 600, (T, n))).astype(np.int64)
    now.sort(axis=0)
    sunrise_h = rng.integers(3600, 86400, n); sunset = rng.integers(3600, 86400, n)
    batt = (cap * np.clip(0.06 + 0.08 * np.sin(now / 13750.0 + rng.uniform(0, 6.3, n)) + rng.normal(0, 0.01, (T, n)), 0.0, 1.0)).astype(np.float32)
    ga, gf, gc = flight(2, batt, clocks=(now, sunrise_h, sunset), load=load, cap=cap)
    for e in range(n):
      oa, osr, oss, op = oracle.power_safety_trace(actions[:, e], now[:, e], batt[:, e].astype(np.float64), sunrise_h[e], sunset[e], 0, load, cap)
      np.testing.assert_array_equal(ga[:, e], oa); np.testing.assert_array_equal(gf[:, e], op)
      np.testing.assert_array_equal(gc[:, e, 1], osr); np.testing.assert_array_equal(gc[:, e, 2], oss)
    assert gf.max() == 1 and gf.min() == 0 and (ga != actions).any()

  # argument checks: an unknown layer, the altitude layer without alpha, the power layer without clocks
  a = _dev(actions[0], np.uint8); v = _dev(sp[0], np.float32); fsm = torch.zeros(n, dtype=torch.uint8).cuda(); eff = torch.empty_like(fsm)
  for args in ((3, a.data_ptr(), v.data_ptr(), None, None), (0, a.data_ptr(), v.data_ptr(), None, None), (2, a.data_ptr(), v.data_ptr(), None, None)):
    assert lib.ble_probe_safety_f32(*args, 183.7, 3058.56, fsm.data_ptr(), eff.data_ptr(), fl.data_ptr(), n, None) == -1      # BLE_E_INVALID_ARG


def test_power_table_exact(ble):
  from balloon_learning_environment_amd import _lib
  lib = _lib.lib()
  d = golden('f5_acs_power_table')
  pr = d['pt_pr'].astype(np.float32); soc = d['pt_soc'].astype(np.float32)
  w = torch.empty(pr.size, dtype=torch.float32).cuda(); fl = torch.zeros(1, dtype=torch.int32).cuda()
  _call(lib, 'ble_power_table_f32', _dev(pr, np.float32), _dev(soc, np.float32), w,
        fl, pr.size, None)
  ref, err = oracle.power_table(pr.astype(np.float64), soc.astype(np.float64))
  np.testing.assert_array_equal(w.cpu().numpy(), ref)
  assert int(fl.item()) == 0 and err == 0
  bad = _dev([0.98, 5.01], np.float32)
  _call(lib, 'ble_power_table_f32', bad, _dev([1.0, 1.0], np.float32), w,
        fl, 2, None)
  assert int(fl.item()) & _lib.FLAG_POWER_TABLE


def test_forecast_f7_and_column(ble):
  from balloon_learning_environment_amd import _lib
  lib = _lib.lib()
  d = golden('f7_wind')
  grid = _dev(d['field'], np.float32)
  x = d['x'].astype(np.float32); y = d['y'].astype(np.float32); p = d['pressure'].astype(np.float32)
  t = d['elapsed_s'].astype(np.int32)
  u = torch.empty(x.size, dtype=torch.float32).cuda(); v = torch.empty_like(u)
  _call(lib, 'ble_forecast_f32', grid, 0, _dev(x, np.float32), _dev(y, np.float32),
        _dev(p, np.float32), _dev(t, np.int32), u, v, x.size, None)
  uo, vo = oracle.wind_forecast(d['field'], x.astype(np.float64), y.astype(np.float64), p.astype(np.float64),
                                t.astype(np.int64))
  # float32 query, fp64 interpolation like scipy's interpn: the float32 output is the rounded reference value
  scale = np.abs(d['field']).max()
  assert np.abs(u.cpu().numpy() - uo).max() < 1.5e-7 * scale and np.abs(v.cpu().numpy() - vo).max() < 1.5e-7 * scale
  # column == point lookups (grid_based_wind_field_test.py:225-234)
  levels = np.linspace(5000.0, 14000.0, 181).astype(np.float32)
  ncol = 64
  out = torch.empty((ncol, 181, 2), dtype=torch.float32).cuda()
  _call(lib, 'ble_forecast_column_f32', grid, 0, _dev(x[:ncol], np.float32),
        _dev(y[:ncol], np.float32), _dev(t[:ncol], np.int32), _dev(levels, np.float32),
        181, out, ncol, None)
  out = out.cpu().numpy()
  for c in range(0, ncol, 7):
    uo, vo = oracle.wind_forecast(d['field'], np.full(181, x[c], np.float64), np.full(181, y[c], np.float64),
                                  levels.astype(np.float64), np.full(181, t[c], np.int64))
    assert np.abs(out[c, :, 0] - uo).max() < 1.5e-7 * scale and np.abs(out[c, :, 1] - vo).max() < 1.5e-7 * scale


def test_invalid_arguments_return_codes(ble):
  from balloon_learning_environment_amd import _lib
  lib = _lib.lib()
  assert lib.ble_forecast_f32(None, 0, None, None, None, None, None, None, 4, None) == -1
  sim = ble.VecSimulator(4)
  sim.set_grid(np.zeros((21, 21, 10, 9, 2), np.float32))
  a = torch.zeros(4, dtype=torch.uint8).cuda()
  assert lib.ble_step_f32(ctypes.byref(sim._struct), a.data_ptr(), sim.grid.data_ptr(), 0, None, sim.reward.data_ptr(),
                          sim.terminal.data_ptr(), None, None, None, 4, 0, None) == -1     # substeps < 1
  assert lib.ble_step_f32(ctypes.byref(sim._struct), a.data_ptr(), sim.grid.data_ptr(), 0, None, sim.reward.data_ptr(),
                          sim.terminal.data_ptr(), None, None, None, 0, 18, None) == 0     # empty batch is a no-op
  # ABI 2: the carried WindGP slab is 7 620 doubles per environment; a caller that still allocates version 1's 7 260 is
  # refused instead of being overrun
  from balloon_learning_environment_amd import _abi
  assert lib.ble_abi_version() == 5
  gp = dict(xyp=torch.zeros(4, 128, 3).cuda(), elapsed_s=torch.zeros(4, 128, dtype=torch.int32).cuda(), err_uv=torch.zeros(4, 128, 2).cuda(),
            count=torch.zeros(4, dtype=torch.int32).cuda(), chol=torch.zeros(4, 7620, dtype=torch.float64).cuda(),
            n_chol=torch.zeros(4, dtype=torch.int32).cuda())
  h = _abi.BleGpHistoryF32()
  for name, ct in (('xyp', ctypes.c_float), ('elapsed_s', ctypes.c_int32), ('err_uv', ctypes.c_float), ('count', ctypes.c_int32),
                   ('chol', ctypes.c_double), ('n_chol', ctypes.c_int32)):
    setattr(h, name, ctypes.cast(ctypes.c_void_p(gp[name].data_ptr()), ctypes.POINTER(ct)))
  obs = torch.zeros(4, 1099).cuda()
  sim.reset_device(seed=1)        # (a valid state for the one call that does launch)
  call = lambda: lib.ble_observe_f32(ctypes.byref(sim._struct), sim.grid.data_ptr(), 0, None, None, ctypes.byref(h), 1, obs.data_ptr(),
                                     None, 4, None)
  h.chol_stride = 7260
  assert call() == -1
  h.chol_stride = 0
  assert call() == -1
  h.chol_stride = 7620
  assert call() == 0
  torch.cuda.synchronize()


# ---------------------------------------------------------------- sampled states, BASELINE configs
def _sampled_batch_parity(ble, n, steps, seed, threads, init=None):
  """Free-running GPU batch from reset_host.sample_initial_state; every step is checked
  against the oracle started from the GPU's own pre-step state (identical inputs).

  Discrete outputs must agree for EVERY environment and every float field of EVERY environment
  must be within 1e-5 (north star) -- no outlier budget.  The reference's vertical dynamics
  amplify errors (d(dp) ~ d(rho V - m) / sqrt|rho V - m|; the fp64 reference
  itself moves by up to 6e-3 under a 1-ulp perturbation of its fp32 inputs,
  tests/test_reference_conditioning.py), which is why the whole vertical chain including the
  thermal and ACS increments is fp64 in the kernel and the solar thresholds are re-decided in fp64.
  """
  import reset_host
  wide = init is not None
  init = init if wide else reset_host.sample_initial_state(n, seed=seed)
  sim = ble.VecSimulator(n)
  sim.set_state(init)
  field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  sim.set_grid(field)
  rng = np.random.default_rng(seed + 1)
  total = 0; outliers = 0; worst = 0.0
  for s in range(steps):
    before = sim.get_state()
    live = before['status'] == 0
    o2 = oracle_state_from_abi(before)
    act = rng.integers(0, 3, n).astype(np.uint8)
    reward, terminal = sim.step(_dev(act, np.uint8))
    torch.cuda.synchronize()
    sim.check_errors()
    ro, to, eo, err = oracle.step(o2, act, field=field, threads=threads)
    assert (err & ~oracle.ERR_TERMINAL_STEP) == 0
    got = sim.get_state()
    for k in ('status', 'last_command', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
      np.testing.assert_array_equal(got[k][live], o2[k][live], err_msg=f'step {s} {k}')
    np.testing.assert_array_equal(got['start_unix'][live] + got['sunrise_h_rel'][live], o2['sunrise_h'][live])
    np.testing.assert_array_equal(sim.effective_action.cpu().numpy()[live], eo[live])
    np.testing.assert_array_equal(terminal.cpu().numpy(), to)
    bad = np.zeros(n, bool)
    for k in STATE_FLOATS:
      e = rel_err(got[k], o2[k], FLOORS[k])
      e[~live] = 0.0
      if wide and k == 'acs_mass_flow':
        # a venting balloon: the valve flow is ~ sqrt(sp), d ln(flow) / d sp = 1 / (2 sp), and the superpressure itself is held
        # to 1e-5 x max(sp, 100 Pa) = 1e-3 Pa -- which near sp -> 0 is all of the flow (1e-8 .. 1e-7 kg/s on such a stride)
        ref = np.abs(o2[k])
        e -= np.where(eo == 2, ref / np.maximum(ref, FLOORS[k]) * 0.5 * (RTOL * FLOORS['superpressure']) / np.maximum(o2['superpressure'], 1e-30), 0.0)
      bad |= e > RTOL
      worst = max(worst, float(e.max()))
    rew_err = np.abs(reward.cpu().numpy() - ro)
    rew_err[~live] = 0.0
    bad |= rew_err > 1e-5
    total += int(live.sum()); outliers += int(bad.sum())
  return total, outliers, worst


def test_long_rollout_checkpoints_match_oracle(ble):
  """Two-day rollouts (1 000 agent steps = 50 h: past the 48 h wind-field horizon where the time
  axis boomerangs, through two sunsets and every safety-layer state), with auto-reset of
  terminated environments; every 125th step is checked against the oracle from the GPU's own
  pre-step state."""
  import reset_host
  n = 2048
  sim = ble.VecSimulator(n)
  sim.set_state(reset_host.sample_initial_state(n, seed=77))
  field = (np.random.default_rng(3).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  sim.set_grid(field)
  rng = np.random.default_rng(78)
  total = outliers = 0; worst = 0.0; max_elapsed = 0
  for s in range(1000):
    act = rng.integers(0, 3, n).astype(np.uint8)
    # a sticky policy, so that balloons really climb and sink instead of dithering
    if s % 40 < 25:
      act = np.where(np.arange(n) % 3 == 0, 2, np.where(np.arange(n) % 3 == 1, 0, act)).astype(np.uint8)
    check = s % 125 == 124 or s >= 995
    if check:
      before = sim.get_state()
      live = before['status'] == 0
      o2 = oracle_state_from_abi(before)
    reward, terminal = sim.step(_dev(act, np.uint8))
    if check:
      torch.cuda.synchronize(); sim.check_errors()
      ro, to, eo, err = oracle.step(o2, act, field=field, threads=8)
      got = sim.get_state()
      for k in ('status', 'last_command', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
        np.testing.assert_array_equal(got[k][live], o2[k][live], err_msg=f'step {s} {k}')
      np.testing.assert_array_equal(sim.effective_action.cpu().numpy()[live], eo[live])
      bad = np.zeros(n, bool)
      for k in STATE_FLOATS:
        e = rel_err(got[k], o2[k], FLOORS[k]); e[~live] = 0.0
        bad |= e > RTOL; worst = max(worst, float(e.max()))
      total += int(live.sum()); outliers += int(bad.sum())
      max_elapsed = max(max_elapsed, int(got['time_elapsed_s'].max()))
    if s % 50 == 49:                      # new episodes for the terminated ones (same seed stream)
      mask = (sim.state['status'] != 0).to(torch.uint8)
      sim.reset_device(seed=5, mask=mask)
  sim.check_errors()
  print(f'long rollout: {total} checked env-steps, {outliers} beyond 1e-5, worst {worst:.2g}, max elapsed {max_elapsed / 3600:.1f} h')
  assert max_elapsed > 48 * 3600
  assert outliers == 0 and worst <= RTOL


@pytest.mark.parametrize('substeps', [1, 7, 36, 60])
def test_other_step_lengths_every_env(ble, substeps):
  """Balloon.simulate_step takes any time_delta that is a multiple of the stride (balloon.py:316-319); the agent step is 18
  strides.  1, 7, 36 and BLE_MAX_SUBSTEPS = 60 strides per step (10 s .. 10 min) on 4 096 sampled environments, four steps each:
  every environment within 1e-5 of the oracle stepping with the same stride count; 61 is refused."""
  import reset_host
  n = 4096
  field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  sim = ble.VecSimulator(n); sim.set_state(reset_host.sample_initial_state(n, seed=substeps)); sim.set_grid(field)
  rng = np.random.default_rng(substeps)
  for s in range(4):
    before = sim.get_state()
    live = before['status'] == 0
    o2 = oracle_state_from_abi(before)
    act = rng.integers(0, 3, n).astype(np.uint8)
    reward, terminal = sim.step(_dev(act, np.uint8), substeps=substeps)
    torch.cuda.synchronize(); sim.check_errors()
    ro, to, eo, err = oracle.step(o2, act, field=field, threads=16, substeps=substeps)
    got = sim.get_state()
    assert (got['time_elapsed_s'][live] - before['time_elapsed_s'][live] <= 10 * substeps).all()
    for k in ('status', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
      np.testing.assert_array_equal(got[k][live], o2[k][live], err_msg=f'{substeps} strides, step {s}: {k}')
    for k in STATE_FLOATS:
      e = rel_err(got[k], o2[k], FLOORS[k])[live]
      assert e.max() <= RTOL, f'{substeps} strides, step {s}: {k} {e.max():.3g}'
    np.testing.assert_array_equal(terminal.cpu().numpy(), to)
    np.testing.assert_allclose(reward.cpu().numpy()[live], ro[live], rtol=0, atol=1e-5)
  with pytest.raises(Exception):
    sim.step(_dev(act, np.uint8), substeps=61)


def test_solar_threshold_crossings_at_60_strides_every_env(ble):
  """the band inside which a stride's solar decisions are re-made on the reference's fp64 chain must follow the step
  length (the quadratic interpolation's error grows with its cube: csrc/ble_physics.h, sun_band).  32 768 environments at
  BLE_MAX_SUBSTEPS = 60 strides (10 minutes = 2.5 deg of hour angle per step): half of them start 0 .. 600 s before their own
  sunset / sunrise (the -4.242 deg day / night threshold is crossed inside the step), the other half anywhere in the day (the
  two panel-shadow elevations and the 5 deg refraction branch are crossed by ~3 % of them per step).  Every environment's
  charging, battery, load and temperatures within 1e-5 of the oracle; a decision taken one stride early would move the battery by
  1.3 Wh (4e-4) and the internal temperature by 0.07 K (3e-4)."""
  import reset_host
  n, substeps = 32768, 60
  field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  init = reset_host.sample_initial_state(n, seed=606)
  rng = np.random.default_rng(606)
  half = n // 2
  edge = np.where(rng.random(half) < 0.5, init['sunset_rel'][:half], init['sunrise_h_rel'][:half] - 1800)
  elapsed = np.empty(n, np.int64)
  elapsed[:half] = np.maximum(edge - rng.integers(0, 600, half), 0)
  elapsed[half:] = rng.integers(0, 86400, n - half)
  init['time_elapsed_s'] = elapsed.astype(init['time_elapsed_s'].dtype)
  sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(field)
  for s in range(2):
    before = sim.get_state()
    live = before['status'] == 0
    o2 = oracle_state_from_abi(before)
    act = rng.integers(0, 3, n).astype(np.uint8)
    reward, terminal = sim.step(_dev(act, np.uint8), substeps=substeps)
    torch.cuda.synchronize(); sim.check_errors()
    ro, to, eo, err = oracle.step(o2, act, field=field, threads=16, substeps=substeps)
    got = sim.get_state()
    for k in ('status', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
      np.testing.assert_array_equal(got[k][live], o2[k][live], err_msg=f'step {s}: {k}')
    # What a solar decision moves -- charging, battery, load, the two temperatures -- and the position: every environment at 1e-5.
    # The vertical chain (pressure, superpressure, volume, air, ACS) is the reference's ill-conditioned part
    # (tests/test_reference_conditioning.py: the oracle's own output moves beyond 1e-5 under a 1-ulp change of its float32 inputs, and
    # 60 strides amplify over 3.3 x the reference's step): held to 1e-5 on all but a counted handful, none of them grossly off.
    solar_fields = ('solar_charging', 'battery_charge', 'power_load', 'internal_temperature', 'ambient_temperature', 'x', 'y')
    for k in STATE_FLOATS:
      e = rel_err(got[k], o2[k], FLOORS[k])[live]
      if k in solar_fields:
        assert e.max() <= RTOL, f'60 strides, step {s}: {k} {e.max():.3g} at env {int(np.flatnonzero(live)[e.argmax()])}'
      else:
        assert (e > RTOL).mean() <= 2e-3 and e.max() <= 5e-3, f'60 strides, step {s}: {k} {(e > RTOL).sum()} beyond 1e-5, worst {e.max():.3g}'
    np.testing.assert_array_equal(terminal.cpu().numpy(), to)
    np.testing.assert_allclose(reward.cpu().numpy()[live], ro[live], rtol=0, atol=1e-5)


def test_shards_reset_and_fly_what_the_unsharded_batch_does(ble):
  """ABI 4 (`ble_reset_at_f32`, `ble_wind_noise_at_f32`, `ble_noise_gen.env_offset`): the Philox streams of the device reset and
  of the wind noise are keyed by the GLOBAL environment index, so the shards of a batch -- here 1 500 + 2 596 of 4 096, as two
  simulators with env_offset 0 and 1 500 -- reset to, draw the noise of and fly through exactly the states of the unsharded
  batch with the same seeds: initial states, a noise evaluation, an 8-step fused rollout in the ground-truth wind (noise
  generated in-kernel), and a second, masked reset.  Bit for bit on every array."""
  n, cut, k = 4096, 1500, 8
  field = (np.random.default_rng(3).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  acts = torch.from_numpy(np.random.default_rng(4).integers(0, 3, (k, n)).astype(np.uint8)).cuda()
  whole = ble.VecSimulator(n)
  parts = [(ble.VecSimulator(cut, env_offset=0), slice(0, cut)), (ble.VecSimulator(n - cut, env_offset=cut), slice(cut, n))]

  def same(what):
    got = whole.get_state()
    for sim, sl in parts:
      st = sim.get_state()
      for name in got:
        np.testing.assert_array_equal(st[name], got[name][sl], err_msg=f'{what}: {name}, shard at {sim.env_offset}')

  for sim in [whole] + [p for p, _ in parts]:
    sim.set_grid(field); sim.reset_device(seed=99); sim.check_errors()
  same('reset')
  assert len(np.unique(whole.get_state()['x'])) > n - 8                      # (distinct draws: not one stream n times)
  noise = whole.wind_noise(seed=5).cpu().numpy()
  for sim, sl in parts:
    np.testing.assert_array_equal(sim.wind_noise(seed=5).cpu().numpy(), noise[sl])
  rew = torch.zeros((k, n), dtype=torch.float32).cuda(); term = torch.zeros((k, n), dtype=torch.uint8).cuda()
  whole.step_n(acts, rew, term, noise_seed=5)
  for sim, sl in parts:
    r = torch.zeros((k, sim.n), dtype=torch.float32).cuda(); t = torch.zeros((k, sim.n), dtype=torch.uint8).cuda()
    sim.step_n(acts[:, sl].contiguous(), r, t, noise_seed=5)
    np.testing.assert_array_equal(r.cpu().numpy(), rew.cpu().numpy()[:, sl])
    np.testing.assert_array_equal(t.cpu().numpy(), term.cpu().numpy()[:, sl])
  same('fused rollout in the ground-truth wind')
  mask = torch.from_numpy((np.random.default_rng(6).random(n) < 0.3).astype(np.uint8)).cuda()
  whole.reset_device(seed=99, mask=mask)
  for sim, sl in parts:
    sim.reset_device(seed=99, mask=mask[sl].contiguous())
  same('second, masked reset')
  np.testing.assert_array_equal(np.concatenate([p.episode.cpu().numpy() for p, _ in parts]), whole.episode.cpu().numpy())


def test_shards_decode_the_unsharded_batchs_per_env_wind_fields(ble):
  """with per_env_fields=True every shard used to decode IDENTICAL wind fields (the latents came from one generator stream that
  did not know the shard's offset).  The latents are keyed by (seed, GLOBAL environment index, episode) now: two VecBalloonArenas with
  env_offset 0 / 96 hold exactly the grids of the 256-environment arena's lanes, after reset() and after a masked refresh; and the fields
  of different environments differ."""
  from balloon_learning_environment_amd.env import balloon_arena
  n, cut = 256, 96
  whole = balloon_arena.VecBalloonArena(n, seed=17, per_env_fields=True)
  parts = [(balloon_arena.VecBalloonArena(cut, seed=17, per_env_fields=True, env_offset=0), slice(0, cut)),
           (balloon_arena.VecBalloonArena(n - cut, seed=17, per_env_fields=True, env_offset=cut), slice(cut, n))]
  # (the latents are equal bit for bit; the decoder's four library GEMMs run at another batch size in a shard -- another tiling,
  #  another summation order -- so the decoded winds agree to GEMM rounding, not to the bit)
  sampler = whole.wind_field._wind_field_sampler
  lat = sampler.sample_latents_keyed(torch.arange(n, device='cuda'), whole.sim.episode, whole._seed)
  for arena, sl in parts:
    idx = torch.arange(arena.num_envs, device='cuda')
    assert torch.equal(sampler.sample_latents_keyed(idx + arena.sim.env_offset, arena.sim.episode, arena._seed), lat[sl])
    assert float((arena._grids - whole._grids[sl]).abs().max()) <= 1e-3, f'shard at {arena.sim.env_offset} after reset()'
  flat = whole._grids.reshape(n, -1)
  assert not torch.equal(flat[0], flat[cut]) and float((flat[0] - flat[cut]).abs().max()) > 0.1         # (what ADVICE r5 found equal)
  assert len({float(v) for v in flat[:, 1234].cpu()}) > n - 4
  mask = torch.from_numpy((np.random.default_rng(8).random(n) < 0.25).astype(np.uint8)).cuda()
  before = whole._grids.clone()
  whole.reset_lanes(mask); assert whole.refresh_fields() == int(mask.sum())
  for arena, sl in parts:
    arena.reset_lanes(mask[sl].contiguous()); arena.refresh_fields()
    assert float((arena._grids - whole._grids[sl]).abs().max()) <= 1e-3, f'shard at {arena.sim.env_offset} after a masked refresh'
  changed = (whole._grids.reshape(n, -1) != before.reshape(n, -1)).any(dim=1).cpu().numpy()
  np.testing.assert_array_equal(changed, mask.cpu().numpy() != 0)


def test_checkpoint_from_another_shard_offset_rekeys_noise(ble):
  """load_state_dict takes the checkpoint's env_offset; the harmonic-draw cache (keyed by seed and episode, not by offset) and
  the generators prepared launches hold are re-keyed with it -- a simulator that loads shard B's checkpoint flies shard B's noise."""
  n, k = 512, 4
  field = (np.random.default_rng(3).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  acts = torch.from_numpy(np.random.default_rng(4).integers(0, 3, (k, n)).astype(np.uint8)).cuda()
  b = ble.VecSimulator(n, env_offset=4096); b.set_grid(field); b.reset_device(seed=9)
  ckpt = b.state_dict()
  rb = torch.zeros(k, n, device='cuda'); tb = torch.zeros(k, n, dtype=torch.uint8, device='cuda')
  b.step_n(acts, rb, tb, noise_seed=7)
  a = ble.VecSimulator(n, env_offset=0); a.set_grid(field); a.reset_device(seed=9)
  ra = torch.zeros(k, n, device='cuda'); ta = torch.zeros(k, n, dtype=torch.uint8, device='cuda')
  launch = a.prepare_step_n(acts, ra, ta, noise_seed=7)
  launch(); torch.cuda.synchronize()                 # shard A's own flight: fills A's draw cache for (seed 7, episode 1)
  assert not torch.equal(ra, rb)
  a.load_state_dict(ckpt)
  assert a.env_offset == 4096
  launch(); torch.cuda.synchronize(); a.check_errors()          # the PREPARED launch, after the load
  assert torch.equal(ra, rb) and torch.equal(ta, tb)
  sa, sb = a.get_state(), b.get_state()
  for name in sa:
    np.testing.assert_array_equal(sa[name], sb[name], err_msg=name)
  bad = dict(ckpt, noise_primitive_version=1)
  with pytest.raises(ValueError, match='noise primitive'):
    a.load_state_dict(bad)


def test_wide_domain_states_every_env(ble):
  """16 385 environments drawn far outside the flight envelope (helpers.wide_domain_states): from 1 200 Pa (above the
  atmosphere window's 21 km) to 40 000 Pa, 85 deg of latitude, beyond the wind grid, 110 h into the episode, safety layers
  in any state; half of them burst, deflate or run out of power within three steps.  Same bar as everywhere: every
  environment, every field, 1e-5; discrete outputs and the terminal strides exact."""
  from helpers import wide_domain_states
  n = 16385
  total, outliers, worst = _sampled_batch_parity(ble, n, steps=3, seed=77, threads=16, init=wide_domain_states(n, 77))
  print(f'wide-domain states: {total} env-steps, worst relative error {worst:.3g}')
  assert total > 25000 and outliers == 0


def test_one_lane_kernel_episodes_ending_inside_a_step_match_oracle(ble):
  """The one-lane kernel's stride loop is wave-uniform: a lane whose episode ends inside an agent step parks its final state in LDS on a
  rare path and takes it back after the loop (csrc/ble_step_core.h, agent_step).  Forced here (_lib.step_form(1): the host would pick the
  four-wave kernel at this size) on a batch in which a good part of the environments run out of power or burst inside the rollout, every
  environment against the oracle from the kernel's own pre-step state: status, strides run (time_elapsed_s), state, reward, terminal."""
  import reset_host
  n = 4096
  init = reset_host.sample_initial_state(n, seed=4242)
  init['battery_charge'][: n // 4] = np.linspace(0.05, 30.0, n // 4).astype(np.float32)          # out of power within a few strides .. steps
  init['superpressure'][n // 4: n // 4 + 256] = np.linspace(2300.0, 2379.0, 256).astype(np.float32)   # close to the burst limit
  with _lib.step_form(1):
    total, outliers, worst = _sampled_batch_parity(ble, n, 6, seed=4243, threads=8, init=init)
  assert outliers == 0, (outliers, total, worst)
  assert total < 6 * n - 200                       # (episodes did end: the live count of later steps is smaller)


def test_config_4096_envs_random_policy(ble):
  """BASELINE.json configs[1]: 4 096 vectorised envs, random policy, one decoded wind field."""
  total, outliers, worst = _sampled_batch_parity(ble, 4096, steps=12, seed=41, threads=8)
  print(f'4096 envs: {total} env-steps, {outliers} beyond 1e-5, worst {worst:.2g}')
  assert outliers == 0 and worst <= RTOL


def test_config_65536_envs_full_size(ble):
  """BASELINE.json configs[2] at full size: every environment of a 65 536 batch against the oracle."""
  total, outliers, worst = _sampled_batch_parity(ble, 65536, steps=3, seed=43, threads=32)
  print(f'65536 envs: {total} env-steps, {outliers} beyond 1e-5, worst {worst:.2g}')
  assert outliers == 0 and worst <= RTOL


def test_full_size_properties_and_determinism(ble):
  """Size-independent properties at 65 536 envs: bitwise determinism, clocks, bounds, exact
  wind displacement, frozen terminal lanes, per-env grids == shared grid."""
  import reset_host
  n = 65536
  init = reset_host.sample_initial_state(n, seed=77)
  field = (np.random.default_rng(3).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  acts = torch.from_numpy(np.random.default_rng(5).integers(0, 3, (8, n)).astype(np.uint8)).cuda()

  def rollout(per_env_grid=False, m=n):
    sim = ble.VecSimulator(m)
    sim.set_state({k: v[:m] for k, v in init.items()})
    if per_env_grid:
      sim.set_grid(np.broadcast_to(field, (m,) + field.shape).copy(), per_env=True)
    else:
      sim.set_grid(field)
    rewards = []
    stepped = 0                    # environments that were live when a step began: what the counter must add up to
    for k in range(acts.shape[0]):
      stepped += int((sim.state['status'] == 0).sum().item())
      r, _ = sim.step(acts[k, :m].contiguous())
      rewards.append(r.clone())
    torch.cuda.synchronize()
    sim.check_errors()
    assert int(sim.active_count.item()) == stepped
    return sim.get_state(), torch.stack(rewards).cpu().numpy(), stepped

  a, ra, live_a = rollout()
  b, rb, live_b = rollout()
  for k in a:
    np.testing.assert_array_equal(a[k], b[k], err_msg=f'non-deterministic {k}')
  np.testing.assert_array_equal(ra, rb)
  assert live_a == live_b
  ok = a['status'] == 0
  assert (a['time_elapsed_s'][ok] == 8 * 180).all()                       # balloon_env_test.py:77-85
  assert ((a['time_elapsed_s'] % 10) == 0).all() and (a['time_elapsed_s'] <= 8 * 180).all()
  assert (ra >= 0).all() and (ra <= 1).all()                              # reward_range
  assert (a['battery_charge'] >= 0).all() and (a['battery_charge'] <= np.float32(3058.56)).all()
  assert (a['mols_air'] >= 0).all() and (a['superpressure'] >= 0).all()
  assert (a['envelope_volume'][a['superpressure'] == 0] <= 1804.0 + 1e-3).all()
  # (the counter itself is checked inside rollout against the environments whose status was OK when each step began)
  assert live_a <= 8 * n and live_a >= 8 * int(ok.sum())                  # an ended episode is never counted again
  # per-env forecasts (config 5 layout) with identical grids reproduce the shared-grid run bit for bit
  m = 2048
  c, rc, _ = rollout(per_env_grid=True, m=m)
  for k in c:
    np.testing.assert_array_equal(c[k], a[k][:m], err_msg=f'per-env grid {k}')


def test_balloon_env_gym_surface(ble):
  """The reference-shaped facade: BalloonEnv / BalloonArena (balloon_env_test.py, balloon_arena_test.py)."""
  from balloon_learning_environment_amd.env import balloon_env
  from balloon_learning_environment_amd.env.balloon import balloon as balloon_lib
  env1 = balloon_env.BalloonEnv(seed=123)
  env2 = balloon_env.BalloonEnv(seed=123)
  s1, s2 = env1.get_simulator_state().balloon_state, env2.get_simulator_state().balloon_state
  assert s1.x == s2.x and s1.pressure == s2.pressure                    # seeding determinism (:208-241)
  assert units_distance(s1) <= 200.0                                    # balloon_arena_test.py: within 200 km
  obs_shape = env1.observation_space.shape
  total_reward = 0.0
  for i in range(20):
    a = i % 3
    o1, r1, t1, info1 = env1.step(a)
    o2, r2, t2, info2 = env2.step(a)
    assert o1.shape == obs_shape and o1.dtype == np.float32
    np.testing.assert_array_equal(o1, o2); assert r1 == r2 and t1 == t2
    assert 0.0 <= r1 <= 1.0
    assert info1['time_elapsed'].total_seconds() == 180 * (i + 1)
    total_reward += r1
  # the kernel's reward equals the host restatement of perciatelli_reward_function
  host = balloon_env.perciatelli_reward_function(env1.get_simulator_state())
  assert abs(host - r1) < 2e-5
  # out of power is terminal and stepping a terminal balloon raises (balloon.py:288-290)
  st = env1.arena.get_balloon_state()
  st.battery_charge = type(st.battery_charge)(watt_hours=1e-4)
  st.date_time = st.date_time  # unchanged
  env1.arena.set_balloon_state(st)
  _, _, terminal, info = env1.step(0)
  if not terminal:   # daytime: the panels may out-charge the load; force night-like drain by repeating
    for _ in range(3):
      st = env1.arena.get_balloon_state(); st.battery_charge = type(st.battery_charge)(watt_hours=0.0)
      st.solar_charging = type(st.solar_charging)(watts=0.0)
      env1.arena.set_balloon_state(st)
      _, _, terminal, info = env1.step(0)
      if terminal:
        break
  if terminal:
    assert info['out_of_power']
    with pytest.raises(AssertionError):
      env1.step(1)


def test_perciatelli_features_device_forecast(ble):
  """the 1099-feature observation with the device forecast kernel behind
  GridBasedWindField, against the reference's PerciatelliFeatureConstructor output (F11).
  Tolerance 2e-4 absolute: ble_forecast_f32 hands the host constructor float32 winds (6e-8 relative on u, v; the
  reference's interpn returns float64) and the fixture's float64 states reach the device as float32; the bearing feature
  is arccos(.)/pi, whose error near aligned/opposed winds is sqrt(2 eps) ~ 1e-4 (tests/test_gpu_observe.py computes that
  sensitivity of the reference itself).  The device constructor (ble_observe_f32) is held to 1e-5 there."""
  import test_features_host as tfh
  from balloon_learning_environment_amd.env import grid_based_wind_field, grid_wind_field_sampler
  g = golden('f11_features')
  wf = grid_based_wind_field.GridBasedWindField(grid_wind_field_sampler.GaussianFieldSampler())
  wf.set_field(tfh.field_of(g))
  for j in range(3):
    got = tfh.run_constructor(g, wf, j, n_steps=16)
    want = g['features'][j, :16]
    unreach = lambda f: (f[:, 16::3] == 0) & (f[:, 17::3] == 1) & (f[:, 18::3] == 1)
    np.testing.assert_array_equal(unreach(got), unreach(want))
    err = np.abs(got.astype(np.float64) - want)
    assert err.max() <= 2e-4, (j, err.max())
    assert np.median(err[err > 0]) < 1e-6 if (err > 0).any() else True


def test_balloon_env_emits_perciatelli_observation(ble):
  from balloon_learning_environment_amd.env import balloon_env, features
  env = balloon_env.BalloonEnv(seed=7)
  assert env.observation_space.shape == (1099,)
  obs = env.reset()
  assert obs.shape == (1099,) and obs.dtype == np.float32
  for a in (2, 2, 1, 0):
    obs, r, term, info = env.step(a)
    assert env.observation_space.contains(obs)
  named = features.NamedPerciatelliFeatures(obs)
  st = env.get_simulator_state().balloon_state
  np.testing.assert_allclose(named.balloon_pressure, st.pressure, rtol=1e-5)
  assert int(named.last_command) == 0
  assert named.level_is_valid(named.wind_column_center())


def units_distance(s):
  return (s.x.km ** 2 + s.y.km ** 2) ** 0.5


def test_fp64_primitives_on_device(ble):
  """The kernel's libm-free fp64 primitives, measured on the hardware."""
  from balloon_learning_environment_amd import _lib
  lib = _lib.lib()
  rng = np.random.default_rng(0)

  def run(op, x):
    xd = _dev(x, np.float64); yd = torch.empty_like(xd)
    _call(lib, 'ble_probe_f64_prims', xd, yd, op, x.size, None)
    return yd.cpu().numpy()

  x = np.concatenate([rng.uniform(0.5, 2.0, 4000), rng.uniform(1e-3, 1e6, 4000), 10.0 ** rng.uniform(-8, 8, 2000)])
  rel = lambda a, b: np.abs(a - b) / np.abs(b)
  seed_rcp = rel(run(0, x), 1.0 / x).max(); seed_rsq = rel(run(2, x), 1.0 / np.sqrt(x)).max()
  print(f'v_rcp_f64 seed rel err {seed_rcp:.3g}, v_rsq_f64 seed rel err {seed_rsq:.3g}')
  assert seed_rcp < 1e-7 and seed_rsq < 1e-7          # one Newton step from these seeds: ~1e-14
  assert rel(run(1, x), 1.0 / x).max() < 1e-14
  assert rel(run(3, x), 1.0 / np.sqrt(x)).max() < 2e-14
  assert rel(run(4, x), np.sqrt(x)).max() < 1e-15
  assert np.abs(run(5, x) - np.log(x)).max() < 1e-13 and rel(run(5, x[x > 1.1]), np.log(x[x > 1.1])).max() < 2e-14
  t = rng.uniform(-40, 40, 8000)
  assert rel(run(6, t), np.exp(t)).max() < 2e-15
  a = rng.uniform(-200, 200, 8000)
  assert np.abs(run(7, a) - np.sin(a)).max() < 3e-16 and np.abs(run(8, a) - np.cos(a)).max() < 3e-16


@pytest.mark.parametrize('wide', [False, True])
def test_fused_rollout_equals_single_steps(ble, wide):
  """ble_step_n_f32 (K steps in one launch, state in registers) == K x ble_step_f32, bit for bit -- from sampled flight
  states and from helpers.wide_domain_states (half of which end inside the rollout)."""
  import reset_host
  from helpers import wide_domain_states
  n, k = 4096, 7
  init = wide_domain_states(n, 5) if wide else reset_host.sample_initial_state(n, seed=5)
  # make a few environments terminate inside the rollout
  init['battery_charge'][:64] = 0.2
  field = (np.random.default_rng(1).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  acts = torch.from_numpy(np.random.default_rng(2).integers(0, 3, (k, n)).astype(np.uint8)).cuda()
  a = ble.VecSimulator(n); a.set_state(init); a.set_grid(field)
  b = ble.VecSimulator(n); b.set_state(init); b.set_grid(field)
  rew = torch.zeros((k, n), dtype=torch.float32).cuda(); term = torch.zeros((k, n), dtype=torch.uint8).cuda()
  cnt = torch.zeros((k, ble.COUNT_SLOTS), dtype=torch.int64).cuda()
  a.step_n(acts, rew, term, cnt)
  rb, tb = [], []
  for j in range(k):
    r, t = b.step(acts[j].contiguous())
    rb.append(r.clone()); tb.append(t.clone())
  torch.cuda.synchronize()
  sa, sb = a.get_state(), b.get_state()
  for name in sa:
    np.testing.assert_array_equal(sa[name], sb[name], err_msg=name)
  np.testing.assert_array_equal(rew.cpu().numpy(), torch.stack(rb).cpu().numpy())
  np.testing.assert_array_equal(term.cpu().numpy(), torch.stack(tb).cpu().numpy())
  assert (sa['status'] != 0).sum() > 0
  live_per_step = cnt.sum(dim=1).cpu().numpy()
  expect = np.concatenate([[n], n - torch.stack(tb).cpu().numpy()[:-1].sum(axis=1)])
  np.testing.assert_array_equal(live_per_step, expect)
  # the prepared launch (checks and argument marshalling done once) enqueues the same work
  c = ble.VecSimulator(n); c.set_state(init); c.set_grid(field)
  rew_c = torch.zeros_like(rew); term_c = torch.zeros_like(term)
  launch = c.prepare_step_n(acts, rew_c, term_c)
  launch()
  torch.cuda.synchronize()
  sc = c.get_state()
  for name in sa:
    np.testing.assert_array_equal(sa[name], sc[name], err_msg=name)
  np.testing.assert_array_equal(rew.cpu().numpy(), rew_c.cpu().numpy())
  np.testing.assert_array_equal(term.cpu().numpy(), term_c.cpu().numpy())


@pytest.mark.parametrize('waves', [1, 4], ids=['0', '4'])
@pytest.mark.parametrize('with_cache', [True, False])
def test_fused_rollout_in_ground_truth_wind_equals_noise_plus_single_steps(ble, with_cache, waves):
  """ABI 3: ble_step_n_f32 with a noise generator flies every step in WindField.get_ground_truth = forecast + SimplexWindNoise
  (wind_field.py:125-145), the noise evaluated INSIDE the kernel at the pre-step position.  Bit for bit what K rounds of
  ble_wind_noise_f32 followed by ble_step_f32(noise_uv) give -- state, rewards, terminals -- for environments in different
  episodes (the generator is keyed by (seed, env, episode)), with and without the harmonic cache; and it is NOT the forecast
  flight.  `waves`: the fused launch on the one-lane kernel (in-kernel generator on one lane) or on four wavefronts per
  environment (the ten harmonics evaluated on different waves, summed in the reference's order)."""
  import ctypes
  import os
  from balloon_learning_environment_amd import _abi, _lib, device as dev
  import reset_host
  n, k, seed = 4096, 6, 20240917
  init = reset_host.sample_initial_state(n, seed=15)
  init['battery_charge'][:48] = 0.2                 # a few environments end inside the rollout
  field = (np.random.default_rng(1).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  acts = torch.from_numpy(np.random.default_rng(2).integers(0, 3, (k, n)).astype(np.uint8)).cuda()
  episodes = torch.from_numpy(np.random.default_rng(3).integers(0, 5, n).astype(np.int32)).cuda()
  sims = []
  for _ in range(3):
    s = ble.VecSimulator(n); s.set_state(init); s.set_grid(field); s.episode.copy_(episodes); sims.append(s)
  a, b, c = sims
  rew = torch.zeros((k, n), dtype=torch.float32).cuda(); term = torch.zeros((k, n), dtype=torch.uint8).cuda()
  with _lib.step_form(waves):
    if with_cache:
      a.step_n(acts, rew, term, noise_seed=seed)
    else:                                              # harmonic_cache NULL: the draws come straight from the Philox stream
      gen = _abi.BleNoiseGen(seed, a.episode.data_ptr(), None)
      _lib.check(a.lib.ble_step_n_f32(ctypes.byref(a._struct), acts.data_ptr(), a.grid.data_ptr(), 0, ctypes.byref(gen), rew.data_ptr(),
                                      term.data_ptr(), a.err_flags.data_ptr(), None, n, 18, k, dev.stream_ptr(a.device)), 'ble_step_n_f32')
  rb, tb = [], []
  for j in range(k):
    noise = b.wind_noise(seed)
    r, t = b.step(acts[j].contiguous(), noise)
    rb.append(r.clone()); tb.append(t.clone())
  rew_c = torch.zeros_like(rew); term_c = torch.zeros_like(term)
  c.step_n(acts, rew_c, term_c)                     # the forecast flight
  torch.cuda.synchronize()
  a.check_errors(); b.check_errors()
  sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
  for name in sa:
    np.testing.assert_array_equal(sa[name], sb[name], err_msg=name)
  np.testing.assert_array_equal(rew.cpu().numpy(), torch.stack(rb).cpu().numpy())
  np.testing.assert_array_equal(term.cpu().numpy(), torch.stack(tb).cpu().numpy())
  assert (sa['status'] != 0).sum() > 0
  moved = np.hypot(sa['x'] - sc['x'], sa['y'] - sc['y'])
  assert np.median(moved) > 100.0                   # ~1 m/s of noise over 18 minutes


@pytest.mark.parametrize('waves', [4])
@pytest.mark.parametrize('wide', [False, True])
def test_split_kernel_equals_one_lane_kernel(ble, wide, waves):
  """The small-batch form of the transition -- one environment on FOUR wavefronts (csrc/ble_step_split.h: vertical dynamics |
  thermal model | sun + power | envelope + ACS, exchanging through LDS once per stride), which ble_step_f32 / ble_step_n_f32
  select up to BLE_SPLIT_MAX_ENVS environments -- against the one-lane-per-environment kernel, forced with _lib.step_form:
  every state array, reward, terminal, effective action, the live counters and the error word, BIT FOR BIT; fused launches
  and single steps with a noise term, action bytes outside 0 .. 2, environments that end inside the rollout (early in a
  step, so that their lane stops while its neighbours go on), a batch that does not fill its last workgroup."""
  import os
  import reset_host
  from helpers import wide_domain_states
  n, k = 4096 - 37, 9
  init = wide_domain_states(n, 8) if wide else reset_host.sample_initial_state(n, seed=8)
  init['battery_charge'][:96] = np.linspace(0.01, 40.0, 96).astype(np.float32)     # out of power after a few strides / steps
  init['superpressure'][96:128] = 2379.0                                             # about to burst
  init['status'][128:136] = 2                                                        # already terminal on entry
  field = (np.random.default_rng(1).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  acts_h = np.random.default_rng(2).integers(0, 3, (k, n)).astype(np.uint8)
  acts_h[:, 200:232] = np.random.default_rng(3).integers(3, 256, (k, 32)).astype(np.uint8)   # fly like STAY, handed on as given
  acts = torch.from_numpy(acts_h).cuda()
  noise = torch.from_numpy((np.random.default_rng(4).standard_normal((n, 2)) * 1.5).astype(np.float32)).cuda()

  def fly(split):
    with _lib.step_form(waves if split else 1):      # 4 wavefronts per environment (csrc/ble_step_split.h) against 1
      sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(field)
      rew = torch.zeros((k, n), dtype=torch.float32).cuda(); term = torch.zeros((k, n), dtype=torch.uint8).cuda()
      cnt = torch.zeros((k, ble.COUNT_SLOTS), dtype=torch.int64).cuda()
      sim.step_n(acts, rew, term, cnt)                               # a fused launch ...
      singles = []
      for j in range(3):                                             # ... then single steps in a noisy wind
        r, t = sim.step(acts[j].contiguous(), noise)
        singles.append((r.clone(), t.clone(), sim.effective_action.clone()))
      torch.cuda.synchronize()
      flags = int(sim.err_flags.item()); sim.err_flags.zero_()
      return sim.get_state(), rew.cpu().numpy(), term.cpu().numpy(), cnt.cpu().numpy(), singles, flags, int(sim.active_count.item())
  a, b = fly(True), fly(False)
  for name in a[0]:
    np.testing.assert_array_equal(a[0][name], b[0][name], err_msg=name)
  np.testing.assert_array_equal(a[1], b[1]); np.testing.assert_array_equal(a[2], b[2])
  np.testing.assert_array_equal(a[3].sum(axis=1), b[3].sum(axis=1))
  for (ra, ta, ea), (rb, tb, eb) in zip(a[4], b[4]):
    assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(ea, eb)
  assert a[5] == b[5] and a[6] == b[6]
  ended = (a[0]['status'] != 0).sum()
  assert ended >= 8 + 16 and (a[0]['status'] == 1).sum() > 0 and (a[0]['status'] == 2).sum() >= 8
  assert a[2][0].sum() < ended                                        # some ended in later steps, not all in the first


# ---------------------------------------------------------------- device reset
def test_device_reset_derivation_matches_oracle(ble):
  """sample=0: cold start + sunrise search on given inputs (golden F10 + sampled) vs the oracle."""
  import reset_host
  d = golden('f10_reset')
  init = reset_host.sample_initial_state(4096, seed=31)
  cases = [dict(alpha=d['alpha'], x=d['x'], y=d['y'], pressure=d['pressure'], center_lat_deg=d['center_lat_deg'],
                center_lng_deg=d['center_lng_deg'], upwelling_infrared=d['upwelling_infrared'], start_unix=d['unix_s']),
           {k: init[k] for k in ('alpha', 'x', 'y', 'pressure', 'center_lat_deg', 'center_lng_deg', 'upwelling_infrared',
                                 'start_unix')}]
  # the same away from the sampler's +-10 deg: stations up to 85 deg of latitude in every season (the sunrise / sunset search
  # through polar day and night), balloons up to 400 km from the station
  polar = {k: init[k].copy() for k in cases[1]}
  rng = np.random.default_rng(8)
  polar['center_lat_deg'][:] = np.where(np.arange(4096) % 2 == 0, 1, -1) * rng.uniform(30, 85, 4096)
  polar['x'][:] = rng.uniform(-400e3, 400e3, 4096); polar['y'][:] = rng.uniform(-400e3, 400e3, 4096)
  cases.append(polar)
  for c in cases:
    n = c['x'].size
    sim = ble.VecSimulator(n)
    sim.set_state(c)
    sim.state['status'].fill_(2); sim.state['time_elapsed_s'].fill_(999)      # must be overwritten
    sim.reset_device(seed=0, sample=False)
    torch.cuda.synchronize(); sim.check_errors()
    got = sim.get_state()
    f = {k: got[k].astype(np.float64) for k in ('alpha', 'x', 'y', 'pressure', 'center_lat_deg', 'center_lng_deg',
                                                 'upwelling_infrared')}
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
    assert (got['battery_charge'] == np.float32(2905.6)).all()


def test_device_reset_sampling_distributions_and_autoreset(ble):
  """sample=1: the reference's initial-condition distributions (balloon_arena_test.py:56-87,
  utils/sampling.py), determinism per (seed, env, episode), masked auto-reset."""
  from balloon_learning_environment_amd.env import balloon_arena
  n = 65536
  arena = balloon_arena.VecBalloonArena(n, seed=17)
  torch.cuda.synchronize(); arena.sim.check_errors()
  s = arena.sim.get_state()
  r = np.hypot(s['x'].astype(np.float64), s['y'].astype(np.float64))
  assert r.max() <= 200_000.0 and abs(r.mean() / 200_000.0 - 1.2 / 3.2) < 0.01          # Beta(1.2, 2.0) mean
  assert abs((r / 200_000.0).var() - (1.2 * 2.0) / (3.2 ** 2 * 4.2)) < 0.005
  assert s['alpha'].min() >= 0 and s['alpha'].max() < 1 and abs(s['alpha'].mean() - 0.5) < 0.01
  assert np.abs(s['center_lat_deg']).max() <= 10 and np.abs(s['center_lng_deg']).max() <= 175
  assert s['start_unix'].min() >= 1293840000 and s['start_unix'].max() < 1419984000
  assert (s['upwelling_infrared'] >= 225).all() and (s['upwelling_infrared'] <= 315).all()
  p_max, _, _, _ = oracle.at_height(0.0, [15240.0])
  assert (s['pressure'] >= 6500).all()
  for a in (0.1, 0.5, 0.9):
    sel = np.abs(s['alpha'] - a) < 0.01
    pm = oracle.at_height(a, [15240.0])[0][0]
    assert s['pressure'][sel].max() <= pm + 12 and s['pressure'][sel].max() > pm - 250
  assert (s['status'] == 0).all() and (s['superpressure'] > 0).all()
  # determinism: same seed -> same episodes; another seed -> different
  arena2 = balloon_arena.VecBalloonArena(n, seed=17)
  s2 = arena2.sim.get_state()
  for k in s:
    np.testing.assert_array_equal(s[k], s2[k], err_msg=k)
  arena3 = balloon_arena.VecBalloonArena(1024, seed=18)
  assert not np.array_equal(arena3.sim.get_state()['x'], s['x'][:1024])
  # the derived part of a sampled reset agrees with the oracle on the sampled inputs
  f = {k: s[k][:2048].astype(np.float64) for k in ('alpha', 'x', 'y', 'pressure', 'center_lat_deg', 'center_lng_deg', 'upwelling_infrared')}
  ref, _ = oracle.stable_init(f['pressure'], f['center_lat_deg'], f['center_lng_deg'], f['x'], f['y'], s['start_unix'][:2048],
                              f['upwelling_infrared'], f['alpha'])
  np.testing.assert_allclose(s['internal_temperature'][:2048], ref['internal_temperature'], rtol=2e-7)
  # auto-reset: terminate some lanes, reset only those, episode counter advances -> new draws
  arena.sim.state['status'][:100] = 1
  before = arena.sim.get_state()
  assert arena.reset_terminated() == 100
  after = arena.sim.get_state()
  assert (after['status'] == 0).all() and not np.array_equal(after['x'][:100], before['x'][:100])
  for k in after:
    np.testing.assert_array_equal(after[k][100:], before[k][100:], err_msg=k)
  assert (arena.sim.episode.cpu().numpy()[:100] == 2).all() and (arena.sim.episode.cpu().numpy()[100:] == 1).all()
  # and the freshly reset arena steps fine
  reward, terminal = arena.step(torch.randint(0, 3, (n,), dtype=torch.uint8, device='cuda'))
  torch.cuda.synchronize(); arena.sim.check_errors()
  assert float(reward.min()) >= 0 and float(reward.max()) <= 1


@pytest.mark.parametrize('n', [1, 63, 65, 1000])
def test_ragged_batch_sizes(ble, n):
  """Batch sizes that do not fill a wavefront (tail lanes masked), incl. the single-env case."""
  import reset_host
  total, outliers, worst = _sampled_batch_parity(ble, n, steps=3, seed=100 + n, threads=2)
  print(f'n={n}: {total} env-steps, worst {worst:.2g}')
  assert outliers == 0 and worst <= RTOL
  sim = ble.VecSimulator(n)
  sim.set_state(reset_host.sample_initial_state(n, seed=1))
  sim.set_grid(np.zeros((21, 21, 10, 9, 2), np.float32))
  k = 3
  acts = torch.randint(0, 3, (k, n), dtype=torch.uint8, device='cuda')
  rew = torch.full((k, n), -1.0, dtype=torch.float32).cuda(); term = torch.full((k, n), 9, dtype=torch.uint8).cuda()
  sim.step_n(acts, rew, term)
  torch.cuda.synchronize(); sim.check_errors()
  assert float(rew.min()) >= 0.0 and int(term.max()) <= 1          # every element written, nothing beyond n touched


# ---------------------------------------------------------------- BASELINE configs[3] / configs[4] at one GPU's share
def test_config3_shard_8192_envs_every_env(ble):
  """One rank's share of BASELINE.json configs[3] (65 536 envs over 8 GPUs = 8 192 per GPU; the shard of
  rank 5 flies envs [40 960, 49 152) of the global batch, shared broadcast grid): every environment
  against the oracle, 6 free-running steps."""
  from balloon_learning_environment_amd import distributed as bdist
  lay = bdist.preset_layout(3, 5, 8)
  assert (lay['n_local'], lay['lo']) == (8192, 40960)
  total, outliers, worst = _sampled_batch_parity(ble, lay['n_local'], steps=6, seed=1000 + 5, threads=16)
  print(f'config 3 shard: {total} env-steps, {outliers} beyond 1e-5, worst {worst:.2g}')
  assert outliers == 0 and worst <= RTOL


def test_config4_share_32768_envs_per_env_grids_sampled(ble):
  """One GPU's share of BASELINE.json configs[4]: 32 768 environments, each in its OWN forecast decoded on the
  device (32 768 x 317 520 B = 10.4 GB of grids, 64-bit grid offsets).  The whole batch flies three steps
  twice -- fused (ble_step_n_f32, one launch) and as three ble_step_f32 launches -- and the two must agree
  bit for bit; along the unfused flight 384 sampled environments (incl. the first and the last) are checked
  step by step against the oracle, each on its own grid copied back from HBM and from the GPU's own
  pre-step state (identical inputs)."""
  from balloon_learning_environment_amd import distributed as bdist
  import reset_host
  from balloon_learning_environment_amd.env import generative_wind_field
  lay = bdist.preset_layout(4, 0, 8)
  n = lay['n_local']
  assert n == 32768 and lay['per_env_grids'] and not lay['broadcast_grid']
  sampler = generative_wind_field.GenerativeWindFieldSampler(seed=0)
  grids = sampler.decode(sampler.sample_latents(n, seed=100))
  assert grids.numel() * 4 == lay['grid_bytes_per_rank']
  init = reset_host.sample_initial_state(n, seed=1000)
  k = 3
  acts = torch.from_numpy(np.random.default_rng(9).integers(0, 3, (k, n)).astype(np.uint8)).cuda()
  fused = ble.VecSimulator(n); fused.set_state(init); fused.set_grid(grids, per_env=True)
  rew = torch.zeros((k, n), dtype=torch.float32).cuda(); term = torch.zeros((k, n), dtype=torch.uint8).cuda()
  fused.step_n(acts, rew, term)
  torch.cuda.synchronize(); fused.check_errors()
  idx = np.unique(np.concatenate([np.random.default_rng(1).integers(0, n, 382), [0, n - 1]]))
  idx_t = torch.from_numpy(idx).cuda()
  host_grids = grids[idx_t].cpu().numpy()
  sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(grids, per_env=True)
  worst = 0.0
  for s in range(k):
    before = {key: t[idx_t].cpu().numpy() for key, t in sim.state.items()}
    reward, terminal = sim.step(acts[s].contiguous())
    torch.cuda.synchronize(); sim.check_errors()
    assert torch.equal(reward, rew[s]) and torch.equal(terminal, term[s])        # fused == unfused, every env
    after = {key: t[idx_t].cpu().numpy() for key, t in sim.state.items()}
    a_h = acts[s][idx_t].cpu().numpy(); r_h = reward[idx_t].cpu().numpy()
    for j in range(len(idx)):
      o2 = oracle_state_from_abi({key: v[j:j + 1] for key, v in before.items()})
      ro, to, eo, err = oracle.step(o2, a_h[j:j + 1], field=host_grids[j])
      assert abs(r_h[j] - ro[0]) <= 1e-5, (idx[j], s)
      for key in STATE_FLOATS:
        e = float(rel_err(after[key][j], o2[key][0], FLOORS[key]))
        worst = max(worst, e)
        assert e <= RTOL, (idx[j], s, key, e)
      for key in ('status', 'last_command', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
        assert int(after[key][j]) == int(o2[key][0]), (idx[j], s, key)
  for key in sim.state:
    assert torch.equal(sim.state[key], fused.state[key]), key
  print(f'config 4 share: {len(idx)} sampled envs x {k} steps on per-env grids, worst {worst:.2g}; fused == unfused for all {n}')
  # distinct forecasts really are in use
  assert not torch.equal(grids[0], grids[n - 1])


def test_episode_cache_is_transparent(ble):
  """ble_state_f32.episode_cache (per-episode derived constants kept in HBM): a launch that reads them from the cache is
  bit-identical to one that derives them (cache NULL); the reset kernel fills the cache; constants edited by hand
  afterwards are noticed (the entry is keyed by their bit patterns) and never produce a stale result."""
  import ctypes
  from balloon_learning_environment_amd import device as dev
  import reset_host
  n = 4096
  field = (np.random.default_rng(3).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  acts = torch.from_numpy(np.random.default_rng(5).integers(0, 3, (6, n)).astype(np.uint8)).cuda()

  def fly(use_cache, edit=False, device_reset=False):
    sim = ble.VecSimulator(n)
    sim.set_grid(field)
    if device_reset:
      sim.reset_device(seed=5)
      keys = sim.episode_cache[6].view(torch.int64)
      assert bool(((keys >> 31) & 1).all())                  # every entry valid straight after the reset kernel
    else:
      sim.set_state(reset_host.sample_initial_state(n, seed=5))
      assert float(sim.episode_cache.abs().sum()) == 0.0     # host-set state: nothing cached yet
    if not use_cache:
      sim._struct = dev.state_struct(sim.state, None)
    out = []
    for k in range(6):
      if edit and k == 3:                                    # new per-episode constants under the cache's feet
        sim.state['alpha'].copy_(1.0 - sim.state['alpha'])
        sim.state['center_lat_deg'].mul_(-0.5)
        sim.state['upwelling_infrared'].add_(7.0)
      r, t = sim.step(acts[k])
      out.append((r.clone(), t.clone()))
    sim.check_errors()
    return sim.get_state(), out, sim

  for kw in (dict(), dict(edit=True), dict(device_reset=True), dict(device_reset=True, edit=True)):
    a, ra, sim_a = fly(True, **kw)
    b, rb, _ = fly(False, **kw)
    for k in a:
      np.testing.assert_array_equal(a[k], b[k], err_msg=f'{kw} {k}')
    for (r1, t1), (r2, t2) in zip(ra, rb):
      assert torch.equal(r1, r2) and torch.equal(t1, t2)
    live = torch.from_numpy(a['status'] == 0).cuda()
    keys = sim_a.episode_cache[6].view(torch.int64)
    assert bool(((keys >> 31) & 1)[live].all())              # every live lane's entry is valid after a step
    ir_bits = sim_a.state['upwelling_infrared'].view(torch.int32).to(torch.int64) & 0xffffffff
    assert torch.equal(((keys >> 32) & 0xffffffff)[live], ir_bits[live])     # ... and belongs to the CURRENT constants


def test_integration_md_binding_runs_as_written(ble):
  """The ctypes binding INTEGRATION.md section 2 shows a reference maintainer (`HipBalloons`), executed as written (only the
  library path is filled in): one step of 1 000 sampled environments through it equals VecSimulator.step bit for bit."""
  import os, re
  from balloon_learning_environment_amd import _lib
  import reset_host
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  text = open(os.path.join(root, 'INTEGRATION.md')).read()
  block = re.search(r'```python\n(# balloon_learning_environment/env/hip_backend\.py.*?)```', text, re.S).group(1)
  scope = {}
  exec(block.replace("ctypes.CDLL('libble_hip.so')", f'ctypes.CDLL({_lib.LIB_PATH!r})'), scope)
  n = 1000
  init = reset_host.sample_initial_state(n, seed=21)
  field = (np.random.default_rng(3).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  grid = torch.from_numpy(field).cuda()
  act = _dev(np.random.default_rng(4).integers(0, 3, n), np.uint8)
  hip = scope['HipBalloons'](n)
  for k, t in hip.t.items():
    t.copy_(torch.from_numpy(np.asarray(init[k]).astype(t.cpu().numpy().dtype)))
  reward, terminal = hip.step(act, grid)
  sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(grid)
  r2, t2 = sim.step(act)
  torch.cuda.synchronize()
  assert int(hip.flags.item()) == 0
  assert torch.equal(reward, r2) and torch.equal(terminal, t2)
  for k, t in hip.t.items():
    assert torch.equal(t, sim.state[k]), k
