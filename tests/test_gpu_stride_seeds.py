"""The stride's lane functions after the seed merge (one reciprocal square root for dh/dt / dH, the twelfth root's argument in fp32, the ACS
node position read from the table), on the device:

  * the three forms of the transition -- one lane (1), four waves (4), helper wave (12), forced with ble_set_step_form -- fly the same batch
    to the same bits: every state array, reward, terminal, err_flags, live counts; 65 and 257 environments, launches of 1, 3 and 32 steps,
    1, 2, 18 and 19 strides per step;
  * the helper form flies the 257 environments 64 steps against the fp64 oracle, step by step from the device's own pre-step state: discrete
    state exact, floats within 1e-5 over helpers.FLOORS, every environment compared (a frozen one must not move).

The batch holds what the changed expressions branch on: environments within 1 Pa of the 17 km layer transition on either side (p + d across
it: the rare path with its own reciprocal), one at EXACT buoyancy equilibrium (rho V - m == 0 in the kernel's fp64: the 1e-30 floor under the
merged seed), slack envelopes, batteries that run out inside a step.  Needs a real MI355X:  pytest -m gpu."""
import fractions
import functools

import numpy as np
import pytest

from balloon_learning_environment_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

FORMS = (1, 4, _lib.STEP_FORM_HELPER)
EDGE_OFFSETS = np.array([-0.75, -0.5, -0.25, -0.05, 0.05, 0.25, 0.5, 0.75])      # Pa from the transition
N_EDGE = len(EDGE_OFFSETS)
I_EQ, I_SLACK, NIGHT = 8, 9, slice(10, 18)
# p V M / R == m T_amb to the last bit: p V = 2^24 exactly, and the float32 pair (air, T_amb) whose fp64 mass x temperature rounds onto it
EQ = dict(pressure=16384.0, envelope_volume=1024.0, mols_air=1568.153076171875, ambient_temperature=250.02842712402344)
M_AIR, R_GAS, G = 0.028964922481160, 8.3144621, 9.80665
DRY_MASS = 0.004002602 * 6830.0 + 68.5 + 92.5


def _transition_17km(alpha):
  """The pressure of the 17 km transition (standard_atmosphere.py:122-183) in fp64; the kernel's own differs by ~1e-8 Pa."""
  alpha = np.asarray(alpha, np.float64)
  l0 = (1 - alpha) * -0.007 + alpha * -0.0058
  t1 = 300.0 + l0 * (17000.0 - -610.0)
  return 108870.8213 * (t1 / 300.0) ** (-G / ((R_GAS / M_AIR) * l0)), t1


@functools.lru_cache(maxsize=None)
def _batch(n):
  import reset_host
  init = reset_host.sample_initial_state(n, seed=1010)
  f32 = np.float32
  # 0 .. 7: within 1 Pa of the 17 km transition, four on either side; an envelope at 800 Pa of superpressure in the air that goes with it
  p1, t1 = _transition_17km(init['alpha'][:N_EDGE])
  init['pressure'][:N_EDGE] = (p1 + EDGE_OFFSETS).astype(f32)
  init['ambient_temperature'][:N_EDGE] = t1.astype(f32)
  init['internal_temperature'][:N_EDGE] = (t1 - 4.0).astype(f32)
  vol = 1804.0 + 0.0199 * 800.0
  init['superpressure'][:N_EDGE] = 800.0; init['envelope_volume'][:N_EDGE] = vol
  init['mols_air'][:N_EDGE] = ((init['pressure'][:N_EDGE].astype(np.float64) + 800.0) * vol /
                               (R_GAS * init['internal_temperature'][:N_EDGE].astype(np.float64)) - 6830.0).astype(f32)
  # 8: exact buoyancy equilibrium (its envelope is slack too: 1 024 m^3); 9: a slack envelope without air
  for k, v in EQ.items():
    init[k][I_EQ] = v
  init['internal_temperature'][I_EQ] = 1024.0 * 16384.0 / ((6830.0 + EQ['mols_air']) * R_GAS); init['superpressure'][I_EQ] = 0.0
  init['pressure'][I_SLACK] = 30000.0; init['mols_air'][I_SLACK] = 0.0; init['internal_temperature'][I_SLACK] = 230.0
  init['ambient_temperature'][I_SLACK] = 229.0; init['superpressure'][I_SLACK] = 0.0
  init['envelope_volume'][I_SLACK] = 6830.0 * R_GAS * 230.0 / 30000.0
  # 10 .. 17: an hour into their own night, 0.51 Wh per stride: they run out of power at strides spread over the first steps
  init['time_elapsed_s'][NIGHT] = (init['sunset_rel'][NIGHT] + 3600).astype(init['time_elapsed_s'].dtype)
  init['battery_charge'][NIGHT] = np.array([0.05, 0.8, 1.3, 2.4, 4.0, 7.0, 9.5, 14.0], f32)
  for k in ('status', 'alt_fsm', 'env_fsm', 'power_paused'):
    init[k][:18] = 0
  return init


def test_the_batch_holds_the_cases():
  """From the inputs alone (exact rational arithmetic for the equilibrium): no device involved, so a failure here is the test's own."""
  init = _batch(257)
  p1, _ = _transition_17km(init['alpha'][:N_EDGE])
  off = init['pressure'][:N_EDGE].astype(np.float64) - p1
  assert (np.abs(off) < 1.0).all() and (off < -0.01).sum() == 4 and (off > 0.01).sum() == 4
  F = fractions.Fraction
  s = {k: float(init[k][I_EQ]) for k in EQ}
  assert all(s[k] == v for k, v in EQ.items())                                         # (they are float32 values)
  mass = float(F(M_AIR) * F(s['mols_air']) + F(DRY_MASS))                             # d_fma(M, n_air, dry mass): one rounding
  mt = float(F(mass) * F(s['ambient_temperature']))                                    # mass * t_amb: one rounding
  assert F(s['pressure'] * s['envelope_volume']) * F(M_AIR / R_GAS) - F(mt) == 0     # the fma's exact value: +0
  assert init['envelope_volume'][I_EQ] < 1804.0 and init['envelope_volume'][I_SLACK] < 1804.0


def _actions(k, n, seed):
  return np.random.default_rng(seed).integers(0, 3, (k, n)).astype(np.uint8)


@pytest.mark.parametrize('substeps', [1, 2, 18, 19])
@pytest.mark.parametrize('n', [65, 257])
def test_three_forms_fly_the_same_bits(n, substeps):
  from test_gpu_helper_form import _assert_same, _field, _fly
  init = _batch(n)
  field = _field(16)
  for k in (1, 3, 32):
    acts = _actions(k, n, 100 * k + substeps)
    flights = []
    for form in FORMS:
      out = _fly(form, init, acts, field, substeps=substeps)
      assert _lib.lib().ble_last_step_form() == form
      out['active_count'] = out['active_count'].sum(axis=1)            # per step, summed over the slots (their layout is the form's)
      flights.append(out)
    _assert_same(flights[0], flights[1])
    _assert_same(flights[0], flights[2])
    one = flights[0]
    st = one['state']
    # the slack envelopes stop in the first stride (zero pressure); the batteries run out inside the launch, not all in one step
    flown = st['time_elapsed_s'].astype(np.int64) - init['time_elapsed_s'].astype(np.int64)
    assert st['status'][I_EQ] != 0 and st['status'][I_SLACK] != 0 and flown[I_EQ] == 10 and flown[I_SLACK] == 10
    assert (flown[NIGHT] % (10 * substeps) != 0).any() or substeps == 1, 'no episode ended inside a step'
    assert (st['status'][NIGHT] != 0).any() and (st['status'][:N_EDGE] == 0).all()
    assert np.isfinite(st['pressure']).all() and one['err_flags'] & 1 == 0


def test_helper_form_against_the_oracle_64_steps():
  import oracle
  from helpers import FLOORS, STATE_FLOATS, rel_err
  from test_gpu_helper_form import _await, _field
  from test_gpu_parity import RTOL, oracle_state_from_abi
  from balloon_learning_environment_amd import vec_state as ble
  n, k = 257, 64
  init = _batch(n)
  field = _field(16)
  acts_h = _actions(k, n, 640)
  acts = torch.from_numpy(acts_h).cuda()
  states, rewards, terminals, effs = [], [], [], []
  with _lib.step_form(_lib.STEP_FORM_HELPER):
    sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(field)
    states.append(sim.get_state())
    for j in range(k):
      r, t = sim.step(acts[j])
      _await(f'helper form, step {j}')
      assert _lib.lib().ble_last_step_form() == _lib.STEP_FORM_HELPER
      rewards.append(r.cpu().numpy().copy()); terminals.append(t.cpu().numpy().copy()); effs.append(sim.effective_action.cpu().numpy().copy())
      states.append(sim.get_state())
  worst = dict.fromkeys(STATE_FLOATS, 0.0)
  ended_inside = 0
  for j in range(k):
    before, got = states[j], states[j + 1]
    live = before['status'] == 0
    o2 = oracle_state_from_abi(before)
    ro, to, eo, err = oracle.step(o2, acts_h[j], field=field, threads=4)
    assert (err & ~oracle.ERR_TERMINAL_STEP) == 0, f'step {j}: oracle flags {err}'
    for name in ('status', 'last_command', 'alt_fsm', 'env_fsm', 'power_paused', 'time_elapsed_s'):
      np.testing.assert_array_equal(got[name][live], o2[name][live], err_msg=f'step {j}: {name}')
    np.testing.assert_array_equal(got['start_unix'][live] + got['sunrise_h_rel'][live], o2['sunrise_h'][live], err_msg=f'step {j}: sunrise')
    np.testing.assert_array_equal(got['start_unix'][live] + got['sunset_rel'][live], o2['sunset'][live], err_msg=f'step {j}: sunset')
    np.testing.assert_array_equal(effs[j][live], eo[live], err_msg=f'step {j}: effective action')
    np.testing.assert_array_equal(terminals[j], to, err_msg=f'step {j}: terminal')
    for name in STATE_FLOATS:
      e = rel_err(got[name], o2[name], FLOORS[name])[live]
      if e.size:
        worst[name] = max(worst[name], float(e.max()))
        assert e.max() <= RTOL, f'step {j}: {name} {e.max():.3g} at environment {np.flatnonzero(live)[int(e.argmax())]}'
      # an episode that is over does not move
      np.testing.assert_array_equal(got[name][~live].view(np.uint32), before[name][~live].view(np.uint32), err_msg=f'step {j}: frozen {name}')
    np.testing.assert_array_equal(got['status'][~live], before['status'][~live])
    rew_err = np.abs(rewards[j] - ro)[live]
    assert rew_err.size == 0 or rew_err.max() <= 1e-5, f'step {j}: reward {rew_err.max():.3g}'
    ended_inside += int((live & (got['status'] != 0)).sum())
  print('largest relative error per field over 64 steps:', {name: f'{v:.2g}' for name, v in worst.items()})
  assert ended_inside >= 4 and (states[k]['status'][:N_EDGE] == 0).sum() >= N_EDGE // 2
