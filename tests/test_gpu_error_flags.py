"""err_flags against the reference's own exceptions (F18, tests/golden/f18_failures.npz), case by case, in every step form.

Each F18 transition case runs as a launch of its own (n = 1: the flag word is an OR over the launch) and must report the
oracle's bits of that environment (helpers.F18_DEVICE_WORD lists the deliberate differences); raise_for_flags must raise the
reference's class, and the flag must appear at the agent step where the reference raises.  An isolation run then mixes the
offending cases into a large clean batch: the clean lanes fly bit for bit what they fly without them.
No NaN / Inf input comes here (tests/test_kernel_numerics_host.py covers BLE_FLAG_NONFINITE on the host build)."""
import numpy as np
import pytest
import torch

import oracle
from helpers import (F18_CLASSES, f18_device_word, f18_state, f18_step_cases, golden)
from balloon_learning_environment_amd import _lib, vec_state

pytestmark = pytest.mark.gpu

SKIP_CLASS = ('terminal_on_entry', 'p_atm_in_down', 'p_atm_in_stay')   # (their word is F18_DEVICE_WORD; the reference's class differs)


def _class_of(word):
  try:
    vec_state.raise_for_flags(int(word))
  except Exception as exc:      # noqa: BLE001
    return type(exc)
  return None


def _sim_for(ost, vehicle=None):
  sim = vec_state.VecSimulator(ost['x'].size, 'cuda:0')
  st = {k: v for k, v in ost.items() if k not in ('sunrise_h', 'sunset')}
  st['sunrise_h_rel'] = ost['sunrise_h'] - ost['start_unix']
  st['sunset_rel'] = ost['sunset'] - ost['start_unix']
  sim.set_state(st)
  sim.set_grid(np.zeros((21, 21, 10, 9, 2), np.float32))     # the fixed wind of the case comes in as the additive term
  if vehicle is not None:
    sim.set_vehicle(**vehicle)
  return sim


def _expected(d, j, vehicle=None):
  ost = f18_state(d, j)
  _, _, _, err = oracle.step(ost, d['actions'][j:j + 1], wind_uv=d['wind_uv'][j:j + 1], substeps=int(d['substeps'][j]), per_env=True,
                             vehicle=vehicle)
  return f18_device_word(d, j, err['env'][0])


def _run_case(d, j, form, vehicle=None, launches=1):
  """Flag word after each of `launches` single-step launches of case j (the fixed wind as noise_uv)."""
  sim = _sim_for(f18_state(d, j), vehicle)
  a = torch.from_numpy(d['actions'][j:j + 1].copy()).cuda()
  w = torch.from_numpy(d['wind_uv'][j:j + 1].astype(np.float32)).cuda()
  words = []
  with _lib.step_form(form):
    for _ in range(launches):
      sim.err_flags.zero_()
      sim.step(a, noise_uv=w, substeps=int(d['substeps'][j]))
      torch.cuda.synchronize()
      words.append(int(sim.err_flags.item()))
  return words, sim


@pytest.mark.parametrize('form,vehicle', [(1, None), (4, None), (1, {'payload_mass': 95.0})], ids=['one_lane', 'four_wave', 'runtime'])
def test_f18_flag_word_per_case(form, vehicle):
  """The one-lane and the four-wave form with the compile-time vehicle, and a run-time (non-NULL) vehicle -- which always flies the
  one-lane form's second instantiation (ble_kernels.hip), so it has no four-wave variant."""
  d = golden('f18_failures')
  for j in range(f18_step_cases(d)):
    name = str(d['names'][j])
    want = _expected(d, j, vehicle)
    words, sim = _run_case(d, j, form, vehicle)
    assert words[0] == want, (form, name, words[0], want)
    if name not in SKIP_CLASS:
      assert _class_of(words[0]) is F18_CLASSES[int(d['exc'][j])], (form, name)
      if words[0]:
        sim.err_flags.fill_(words[0])
        with pytest.raises(F18_CLASSES[int(d['exc'][j])]):
          sim.check_errors()


def test_f18_second_launch_reads_the_ir_flag_from_the_episode_cache():
  """Second launch of the same episode: the Earth-IR check comes from the episode cache the first launch stored."""
  d = golden('f18_failures')
  names = [str(s) for s in d['names']]
  for name in ('ir_lo_in', 'ir_lo_out', 'ir_hi_in', 'ir_hi_out'):
    j = names.index(name)
    words, sim = _run_case(d, j, 1, launches=2)
    if d['exc'][j]:
      assert words == [2, 2], (name, words)
    else:
      assert words[0] == 0 and words[1] == 0, (name, words)


def test_f18_fused_rollout_reports_the_oracle_bits_of_its_steps():
  """ble_step_n_f32, K = 2 steps in one launch, without noise and with the in-kernel noise.  The case's constant wind fills the
  whole grid (no noise: the oracle flies the same field).  The flag word is an OR over the launch, so it is compared with the OR of
  the oracle's bits over the two steps (the second only where the first left the episode running); with noise, where the wind
  differs, only cases whose flag does not depend on the wind (the first stride's checks, the clean case's silence) are kept."""
  d = golden('f18_failures')
  names = [str(s) for s in d['names']]
  for name in ('t_int_lo_out', 't_int_12_29', 't_int_hi_out', 'hot_stride1_of_18', 'cool_stride1_of_18_flies_on', 'ir_hi_out',
               'ir_lo_in', 'p_solar_out_stay', 'clean'):
    j = names.index(name)
    field = np.broadcast_to(d['wind_uv'][j].astype(np.float32), (21, 21, 10, 9, 2)).copy()
    ost = f18_state(d, j)
    want = 0
    for _ in range(2):
      if ost['status'][0] != 0:
        break
      _, _, _, err = oracle.step(ost, d['actions'][j:j + 1], field=field, per_env=True)
      want |= f18_device_word(d, j, err['env'][0])
    for noise_seed in (None, 5):
      if noise_seed is not None and name in ('hot_stride1_of_18', 'cool_stride1_of_18_flies_on'):
        continue
      sim = _sim_for(f18_state(d, j))
      sim.set_grid(field)
      acts = torch.from_numpy(np.repeat(d['actions'][j:j + 1][None], 2, 0).copy()).cuda()
      rew = torch.zeros(2, 1, dtype=torch.float32, device='cuda:0'); term = torch.zeros(2, 1, dtype=torch.uint8, device='cuda:0')
      sim.step_n(acts, rew, term, substeps=18, noise_seed=noise_seed)
      torch.cuda.synchronize()
      word = int(sim.err_flags.item())
      assert word == want, (name, noise_seed, word, want)


def test_f18_device_reset_flags():
  """ble_reset_at_f32 on F18's reset inputs (sample = 0: the state's own inputs): the reference's class where it raises at the
  reset; a station at |lat| >= 60 deg is computed, not raised."""
  d = golden('f18_failures')
  n0 = int(d['exc'].size)
  names = [str(s) for s in d['names'][n0:]]
  for j, name in enumerate(names):
    sim = vec_state.VecSimulator(1, 'cuda:0')
    sim.set_state({'alpha': d['reset_alpha'][j:j + 1], 'x': d['reset_x'][j:j + 1], 'y': d['reset_y'][j:j + 1],
                   'pressure': d['reset_pressure'][j:j + 1], 'center_lat_deg': d['reset_center_lat_deg'][j:j + 1],
                   'center_lng_deg': d['reset_center_lng_deg'][j:j + 1], 'upwelling_infrared': d['reset_upwelling_infrared'][j:j + 1],
                   'start_unix': d['reset_unix_s'][j:j + 1]})
    sim.reset_device(0, sample=False)
    torch.cuda.synchronize()
    word = int(sim.err_flags.item())
    want = None if name in ('reset_lat_60', 'reset_lat_m75') else F18_CLASSES[int(d['reset_exc'][j])]
    assert _class_of(word) is want, (name, word)
    if d['reset_exc'][j] == 0:
      t = float(sim.state['internal_temperature'].item())
      assert abs(t - d['reset_out_internal_temperature'][j]) <= 1e-5 * d['reset_out_internal_temperature'][j], name


@pytest.mark.parametrize('form', [1, 4], ids=['0', '4'])
def test_f18_isolation_in_a_large_batch(form):
  """4096 - 37 environments, about 5 % of them F18's offending cases (18 substeps), the rest the clean case with varied winds: the
  clean lanes fly bit for bit what the same batch flies with the offending lanes replaced by clean ones, and the flag word is the
  OR of the oracle's per-environment bits."""
  d = golden('f18_failures')
  n_cases = f18_step_cases(d)
  names = [str(s) for s in d['names'][:n_cases]]
  bad = [j for j in range(n_cases) if d['substeps'][j] == 18 and (d['exc'][j] or names[j].startswith('t_int_'))
         and names[j] not in ('terminal_on_entry',)]
  clean = names.index('clean')
  n = 4096 - 37
  rng = np.random.default_rng(18)
  rows = np.full(n, clean)
  lanes = rng.choice(n, n // 20, replace=False)
  rows[lanes] = np.array(bad)[np.arange(lanes.size) % len(bad)]
  wind = rng.normal(0, 5, (n, 2)).astype(np.float32)
  acts = rng.integers(0, 3, n).astype(np.uint8)
  wind[lanes] = d['wind_uv'][rows[lanes]]; acts[lanes] = d['actions'][rows[lanes]]

  def fly(rws):
    sim = _sim_for(f18_state(d, rws))
    with _lib.step_form(form):
      sim.step(torch.from_numpy(acts).cuda(), noise_uv=torch.from_numpy(wind).cuda(), substeps=18)
      torch.cuda.synchronize()
    return sim.get_state(), sim.reward.cpu().numpy(), int(sim.err_flags.item())

  mixed, r_mixed, word = fly(rows)
  pure, r_pure, word_clean = fly(np.full(n, clean))
  assert word_clean == 0
  keep = np.ones(n, bool); keep[lanes] = False
  for k, v in mixed.items():
    assert np.array_equal(v[keep], pure[k][keep]), k
  assert np.array_equal(r_mixed[keep], r_pure[keep])
  ost = f18_state(d, rows)
  _, _, _, err = oracle.step(ost, acts, wind_uv=wind.astype(np.float64), per_env=True)
  want = 0
  for i in lanes:
    want |= f18_device_word(d, rows[i], err['env'][i])
  assert word == want, (word, want)
