"""The twin of the sampled device reset (tests/reset_draws_host.py) on the CPU: its generator against the host build of the kernel's
(tests/emul), its eight fields against their analytic laws, and proof that the checks can fail.  The GPU side
(tests/test_gpu_reset_draws.py) holds the device to this twin draw by draw and to the same laws."""
import ctypes

import numpy as np
import pytest

import reset_draws_host as rd

SEED, KEY, EPISODE = 0x9E3779B97F4A7C15, 2 ** 32 + 5, 7      # a high key word (the fourth counter word) and a non-zero episode
N_LAW = 65536


def _emul_philox(seed, key, episode, n):
  from emul import emul as e
  u, z, g = np.empty(n), np.empty(n), np.empty(n)
  P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
  e.lib().emul_philox(ctypes.c_uint64(seed), ctypes.c_uint64(key), ctypes.c_uint32(episode), ctypes.c_int64(n), P(u), P(z), P(g))
  return u, z, g


@pytest.fixture(scope='module')
def generators():
  """n uniforms, then n normals, then n Gamma(1.2) of 8 streams (keys KEY ..), from the twin and from the host build."""
  n, keys = 1024, KEY + np.arange(8)
  g = rd.Streams(SEED, keys, EPISODE)
  twin = tuple(np.stack([draw() for _ in range(n)], 1) for draw in (g.uniform, g.normal, lambda: g.gamma(1.2)))
  host = tuple(np.stack(a) for a in zip(*[_emul_philox(SEED, int(k), EPISODE, n) for k in keys]))
  return twin, host


def test_generator_matches_host_build(generators):
  (tu, tz, tg), (hu, hz, hg) = generators
  np.testing.assert_array_equal(tu.view(np.uint64), hu.view(np.uint64))
  ez, eg = np.abs(hz / tz - 1.0).max(), np.abs(hg / tg - 1.0).max()
  print(f'normals {ez:.2g}, gammas {eg:.2g} relative')
  assert ez <= 1e-13 and eg <= 1e-13
  # Philox4x32-10 known answer (Random123 kat_vectors: counter 0, key 0), popped from out[3] down
  s = rd.Streams(0, 0, 0)
  assert [int(s.u32()[0]) for _ in range(4)] == [0x9b00dbd8, 0xbc57ac4c, 0xe169c58d, 0x6627e8d5] and int(s.pos[0]) == 4


def test_host_generator_through_twin_formulas_rounds_alike(generators):
  """The condition the GPU test sets the device -- per field at least 99.9 % of the stored float32 values bitwise the twin's, none
  further than one step -- on the host build of the generator: its deviates, put through the twin's formulas for the fields that
  carry a transcendental (x, y from two gammas and an angle; IR from a normal), round to the same float32."""
  (tu, tz, tg), (_, hz, hg) = generators
  f32 = np.float32

  def fields(z, g):
    ga, gb = g[:, 0::2], g[:, 1::2]
    r = rd.RADIUS_M * (ga / (ga + gb))
    angle = 2.0 * np.pi * tu[:, :r.shape[1]]
    with np.errstate(over='ignore'):
      ir = rd.IR_MAX / (1.0 + np.exp(-(rd.IR_MEAN + rd.IR_SCALE * z)))
    return dict(x=(np.cos(angle) * r).astype(f32), y=(np.sin(angle) * r).astype(f32), ir=ir[ir >= rd.IR_MIN].astype(f32))

  ir_t = fields(tz, tg)['ir']
  assert ((ir_t < 315) & (ir_t >= 225)).sum() > 100                     # (values off the saturated plateau take part)
  a, b = fields(tz, tg), fields(hz, hg)
  for k in a:
    assert a[k].shape == b[k].shape, k                                   # (the same accept / reject decisions)
    steps = rd.f32_steps(a[k], b[k])
    print(f'{k}: {np.mean(steps == 0):.5f} bitwise, worst {steps.max()} step(s) of {steps.size}')
    assert steps.max() <= 1 and np.mean(steps == 0) >= 0.999, k


@pytest.fixture(scope='module')
def law_sample():
  return rd.sample(17, np.arange(N_LAW), 0)


def test_laws_of_the_eight_fields(law_sample):
  """KS of every field against its law at the 0.1 % point, the IR atom at 315.0 and the law below it, the acceptance rate of the IR
  loop, pairwise and lag-1 independence, and a stream that runs past 64 words."""
  st = rd.assert_laws(law_sample, 'twin')
  rd.assert_acceptance(law_sample['tries'])
  assert law_sample['words'].max() > 64 and law_sample['words'].min() >= 28
  # the twin's own radius and angle (before x and y are formed and rounded) obey the same laws
  assert rd.ks(rd.beta_cdf(law_sample['radius'] / rd.RADIUS_M)) <= rd.ks_bound(N_LAW)
  assert rd.ks(law_sample['angle'] / (2.0 * np.pi)) <= rd.ks_bound(N_LAW)
  assert 0.95 < rd.ir_saturated_share() < 0.97 and abs(rd.ir_acceptance() - 0.5014) < 1e-4


def test_scalar_and_seeded_forms_are_one_function():
  """sample() keys nothing by position: environment i of a scalar-seed batch at env_offset is (seed, env_offset + i), a seeded
  environment is (seed[i], 0), whatever stands next to it."""
  whole = rd.sample(17, 5 + np.arange(40), np.arange(40) % 3)
  for i in (0, 13, 39):
    one = rd.sample(17, 5 + i, i % 3)
    for k in whole:
      np.testing.assert_array_equal(whole[k][i:i + 1], one[k], err_msg=k)
  a, b = rd.sample([3, 2 ** 64 - 1], 0, 0), rd.sample(np.array([3, -1], np.int64), [0, 0], [0, 0])
  for k in a:
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)
  assert not np.array_equal(rd.sample(17, 2 ** 32, 0)['x'], rd.sample(17, 0, 0)['x'])          # the key's high word counts
  assert not np.array_equal(rd.sample(17, 0, 2 ** 32 - 1)['x'], rd.sample(17, 0, 0)['x'])
  idx = rd.vehicle_index(17, np.arange(4096), 0, 3)
  assert set(idx.tolist()) == {0, 1, 2} and (rd.vehicle_index(17, np.arange(64), 0, 1) == 0).all()


# ----------------------------------------------------------------------- the checks can fail
def test_radius_check_tells_beta_1p2_2p1(law_sample):
  """The fault 'second gamma at shape 2.1' (mean 0.364, variance 0.053: inside the moment bounds of the older test): the same radius
  sample against Beta(1.2, 2.1) is outside the KS bound."""
  r = np.hypot(law_sample['x'].astype(np.float64), law_sample['y'].astype(np.float64)) / rd.RADIUS_M
  d = rd.ks(rd.beta_cdf(r, 1.2, 2.1))
  print(f'KS against Beta(1.2, 2.1): {d:.4f} (bound {rd.ks_bound(N_LAW):.5f})')
  assert d > rd.ks_bound(N_LAW)


def test_swapped_sincos_variant_differs():
  """cos and sin exchanged leaves every law as it is (the angle's is uniform either way) and still differs from the twin, value by
  value: only the draw-by-draw comparison sees it."""
  a, b = rd.sample(17, np.arange(1000), 0), rd.sample(17, np.arange(1000), 0, swap_sincos=True)
  np.testing.assert_array_equal(a['x'], b['y']); np.testing.assert_array_equal(a['y'], b['x'])
  for k in ('x', 'y'):
    assert np.mean(rd.f32_steps(a[k], b[k]) > 1) > 0.99, k
  for k in ('alpha', 'start_unix', 'pressure', 'center_lat_deg', 'center_lng_deg', 'upwelling_infrared', 'words', 'tries'):
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_f32_steps():
  one = np.float32(1.0)
  assert rd.f32_steps([one, -one, 0.0, 0.0], [np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(0)), -0.0, 1e-45]).tolist() == [1, 1, 0, 1]
