"""The evolution strategy of DESIGN 3q on a machine without a GPU: the lane functions of csrc/ble_population.h, built for the host
(tests/emul/es_emul.cpp), against the NumPy twin written from the definition (tests/es_host.py) -- the Philox address and words exactly,
the normal deviate to the tolerance of the other normal-deviate twins (tests/test_reset_draws_host.py: 1e-13 relative in float64, here
seen through the float32 rounding: at most one float32 step, and 99.9 % of the values bitwise), everything after eps bit for bit -- the
centred ranks, the independence of eps from the population size, and the estimator itself on a quadratic, with three wrong estimators
shown to fail the same check."""
import numpy as np
import pytest

import es_host
import reset_draws_host as rd
from emul import es_emul

SEED = 0x9E3779B97F4A7C15


@pytest.mark.parametrize('pair,generation,q', [(0, 0, 0), (5, 7, 1234), (2 ** 31 - 1, 2 ** 32 + 9, 3299), (3, 2 ** 63 + 1, 2 ** 32 + 17)])
def test_address_and_words_exact(pair, generation, q):
  kc, w = es_emul.address(SEED, pair, generation, q)
  key, counter = es_host.address(SEED, pair, generation, q)
  assert [int(v) for v in kc] == [int(key[0]), int(key[1])] + [int(c) for c in counter]
  np.testing.assert_array_equal(w, es_host.words(SEED, pair, generation, q))
  # stated once more in plain integers
  k64 = SEED ^ 0x45564F4C5645
  assert [int(v) for v in kc] == [k64 & 0xFFFFFFFF, (k64 >> 32) ^ (generation >> 32), q & 0xFFFFFFFF, generation & 0xFFFFFFFF, pair,
                                  q >> 32]


def test_noise_matches_host_build():
  host = es_emul.noise(SEED, 3, 6, 4096, q0=100)
  twin = es_host.noise(SEED, 3, 6, 4096, q0=100)
  steps = rd.f32_steps(host, twin)
  print(f'normals: max {steps.max()} float32 steps, {np.mean(steps == 0):.5f} bitwise')
  assert steps.max() <= 1 and np.mean(steps == 0) >= 0.999
  # a standard normal: mean, variance and the fourth moment of 24 576 values within five standard errors
  z = twin.astype(np.float64).ravel()
  n = z.size
  assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n) and abs(np.mean(z ** 4) - 3) < 5 * np.sqrt(96 / n)


def test_after_eps_bit_for_bit():
  rng = np.random.default_rng(1)
  d, streams = 777, 9
  eps = es_emul.noise(SEED, 0, streams, d)
  theta = rng.standard_normal(d).astype(np.float32)
  for sigma in (0.02, 1.0, 0.3):
    hp, hm = es_emul.perturb(theta, sigma, eps[0])
    tp, tm = es_host.perturb(theta, sigma, eps[0])
    np.testing.assert_array_equal(hp.view(np.uint32), tp.view(np.uint32))
    np.testing.assert_array_equal(hm.view(np.uint32), tm.view(np.uint32))
    w = rng.standard_normal(streams).astype(np.float32)
    for wd in (0.0, 0.01):
      got = es_emul.gradient(w, eps, sigma, wd, theta)
      want = es_host.gradient(w, eps, sigma, wd, theta)
      np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
  # one-hot weights at sigma = 1 and four streams: the scaling is exact, -4 grad is eps_i
  for i in range(4):
    np.testing.assert_array_equal(-4.0 * es_emul.gradient(np.eye(4, dtype=np.float32)[i], eps[:4], 1.0, 0.0, theta), eps[i])


def test_centered_ranks_of_a_tied_vector():
  r = es_host.centered_ranks([3.0, 1.0, 3.0, -2.0, 1.0])
  np.testing.assert_array_equal(r, np.array([3, 1, 4, 0, 2], np.float32) / np.float32(4) - np.float32(0.5))
  assert r.min() == -0.5 and r.max() == 0.5 and es_host.centered_ranks([7.0]).tolist() == [0.0]
  np.testing.assert_array_equal(es_host.shape_fitness([3.0, 1.0, 3.0, -2.0], True), np.array([(2 - 1) / 3 / 2, (3 - 0) / 3 / 2], np.float32))
  np.testing.assert_array_equal(es_host.shape_fitness([3.0, 1.0, 2.0], False, 'raw'), np.array([3.0, 1.0, 2.0], np.float32))


def test_noise_independent_of_population_size_and_generations_differ():
  small, large = es_host.noise(SEED, 4, 1, 512), es_host.noise(SEED, 4, 4, 512)        # P = 2 against P = 8
  np.testing.assert_array_equal(small[0], large[0])
  np.testing.assert_array_equal(es_emul.noise(SEED, 4, 1, 512)[0], es_emul.noise(SEED, 4, 4, 512)[0])
  other = es_host.noise(SEED, 5, 4, 512)
  assert np.mean(other == large) < 0.01 and abs(np.corrcoef(other.ravel(), large.ravel())[0, 1]) < 5 / np.sqrt(2048)
  assert np.mean(es_host.noise(SEED + 1, 4, 4, 512) == large) < 0.01
  assert abs(np.corrcoef(large[0], large[1])[0, 1]) < 5 / np.sqrt(512)


# ---- the estimator: f(theta) = -|theta - theta*|^2, d = 8, 512 antithetic pairs, raw shaping, sigma = 0.1
D, PAIRS, SIGMA = 8, 512, 0.1


def _cosine(seed, variant='right'):
  rng = np.random.default_rng(100 + seed)
  theta, target = rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32)
  eps = es_host.noise(seed, 0, PAIRS, D)
  pop = es_host.population(theta, SIGMA, eps)
  if variant == 'shared_halves':               # both halves of a pair fly theta + sigma eps
    pop[1::2] = pop[0::2]
  fitness = -np.sum((pop.astype(np.float64) - target) ** 2, axis=1)
  w = es_host.shape_fitness(fitness.astype(np.float32), True, 'raw')
  grad = es_host.gradient(w, eps, SIGMA, sign=1.0 if variant == 'sign' else -1.0, divide_by_sigma=variant != 'no_sigma')
  truth = (theta - target).astype(np.float64)              # grad of -f is 2 (theta - theta*)
  g = grad.astype(np.float64)
  cos = float(g @ truth / (np.linalg.norm(g) * np.linalg.norm(truth))) if np.linalg.norm(g) > 0 else 0.0
  scale = float(np.linalg.norm(g) / np.linalg.norm(2.0 * truth))
  return cos, scale


@pytest.mark.parametrize('seed', range(5))
def test_estimator_points_at_the_optimum(seed):
  """cosine >= 0.9 with theta - theta* (expected sqrt(n / (n + d)) = 0.99), and the length of the true gradient 2 (theta - theta*) within
  25 % (the estimate's relative error is about sqrt(d / n) = 0.125 in all: two of its standard deviations)."""
  cos, scale = _cosine(seed)
  print(f'seed {seed}: cosine {cos:.4f}, length ratio {scale:.4f}')
  assert cos >= 0.9 and 0.75 <= scale <= 1.25


@pytest.mark.parametrize('variant', ['sign', 'no_sigma', 'shared_halves'])
def test_wrong_estimators_fail_the_same_check(variant):
  for seed in range(5):
    cos, scale = _cosine(seed, variant)
    print(f'{variant} seed {seed}: cosine {cos:.4f}, length ratio {scale:.4f}')
    assert not (cos >= 0.9 and 0.75 <= scale <= 1.25)


def test_loop_twin_learns_a_quadratic():
  """The loop of tests/test_gpu_population.py's learning test on the twin: P = 64, sigma 0.05, lr 0.05, centred ranks, fitness
  -|W_p - W*|^2.  With 32 pairs in 3300 dimensions the estimate's cosine with the gradient is about sqrt(32 / 3332) = 0.1, and Adam
  moves a parameter by at most lr a step: 60 generations take the twin to 0.90 of the start, not to a quarter, at any W*; it crosses a
  quarter near generation 480 and is at 0.15 after 600 (its floor, where the noise of the estimate balances the pull, is 0.11).  The
  GPU test therefore runs 600 generations; the quarter stays."""
  theta0, target = es_host.learning_problem()
  path = es_host.run(theta0, lambda pop: -np.sum((pop.astype(np.float64) - target) ** 2, axis=1).astype(np.float32), 64, 0.05, 0.05,
                     es_host.LEARN_GENERATIONS)
  dist = np.linalg.norm(path.astype(np.float64) - target, axis=1)
  print('distance / start at generations 60, 200, 400, 600:', [round(float(dist[g] / dist[0]), 4) for g in (60, 200, 400, 600)])
  assert dist[es_host.LEARN_GENERATIONS] < 0.2 * dist[0]          # (margin: the GPU test asks for a quarter)
