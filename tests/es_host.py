"""NumPy twin of the evolution strategy, written from the definition there and not from the kernels: the Philox address of
eps_i[q], its normal deviate, the perturbation, the gradient estimate, the centred ranks, and the whole loop with optax's Adam.
TEST TOOLING."""
import numpy as np

import plan_host
import train_host

ES_KEY = 0x45564F4C5645          # "EVOLVE"
M32 = 0xFFFFFFFF
U64 = 2 ** 64 - 1
f32 = np.float32


def address(seed, pair, generation, q):
  """key uint64 [..., 2] and counter uint64 [..., 4] of eps_pair[q] in `generation`; pair and q broadcast."""
  key64 = (int(seed) & U64) ^ ES_KEY
  gen = int(generation) & U64
  pair, q = np.broadcast_arrays(np.asarray(pair, np.uint64), np.asarray(q, np.uint64))
  key = np.empty(q.shape + (2,), np.uint64)
  key[..., 0] = key64 & M32
  key[..., 1] = (key64 >> 32) ^ (gen >> 32)
  counter = np.empty(q.shape + (4,), np.uint64)
  counter[..., 0] = q & np.uint64(M32)
  counter[..., 1] = gen & M32
  counter[..., 2] = pair & np.uint64(M32)
  counter[..., 3] = (pair >> np.uint64(32)) ^ (q >> np.uint64(32))
  return key, counter


def words(seed, pair, generation, q):
  """The four words of the block, uint32 [..., 4]."""
  key, counter = address(seed, pair, generation, q)
  return plan_host.philox4x32(counter, key)


def normal_from_words(w):
  """Box-Muller's cosine branch on (1 - u1, u2): u1 from words 3 (high) and 2, u2 from words 1 (high) and 0, 53 bits each; float64."""
  w = w.astype(np.uint64)
  u1 = (((w[..., 3] << np.uint64(32)) | w[..., 2]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
  u2 = (((w[..., 1] << np.uint64(32)) | w[..., 0]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
  return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2.0 * np.pi * u2)


def noise(seed, generation, streams, d, q0=0):
  """eps float32 [streams, d] of logical parameters q0 .. q0 + d - 1."""
  pair = np.arange(streams, dtype=np.uint64)[:, None]
  q = np.arange(q0, q0 + d, dtype=np.uint64)[None, :]
  return normal_from_words(words(seed, pair, generation, q)).astype(f32)


def perturb(theta, sigma, eps):
  """(theta + fl(sigma eps), theta - fl(sigma eps)) in float32."""
  theta, eps = np.asarray(theta, f32), np.asarray(eps, f32)
  s = f32(sigma) * eps
  return theta + s, theta - s


def population(theta, sigma, eps, antithetic=True):
  """[P, d]: antithetic: rows 2i, 2i + 1 = theta +- sigma eps_i; otherwise row i = theta + sigma eps_i."""
  plus, minus = perturb(np.asarray(theta, f32)[None, :], sigma, eps)
  if not antithetic:
    return plus
  out = np.empty((2 * eps.shape[0], eps.shape[1]), f32)
  out[0::2], out[1::2] = plus, minus
  return out


def gradient(w, eps, sigma, weight_decay=0.0, theta=None, sign=-1.0, divide_by_sigma=True):
  """grad float32 [d] = fl32(-(1 / (streams sigma)) sum_i w_i eps_i) with the sum ascending in float64, each product rounded first;
  then + fl32(wd theta).  sign / divide_by_sigma: the deliberately wrong variants the tests show they can tell."""
  w, eps = np.asarray(w, f32).astype(np.float64), np.asarray(eps, f32).astype(np.float64)
  acc = np.zeros(eps.shape[1], np.float64)
  for i in range(eps.shape[0]):
    acc = acc + w[i] * eps[i]
  denom = float(eps.shape[0]) * (float(f32(sigma)) if divide_by_sigma else 1.0)
  g = ((sign * (1.0 / denom)) * acc).astype(f32)
  if weight_decay != 0.0:
    g = g + f32(weight_decay) * np.asarray(theta, f32)
  return g


def centered_ranks(fitness):
  """float32 [P] in [-0.5, 0.5]; equal values in member order."""
  fitness = np.asarray(fitness, f32)
  p = fitness.size
  order = np.argsort(fitness, kind='stable')
  rank = np.empty(p, np.int64)
  rank[order] = np.arange(p)
  if p == 1:
    return np.zeros(1, f32)
  return rank.astype(f32) / f32(p - 1) - f32(0.5)


def shape_fitness(fitness, antithetic=True, shaping='centered_rank'):
  u = centered_ranks(fitness) if shaping == 'centered_rank' else np.asarray(fitness, f32)
  return (u[0::2] - u[1::2]) * f32(0.5) if antithetic else u


def run(theta0, fitness_fn, members, sigma, lr, generations, seed=0, shaping='centered_rank', adam_eps=1e-8):
  """The loop on a flat parameter vector: perturb, fitness_fn(population [P, d]) -> [P], shape, gradient, Adam (float64 state, the
  parameters rounded to float32 after every step).  -> the centre after every generation, [generations + 1, d]."""
  theta = np.asarray(theta0, f32).copy()
  m, v = np.zeros(theta.size), np.zeros(theta.size)
  out = [theta.copy()]
  for g in range(generations):
    eps = noise(seed, g, members // 2, theta.size)
    w = shape_fitness(fitness_fn(population(theta, sigma, eps)), True, shaping)
    grad = gradient(w, eps, sigma)
    new, m, v = train_host.adam(theta, grad, m, v, g + 1, lr, eps=adam_eps)
    theta = new.astype(f32)
    out.append(theta.copy())
  return np.stack(out)


# ---- the logical parameter order of a network: layer by layer, the kernel row-major [in][out], then the bias
def flatten(kernels, biases):
  return np.concatenate([np.concatenate([np.asarray(k, f32).ravel(), np.asarray(b, f32).ravel()]) for k, b in zip(kernels, biases)])


def unflatten(flat, kernels, biases):
  """flat -> (kernels, biases) shaped like the given ones."""
  ks, bs, at = [], [], 0
  for k, b in zip(kernels, biases):
    ks.append(np.asarray(flat[at:at + k.size], f32).reshape(k.shape)); at += k.size
    bs.append(np.asarray(flat[at:at + b.size], f32).reshape(b.shape)); at += b.size
  assert at == np.size(flat)
  return ks, bs


# ---- the learning test's problem, shared by tests/test_es_host.py (the twin) and tests/test_gpu_population.py (the device)
LEARN_GENERATIONS = 600


def learning_problem():
  """The centre's start (a (1, -, 1) network's 3300 parameters in logical order) and the optimum W* = start + U(-4, 4)."""
  rng = np.random.default_rng(0)
  d = 1099 * 3 + 3
  theta0 = rng.uniform(-0.07, 0.07, d).astype(f32)
  return theta0, (theta0 + rng.uniform(-4.0, 4.0, d)).astype(f32)
