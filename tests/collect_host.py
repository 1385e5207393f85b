"""NumPy twins of the acting and collecting half of training ("The two draw contracts"), written from the text there and
not from the kernels: the epsilon-greedy step (ble_qnet_explore_u8) and the window the uniform replay sampler draws
(ble_replay_sample_f32), both on reset_draws_host.Streams, i.e. Philox4x32-10 in this project's word order.  Also the laws the CPU
test holds the explore twin to and the GPU test the device's own output.  TEST TOOLING."""
import numpy as np

import reset_draws_host
import train_host

M32 = 0xFFFFFFFF
U64 = 2 ** 64 - 1
NUM_ACTIONS = 3
MAX_TRIES = 64
Z_POINT = 3.29             # the 0.1 % two-sided point of a standard normal
CHI2_POINT = 13.82         # the 0.1 % point of chi-squared with 2 degrees of freedom


# ---------------------------------------------------------------------------------------------------------------------- epsilon-greedy
def explore_draws(n, seed, step):
  """(uf, random) of environments 0 .. n - 1 at (seed, step): the first two words u, r of the stream of
  (seed ^ ((step >> 32) << 32), key = i, episode = step & 0xFFFFFFFF); uf = float32(u >> 8) * 2^-24, random = (r * 3) >> 32."""
  seed, step = int(seed) & U64, int(step) & U64
  g = reset_draws_host.Streams(seed ^ ((step >> 32) << 32), np.arange(n, dtype=np.uint64), step & M32, blocks=1)
  u = g.u32()
  r = g.u32()
  uf = (u >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
  return uf, ((r * np.uint64(NUM_ACTIONS)) >> np.uint64(32)).astype(np.uint8)


def explore(actions, epsilon, seed, step):
  """The epsilon-greedy step on uint8 actions [n]: (new actions, replaced mask, uf, random); lane i is replaced by random[i] iff
  uf[i] < float32(epsilon)."""
  actions = np.asarray(actions, np.uint8)
  uf, random = explore_draws(actions.size, seed, step)
  mask = uf < np.float32(epsilon)
  return np.where(mask, random, actions), mask, uf, random


LAW_N, LAW_EPSILON = 65536, 0.1
LAW_CASES = ((3, 0), (3, 1), (2 ** 40 + 5, 2 ** 32 + 1), (11, 2 ** 32 - 1))      # (seed, step)
SENTINEL = 3          # an incoming action no draw gives: a lane that still holds it was left alone


def chi2_uniform(values, bins=NUM_ACTIONS):
  """Pearson's chi-squared of integer values against the uniform law on 0 .. bins - 1."""
  count = np.bincount(np.asarray(values, np.int64), minlength=bins).astype(np.float64)
  expect = count.sum() / bins
  return float(((count - expect) ** 2 / expect).sum())


def corr(a, b):
  return float(np.corrcoef(np.asarray(a, np.float64), np.asarray(b, np.float64))[0, 1])


def assert_explore_laws(run, label=''):
  """The laws of the epsilon-greedy step, on whatever `run(actions, epsilon, seed, step) -> new actions` computes (the twin on the CPU,
  the kernel on the GPU): n = 65 536 lanes that come in holding SENTINEL, epsilon = 0.1 at the four LAW_CASES.  The explored count
  within 3.29 sigma of n epsilon; chi-squared of the actions of the explored lanes and (at epsilon = 1) of all lanes below 13.82; the
  masks of steps 0 and 1, and of neighbouring environments, uncorrelated within 3.29 / sqrt(n).  Prints every figure, then asserts;
  returns the figures."""
  n, eps = LAW_N, LAW_EPSILON
  sigma = np.sqrt(n * eps * (1.0 - eps))
  held = np.full(n, SENTINEL, np.uint8)
  out, masks = {'z': [], 'chi2_explored': [], 'chi2_all': []}, {}
  for seed, step in LAW_CASES:
    got = np.asarray(run(held.copy(), eps, seed, step))
    mask = got != SENTINEL
    assert got.shape == (n,) and (got[mask] < NUM_ACTIONS).all()
    every = np.asarray(run(held.copy(), 1.0, seed, step))
    assert (every < NUM_ACTIONS).all(), 'epsilon = 1 left a lane alone'
    assert np.array_equal(every[mask], got[mask]), 'the action drawn depends on epsilon'
    masks[seed, step] = mask
    out['z'].append(float((mask.sum() - n * eps) / sigma))
    out['chi2_explored'].append(chi2_uniform(got[mask]))
    out['chi2_all'].append(chi2_uniform(every))
  first = masks[LAW_CASES[0]]
  out['corr_steps'] = corr(first, masks[LAW_CASES[1]])
  out['corr_neighbours'] = corr(first[:-1], first[1:])
  print(f'{label} explore laws n={n} eps={eps}: ' + ' '.join(
      f'{k}=' + (f'{v:.4f}' if isinstance(v, float) else '[' + ', '.join(f'{x:.2f}' for x in v) + ']') for k, v in out.items()))
  assert all(abs(z) < Z_POINT for z in out['z']), out['z']
  assert all(c < CHI2_POINT for c in out['chi2_explored']), out['chi2_explored']
  assert all(c < CHI2_POINT for c in out['chi2_all']), out['chi2_all']
  bound = Z_POINT / np.sqrt(n)
  assert abs(out['corr_steps']) < bound and abs(out['corr_neighbours']) < bound, (out['corr_steps'], out['corr_neighbours'], bound)
  return out


# ------------------------------------------------------------------------------------------------------------- the uniform replay draw
def candidates(count, capacity, horizon):
  """(lo_t, span): the candidate window starts are lo_t .. lo_t + span - 1 (steps t .. t + horizon are held)."""
  lo_t = max(int(count) - int(capacity), 0)
  return lo_t, int(count) - int(horizon) - lo_t


def valid_windows(terminal, episode_end, count, capacity, horizon):
  """bool [max(span, 0), N]: whether the window that starts at step lo_t + row of environment env is valid, by train_host.nstep's rule.
  terminal, episode_end: the ring, [capacity, N] (step s lies in row s % capacity)."""
  terminal, episode_end = np.asarray(terminal), np.asarray(episode_end)
  assert terminal.shape == episode_end.shape and terminal.shape[0] == capacity
  lo_t, span = candidates(count, capacity, horizon)
  n_env = terminal.shape[1]
  if span <= 0:
    return np.zeros((0, n_env), bool)
  rows = (lo_t + np.arange(count - lo_t)) % capacity                  # the steps still held, oldest first
  term, end = terminal[rows], episode_end[rows]
  reward = np.zeros(term.shape, np.float32)
  return np.array([[train_host.nstep(reward, term, end, t, env, horizon, 0.5) is not None for env in range(n_env)] for t in range(span)])


def uniform_draws(terminal, episode_end, count, capacity, horizon, batch, seed, counter, max_tries=MAX_TRIES, valid=None):
  """The (t, env) every batch row draws: (index int64 [B, 2], tries used int64 [B]).  Row b reads the stream of
  (seed, key = b | (counter >> 32) << 32, episode = counter & 0xFFFFFFFF); a try takes three words hi, lo, e:
  t = lo_t + mulhi64((hi << 32) | lo, span), env = (e * N) >> 32; the first try whose window is valid wins.  span <= 0 or max_tries
  invalid tries: (-1, -1).  valid: valid_windows(...) of this ring, if the caller has it already."""
  counter, n_env = int(counter) & U64, np.asarray(terminal).shape[1]
  lo_t, span = candidates(count, capacity, horizon)
  index = np.full((batch, 2), -1, np.int64)
  tries = np.zeros(batch, np.int64)
  if span <= 0 or batch == 0:
    return index, tries
  if valid is None:
    valid = valid_windows(terminal, episode_end, count, capacity, horizon)
  key = np.arange(batch, dtype=np.uint64) | np.uint64((counter >> 32) << 32)
  g = reset_draws_host.Streams(int(seed) & U64, key, counter & M32)
  active = np.ones(batch, bool)
  for _ in range(max_tries):
    if not active.any():
      break
    hi, lo, e = g.u32(active), g.u32(active), g.u32(active)
    x = ((hi << np.uint64(32)) | lo).astype(object)                   # (Python integers: the 128-bit product, exactly)
    t = lo_t + np.array((x * span) >> 64, np.int64)
    env = ((e * np.uint64(n_env)) >> np.uint64(32)).astype(np.int64)
    tries += active
    win = active & valid[np.where(active, t - lo_t, 0), np.where(active, env, 0)]
    index[win, 0], index[win, 1] = t[win], env[win]
    active &= ~win
  return index, tries


def random_ring(rng, capacity, n_env, terminal_rate, end_rate):
  """(terminal, episode_end) uint8 [capacity, N]: terminals at terminal_rate, then time-limit ends at end_rate on top of them."""
  terminal = rng.random((capacity, n_env)) < terminal_rate
  episode_end = terminal | (rng.random((capacity, n_env)) < end_rate)
  return terminal.astype(np.uint8), episode_end.astype(np.uint8)


def easy_and_hard_ring():
  """The two fillings the retry and the failure path are held on: N = 37, capacity 24, horizon 5, count 60, one default_rng(0),
  terminal rate 0.02, time-limit ends at 0.05 (easy: most windows are valid) and then at 0.55 (hard: about one in twenty is)."""
  rng = np.random.default_rng(0)
  return random_ring(rng, 24, 37, 0.02, 0.05), random_ring(rng, 24, 37, 0.02, 0.55)
