"""NumPy twin of the scenario winds, written from the definition there and not from the kernels: the scenario stream
(Philox4x32-10 of tests/plan_host.py), the prior field f_m (oracle/noise_oracle.py's composition over the stream's harmonics), the
pathwise conditioning alpha^m = (K + 0.05 I)^-1 (y - f_m(X)) by cho_solve over the window frozen at the anchor (tests/wind_gp_host.py's
kernel), the scenario wind f_m(x) + k(X, x) alpha^m, and the risk score.  TEST TOOLING."""
import numpy as np
import scipy.linalg

import noise_oracle
import plan_host
import wind_gp_host

SCENARIO_KEY = 0x5343454E4152          # "SCENAR"
TRUTH_KEY = 0x5EEDF00D                 # the key constant of the environment's true noise
BLOCKS_PER_SCENARIO = 32
ROWS = 120
HORIZON_S = 6 * 3600
NOISE2 = wind_gp_host._SIGMA_NOISE_SQUARED
M64 = 2 ** 64 - 1


def stream_words(seed, key, episode, first_block, blocks, key_constant=SCENARIO_KEY):
  """The words of a stream from block `first_block` on, in the order they are taken: 3, 2, 1, 0 of every block.  uint32 [4 blocks]."""
  k = (int(seed) & M64) ^ key_constant
  counter = np.zeros((blocks, 4), np.uint64)
  counter[:, 0] = first_block + np.arange(blocks)
  counter[:, 1] = int(episode) & 0xFFFFFFFF
  counter[:, 2] = int(key) & 0xFFFFFFFF
  counter[:, 3] = (int(key) >> 32) & 0xFFFFFFFF
  out = plan_host.philox4x32(counter, np.broadcast_to(np.array([k & 0xFFFFFFFF, k >> 32], np.uint64), (blocks, 2)))
  return out[:, ::-1].reshape(-1)


def harmonics_of_words(words):
  """Ten harmonics from 90 words: (seeds uint32 [2, 5], offsets float32 [2, 5, 4]); harmonic k = 5 comp + h takes words 9 k .. 9 k + 8:
  the generator seed, then (hi, lo) of four uniforms u = ((hi << 32 | lo) >> 11) 2^-53, offset = float32(2 u - 1) of x, y, p, t."""
  w = np.asarray(words[:90], np.uint64).reshape(10, 9)
  seeds = w[:, 0].astype(np.uint32).reshape(2, 5)
  u = (((w[:, 1::2] << np.uint64(32)) | w[:, 2::2]) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
  return seeds, (2.0 * u - 1.0).astype(np.float32).reshape(2, 5, 4)


def harmonics(seed, key, episode, m):
  """The harmonics of scenario m of the environment with stream (seed, key, episode): key = env_offset + e under a batch seed, 0 under a
  seed per environment."""
  return harmonics_of_words(stream_words(seed, key, episode, BLOCKS_PER_SCENARIO * int(m), 23))


def truth_harmonics(seed, key, episode):
  """The harmonics of the environment's TRUE noise (csrc/ble_noise.h: seed ^ 0x5EEDF00D, blocks from 0)."""
  return harmonics_of_words(stream_words(seed, key, episode, 0, 23, TRUTH_KEY))


def words_of_harmonics(seeds, offsets):
  """The 50 words the device keeps per generator: uint32 [10, 5] = (seed, bits of ox, oy, op, ot)."""
  return np.concatenate([np.asarray(seeds, np.uint32).reshape(10, 1), np.asarray(offsets, np.float32).reshape(10, 4).view(np.uint32)], 1)


def prior(seeds, offsets, x, y, p, t, dtype=np.float32):
  """f_m at the points: [q, 2] float64 (dtype: the precision of the coordinates and the primitive, float32 as the device)."""
  return noise_oracle.wind_noise(np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(p, np.float32), np.asarray(t), seeds,
                                 offsets, dtype)


class Window:
  """The window FROZEN at `anchor`: the newest 120 ring entries with |t_i - anchor| < 6 h, and its factor."""

  def __init__(self, ring, anchor):
    xyp, t, err = ring
    self.keep = np.flatnonzero(np.abs(np.asarray(t, np.float64) - float(anchor)) < HORIZON_S)[-ROWS:]
    self.n_obs = len(self.keep)
    self.xyp, self.t = np.asarray(xyp, np.float64)[self.keep], np.asarray(t, np.float64)[self.keep]
    self.loc = np.column_stack([self.xyp, self.t])
    self.y = np.asarray(err, np.float64)[self.keep]
    if self.n_obs:
      k = wind_gp_host._kernel(self.loc, self.loc)
      k[np.diag_indices_from(k)] += NOISE2
      self.k = k
      self.chol = (scipy.linalg.cholesky(k, lower=True), True)

  def solve(self, rhs):
    return scipy.linalg.cho_solve(self.chol, np.asarray(rhs, np.float64)) if self.n_obs else np.zeros((0, 2))

  def alpha(self, f_at_window):
    """alpha^m = (K + 0.05 I)^-1 (y - f_m(X)); f_at_window [n_obs, 2]: the prior at the window's points."""
    return self.solve(self.y - np.asarray(f_at_window, np.float64))

  def belief_alpha(self):
    return self.solve(self.y)

  def correction(self, alpha, points, t):
    """sum_i k(loc_i, x) alpha_i at points [q, 3], times t [q]: [q, 2] float64."""
    if not self.n_obs:
      return np.zeros((len(points), 2))
    return wind_gp_host._kernel(np.column_stack([np.asarray(points, np.float64), np.asarray(t, np.float64)]), self.loc) @ alpha


def scenario_wind(prior_uv, correction_uv):
  """ONE float32 addition of two float32 values: the prior and the correction, each rounded to float32 first."""
  return np.asarray(prior_uv).astype(np.float32) + np.asarray(correction_uv).astype(np.float32)


def risk_order(ret):
  """The scenarios of one plan, smallest return first: the return ascending (-0 == +0), then m ascending."""
  value = np.asarray(ret, np.float32).astype(np.float64) + 0.0
  return np.lexsort((np.arange(len(value)), value))


def risk_score(ret, tail):
  """The mean of the `tail` smallest of the M returns: a float64 sum from 0.0 in that order, one division, one rounding to float32.  Any
  non-finite return: NaN."""
  ret = np.asarray(ret, np.float32)
  if not np.isfinite(ret).all():
    return np.float32(np.nan)
  total = 0.0
  for m in risk_order(ret)[:int(tail)]:
    total = total + float(ret[m])
  return np.float32(total / float(tail))


def risk_scores(ret, tail):
  """ret [..., M] -> [...] float32."""
  ret = np.asarray(ret, np.float32)
  flat = ret.reshape(-1, ret.shape[-1])
  return np.array([risk_score(r, tail) for r in flat], np.float32).reshape(ret.shape[:-1])
