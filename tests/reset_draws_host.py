"""NumPy twin of the sampled device reset ("The reset sampler's contract"), written from the definition there and not from
the kernel: the Philox4x32-10 word stream of one (seed, key, episode), its uniform / normal / gamma deviates and the eight draws of
reset_device(sample=True), in fp64, rounded to float32 where the state stores float32.  Vectorised over environments: every
environment keeps its own position in its own stream, the two rejection loops run under masks.  Also the analytic laws of the eight
fields and the statistics (Kolmogorov-Smirnov, correlations) the CPU and the GPU tests hold a sample to.  TEST TOOLING."""
import numpy as np
import scipy.special

import plan_host
import reset_host

FLEET_KEY = 0xF1EE7C0DE
UNIX_2011 = 1293840000
START_SPAN = 126144000          # 2011-01-01 .. 2014-12-31, seconds
RADIUS_M = 200000.0
MIN_ALTITUDE_M = 15240.0        # 50 000 ft
P_MIN = 6500.0
IR_MAX, IR_MIN, IR_MEAN, IR_SCALE, IR_SATURATE, IR_TRIES, GAMMA_TRIES = 315.0, 225.0, 2.0, 315.0, 700.0, 64, 64
M32 = np.uint64(0xFFFFFFFF)
U64 = 2 ** 64 - 1
FLOAT_FIELDS = ('x', 'y', 'pressure', 'center_lat_deg', 'center_lng_deg', 'upwelling_infrared')


def u64(a):
  """Python ints or any integer array -> uint64 array (two's complement for negative int64)."""
  if not isinstance(a, np.ndarray):
    a = np.asarray(a, object)                  # (Python ints of any size, exactly)
  if a.dtype == object:
    return np.array([int(v) & U64 for v in np.ravel(a)], np.uint64).reshape(a.shape)
  assert a.dtype.kind in 'iu', a.dtype
  return a.astype(np.int64).view(np.uint64) if a.dtype.kind == 'i' else a.astype(np.uint64)


class Streams:
  """One word stream per environment: key (seed lo, seed hi), counter (block, episode, key lo, key hi); words are popped from out[3]
  down to out[0], then the block advances.  blocks: how many blocks are generated at a time (a caller that reads few words asks
  for few)."""

  def __init__(self, seed, key, episode, blocks=16):
    seed, key, episode = np.broadcast_arrays(np.atleast_1d(u64(seed)), np.atleast_1d(u64(key)), np.atleast_1d(u64(episode)))
    self.n = seed.size
    self._key = np.stack([seed & M32, seed >> np.uint64(32)], -1)
    self._tail = np.stack([episode & M32, key & M32, key >> np.uint64(32)], -1)
    self._words = np.empty((self.n, 0), np.uint64)
    self.pos = np.zeros(self.n, np.int64)             # words consumed so far
    self._rows = np.arange(self.n)
    self._blocks = blocks

  def _extend(self):
    blocks = self._blocks
    first = self._words.shape[1] // 4
    counter = np.empty((self.n, blocks, 4), np.uint64)
    counter[..., 0] = np.arange(first, first + blocks, dtype=np.uint64)[None, :]
    counter[..., 1:] = self._tail[:, None, :]
    out = plan_host.philox4x32(counter, np.broadcast_to(self._key[:, None, :], (self.n, blocks, 2)))
    self._words = np.concatenate([self._words, out[..., ::-1].reshape(self.n, 4 * blocks).astype(np.uint64)], 1)

  def u32(self, mask=None):
    """The next word of every environment in `mask` (all if None); the others keep their position (their entry is meaningless)."""
    mask = np.ones(self.n, bool) if mask is None else mask
    while self.pos[mask].max(initial=-1) >= self._words.shape[1]:
      self._extend()
    w = self._words[self._rows, np.minimum(self.pos, self._words.shape[1] - 1)]
    self.pos = self.pos + mask
    return w

  def uniform(self, mask=None):
    hi = self.u32(mask)
    lo = self.u32(mask)
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53

  def normal(self, mask=None):
    """Box-Muller on (1 - u, u), the cosine branch."""
    u1 = 1.0 - self.uniform(mask)
    u2 = self.uniform(mask)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)

  def gamma(self, shape, mask=None):
    """Marsaglia-Tsang, shape >= 1: x normal, t = 1 + c x; t <= 0 consumes the normal only; else u = 1 - uniform and accept when
    log u < x^2 / 2 + d - d t^3 + d log t^3.  d after 64 rejected tries."""
    d = shape - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    active = np.ones(self.n, bool) if mask is None else mask.copy()
    out = np.full(self.n, d)
    for _ in range(GAMMA_TRIES):
      if not active.any():
        break
      x = self.normal(active)
      t = 1.0 + c * x
      live = active & (t > 0.0)
      v = np.where(live, t * t * t, 1.0)
      u = 1.0 - self.uniform(live)
      accept = live & (np.log(u) < 0.5 * x * x + d - d * v + d * np.log(v))
      out = np.where(accept, d * v, out)
      active &= ~accept
    return out


def p_max(alpha):
  """The pressure at 50 000 ft in the atmosphere of (float32) alpha."""
  return reset_host.AtmosphereTables(np.asarray(alpha, np.float64)).at_height(MIN_ALTITUDE_M)[0]


def sample(seed, key, episode, swap_sincos=False):
  """The eight draws of every environment, in order, from the stream of (seed[i], key[i], episode[i]).  -> dict: the stored fields
  (float32 / int64), `radius` and `angle` (fp64, before x and y are formed), `words` consumed and IR `tries`.
  swap_sincos: the deliberately wrong variant x = sin r, y = cos r (the tests show that they can tell it)."""
  g = Streams(seed, key, episode)
  f32 = np.float32
  alpha = g.uniform().astype(f32)
  start = UNIX_2011 + np.trunc(g.uniform() * float(START_SPAN)).astype(np.int64)
  ga = g.gamma(1.2)
  gb = g.gamma(2.0)
  radius = RADIUS_M * (ga / (ga + gb))
  angle = 2.0 * np.pi * g.uniform()
  cs, sn = (np.sin(angle), np.cos(angle)) if swap_sincos else (np.cos(angle), np.sin(angle))
  lat = -10.0 + 20.0 * g.uniform()
  lng = -175.0 + 350.0 * g.uniform()
  pm = p_max(alpha)
  pressure = P_MIN + (pm - P_MIN) * g.uniform()
  active = np.ones(g.n, bool)
  ir = np.full(g.n, IR_MAX)
  tries = np.zeros(g.n, np.int64)
  for _ in range(IR_TRIES):
    if not active.any():
      break
    z = IR_MEAN + IR_SCALE * g.normal(active)
    with np.errstate(over='ignore'):
      value = np.where(z > IR_SATURATE, IR_MAX, np.where(z < -IR_SATURATE, 0.0, IR_MAX / (1.0 + np.exp(-z))))
    ir = np.where(active, value, ir)          # (after 64 rejected tries the last value stands)
    tries += active
    active &= ~(value >= IR_MIN)
  return dict(alpha=alpha, start_unix=start, x=(cs * radius).astype(f32), y=(sn * radius).astype(f32), center_lat_deg=lat.astype(f32),
              center_lng_deg=lng.astype(f32), pressure=pressure.astype(f32), upwelling_infrared=ir.astype(f32),
              radius=radius, angle=angle, words=g.pos.copy(), tries=tries)


def vehicle_index(seed, key, episode, n_vehicles):
  """The palette entry a fleet with sample_per_episode draws: (first word of stream(seed ^ FLEET_KEY, key, episode) * n_vehicles) >> 32."""
  word = Streams(u64(seed) ^ np.uint64(FLEET_KEY), key, episode).u32()
  return ((word * np.uint64(n_vehicles)) >> np.uint64(32)).astype(np.uint8)


# ----------------------------------------------------------------------- float32 distance
def f32_steps(a, b):
  """|a - b| in float32 steps (units in the last place along the ordered float32 line), int64."""
  def line(v):
    i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)
  return np.abs(line(a) - line(b))


# ----------------------------------------------------------------------- the laws
def ks(sample_cdf_hi, sample_cdf_lo=None):
  """The Kolmogorov-Smirnov statistic sup |F_n - F| from the law's CDF at the sample points: for a continuous law pass F(x_i); for a
  law with atoms pass F(x_i) and F(x_i -).  Ties in the sample are handled (F_n jumps once at a tied value)."""
  hi = np.asarray(sample_cdf_hi, np.float64)
  lo = hi if sample_cdf_lo is None else np.asarray(sample_cdf_lo, np.float64)
  order = np.argsort(hi, kind='stable')
  hi, lo = hi[order], lo[order]
  n = hi.size
  last = np.r_[hi[1:] != hi[:-1], True]               # the last of each run of ties
  first = np.r_[True, hi[1:] != hi[:-1]]
  rank = np.arange(1, n + 1)
  return float(max(np.abs(rank[last] / n - hi[last]).max(), np.abs((rank[first] - 1) / n - lo[first]).max()))


def ks_bound(n):
  """The asymptotic 0.1 % point of the statistic, sqrt(ln(2000) / 2) / sqrt(n)."""
  return 1.95 / np.sqrt(n)


def beta_cdf(x, a=1.2, b=2.0):
  return scipy.special.betainc(a, b, np.clip(x, 0.0, 1.0))


def _phi(x):
  return scipy.special.ndtr(x)


def _ir_of(z):
  return IR_MAX / (1.0 + np.exp(-z))


def ir_saturation_z():
  """z*: the smallest z at which 315 sigmoid(z), rounded to float32, is 315.0 (bisection on the rounding itself)."""
  lo, hi = 1.0, 40.0
  for _ in range(200):
    mid = 0.5 * (lo + hi)
    if np.float32(_ir_of(mid)) == np.float32(IR_MAX):
      hi = mid
    else:
      lo = mid
  return hi


Z_ACCEPT = float(np.log(IR_MIN / (IR_MAX - IR_MIN)))             # 315 sigmoid(z) >= 225  <=>  z >= ln 2.5


def ir_acceptance():
  """P(N(2, 315) >= ln 2.5): the share of IR tries that are accepted."""
  return float(1.0 - _phi((Z_ACCEPT - IR_MEAN) / IR_SCALE))


def ir_saturated_share():
  """P(stored IR == 315.0) = P(z >= z*) / P(z >= ln 2.5)."""
  return float((1.0 - _phi((ir_saturation_z() - IR_MEAN) / IR_SCALE)) / ir_acceptance())


def ir_below_cdf(v):
  """P(IR <= v | IR stored below 315) for fp64 v: the logit-normal law truncated to ln 2.5 <= z < z*."""
  v = np.asarray(v, np.float64)
  with np.errstate(divide='ignore'):
    z = np.log(v / (IR_MAX - v))
  a, b = _phi((Z_ACCEPT - IR_MEAN) / IR_SCALE), _phi((ir_saturation_z() - IR_MEAN) / IR_SCALE)
  return np.clip((_phi((z - IR_MEAN) / IR_SCALE) - a) / (b - a), 0.0, 1.0)


def ir_below_ks(ir):
  """KS of the stored (float32) values below 315 against the law of the STORED value.  Near 315 the float32 grid is coarse for this
  law (the value one step below 315 alone holds 7 % of it), so the law has atoms: a stored v holds the mass of its rounding cell,
  F(v) is the continuous CDF at the cell's upper edge and F(v -) at its lower edge."""
  v = np.asarray(ir, np.float32)
  v = v[v < np.float32(IR_MAX)]
  up = (v.astype(np.float64) + np.nextafter(v, np.float32(np.inf)).astype(np.float64)) / 2.0
  down = (v.astype(np.float64) + np.nextafter(v, np.float32(-np.inf)).astype(np.float64)) / 2.0
  return ks(ir_below_cdf(up), ir_below_cdf(down)), v.size


FIELDS = ('alpha', 'start', 'radius', 'angle', 'lat', 'lng', 'pressure', 'ir')


def unit_fields(s):
  """The eight independent quantities of a sample (stored fields only, so a device's state serves as well), each mapped so that its
  law is the one named in `laws`: alpha, (start - 2011) / span, radius / 200 km from (x, y), angle / 2 pi from (x, y), latitude and
  longitude on [0, 1), (p - 6500) / (p_max(alpha) - 6500), and IR as stored."""
  x, y = np.asarray(s['x'], np.float64), np.asarray(s['y'], np.float64)
  alpha = np.asarray(s['alpha'], np.float64)
  return dict(alpha=alpha, start=(np.asarray(s['start_unix'], np.float64) - UNIX_2011) / START_SPAN,
              radius=np.hypot(x, y) / RADIUS_M, angle=np.mod(np.arctan2(y, x), 2.0 * np.pi) / (2.0 * np.pi),
              lat=(np.asarray(s['center_lat_deg'], np.float64) + 10.0) / 20.0, lng=(np.asarray(s['center_lng_deg'], np.float64) + 175.0) / 350.0,
              pressure=(np.asarray(s['pressure'], np.float64) - P_MIN) / (p_max(alpha) - P_MIN),
              ir=np.asarray(s['upwelling_infrared'], np.float64))


def law_statistics(s):
  """Everything the law tests assert, as numbers: KS per continuous field, the IR share at 315.0 and the KS below it, the largest
  pairwise and lag-1 correlations."""
  f = unit_fields(s)
  out = {k: ks(f[k]) for k in ('alpha', 'start', 'angle', 'lat', 'lng', 'pressure')}
  out['radius'] = ks(beta_cdf(f['radius']))
  ir = np.asarray(s['upwelling_infrared'], np.float32)
  out['ir_share'] = float((ir == np.float32(IR_MAX)).mean())
  out['ir_below'], out['ir_below_n'] = ir_below_ks(ir)
  m = np.stack([f[k] for k in FIELDS])
  c = np.corrcoef(m)
  out['corr'] = float(np.abs(c[np.triu_indices(len(FIELDS), 1)]).max())
  lag = np.corrcoef(m[:, :-1], m[:, 1:])[:len(FIELDS), len(FIELDS):]          # field a of environment i with field b of i + 1
  out['lag1'] = float(np.abs(lag).max())
  return out


def assert_laws(s, label=''):
  """The law checks shared by the CPU test (on the twin) and the GPU test (on the device's state); prints every figure first."""
  n = np.asarray(s['x']).size
  st = law_statistics(s)
  print(f'{label} n={n} ' + ' '.join(f'{k}={v:.4f}' if isinstance(v, float) else f'{k}={v}' for k, v in st.items()))
  for k in ('alpha', 'start', 'radius', 'angle', 'lat', 'lng', 'pressure'):
    assert st[k] <= ks_bound(n), (k, st[k], ks_bound(n))
  assert st['ir_below'] <= ks_bound(st['ir_below_n']), (st['ir_below'], st['ir_below_n'])
  share = ir_saturated_share()
  assert abs(st['ir_share'] - share) <= 5.0 * np.sqrt(share * (1.0 - share) / n), (st['ir_share'], share)
  assert st['corr'] < 5.0 / np.sqrt(n) and st['lag1'] < 5.0 / np.sqrt(n), (st['corr'], st['lag1'])
  return st


def assert_acceptance(tries):
  """1 / mean(tries) against P(accept) within 5 standard deviations (tries is geometric; delta method: p sqrt((1 - p) / n))."""
  p = ir_acceptance()
  got = 1.0 / np.mean(tries)
  print(f'IR acceptance {got:.4f} (analytic {p:.4f})')
  assert abs(got - p) <= 5.0 * p * np.sqrt((1.0 - p) / np.size(tries)), (got, p)
  return got
