"""ONE table of WindGP rings and anchors for the kernels that take their window from ble_gp_factor.h (ble_gp_query.h, ble_gp_belief.h's
ble_gp_fit_kernel, ble_scenarios.h's ble_gp_fit_scenarios_kernel: one copy of the rule, three callers with exits of their own): windows that end at the wave boundary of the ballot pair, anchors
that make the window a suffix, an interior slice or a prefix of the ring, the strict < 21 600 s edge from both sides, the wrapped and
over-full ring with and without the documented exception.  Host only (NumPy); tests/test_gp_window_cases_host.py checks the table
itself, tests/test_gpu_gp_windows.py holds the three kernels to it.  TEST TOOLING.

What must come out of a case -- n_obs (-1: NaN) and whether BLE_FLAG_GP_WINDOW is raised -- is `expected`: include/ble_abi.h's rule
(ble_gp_query_f32, ble_gp_fit_f32) restated over the entries the ring holds, in the order helpers.ring_back gives them.  No kernel and
no twin enters it.  The posterior is `Twin`: tests/wind_gp_host.py's kernel and scikit-learn's algebra over a GIVEN set of entries, so
that the window can be shifted by one entry on purpose (the host test's condition on the inputs)."""
import dataclasses
from typing import Callable, Optional

import numpy as np
import scipy.linalg

import helpers
import wind_gp_host

CAP = helpers.GP_CAPACITY          # 128
ROWS = helpers.GP_ROWS             # 120
HORIZON_S = helpers.GP_HORIZON_S   # 21 600
Q = 8                              # query points per case


@dataclasses.dataclass(frozen=True)
class Case:
  name: str
  count: int
  spacing: int
  end: Optional[int]                                  # time of the newest observation (None: spacing * (count - 1))
  anchor: Callable[[np.ndarray], int]                 # of the times of ALL `count` observations, chronological
  in_window: Optional[int]                            # held entries with |t - anchor| < 6 h (None: not looked at, a restart is pending)
  n_obs: int                                          # the table's column: what the header's rule gives (-1: NaN)
  flag: int
  move: Optional[Callable[[np.ndarray, int], dict]] = None      # (times, anchor) -> {index: new time}: entries put on the strict edge
  reset: bool = False                                 # a history restart is pending (reset_mask[e] != 0)


def _newest(offset=0):
  return lambda t: int(t[-1]) + offset


CASES = tuple(
    [Case(f'suffix_{m}', m, 180, None, _newest(), m, m, 0) for m in (63, 64, 65, 119)] + [
        Case('ahead_2h', 100, 180, None, _newest(7200), 80, 80, 0),          # the entry aged exactly 21 600 s is out
        Case('behind_20min', 100, 180, None, _newest(-1200), 100, 100, 0),
        Case('interior', 128, 400, 60000, lambda t: int(t[64]), 107, 107, 0),          # both ends cut
        Case('prefix', 128, 400, 60000, lambda t: int(t[0]) - 3600, 45, 45, 0),        # the oldest inside, not wrapped
        Case('prefix_wrapped', 129, 400, 60000, lambda t: int(t[1]) - 3600, 45, -1, 1),
        Case('wrapped_suffix', 200, 180, None, _newest(), 120, 120, 0),
        Case('overfull_wrapped_now', 300, 60, None, _newest(), 128, 120, 1),
        Case('overfull_wrapped_ahead', 300, 60, None, _newest(600), 128, 120, 1),
        Case('overfull_wrapped_one_back', 300, 60, None, _newest(-60), 128, -1, 1),
        Case('overfull_interior_unwrapped', 128, 60, None, lambda t: int(t[64]), 128, 120, 1),          # the newest 120
        Case('upper_wave_only', 128, 300, 60000, lambda t: int(t[63]) + HORIZON_S, 64, 64, 0),          # lanes 0 .. 63 all out
        Case('lower_wave_only', 128, 300, 60000, lambda t: int(t[64]) - HORIZON_S, 64, 64, 0),          # lanes 64 .. 127 all out
        Case('empty_far_ahead', 200, 180, None, _newest(7 * 3600), 0, 0, 0),
        Case('pending_restart', 40, 180, None, _newest(), None, 0, 0, reset=True),
        # the strict edge from both sides (the regular grids above only ever hit "exactly 21 600"): 21 600 is out, 21 599 is in
        Case('edge_old_side', 50, 180, 40000, _newest(), 49, 49, 0, move=lambda t, a: {0: a - HORIZON_S, 1: a - HORIZON_S + 1}),
        Case('edge_new_side', 50, 180, 40000, lambda t: int(t[0]), 49, 49, 0,
             move=lambda t, a: {len(t) - 2: a + HORIZON_S - 1, len(t) - 1: a + HORIZON_S}),
    ])
NAMES = tuple(c.name for c in CASES)


def index(name):
  return NAMES.index(name)


def build(i):
  """Case i: (observations (xyp [count, 3] f32, t [count] i32, err [count, 2] f32) for helpers.write_ring, anchor)."""
  case = CASES[i]
  xyp, t, err = helpers.observations(np.random.default_rng(i), case.count, case.spacing, case.end)
  anchor = case.anchor(t)
  if case.move is not None:
    t = t.copy()
    for k, value in case.move(t, anchor).items():
      t[k] = value
    assert (np.diff(t) > 0).all(), case.name          # the ring stays chronological
  return (xyp, t, err), int(anchor)


def held(obs):
  """What the ring holds after helpers.write_ring(obs), as helpers.ring_back reads it back: the newest 128, chronological, float64."""
  xyp, t, err = obs
  return xyp[-CAP:].astype(np.float64), t[-CAP:].astype(np.float64), err[-CAP:].astype(np.float64)


def expected(count, held_t, anchor, reset=False):
  """include/ble_abi.h's rule over the held entries (chronological): (entries inside the window, n_obs, flag).
    - count == 0 or a pending restart: n_obs 0
    - the window: every held entry with |t_i - anchor| < 21 600 s, strict
    - more than 120 inside: the newest 120, and the flag
    - count > 128 and the oldest held entry inside the window: -1 (NaN) and the flag -- unless the window was cut to its newest 120
      for an anchor not earlier than the newest observation."""
  if reset or count == 0:
    return None, 0, 0
  ages = [abs(int(ti) - int(anchor)) for ti in held_t]
  inside = [a < HORIZON_S for a in ages]
  n_in = sum(inside)
  cut = n_in > ROWS
  if count > CAP and inside[0] and not (cut and int(anchor) >= int(held_t[-1])):
    return n_in, -1, 1
  return n_in, min(n_in, ROWS), int(cut)


def kept(held_t, anchor):
  """Indices (into the held entries) of the window the posterior is built from: the newest 120 inside the strict 6 h."""
  return helpers.gp_window(held_t, anchor)


class Twin:
  """The posterior over the held entries `keep` (chronological indices into the ring read back): tests/wind_gp_host.py's algebra."""

  def __init__(self, ring, keep):
    xyp, t, err = ring
    self.keep = np.asarray(keep, np.int64)
    self.n_obs = len(self.keep)
    self.xyp, self.t, self.y = xyp[self.keep], t[self.keep], err[self.keep]
    self.loc = np.column_stack([self.xyp, self.t])
    if self.n_obs:
      k = wind_gp_host._kernel(self.loc, self.loc)
      k[np.diag_indices_from(k)] += wind_gp_host._SIGMA_NOISE_SQUARED
      self.k = k
      self.chol = scipy.linalg.cholesky(k, lower=True)
      self.alpha = self.solve(self.y)

  def solve(self, rhs):
    return scipy.linalg.cho_solve((self.chol, True), np.asarray(rhs, np.float64)) if self.n_obs else np.zeros((0, 2))

  def _k_star(self, points, t):
    t = np.broadcast_to(np.asarray(t, np.float64), (len(points),))
    return wind_gp_host._kernel(np.column_stack([np.asarray(points, np.float64), t]), self.loc)

  def mean(self, points, t, alpha=None):
    """sum_i k(loc_i, (x, y, p, t)) alpha_i at points [q, 3], time(s) t: [q, 2] float64 (alpha: the belief's K^-1 y by default)."""
    if not self.n_obs:
      return np.zeros((len(points), 2))
    return self._k_star(points, t) @ (self.alpha if alpha is None else alpha)

  def deviation(self, points, t):
    if not self.n_obs:
      return np.zeros(len(points))
    v = scipy.linalg.solve_triangular(self.chol, self._k_star(points, t).T, lower=True)
    var = wind_gp_host._SIGMA_EXP_SQUARED - np.einsum('ij,ij->j', v, v)
    return np.where(var < 0.0, 0.0, var) / wind_gp_host._SIGMA_EXP_SQUARED


def points(i, ring, keep):
  """The Q query points of case i, [Q, 3] float32, and the indices of its BOUNDARY points among them: the (x, y, p) of the oldest and
  the newest observation the twin keeps and of the first one it leaves out on either side, where there is one; the rest random."""
  rng = np.random.default_rng(1000 + i)
  pts = np.concatenate([rng.uniform(-2.5e5, 2.5e5, (Q, 2)), rng.uniform(4000.0, 15000.0, (Q, 1))], -1).astype(np.float32)
  boundary = []
  if len(keep):
    xyp = ring[0]
    at = [keep[0], keep[-1]] + ([keep[0] - 1] if keep[0] > 0 else []) + ([keep[-1] + 1] if keep[-1] + 1 < len(xyp) else [])
    for j, k in enumerate(at):
      pts[j] = xyp[k].astype(np.float32)
      boundary.append(j)
  return pts, boundary


def shifted_windows(keep, m):
  """The window moved by one entry at its old end and at its new end, each way: {name: indices} over m held entries."""
  first, last = int(keep[0]), int(keep[-1])
  out = {'old end, one fewer': np.arange(first + 1, last + 1), 'new end, one fewer': np.arange(first, last)}
  if first > 0:
    out['old end, one more'] = np.arange(first - 1, last + 1)
  if last + 1 < m:
    out['new end, one more'] = np.arange(first, last + 2)
  if last + 1 < m:
    out['slid one newer'] = np.arange(first + 1, last + 2)
  if first > 0:
    out['slid one older'] = np.arange(first - 1, last)
  return out
