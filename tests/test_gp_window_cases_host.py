"""The table of WindGP windows (tests/gp_window_cases.py) checked on its own, without a GPU, so that a failure of
tests/test_gpu_gp_windows.py is never the table's fault: the header's rule restated in `expected` reproduces the n_obs / flag column
written into the table, every shift of a window by one entry moves the twin's mean at the case's boundary points far above the GPU
test's 1e-5 bar, and every window is as well conditioned as tests/test_gpu_belief.py's docstring bounds it."""
import numpy as np

import gp_window_cases as wc
import helpers

# case: (entries inside the window, n_obs, flag) -- the column as the table's issue states it, literally
COLUMN = {
    'suffix_63': (63, 63, 0), 'suffix_64': (64, 64, 0), 'suffix_65': (65, 65, 0), 'suffix_119': (119, 119, 0),
    'ahead_2h': (80, 80, 0), 'behind_20min': (100, 100, 0), 'interior': (107, 107, 0), 'prefix': (45, 45, 0),
    'prefix_wrapped': (45, -1, 1), 'wrapped_suffix': (120, 120, 0), 'overfull_wrapped_now': (128, 120, 1),
    'overfull_wrapped_ahead': (128, 120, 1), 'overfull_wrapped_one_back': (128, -1, 1), 'overfull_interior_unwrapped': (128, 120, 1),
    'upper_wave_only': (64, 64, 0), 'lower_wave_only': (64, 64, 0), 'empty_far_ahead': (0, 0, 0), 'pending_restart': (None, 0, 0),
    'edge_old_side': (49, 49, 0), 'edge_new_side': (49, 49, 0),
}
SHIFT_BAR = 1e-3          # m/s: 100 x the GPU test's 1e-5
COND_BAR = 3.2e4          # lambda_max <= 120 x 12.96 + 0.05, lambda_min >= 0.05 (tests/test_gpu_belief.py)


def test_the_rule_reproduces_the_column():
  assert sorted(COLUMN) == sorted(wc.NAMES) and len(wc.CASES) == 20
  print()
  print(f'{"case":30s} {"count":>5s} {"in window":>9s} {"n_obs":>5s} {"flag":>4s}')
  for i, case in enumerate(wc.CASES):
    obs, anchor = wc.build(i)
    ring = wc.held(obs)
    got = wc.expected(case.count, ring[1], anchor, case.reset)
    print(f'{case.name:30s} {case.count:5d} {str(got[0]):>9s} {got[1]:5d} {got[2]:4d}')
    assert got == COLUMN[case.name] == (case.in_window, case.n_obs, case.flag), (case.name, got)
    # the window the twin keeps is what the rule counts, wherever the rule gives a posterior
    if got[1] > 0:
      keep = wc.kept(ring[1], anchor)
      assert len(keep) == got[1] and (np.diff(keep) == 1).all(), case.name
      assert (keep[-1] == np.flatnonzero(np.abs(ring[1] - anchor) < wc.HORIZON_S)[-1]), case.name


def test_the_cases_reach_what_they_are_named_for():
  def inside(name):
    i = wc.index(name)
    obs, anchor = wc.build(i)
    t = wc.held(obs)[1]
    return np.abs(t - anchor) < wc.HORIZON_S, t, anchor, obs
  # the wave boundary of the ballot pair: held entries 0 .. 63 vote on lane, 64 .. 127 on lane + 64
  up, *_ = inside('upper_wave_only')
  assert not up[:64].any() and up[64:].all()
  low, *_ = inside('lower_wave_only')
  assert low[:64].all() and not low[64:].any()
  mid, *_ = inside('interior')
  assert not mid[0] and not mid[-1] and mid[11:118].all() and mid.sum() == 107
  pre, t, anchor, _ = inside('prefix')
  assert pre[0] and not pre[-1] and anchor < t[0]
  # the strict edge: ages 21 600 (out) and 21 599 (in) next to each other, on either side of the anchor
  old, t, anchor, _ = inside('edge_old_side')
  assert (anchor - t[:2]).tolist() == [21600, 21599] and old.tolist() == [False] + [True] * 49
  new, t, anchor, _ = inside('edge_new_side')
  assert (t[-2:] - anchor).tolist() == [21599, 21600] and new.tolist() == [True] * 49 + [False] and anchor < t[-1]
  ahead, t, anchor, _ = inside('ahead_2h')
  assert anchor - t[19] == 21600 and not ahead[19] and ahead[20]
  # wrapped: the ring holds the newest 128 of more, in slots that straddle slot 0
  for name in ('prefix_wrapped', 'wrapped_suffix', 'overfull_wrapped_now', 'overfull_wrapped_ahead', 'overfull_wrapped_one_back',
               'empty_far_ahead'):
    assert wc.CASES[wc.index(name)].count > wc.CAP, name
  # the exception and its complement differ by the anchor alone
  _, t, anchor, _ = inside('overfull_wrapped_one_back')
  assert anchor == t[-1] - 60
  assert helpers.GP_CAPACITY == 128 and helpers.GP_ROWS == 120 and helpers.GP_HORIZON_S == 21600


def test_a_window_shifted_by_one_entry_moves_the_mean_and_k_is_well_conditioned():
  smallest, worst_cond = (np.inf, None), 0.0
  print()
  for i, case in enumerate(wc.CASES):
    if case.n_obs <= 0:
      continue
    obs, anchor = wc.build(i)
    ring = wc.held(obs)
    keep = wc.kept(ring[1], anchor)
    twin = wc.Twin(ring, keep)
    pts, boundary = wc.points(i, ring, keep)
    assert pts.shape == (wc.Q, 3) and pts.dtype == np.float32 and 2 <= len(boundary) <= 4
    mean = twin.mean(pts[boundary], anchor)
    moved = {}
    for what, other in wc.shifted_windows(keep, len(ring[1])).items():
      moved[what] = float(np.abs(wc.Twin(ring, other).mean(pts[boundary], anchor) - mean).max())
      assert moved[what] > SHIFT_BAR, (case.name, what, moved[what])
    cond = float(np.linalg.cond(twin.k))
    worst_cond = max(worst_cond, cond)
    assert cond <= COND_BAR, (case.name, cond)
    low = min(moved, key=moved.get)
    if moved[low] < smallest[0]:
      smallest = (moved[low], f'{case.name}, {low}')
    print(f'{case.name:30s} n_obs {twin.n_obs:3d}  cond(K + 0.05 I) {cond:7.1f}  a shift by one entry moves the mean by '
          f'{moved[low]:.3f} .. {max(moved.values()):.3f} m/s')
  print(f'smallest move {smallest[0]:.3f} m/s ({smallest[1]}); largest cond {worst_cond:.1f}')
  i = wc.index('interior')                                 # where both ends are cut, both left-out neighbours are among the points
  obs, anchor = wc.build(i)
  assert len(wc.points(i, wc.held(obs), wc.kept(wc.held(obs)[1], anchor))[1]) == 4
