"""The stride's merged fp64 seed, the fp32 root argument and the ACS node table against the expressions they replaced, on the host build of
the lane functions (tests/stride_seeds_host.cpp, built like tests/emul: the fp64 seeds are float32-precise and refined by the same Newton
steps as on the device).

  * sqrt(arg) / dH through ONE reciprocal square root (atm_rate_over_delta_height_f64) against sqrt(arg) and 1 / dH through a seed each;
  * the thermal increment with the twelfth root's argument formed in fp32 against the same increment with the argument in fp64;
  * the ACS table's node positions against fma(0.025, i, 0.05), and acs_down_poly against the form that took interval and node from the index.

The reference of the first two is the same expression in numpy.longdouble (64-bit mantissa) on the same double inputs.

THE GATE, input by input:  error_new(x) <= 2 max(error_old(x), floor(x)).  The factor 2 covers one more rounding in a product chain.  The
floor is there because on a single input the old form's error can be anything down to zero (sqrt(1e-30) is ONE number with ONE seed, which
happens to be a good one), and twice nothing is no bound; it is the error a single refined seed may have, from the formats alone:
  rate      1.5 e^2 + 4 u = 3.4e-14 relative: one Newton step of y <- y (1.5 - 0.5 x y^2) leaves 1.5 e^2 of a seed good to e; e = 2.5 x 2^-24 for
            the host's seed (float32 rounding of the argument, sqrtf, the division: half an ulp each, the argument's halved by the root), which
            the device's v_rsq_f64 / v_rcp_f64 (2^29 ulp = 2^-23) match; u = 2^-53 for the four multiplications around it.  The OLD form holds
            two such seeds (d_sqrt_rs and d_rcp), so the floor is below what the old form itself may err by.
  thermal   the fp32 root's own error carried into the increment: 4 x 2^-24 (log2, the product with 1/12, exp2, the rounding of the result) of
            the root, times d increment / d root from the reference, plus 8 u of the four heat flows.  Both forms take the root in fp32.
On top of it, per item: the largest new error over ALL its inputs may not exceed twice the largest old error over all of them.
Measured maxima (relative to the reference; printed by every run, group by group):
  rate     old 1.59e-14  new 1.65e-14, at most 0.49 of the floor  (flight grid 1.59e-14 / 1.60e-14; arg == 0 and the 1e-30 floor 7.3e-15 / 1.65e-14; domain maximum
           7.0e-15 / 1.24e-14; slack envelope 1.25e-14 / 7.5e-15; within 1 Pa of a transition 7.3e-15 / 1.24e-14)
  thermal  old 2.57e-9 K  new 2.57e-9 K per stride (absolute; largest error / floor: old 0.64, new 0.64)
The rare paths (isothermal layer, p and p + d on two sides of a transition) keep their own reciprocal and take sqrt(arg) there: the same bits
as before, asserted."""
import ctypes
import fractions
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
_SO = os.path.join(_HERE, 'libstride_seeds_host.so')
L = np.longdouble



@pytest.fixture(scope='module')
def lib():
  srcs = [os.path.join(_HERE, 'stride_seeds_host.cpp'), os.path.join(_HERE, 'emul', 'ble_intrinsics.h'),
          os.path.join(_CSRC, 'ble_physics.h'), os.path.join(_CSRC, 'ble_step_core.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', srcs[1], '-o', _SO, srcs[0]])
  assert np.finfo(np.longdouble).nmant >= 63, 'numpy.longdouble is no wider than double here: no reference'
  l = ctypes.CDLL(_SO)
  for name in ('seeds_thermal_scale', 'seeds_acs_node', 'seeds_acs_node_fma'):
    getattr(l, name).restype = ctypes.c_double
  return l


def _ptr(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _f64(*arrays):
  return [np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), np.broadcast(*arrays).shape).ravel()) for a in arrays]


# ---------------------------------------------------------------- sqrt(arg) / dH
def _rate(lib, alpha, p, arg, d):
  """(old, new, reference, rare) of sqrt(max(arg, 1e-30)) / (H(p + d) - H(p)) in the window the transition builds around p."""
  alpha, p, arg, d = _f64(alpha, p, arg, d)
  a = np.maximum(arg, 1e-30)                        # stride_pressure's floor
  out = np.empty((p.size, 16))
  lib.seeds_rate(ctypes.c_int64(p.size), _ptr(alpha), _ptr(p), _ptr(a), _ptr(d), _ptr(out))
  assert (out[:, 13] == 0).all(), 'a pressure outside the atmosphere'
  rp, t_p, l0, lm1, lp1, pb, pt, tb, tt, r_pb, r_pt = (out[:, k].astype(L) for k in range(2, 13))
  kl, c = out[:, 14].astype(L), out[:, 15].astype(L)
  pl, dl = p.astype(L), d.astype(L)
  third, sixth = L(1.0 / 3.0), L(1.0 / 6.0)
  x = dl * rp
  lg = x * (1 + x * (L(-0.5) + x * third))
  y = kl * lg
  em1 = y * (1 + y * (L(0.5) + y * sixth))
  iso = out[:, 4] == 0.0
  with np.errstate(divide='ignore', invalid='ignore'):
    dh = np.where(iso, c * t_p * lg, t_p * em1 / l0)
  q = pl + dl
  below, above = q > pb, ~(q > pt)
  bp, r_b, t_b = np.where(below, pb, pt), np.where(below, r_pb, r_pt), np.where(below, tb, tt)

  def height(qq, lapse):
    xx = (qq - bp) * r_b
    lgg = xx * (1 + xx * (L(-0.5) + xx * (third + xx * L(-0.25))))
    yy = c * lapse * lgg
    e = yy * (1 + yy * (L(0.5) + yy * (sixth + yy * L(1.0 / 24.0))))
    with np.errstate(divide='ignore', invalid='ignore'):
      return np.where(lapse == 0, c * t_b * lgg, t_b * e / lapse)
  rare = below | above
  dh = np.where(rare, height(q, np.where(below, lm1, lp1)) - height(pl, l0), dh)
  return out[:, 0], out[:, 1], np.sqrt(a.astype(L)) / dh, rare | iso


E_SEED = 2.5 * 2.0 ** -24                 # a float32-precise seed of 1 / sqrt(x): see the module docstring
RATE_FLOOR = 1.5 * E_SEED ** 2 + 4 * 2.0 ** -53
E_POW_F32 = 4 * 2.0 ** -24


class Pool:
  """The cases of one item, group by group; errors and floors in the same unit (relative to the reference unless the caller says otherwise).
  add(): the gate input by input.  check(): the item's largest new error against twice its largest old error."""

  def __init__(self, name):
    self.name, self.groups = name, []

  def add(self, group, old, new, ref, floor, scale=None):
    scale = np.abs(ref) if scale is None else scale
    assert np.isfinite(new).all() and np.isfinite(old).all(), group
    e_old = (np.abs(old.astype(L) - ref) / scale).astype(np.float64); e_new = (np.abs(new.astype(L) - ref) / scale).astype(np.float64)
    floor = np.broadcast_to(np.asarray(floor, np.float64), e_old.shape)
    over = e_new / (2.0 * np.maximum(e_old, floor))
    self.groups.append((group, old.size, float(e_old.max()), float(e_new.max()), float(over.max()), float((e_new / floor).max()), float((e_old / floor).max())))
    worst = int(over.argmax())
    assert over.max() <= 1.0, (f'{self.name}, {group}: input {worst}: new {e_new[worst]:.3g} against old {e_old[worst]:.3g}, floor {floor[worst]:.3g}')

  def check(self):
    for group, size, e_old, e_new, over, nf, of in self.groups:
      print(f'{self.name}, {group}: {size} inputs, largest error old {e_old:.3g} new {e_new:.3g}; error / floor old {of:.2f} new {nf:.2f}; '
            f'largest new / (2 max(old, floor)) {over:.2f}')
    bound, worst_new = max(g[2] for g in self.groups), max(g[3] for g in self.groups)
    print(f'{self.name}: largest error old {bound:.3g} new {worst_new:.3g}')
    assert worst_new <= 2.0 * bound, f'{self.name}: new {worst_new:.3g} against old {bound:.3g}'
    return bound, worst_new


ALPHAS = (0.0, 0.37, 1.0)
P_GRID = np.geomspace(3000.0, 102000.0, 67)
EDGE_OFFSETS = np.array([-0.999, -0.5, -0.25, -1e-3, 1e-3, 0.25, 0.5, 0.999])      # Pa from a transition pressure


def _domain_arg_max(lib):
  """The largest arg among the corners of the state domain of helpers.wide_domain_states (1.2 .. 40 kPa, T_int 180 .. 300 K, T_amb 180 .. 280 K,
  superpressure 20 .. 2 300 Pa fixing volume and air) and of the flight grid's pressure and temperature range."""
  p, t_int, t_amb, sp = (g.ravel() for g in np.meshgrid([1200.0, 3000.0, 40000.0, 102000.0], [180.0, 300.0], [180.0, 280.0, 320.0], [20.0, 2300.0]))
  vol = 1804.0 + 0.0199 * sp
  n_air = np.maximum((p + sp) * vol / (8.3144621 * t_int) - 6830.0, 0.0)
  arg, d = np.empty(p.size), np.empty(p.size)
  lib.seeds_arg(ctypes.c_int64(p.size), *(_ptr(np.ascontiguousarray(v)) for v in (p, vol, n_air, t_amb)), _ptr(arg), _ptr(d))
  return float(arg.max())


def _transition_pressures(lib, alpha):
  pb, pt = ctypes.c_double(), ctypes.c_double()
  lib.seeds_window(ctypes.c_double(alpha), ctypes.c_double(8000.0), ctypes.byref(pb), ctypes.byref(pt))
  assert 8000.0 < pb.value < 12000.0 and 3000.0 < pt.value < 6000.0
  return np.concatenate([pb.value + EDGE_OFFSETS, pt.value + EDGE_OFFSETS])


def test_rate_through_one_seed(lib):
  """The flight grid (3 .. 102 kPa, three atmospheres, arg over 14 decades, both directions) and the edges: arg == 0 and arg at the 1e-30
  floor, arg at the domain's maximum, a slack envelope's arg as stride_pressure forms it, p within 1 Pa of both transition pressures of a
  window on either side (the lanes that stay on the common path there)."""
  pool = Pool('rate')
  a_max = _domain_arg_max(lib)
  print(f'largest arg of the state domain: {a_max:.4g} m^2/s^2')
  assert 1.0 < a_max < 6700.0                      # the range the lane function's comment works out
  args = np.array([1e-12, 1e-6, 1e-3, 0.04, 1.0, 9.0, 100.0])
  for d in (1.0, -1.0):
    al, p, a = np.meshgrid(ALPHAS, P_GRID, args, indexing='ij')
    old, new, ref, rare = _rate(lib, al, p, a, d)
    assert not rare.any()
    pool.add(f'flight grid, d = {d:+.0f}', old, new, ref, RATE_FLOOR)
    al, p = np.meshgrid(ALPHAS, P_GRID, indexing='ij')
    for name, a in (('arg == 0', 0.0), ('floor 1e-30', 1e-30), ('domain maximum', a_max)):
      old, new, ref, rare = _rate(lib, al, p, a, d)
      assert not rare.any()
      pool.add(f'{name}, d = {d:+.0f}', old, new, ref, RATE_FLOOR)
  # a slack envelope (volume below 1 804 m^3, no superpressure), low in the troposphere
  p = np.array([60000.0, 85000.0, 101000.0]); t_int = np.array([250.0, 270.0, 285.0]); t_amb = np.array([255.0, 272.0, 288.0])
  vol = 6830.0 * 8.3144621 * t_int / p
  assert (vol < 1804.0).all()
  arg, d = np.empty(3), np.empty(3)
  lib.seeds_arg(ctypes.c_int64(3), *(_ptr(v) for v in (p, vol, np.zeros(3), t_amb)), _ptr(arg), _ptr(d))
  al, pp = np.meshgrid(ALPHAS, p, indexing='ij')
  old, new, ref, rare = _rate(lib, al.ravel(), pp.ravel(), np.tile(arg, 3), np.tile(d, 3))
  assert not rare.any()
  pool.add('slack envelope', old, new, ref, RATE_FLOOR)
  for alpha in ALPHAS:
    p = _transition_pressures(lib, alpha)
    for d in (1.0, -1.0):
      pa, aa = np.meshgrid(p, [0.0, 0.04, 9.0], indexing='ij')
      old, new, ref, rare = _rate(lib, alpha, pa, aa, d)
      assert (~rare).sum() >= 8 * 3
      pool.add(f'within 1 Pa of a transition, alpha = {alpha}, d = {d:+.0f}', old[~rare], new[~rare], ref[~rare], RATE_FLOOR)
  pool.check()
  # the merged seed's argument a wd^2 at the floor stays a normal number, in float32 too (the host seed goes through it): wd = sqrt(a) L / rate
  al, p = np.meshgrid(ALPHAS, P_GRID, indexing='ij')
  _, new, _, _ = _rate(lib, al, p, 1e-30, 1.0)
  lapse = np.where(p.ravel() > 22000.0, 0.0058, 0.001)      # (a lower bound of |L| per layer bounds the argument from below)
  assert (1e-30 * (np.sqrt(1e-30) * lapse / np.abs(new)) ** 2 > 1.2e-38).all()


def test_rate_on_the_rare_paths_keeps_its_bits(lib):
  """Where p + d lies across a transition, and in the isothermal layer (lapse == 0: 47-51 km), the rare path forms its own reciprocal and
  multiplies by sqrt(arg), taken there: the bits of the two-seed form."""
  rare_seen = 0
  for alpha in ALPHAS:
    p = _transition_pressures(lib, alpha)
    for d in (1.0, -1.0):
      for a in (0.0, 0.04, 9.0):
        old, new, ref, rare = _rate(lib, alpha, p, a, d)
        rare_seen += int(rare.sum())
        np.testing.assert_array_equal(old[rare], new[rare])
        assert (np.abs(new[rare].astype(L) - ref[rare]) <= 1e-9 * np.abs(ref[rare])).all()      # (dH is a difference of two heights there)
  assert rare_seen >= 3 * 2 * 3 * 6                  # |offset| < 1 Pa: p + d is across for one of the two directions
  p_iso = np.array([60.0, 75.0, 88.0])                # (the layer spans 54.2 .. 91.3 Pa)
  for d in (1.0, -1.0):
    old, new, ref, rare = _rate(lib, 0.5, p_iso, 0.04, d)
    assert rare.all()
    np.testing.assert_array_equal(old, new)
    assert (np.abs(new.astype(L) - ref) <= 1e-12 * np.abs(ref)).all()


# ---------------------------------------------------------------- the thermal increment
def _thermal_reference(lib, vol, yc, t_int, t_amb, p, q_solar, q_earth):
  vol, yc, t_int, t_amb, p, q_solar, q_earth = (v.astype(L) for v in (vol, yc, t_int, t_amb, p, q_solar, q_earth))
  mu = L(1.458e-6) / (L(0.028964922481160) / L(8.3144621))
  scale = L(9.80665) / mu / mu * (6 / L(np.pi))
  rho = 1 / (1 - L(0.0291)); c1 = L(0.000232); c0 = L(0.04587) - c1 * 210; sigma = L(0.000000056704)
  ea, eb, ec = sigma * (-rho * c1 * c1), sigma * (2 * c1 - 2 * rho * c1 * c0), sigma * (2 * c0 - rho * c0 * c0)
  cond10 = (L(0.0241) * L(0.006415624181362592)) / (2 * L(0.62035049089940009))
  q_emit = t_int ** 4 * ((ea * t_int + eb) * t_int + ec)
  pw = p * (t_amb + L(110.4)); dt = t_amb - t_int
  ra = np.maximum(((L(-3.25e-4) * t_amb + L(0.804)) * scale) * pw * pw * vol * np.abs(dt) / t_amb ** 6, L(1e-30))
  nusselt = L(0.457) * ra ** L(0.25) + 2 + (1 + L(2.69e-8) * ra) ** (1 / L(12))
  tw = (1 + L(2.69e-8) * ra) ** (1 / L(12))
  per_nusselt = t_amb ** L(0.9) * cond10 * yc * dt                 # d q_conv / d Nusselt = d q_conv / d root
  q_conv = nusselt * per_nusselt
  to_kelvin = (vol * yc) * L(lib.seeds_thermal_scale())
  floor = (E_POW_F32 * tw * np.abs(per_nusselt) + 8 * 2.0 ** -53 * (np.abs(q_solar + q_earth) + np.abs(q_conv) + np.abs(q_emit))) * to_kelvin
  return (q_solar + q_earth + (q_conv - q_emit)) * to_kelvin, floor.astype(np.float64)


def test_thermal_increment_with_the_root_argument_in_float32(lib):
  p, t_amb, dt, vol, q_solar = _f64(*np.meshgrid(np.geomspace(3000.0, 102000.0, 23), np.linspace(180.0, 320.0, 15),
                                                 [-60.0, -15.0, -1.0, -1e-3, 0.0, 1e-6, 0.5, 12.0, 45.0],
                                                 [1650.0, 1804.0, 1804.0 + 0.0199 * 1200.0, 1804.0 + 0.0199 * 2380.0], [0.0, 4.5]))
  t_int = t_amb + dt
  q_earth = np.full(p.size, 3.1)
  out = np.empty((p.size, 3))
  lib.seeds_thermal(ctypes.c_int64(p.size), *(_ptr(np.ascontiguousarray(v)) for v in (vol, t_int, t_amb, p, q_solar, q_earth)), _ptr(out))
  ref, floor = _thermal_reference(lib, vol, out[:, 2], t_int, t_amb, p, q_solar, q_earth)
  # (errors and floor in kelvin per stride: the gate's inequality is the same in any unit, and the increment itself passes through zero)
  pool = Pool('thermal increment [K per stride]')
  pool.add('flight grid, slack and taut envelopes', out[:, 0], out[:, 1], ref, floor, scale=L(1.0))
  e_old, e_new = pool.check()
  assert e_old < 1e-8                                # (the reference is the same function: what is left is the fp32 root's 1e-7 of a term of ~2 next to ~300)
  assert (out[:, 0] != out[:, 1]).any()


# ---------------------------------------------------------------- the ACS table
def test_acs_node_positions_are_the_fused_ones(lib):
  for i in range(12):
    node = lib.seeds_acs_node(ctypes.c_int(i))
    exact = fractions.Fraction(0.025) * i + fractions.Fraction(0.05)       # the fma's value before its one rounding
    assert node == float(exact), i                                           # (float(Fraction) rounds correctly)
    assert node == lib.seeds_acs_node_fma(ctypes.c_int(i)), i
  assert any(lib.seeds_acs_node(ctypes.c_int(i)) != 0.05 + 0.025 * i for i in range(12))      # (why they are spelled out)


def test_acs_down_poly_keeps_its_bits(lib):
  """Against the form that took interval and node from (prm1 - 0.05) x 40 and fma(0.025, i, 0.05): the same bits wherever both pick the same
  interval.  The interval now comes from fma(prm1, 40, -2); within an ulp of a node the two may pick neighbouring intervals, whose cubics
  meet there: power and mass flow agree to the table's own rounding (a few ulp)."""
  nodes = 0.05 + 0.025 * np.arange(14)
  near = np.concatenate([nodes, np.nextafter(nodes, 0.0), np.nextafter(nodes, 1.0), np.nextafter(np.nextafter(nodes, 0.0), 0.0),
                         np.nextafter(np.nextafter(nodes, 1.0), 1.0)])
  prm1 = np.concatenate([np.linspace(-0.1, 0.5, 24001), near, [0.0, 1e-300, 5.0]])
  out = np.empty((prm1.size, 4))
  lib.seeds_acs(ctypes.c_int64(prm1.size), _ptr(prm1), _ptr(out))
  at_node = np.abs(prm1[:, None] - nodes[None, :]).min(1) <= 4 * np.spacing(prm1)
  differ = (out[:, 0] != out[:, 2]) | (out[:, 1] != out[:, 3])
  print(f'acs_down_poly: {int(differ.sum())} of {prm1.size} arguments differ, all of them within 4 ulp of a node: {bool(at_node[differ].all())}; '
        f'largest relative difference power {np.max(np.abs(out[:, 0] - out[:, 2]) / out[:, 2]):.3g}, '
        f'mass flow {np.max(np.abs(out[:, 1] - out[:, 3]) / np.maximum(np.abs(out[:, 3]), 1e-3)):.3g}')
  np.testing.assert_array_equal(out[~at_node, 0].view(np.uint64), out[~at_node, 2].view(np.uint64))
  np.testing.assert_array_equal(out[~at_node, 1].view(np.uint64), out[~at_node, 3].view(np.uint64))
  assert (np.abs(out[:, 0] - out[:, 2]) <= 8 * np.spacing(out[:, 2])).all()
  assert (np.abs(out[:, 1] - out[:, 3]) <= 8 * np.spacing(np.maximum(np.abs(out[:, 3]), 1e-3))).all()
