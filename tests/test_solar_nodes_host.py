"""The step's solar nodes without their reciprocal roots, on the host build of the lane functions (tests/solar_nodes_host.cpp, built like
tests/stride_seeds_host.cpp: the fp64 seeds are float32-precise and refined by the same Newton steps as on the device).

  * sun_one_minus_sin_f64 in the form that needs no reciprocal root (see the comment above it in csrc/ble_physics.h) against its former body
    (`..._seeded` in the .cpp: three reciprocal square roots and the selects of d == 0);
  * solar_nodes_time's cos(decl) and its rate through ONE reciprocal square root against d_sqrt_fast and a division.

The reference of both is the reference's formula chain (spherical_geometry.py:44-76 folded into solar.py:136-139) in numpy.longdouble
(64-bit mantissa) on the same double inputs -- the site's latitude among them, as the chain starts from it: the lane functions take its
sincos_f64 pair --, with true roots, divisions, sines and cosines.

THE GATES (the inputs: 200 000 seeded draws, |lat0| <= 85 deg, |x|, |y| <= 600 km, 1 000 of them at the origin and 1 000 within a metre of it,
b in [0, 360 deg), |decl| <= 23.5 deg):
  * 1 - sin(el): the new form's largest absolute error is at most the former body's on the same draws, and at most 2e-15;
  * (float) of the two forms -- what becomes c0 -- differs in at most 1 draw of 10 000;
  * the second difference f2 - 2 f1 + f0 along a 180 s track (|u|, |v| <= 60 m/s) -- what becomes c2 -- is within 5e-15 of the
    reference's and no worse than the former body's;
  * at x = y = 0 both forms, the former one with the device's contractions, are compared bit by bit and the difference is stated in ulps;
  * no NaN anywhere;
  * cd0 keeps the bits of d_sqrt_fast(1 - sd0^2); hcd is within 4 ulp of -(sd0 / cd0) hsd.

Measured here (printed by every run; the former body's figures are its seeds': 1.5 e^2 of a float32-precise seed, like the device's):
  1 - sin(el)      former 1.5e-14, new 3.8e-16; (float) differs in 0 of 200 000
  f2 - 2 f1 + f0   former 5.0e-14, new 9.1e-16 (median magnitude 1.7e-5)
  origin           new and former (contracted) differ in 747 of 1 000 draws by at most 1.3e-14 absolute -- the former body's error there
                   (new 2.5e-16 from the reference); 45 056 ulp of a result that is 1e-10 near the zenith
  hcd              at most 2.4 ulp.  The reciprocal root alone, as d_sqrt_fast forms it, leaves 133 ulp (its Newton step's 2e-14): solar_nodes_time
                   corrects it with the root's own residual, one fp64 instruction more than a second seed's refinement, no seed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_ROOT, 'balloon_learning_environment_amd', 'csrc')
_SO = os.path.join(_HERE, 'libsolar_nodes_host.so')
L = np.longdouble
R_EARTH = 6371000.0
N_DRAWS, N_ORIGIN, N_NEAR = 200_000, 1_000, 1_000


@pytest.fixture(scope='module')
def lib():
  srcs = [os.path.join(_HERE, 'solar_nodes_host.cpp'), os.path.join(_HERE, 'emul', 'ble_intrinsics.h'),
          os.path.join(_CSRC, 'ble_physics.h'), os.path.join(_CSRC, 'ble_step_core.h')]
  if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-include', srcs[1], '-o', _SO, srcs[0]])
  assert np.finfo(np.longdouble).nmant >= 63, 'numpy.longdouble is no wider than double here: no reference'
  return ctypes.CDLL(_SO)


def _ptr(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def _forms(lib, sl0, cl0, x, y, sb, cb, sd, cd):
  """(new, former, former with the device's contractions) of 1 - sin(el)"""
  a = np.ascontiguousarray(np.stack([sl0, cl0, x, y, sb, cb, sd, cd], axis=1))
  out = np.empty((a.shape[0], 3))
  lib.solar_oms(ctypes.c_int64(a.shape[0]), _ptr(a), _ptr(out))
  return out[:, 0], out[:, 1], out[:, 2]


def _reference(lat0_rad, x, y, sb, cb, sd, cd):
  """The reference's chain in longdouble from the site's latitude (the double the lane functions take the sine and cosine of): heading and
  angle, the new latitude, d_lng, the hour angle's cosine, 1 - sin(el)."""
  lat0_rad, x, y, sb, cb, sd, cd = (v.astype(L) for v in (lat0_rad, x, y, sb, cb, sd, cd))
  sl0, cl0 = np.sin(lat0_rad), np.cos(lat0_rad)
  d = np.sqrt(x * x + y * y)
  moved = d > 0
  safe = np.where(moved, d, L(1))
  cos_h, sin_h = np.where(moved, y / safe, L(1)), np.where(moved, x / safe, L(0))      # atan2(0, 0) = 0
  a = d / L(R_EARTH)
  sin_a, cos_a = np.sin(a), np.cos(a)
  sin_lat = cos_a * sl0 + sin_a * cl0 * cos_h
  cos_lat = np.sqrt(1 - sin_lat * sin_lat)
  yy, xx = sin_a * cl0 * sin_h, cos_a - sl0 * sin_lat
  cos_bl = (cb * xx - sb * yy) / np.sqrt(xx * xx + yy * yy)
  return 1 - (sin_lat * sd - cos_lat * cd * cos_bl)


@pytest.fixture(scope='module')
def draws(lib):
  rng = np.random.default_rng(20240611)
  n = N_DRAWS
  lat0 = rng.uniform(-85.0, 85.0, n)
  x, y = rng.uniform(-6e5, 6e5, n), rng.uniform(-6e5, 6e5, n)
  x[:N_ORIGIN] = 0.0; y[:N_ORIGIN] = 0.0
  r, phi = rng.uniform(0.0, 1.0, N_NEAR), rng.uniform(0.0, 2 * np.pi, N_NEAR)
  x[N_ORIGIN:N_ORIGIN + N_NEAR] = r * np.cos(phi); y[N_ORIGIN:N_ORIGIN + N_NEAR] = r * np.sin(phi)
  # the position is a float32 in the state
  x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
  lat0 = np.ascontiguousarray(np.float32(lat0).astype(np.float64) * (np.pi / 180.0))      # hoist_constants: (double)lat0_deg * (pi / 180)
  sl0, cl0 = np.empty(n), np.empty(n)
  lib.solar_sincos(ctypes.c_int64(n), _ptr(lat0), _ptr(sl0), _ptr(cl0))
  b = rng.uniform(0.0, 2 * np.pi, n)
  decl = rng.uniform(-23.5, 23.5, n) * (np.pi / 180.0)
  sd = np.sin(decl).astype(np.float32).astype(np.float64)        # the ephemeris's float32 sine; the cosine normalises it in fp64 (solar_nodes_time)
  cd = np.sqrt(1.0 - sd * sd)
  return dict(lat0=lat0, sl0=sl0, cl0=cl0, x=x, y=y, b=b, sd=sd, cd=cd, rng=rng)


def test_one_minus_sin_without_the_seeds(lib, draws):
  d = draws
  args = (d['sl0'], d['cl0'], d['x'], d['y'], np.sin(d['b']), np.cos(d['b']), d['sd'], d['cd'])
  new, old, _ = _forms(lib, *args)
  ref = _reference(d['lat0'], *args[2:])
  assert np.isfinite(new).all() and np.isfinite(old).all()
  e_new, e_old = float(np.abs(new.astype(L) - ref).max()), float(np.abs(old.astype(L) - ref).max())
  differ = int((new.astype(np.float32) != old.astype(np.float32)).sum())
  print(f'1 - sin(el), {new.size} draws: largest absolute error former {e_old:.3g}, new {e_new:.3g}; (float) differs in {differ}')
  assert e_new <= e_old
  assert e_new <= 2e-15
  assert differ * 10_000 <= new.size


def test_second_difference_along_a_track(lib, draws):
  """Three nodes of a 180 s step the way solar_node places them: the position moves with a constant wind, the hour-angle base turns by the half
  step's 0.375 deg, the declination pair moves linearly."""
  d, rng = draws, np.random.default_rng(77)
  n = d['x'].size
  u, v = (rng.uniform(-60.0, 60.0, n).astype(np.float32).astype(np.float64) for _ in range(2))
  hsd = rng.uniform(-8e-8, 8e-8, n) * 90.0                         # |d sin(decl) / dt| <= 0.4 x 2 pi / year
  hcd = -(d['sd'] / d['cd']) * hsd
  half_b = 0.375 * (np.pi / 180.0)
  f_new, f_old, f_ref = [], [], []
  for j in range(3):
    bj = d['b'] + j * half_b
    args = (d['sl0'], d['cl0'], d['x'] + j * (90.0 * u), d['y'] + j * (90.0 * v), np.sin(bj), np.cos(bj), d['sd'] + j * hsd, d['cd'] + j * hcd)
    new, old, _ = _forms(lib, *args)
    assert np.isfinite(new).all() and np.isfinite(old).all()
    f_new.append(new.astype(L)); f_old.append(old.astype(L)); f_ref.append(_reference(d['lat0'], *args[2:]))
  dd = lambda f: f[2] - 2 * f[1] + f[0]
  e_new, e_old = float(np.abs(dd(f_new) - dd(f_ref)).max()), float(np.abs(dd(f_old) - dd(f_ref)).max())
  print(f'f2 - 2 f1 + f0, {n} tracks: median magnitude {float(np.median(np.abs(dd(f_ref)))):.3g}; largest absolute error former {e_old:.3g}, new {e_new:.3g}')
  assert e_new <= 5e-15
  assert e_new <= e_old


def test_origin(lib, draws):
  """At x = y = 0 the new form is sin_lat = sin_lat0, xx = cos_lat0 exactly; the former body goes through sqrt(1 - sin_lat0^2) and
  xx / sqrt(xx^2): the two are not the same bits.  The difference is stated (in ulps of the result) and both are held to the reference."""
  d = draws
  k = slice(0, N_ORIGIN)
  assert (d['x'][k] == 0).all() and (d['y'][k] == 0).all()
  args = tuple(a[k] for a in (d['sl0'], d['cl0'], d['x'], d['y'], np.sin(d['b']), np.cos(d['b']), d['sd'], d['cd']))
  new, _, old_fma = _forms(lib, *args)
  ref = _reference(d['lat0'][k], *args[2:])
  assert np.isfinite(new).all() and np.isfinite(old_fma).all()
  ulps = np.abs(new - old_fma) / np.spacing(np.maximum(np.abs(new), np.abs(old_fma)))
  print(f'origin, {new.size} draws: new and former (contracted) differ in {int((new != old_fma).sum())}, by at most {ulps.max():.0f} ulp of the result, '
        f'{np.abs(new - old_fma).max():.3g} absolute; error new {float(np.abs(new.astype(L) - ref).max()):.3g}, former {float(np.abs(old_fma.astype(L) - ref).max()):.3g}')
  assert float(np.abs(new.astype(L) - ref).max()) <= 2e-15
  # within a metre of the origin: finite and as close
  k = slice(N_ORIGIN, N_ORIGIN + N_NEAR)
  args = tuple(a[k] for a in (d['sl0'], d['cl0'], d['x'], d['y'], np.sin(d['b']), np.cos(d['b']), d['sd'], d['cd']))
  assert (np.hypot(args[2], args[3]) <= 1.0 + 1e-6).all()
  new, old, _ = _forms(lib, *args)
  assert np.isfinite(new).all() and np.isfinite(old).all()
  assert float(np.abs(new.astype(L) - _reference(d['lat0'][k], *args[2:])).max()) <= 2e-15


def test_declination_pair_through_one_seed(lib):
  rng = np.random.default_rng(5)
  n = 20_000
  decl = np.concatenate([rng.uniform(-23.5, 23.5, n - 3), [-23.5, 0.0, 23.5]]) * (np.pi / 180.0)
  sd = np.sin(decl).astype(np.float32)
  rate = rng.uniform(-8e-8, 8e-8, n).astype(np.float32)
  for step_s in (10.0, 180.0, 330.0):
    out = np.empty((n, 4))
    lib.solar_time_nodes(ctypes.c_int64(n), _ptr(sd), _ptr(rate), ctypes.c_float(step_s), _ptr(out))
    cd0, hcd, hsd, cd_ref = out.T
    np.testing.assert_array_equal(cd0.view(np.uint64), cd_ref.view(np.uint64))
    np.testing.assert_array_equal(hsd, 0.5 * (rate * np.float32(step_s)).astype(np.float64))
    sdl = sd.astype(L)
    want = -(sdl / np.sqrt(1 - sdl * sdl)) * hsd.astype(L)
    ulps = np.abs(hcd.astype(L) - want) / np.spacing(np.abs(hcd)).astype(L)
    ulps = np.where(hcd == 0, np.where(want == 0, 0, np.inf), ulps)
    print(f'hcd, step {step_s:.0f} s, {n} draws: at most {float(ulps.max()):.2f} ulp from -(sd0 / cd0) hsd')
    assert ulps.max() <= 4
