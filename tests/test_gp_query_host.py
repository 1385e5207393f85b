"""ble_gp_query_f32 on a machine without a GPU: the entry is declared, exported and mirrored, and every invalid argument answers
BLE_E_INVALID_ARG before any HIP call (no call below has valid arguments and n > 0: that would launch)."""
import ctypes
import os
import re
import subprocess

import pytest

from balloon_learning_environment_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID_ARG = -1
_FAKE = 0x1000          # a non-NULL address that is never dereferenced (the checks come before any HIP call)
_RING = ('xyp', 'elapsed_s', 'err_uv', 'count')


def _hist(null=None):
  h = _abi.BleGpHistoryF32()
  for name, ct in (('xyp', ctypes.c_float), ('elapsed_s', ctypes.c_int32), ('err_uv', ctypes.c_float), ('count', ctypes.c_int32)):
    setattr(h, name, ctypes.cast(ctypes.c_void_p(None if name == null else _FAKE), ctypes.POINTER(ct)))
  return h


def _query(**over):
  f = dict(n=0, q=16, add_forecast=0, xyp=_FAKE, time_s=_FAKE, wind_grid=None, grid_env_stride=0, mean_uv=_FAKE, deviation=_FAKE)
  f.update(over)
  return _abi.BleGpQueryF32(**f)


def _call(hist, query, reset_mask=None):
  return _lib.lib().ble_gp_query_f32(None if hist is None else ctypes.byref(hist), reset_mask, None if query is None else ctypes.byref(query),
                                     None, None)


def test_declared_exported_and_mirrored():
  header = open(os.path.join(ROOT, 'include', 'ble_abi.h')).read()
  assert re.search(r'\bint ble_gp_query_f32\(const ble_gp_history_f32\* hist, const uint8_t\* reset_mask,', header)
  assert 'struct ble_gp_query_f32 {' in header
  assert re.search(r'#define BLE_ABI_VERSION 5\b', header)            # additive: the ABI stays 5
  assert 'ble_gp_query_f32' in _lib.EXPORTS and 'ble_gp_query_f32' in _lib.ADDITIVE_EXPORTS and _lib.ABI_VERSION == 5
  assert any(s.endswith('ble_gp_query.h') for s in _lib._SOURCES)
  symbols = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
  assert re.search(r' T ble_gp_query_f32$', symbols, re.M)
  assert _lib.lib().ble_gp_query_f32.argtypes is not None and len(_lib.lib().ble_gp_query_f32.argtypes) == 5


def test_struct_layout_matches_the_header():
  # int64, 2 x int32, 3 pointers, int64, 2 pointers: no padding anywhere
  assert ctypes.sizeof(_abi.BleGpQueryF32) == 8 + 4 + 4 + 3 * 8 + 8 + 2 * 8
  assert [f[0] for f in _abi.BleGpQueryF32._fields_] == ['n', 'q', 'add_forecast', 'xyp', 'time_s', 'wind_grid', 'grid_env_stride',
                                                         'mean_uv', 'deviation']
  assert _abi.BleGpQueryF32.q.offset == 8 and _abi.BleGpQueryF32.xyp.offset == 16 and _abi.BleGpQueryF32.mean_uv.offset == 48


def test_empty_batch_is_ok_without_a_launch():
  assert _call(_hist(), _query()) == _lib.BLE_OK
  assert _call(_hist(), _query(add_forecast=1, wind_grid=_FAKE)) == _lib.BLE_OK
  assert _call(_hist(), _query(), reset_mask=_FAKE) == _lib.BLE_OK


_CASES = {
    'null_hist': lambda n: (None, _query(n=n)),
    'null_query': lambda n: (_hist(), None),
    **{f'null_ring_{f}': (lambda n, f=f: (_hist(null=f), _query(n=n))) for f in _RING},
    **{f'null_{f}': (lambda n, f=f: (_hist(), _query(n=n, **{f: None}))) for f in ('xyp', 'time_s', 'mean_uv', 'deviation')},
    'negative_n': lambda n: (_hist(), _query(n=-1)),
    'q_0': lambda n: (_hist(), _query(n=n, q=0)),
    'q_negative': lambda n: (_hist(), _query(n=n, q=-3)),
    'n_times_q_2_31': lambda n: (_hist(), _query(n=2 ** 20, q=2 ** 11)),
    'n_times_q_beyond_2_31': lambda n: (_hist(), _query(n=2 ** 31, q=1)),
    'n_times_q_wraps_int64': lambda n: (_hist(), _query(n=2 ** 62, q=4)),
    'forecast_without_grid': lambda n: (_hist(), _query(n=n, add_forecast=1, wind_grid=None)),
}


@pytest.mark.parametrize('n', [0, 64])
@pytest.mark.parametrize('case', sorted(_CASES))
def test_invalid_argument(case, n):
  hist, query = _CASES[case](n)
  assert _call(hist, query) == E_INVALID_ARG


def test_largest_legal_product_passes_the_checks():
  # n * q = 2^31 - 1 is legal; with n == 0 nothing is launched, so only the product's bound is in play here
  assert _call(_hist(), _query(n=0, q=2 ** 31 - 1)) == _lib.BLE_OK


def test_no_package_file_names_the_host_twin():
  pkg = os.path.join(ROOT, 'balloon_learning_environment_amd')
  for dirpath, _, files in os.walk(pkg):
    for f in files:
      if f.endswith('.py'):
        assert 'wind_gp' not in open(os.path.join(dirpath, f)).read(), f
  assert os.path.exists(os.path.join(pkg, 'env', 'windgp.py')) and not os.path.exists(os.path.join(pkg, 'env', 'wind_gp.py'))
