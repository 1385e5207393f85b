"""WindGP for ONE environment, backed by the device: the interface of the reference's WindGP module (reset / observe / query /
query_batch, time_horizon) over a one-environment observation ring in device memory and `ble_gp_query_f32`.

A Gaussian process over the errors between measured winds and a forecast: Matern nu = 0.5 kernel with fixed length scales, refit
on the observations of the last six hours at every query.  The algebra runs in the HIP library (fp64); this class keeps the ring,
turns locations into the kernel's inputs and adds the forecast in float64 exactly as the reference does, so it works with any
WindField, SimpleStaticWindField included.

What the device form cannot mirror: query points with DIFFERING times (the reference then uses every observation of the episode,
which a ring of 128 does not hold) -- query_batch raises ValueError -- and windows of more than 120 observations (agent steps
shorter than 180 s), for which it raises OverflowError.  Locations are stored in float32 and times as whole seconds, like the
batched simulator's own history.
"""
import ctypes
import datetime as dt
from typing import Tuple

import numpy as np
import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd import vec_state
from balloon_learning_environment_amd.env import wind_field
from balloon_learning_environment_amd.utils import units


def _whole_seconds(seconds: float, what: str) -> int:
  if seconds != int(seconds):
    raise ValueError(f'WindGP keeps times as whole seconds on the device: {what} {seconds!r} s is not integral')
  return int(seconds)


class WindGP(object):
  """Wrapper around a Gaussian process that handles wind estimates (one environment)."""

  def __init__(self, forecast: wind_field.WindField, device='cuda:0') -> None:
    self.time_horizon = 6 * 3600
    self.device = dev.require_gpu(device)
    self.lib = _lib.lib()
    cap = _lib.GP_CAPACITY
    with torch.cuda.device(self.device):
      self._ring = dict(xyp=torch.zeros(1, cap, 3, dtype=torch.float32, device=self.device),
                        elapsed_s=torch.zeros(1, cap, dtype=torch.int32, device=self.device),
                        err_uv=torch.zeros(1, cap, 2, dtype=torch.float32, device=self.device),
                        count=torch.zeros(1, dtype=torch.int32, device=self.device))
      self._err_flags = torch.zeros(1, dtype=torch.int32, device=self.device)
    self._hist = vec_state.gp_history_struct(self._ring)
    self.reset(forecast)

  def reset(self, forecast: wind_field.WindField) -> None:
    """Resets the the WindGP, forgetting every observation."""
    self.wind_forecast = forecast
    self._count = 0
    self._ring['count'].zero_()

  def observe(self, x: units.Distance, y: units.Distance, pressure: float, elapsed_time: dt.timedelta,
              measurement: wind_field.WindVector) -> None:
    """Adds the given measurement to the Gaussian Process: the error between it and the forecast at that location."""
    seconds = _whole_seconds(elapsed_time.total_seconds(), 'the observation time')
    forecast = self.wind_forecast.get_forecast(x, y, pressure, elapsed_time)
    error = ((measurement.u - forecast.u).meters_per_second, (measurement.v - forecast.v).meters_per_second)
    slot = self._count % _lib.GP_CAPACITY
    r = self._ring
    r['xyp'][0, slot] = torch.tensor([x.meters, y.meters, pressure], dtype=torch.float32)
    r['elapsed_s'][0, slot] = seconds
    r['err_uv'][0, slot] = torch.tensor(error, dtype=torch.float32)
    self._count += 1
    r['count'].fill_(self._count)

  def query(self, x: units.Distance, y: units.Distance, pressure: float,
            elapsed_time: dt.timedelta) -> Tuple[np.ndarray, np.ndarray]:
    """Returns (mean [2], deviation) of the wind at the given location."""
    means, deviations = self.query_batch(np.array([[x.meters, y.meters, pressure, elapsed_time.total_seconds()]]))
    return means[0], deviations[0]

  def query_batch(self, locations: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """locations [N, 4] float64 of (x m, y m, pressure Pa, seconds elapsed), all with ONE time (and, like the reference, one x and
    y) -> (means [N, 2] float64 m/s, deviations [N] float64 = variance / sigma^2)."""
    locations = np.asarray(locations, np.float64)
    assert locations.ndim == 2 and locations.shape[1] == 4 and locations.shape[0] >= 1, locations.shape
    if not np.all(locations[:, 3] == locations[0, 3]):
      raise ValueError('the device WindGP answers query points that share ONE time: with differing times the reference uses every '
                       'observation of the episode, which the ring of the last 128 does not hold')
    seconds = _whole_seconds(float(locations[0, 3]), 'the query time')
    n = locations.shape[0]
    with torch.cuda.device(self.device):
      xyp = torch.from_numpy(np.ascontiguousarray(locations[:, :3], np.float32)).to(self.device).reshape(1, n, 3).contiguous()
      time_s = torch.tensor([seconds], dtype=torch.int32, device=self.device)
      mean_uv = torch.empty(1, n, 2, dtype=torch.float32, device=self.device)
      deviation = torch.empty(1, n, dtype=torch.float32, device=self.device)
      query = _abi.BleGpQueryF32(1, n, 0, xyp.data_ptr(), time_s.data_ptr(), None, 0, mean_uv.data_ptr(), deviation.data_ptr())
      _lib.check(self.lib.ble_gp_query_f32(ctypes.byref(self._hist), None, ctypes.byref(query), self._err_flags.data_ptr(),
                                           dev.stream_ptr(self.device)), 'ble_gp_query_f32')
      flags = int(self._err_flags.item())
    if flags:
      self._err_flags.zero_()
      vec_state.raise_for_flags(flags)            # (OverflowError: the window does not fit the device's 120 / the ring's 128)
    means = mean_uv[0].cpu().numpy().astype(np.float64)
    deviations = deviation[0].cpu().numpy().astype(np.float64)
    # the forecast is added on the host, in float64, as the reference does (any WindField)
    assert (locations[1:, [0, 1, 3]] == locations[0, [0, 1, 3]]).all()
    forecasts = self.wind_forecast.get_forecast_column(units.Distance(m=locations[0, 0]), units.Distance(m=locations[0, 1]),
                                                       locations[:, 2], dt.timedelta(seconds=locations[0, 3]))
    for i, f in enumerate(forecasts):
      means[i][0] += f.u.meters_per_second
      means[i][1] += f.v.meters_per_second
    return means, deviations
