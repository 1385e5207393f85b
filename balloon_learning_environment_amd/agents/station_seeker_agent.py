"""StationSeekerAgent (agents/station_seeker_agent.py of the reference) on the device.

The score of every pressure level, the choice of the best one and the action are `ble_station_seeker_f32` (csrc/ble_agent.h): one
wave per environment, float64 on the float32 features.  `VecStationSeekerAgent` is the native object -- a batch of observations on
the device in, uint8 actions on the device out, no host synchronisation, capturable in a graph.  `StationSeekerAgent` is the
reference-shaped single-environment agent over it (one launch and one copy back per decision).
"""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev
from balloon_learning_environment_amd.agents import agent
from balloon_learning_environment_amd.env import features

NUM_LEVELS = _lib.SEEKER_LEVELS     # 2 x 181 - 1 relative pressure levels


class VecStationSeekerAgent:
  """StationSeeker for N environments at once: act(obs [N, 1099] float32 device) -> uint8 [N] device.

  err_flags: the device word BLE_FLAG_AGENT_NO_LEVEL is OR-ed into when an environment has no valid level or a non-finite feature
  (its action is then STAY); pass a VecSimulator's `err_flags` to have its check_errors() raise it.  Default: a word of its own,
  raised by check_errors() here."""

  def __init__(self, device='cuda:0', err_flags: Optional[torch.Tensor] = None):
    self.device = dev.require_gpu(device)
    self.lib = _lib.lib()
    with torch.cuda.device(self.device):
      self.err_flags = err_flags if err_flags is not None else torch.zeros(1, dtype=torch.int32, device=self.device)

  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, level: Optional[torch.Tensor] = None,
          scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """obs: [N, >= 1099] float32 on this agent's device (rows may be padded: stride(0) >= 1099, stride(1) == 1).
    out: optional uint8 [N] for the actions; level: optional int32 [N] for the chosen levels; scores: optional float64 [N, 361]."""
    assert obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] >= _lib.OBS_DIM and obs.stride(1) == 1, (obs.dtype, obs.shape)
    assert obs.device == self.device
    n = obs.shape[0]
    if out is None:
      out = torch.empty(n, dtype=torch.uint8, device=self.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n
    if level is not None:
      assert level.dtype == torch.int32 and level.is_contiguous() and level.numel() == n
    if scores is not None:
      assert scores.dtype == torch.float64 and scores.is_contiguous() and scores.numel() == n * NUM_LEVELS
    stride = obs.stride(0) if n > 1 else max(obs.stride(0), _lib.OBS_DIM)
    _lib.check(self.lib.ble_station_seeker_f32(obs.data_ptr(), stride, out.data_ptr(), dev.ptr(level), dev.ptr(scores),
                                               self.err_flags.data_ptr(), n, dev.stream_ptr(self.device)), 'ble_station_seeker_f32')
    return out

  __call__ = act

  def check_errors(self) -> None:
    """Synchronises; raises AssertionError (the reference's) if some environment had no valid level since the last call."""
    flags = int(self.err_flags.item())
    if flags:
      self.err_flags.zero_()
      from balloon_learning_environment_amd import vec_state
      vec_state.raise_for_flags(flags)

  def get_name(self) -> str:
    return 'StationSeekerAgent'


class StationSeekerAgent(agent.Agent):
  """Implementation of the StationSeeker controller (the reference's interface; the arithmetic runs on the device)."""

  def __init__(self, num_actions: int, observation_shape: Sequence[int], device='cuda:0'):
    del num_actions
    del observation_shape
    # StationSeeker constants (the reference's attributes; the kernel holds the same numbers)
    self.half_radius = 35
    self.magnitude_weight = 0.07
    self.close_bearing_weight = 0.6
    self.far_bearing_weight = 0.45
    self.close_bearing = 250
    self.far_bearing = 500
    self.default_score = 0.5
    self.hysteresis_k2 = 0.05
    self.hysteresis_k3 = 0.001
    self.confidence_epsilon = 0.01
    self.max_altitude_score = 1 + self.hysteresis_k2 + self.confidence_epsilon
    self._vec = VecStationSeekerAgent(device)
    self.device = self._vec.device
    with torch.cuda.device(self.device):
      self._obs = torch.zeros(1, _lib.OBS_DIM, dtype=torch.float32, device=self.device)
      self._action = torch.zeros(1, dtype=torch.uint8, device=self.device)
      self._level = torch.zeros(1, dtype=torch.int32, device=self.device)
      self._scores = torch.zeros(1, NUM_LEVELS, dtype=torch.float64, device=self.device)
    super().__init__(3, (_lib.OBS_DIM,))

  def begin_episode(self, observation: np.ndarray) -> int:
    assert observation is not None
    return self.pick_action(observation)

  def step(self, reward: float, observation: np.ndarray) -> int:
    del reward
    assert observation is not None
    return self.pick_action(observation)

  def end_episode(self, reward: float, terminal: bool) -> None:
    pass

  def _run(self, features_as_vector) -> Tuple[int, int, np.ndarray]:
    f = features_as_vector
    if isinstance(f, torch.Tensor):
      f = f.detach().to(self.device, torch.float32).reshape(1, -1)
    else:
      f = torch.from_numpy(np.ascontiguousarray(np.asarray(f, np.float32).reshape(1, -1)))
    self._obs.copy_(f)
    self._vec.act(self._obs, out=self._action, level=self._level, scores=self._scores)
    self._vec.check_errors()
    return int(self._action.item()), int(self._level.item()), self._scores[0].cpu().numpy()

  def pick_action(self, features_as_vector) -> int:
    """Picks the action based on the best pressure level (UP 2 below the centre level, DOWN 0 above it, STAY 1 at it)."""
    return self._run(features_as_vector)[0]

  def find_best_pressure_level(self, named_features: features.NamedPerciatelliFeatures) -> Tuple[int, np.ndarray]:
    """(best level, the altitude score of every level -- 0 where not valid).  Raises AssertionError when no level is valid."""
    v = np.zeros(_lib.OBS_DIM, np.float32)
    v[7] = named_features.distance_to_station          # the score reads the distance and the wind column only
    v[16:] = np.asarray(named_features._winds, np.float32)
    _, level, scores = self._run(v)
    return level, scores
