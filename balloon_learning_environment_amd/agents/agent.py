"""Agent interface (agents/agent.py of the reference): what eval_lib.eval_agent drives.

The reference's TensorBoard summary writer and checkpoint hooks are kept as no-ops so that code written against its interface
runs unchanged.
"""
import abc
import enum
from typing import Sequence, Union

import numpy as np


class AgentMode(enum.Enum):
  """An enum for the agent mode."""
  TRAIN = 'train'
  EVAL = 'eval'


class Agent(abc.ABC):
  """Abstract class for defining Balloon Learning Environment agents."""

  def __init__(self, num_actions: int, observation_shape: Sequence[int]):
    self._num_actions = num_actions
    self._observation_shape = observation_shape
    self.set_mode(AgentMode.TRAIN)

  def get_name(self) -> str:
    return self.__class__.__name__

  @abc.abstractmethod
  def begin_episode(self, observation: np.ndarray) -> int:
    """The first observation of an episode -> the action to apply."""

  @abc.abstractmethod
  def step(self, reward: float, observation: np.ndarray) -> int:
    """The last reward and observation -> the next action."""

  @abc.abstractmethod
  def end_episode(self, reward: float, terminal: bool = True) -> None:
    """The episode has ended (terminal is False for an episode cut at a fixed length)."""

  def set_summary_writer(self, summary_writer) -> None:
    self.summary_writer = summary_writer

  def set_mode(self, mode: Union[AgentMode, str]) -> None:
    """No-op; an agent that trains overrides it."""

  def save_checkpoint(self, checkpoint_dir: str, iteration_number: int) -> None:
    """No-op."""

  def load_checkpoint(self, checkpoint_dir: str, iteration_number: int) -> None:
    """No-op."""

  def reload_latest_checkpoint(self, checkpoint_dir: str) -> int:
    """No checkpoints: -1, as the reference's base class returns."""
    return -1
