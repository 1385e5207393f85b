"""A NumPy restatement of Marco Polo exploration over a random walk (the reference's MarcoPoloExploration + RandomWalkAgent, as the
device kernel ble_marco_polo_u8 states it), N lanes, its draws given as inputs."""
import numpy as np

RL_STEPS, EXPLORE_STEPS = 80, 40


def u24(u):
  """The kernel's 24-bit float32 uniform from a 53-bit double in [0, 1)."""
  return (np.floor(np.asarray(u, np.float64) * 16777216.0) / 16777216.0).astype(np.float32)


def target_from_uniform(u):
  """jax.random.uniform(minval=6500, maxval=11400) in float32: max(minval, u (max - min) + min)."""
  u = np.asarray(u, np.float32)
  return np.maximum(np.float32(6500), u * np.float32(4900) + np.float32(6500)).astype(np.float64)


def pressure(f0):
  """NamedPerciatelliFeatures.balloon_pressure: 5000 + f0 (14000 - 5000), float32."""
  return np.float32(5000) + np.asarray(f0, np.float32) * np.float32(9000)


class MarcoPolo:
  def __init__(self, n, probability=0.8):
    self.p = float(probability)
    self.phase_clock = np.zeros(n, np.int32)
    self.walk_clock = np.zeros(n, np.int32)
    self.exploratory_episode = np.zeros(n, np.uint8)
    self.exploratory_phase = np.zeros(n, np.uint8)
    self.target = np.zeros(n)

  def __call__(self, f0, actions, begin, u_target, u_episode, z):
    """actions (the agent's) -> the actions taken.  u_target, u_episode: 24-bit uniforms (used where begin); z: normals."""
    a = np.array(actions, np.uint8)
    b = np.asarray(begin).astype(bool)
    self.walk_clock[b] = 0
    self.target[b] = target_from_uniform(np.asarray(u_target)[b])
    self.phase_clock[b] = 0
    self.exploratory_episode[b] = (np.asarray(u_episode, np.float64)[b] <= self.p).astype(np.uint8)
    self.exploratory_phase[b] = 0
    s = ~b
    self.phase_clock[s] += 1
    limit = np.where(self.exploratory_phase == 1, EXPLORE_STEPS, RL_STEPS)
    flip = s & (self.exploratory_episode == 1) & (self.phase_clock >= limit)
    self.exploratory_phase[flip] ^= 1
    self.phase_clock[flip] = 0
    x = s & (self.exploratory_phase == 1)
    self.walk_clock[x] += 1
    self.target[x] = self.target[x] + (self.walk_clock[x].astype(np.float64) * 180.0) * 0.1666 * np.asarray(z, np.float64)[x]
    p = pressure(f0)
    up = (p - np.float32(100)).astype(np.float64) > self.target
    down = (p + np.float32(100)).astype(np.float64) < self.target
    a[x] = np.where(up, 2, np.where(down, 0, 1)).astype(np.uint8)[x]
    return a
