"""bench.py --dump-outputs on CPU: what dump_outputs writes for a rollout (CPU tensors in the device state's dtypes)."""
import os
import types

import numpy as np
import torch

import bench
from balloon_learning_environment_amd import _abi


def _rollout(n, steps_in_last_launch=3):
  g = torch.Generator().manual_seed(0)
  state = {}
  for name in _abi.FIELD_NAMES:
    dt = _abi.FIELD_DTYPES[name]
    if dt == np.float32:
      state[name] = torch.randn(n, generator=g)
    elif dt == np.uint8:
      state[name] = torch.randint(0, 3, (n,), dtype=torch.uint8, generator=g)
    else:
      state[name] = torch.randint(0, 1 << 30, (n,), generator=g).to({np.int32: torch.int32, np.int64: torch.int64}[dt])
  state['start_unix'] += 1_600_000_000
  rewards = torch.rand(steps_in_last_launch, n, generator=g)
  terminals = torch.randint(0, 2, (steps_in_last_launch, n), dtype=torch.uint8, generator=g)
  return types.SimpleNamespace(np=np, n=n, sim=types.SimpleNamespace(state=state), timed_plan=[(None, None, None, None), (None, None, rewards, terminals)])


def test_dump_writes_the_last_step_and_the_state_exactly(tmp_path):
  roll = _rollout(1000)
  bench.dump_outputs(str(tmp_path), roll)
  names = sorted(f[:-4] for f in os.listdir(tmp_path))
  assert names == sorted(['env_index', 'reward', 'terminal'] + ['state_' + k for k in _abi.FIELD_NAMES])
  assert np.array_equal(np.load(tmp_path / 'env_index.npy'), np.arange(1000))
  reward = np.load(tmp_path / 'reward.npy')
  assert reward.dtype == np.float32 and np.array_equal(reward, roll.timed_plan[-1][2][-1].numpy())
  assert np.array_equal(np.load(tmp_path / 'terminal.npy'), roll.timed_plan[-1][3][-1].numpy())
  for k, t in roll.sim.state.items():
    a = np.load(tmp_path / f'state_{k}.npy')
    assert a.dtype in (np.float32, np.float64), k
    assert np.array_equal(a, t.numpy()), k           # exact: int32 / int64 fields are written as float64


def test_dump_above_the_limit_writes_a_fixed_sample(tmp_path, monkeypatch):
  monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 20000)
  roll = _rollout(1000)
  for out in ('a', 'b'):
    bench.dump_outputs(str(tmp_path / out), roll)
  total = sum(os.path.getsize(tmp_path / 'a' / f) - 128 for f in os.listdir(tmp_path / 'a'))     # (128 B .npy header each)
  assert total <= 20000
  idx = np.load(tmp_path / 'a' / 'env_index.npy').astype(np.int64)
  assert 0 < idx.size < 1000 and np.all(np.diff(idx) > 0)
  assert np.array_equal(np.load(tmp_path / 'a' / 'state_x.npy'), roll.sim.state['x'].numpy()[idx])
  for f in os.listdir(tmp_path / 'a'):
    assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)), f
