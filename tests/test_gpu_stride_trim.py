"""The fused one-lane kernel against the split kernel: the same seeded batch through both forms, every state array, reward and terminal
row BIT FOR BIT.  The two forms inline the same lane functions (csrc/ble_step_core.h), so this test guards what differs AROUND them --
agent_step keeps the ACS mass flow in fp64 and converts it where it is read (after the loop, or on the path that parks a lane whose
episode ends inside a step), the split form converts it every stride for its LDS hand-over -- and not the values themselves: an error
inside a shared lane function moves both forms together, and only the oracle parity suite (tests/test_gpu_parity.py) sees it.  The batch
is checked to hold an episode that ends at a stride inside a step, and DOWN with a full battery on both sides of the reward's
excess-energy branch.  Needs a real MI355X:  pytest -m gpu."""
import numpy as np
import pytest

from balloon_learning_environment_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def test_fused_one_lane_equals_split_bit_for_bit():
  if not torch.cuda.is_available():
    pytest.fail('-m gpu tests need a HIP device; none visible')
  from balloon_learning_environment_amd import vec_state as ble
  import reset_host
  _lib.lib()
  n, k = 2048 - 19, 12                       # (the split form is selectable up to 32 768 environments; a last workgroup that is not full)
  init = reset_host.sample_initial_state(n, seed=21)
  init['battery_charge'][:64] = np.linspace(0.01, 30.0, 64).astype(np.float32)      # out of power inside the first steps: stride-level ends
  init['superpressure'][64:96] = 2379.0                                              # about to burst
  init['battery_charge'][96:352] = np.float32(3058.56)                               # full battery ...
  init['x'][96:352] = 0.0; init['y'][96:352] = 0.0                                   # ... inside the 50 km radius: the base reward is exactly 1
  acts_h = np.random.default_rng(5).integers(0, 3, (k, n)).astype(np.uint8)
  acts_h[:, 96:352] = 0                                                              # ... and DOWN on every step
  field = (np.random.default_rng(6).standard_normal((21, 21, 10, 9, 2)) * 5.0).astype(np.float32)
  acts = torch.from_numpy(acts_h).cuda()

  def fly(form):
    with _lib.step_form(form):
      sim = ble.VecSimulator(n); sim.set_state(init); sim.set_grid(field)
      rew = torch.zeros((k, n), dtype=torch.float32).cuda(); term = torch.zeros((k, n), dtype=torch.uint8).cuda()
      cnt = torch.zeros((k, ble.COUNT_SLOTS), dtype=torch.int64).cuda()
      sim.step_n(acts, rew, term, cnt)
      torch.cuda.synchronize()
      return sim.get_state(), rew.cpu().numpy(), term.cpu().numpy(), int(sim.err_flags.item())

  one, split = fly(1), fly(4)
  for name in one[0]:
    np.testing.assert_array_equal(one[0][name], split[0][name], err_msg=name)
  np.testing.assert_array_equal(one[1].view(np.uint32), split[1].view(np.uint32))
  np.testing.assert_array_equal(one[2], split[2])
  assert one[3] == split[3]
  # the cases are really there.  An episode that ended at a stride INSIDE a step: its clock stopped off the 180 s grid of agent steps
  ended = one[0]['status'] != 0
  flown_s = one[0]['time_elapsed_s'].astype(np.int64) - init['time_elapsed_s'].astype(np.int64)
  inside = ended & (flown_s % 180 != 0)
  assert inside.sum() >= 1, 'no stride-level termination in the batch'
  # DOWN with a full battery, both ways: excess energy (no penalty: the base reward 1.0 as it is) and none (at most 0.95)
  down = one[1][:, 96:352][one[2][:, 96:352] == 0]
  assert (down == 1.0).sum() >= 1, 'no DOWN step took the excess-energy branch'
  assert (down <= 0.95).sum() >= 1, 'no DOWN step was penalised'
  print(f'{int(ended.sum())} of {n} episodes ended, {int(inside.sum())} of them at a stride inside a step; DOWN steps with excess energy: '
        f'{int((down == 1.0).sum())}, penalised: {int((down <= 0.95).sum())}')
