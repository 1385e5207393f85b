"""The headline shape for a profiler: 32-step launches (ble_step_n_f32) of 65 536 environments, 8 launches after 2 of warm-up.

    python profiles/step_fused.py [n_envs] [form]        # form: ble_set_step_form's value (0 automatic, 1, 4, 12)
Prints the form the library reports for its last launch (ble_last_step_form, where the library has it)."""
import os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from balloon_learning_environment_amd import _lib, vec_state
sys.path.insert(0, os.path.join(ROOT, 'tests'))      # (the host-side state sampler is test tooling)
import reset_host  # noqa: E402
n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
form = int(sys.argv[2]) if len(sys.argv) > 2 else 0
sim = vec_state.VecSimulator(n)
field = (np.random.default_rng(0).standard_normal((21, 21, 10, 9, 2)) * 5).astype(np.float32)
sim.set_grid(torch.from_numpy(field).cuda())
sim.set_state(reset_host.sample_initial_state(n, seed=1000))
gen = torch.Generator(device='cuda'); gen.manual_seed(7)
acts = torch.randint(0, 3, (32, n), dtype=torch.uint8, device='cuda', generator=gen)
rew = torch.zeros((32, n), device='cuda'); term = torch.zeros((32, n), dtype=torch.uint8, device='cuda')
with _lib.step_form(form):
  for i in range(10):
    sim.step_n(acts, rew, term)
  torch.cuda.synchronize()
  query = getattr(_lib.lib(), 'ble_last_step_form', None)
  print('form of this launch:', query() if query is not None else 'no query in this library')
sim.check_errors()
