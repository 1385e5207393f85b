"""Rate of the Q-network forward pass (ble_qnet_forward_f32) against the fp32 matrix peak, and a torch fp32 chain on the same weights.

  python profiles/qnet_rate.py [--out profiles/qnet_rate.jsonl] [--reps 20]

For the (8, 600, 51) QR-DQN and (8, 600, 1) DQN shapes (init_params weights) at N in {1, 1024, 10000, 16384, 65536}: device-event time
of one VecQNetworkAgent.act (median of --reps after a warm-up) and of torch's addmm / relu chain plus the atom mean and argmax on the
same weights, each with the TFLOP/s of the reference's FLOPs (2 x the multiply-adds of the unpadded shapes) against 157.3 TF.  One JSON
line per shape and N.  Each shape also gets a line on batch invariance: whether the q-values of row 0 are bit-identical at N = 1 and
N = 10000, for the kernel and for the torch chain.  Kernel times proper come from a separate `rocprofv3 --kernel-trace --stats` run of
this script.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 157.3


def _time(fn, reps):
  import torch
  fn()
  torch.cuda.synchronize()
  ts = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ts.append(a.elapsed_time(b) * 1e-3)
  return float(np.median(ts))


def torch_chain(params, atoms):
  import torch
  layers = [(torch.from_numpy(v['kernel']).cuda(), torch.from_numpy(v['bias']).cuda()) for _, v in sorted(params['params'].items(),
                                                                                                   key=lambda kv: int(kv[0][6:]))]

  def q_of(x):
    h = x
    for i, (k, b) in enumerate(layers):
      h = torch.addmm(b, h, k)
      if i < len(layers) - 1:
        h = torch.relu(h)
    return h.reshape(h.shape[0], 3, atoms).mean(dim=2)
  return q_of


def main():
  import torch
  from balloon_learning_environment_amd.agents import qnet
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=None)
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--sizes', default='1,1024,10000,16384,65536')
  a = ap.parse_args()
  torch.backends.cuda.matmul.allow_tf32 = False
  sizes = [int(v) for v in a.sizes.split(',')]
  lines = []
  x_all = torch.rand(max(sizes), 1099, device='cuda', generator=torch.Generator('cuda').manual_seed(0))
  for kind, atoms in (('quantile', 51), ('mlp', 1)):
    params = qnet.init_params(kind, 0, 8, 600, atoms)
    net = qnet.QNetwork.from_params(params)
    agent = qnet.VecQNetworkAgent(net)
    chain = torch_chain(params, atoms)
    flops = net.flops_per_row()
    for n in sizes:
      x = x_all[:n]
      out = torch.empty(n, dtype=torch.uint8, device='cuda')
      t_k = _time(lambda: agent.act(x, out=out), a.reps)
      t_t = _time(lambda: torch.argmax(chain(x), dim=1), a.reps)
      line = {'shape': [8, 600, atoms], 'n': n, 'kernel_s': t_k, 'kernel_tflops': flops * n / t_k / 1e12,
              'kernel_peak_frac': flops * n / t_k / 1e12 / PEAK_TF, 'torch_s': t_t, 'torch_tflops': flops * n / t_t / 1e12}
      lines.append(line)
      print(json.dumps(line), flush=True)
    q1, q_big = torch.empty(1, 3, device='cuda'), torch.empty(10000, 3, device='cuda')
    agent.act(x_all[:1].contiguous(), q_values=q1)
    agent.act(x_all[:10000], q_values=q_big)
    t1, t_big = chain(x_all[:1].contiguous()), chain(x_all[:10000])
    torch.cuda.synchronize()
    line = {'shape': [8, 600, atoms], 'row0_bit_identical_n1_vs_n10000': {
        'kernel': bool(torch.equal(q1[0], q_big[0])), 'torch': bool(torch.equal(t1[0], t_big[0])),
        'torch_max_abs_diff': float((t1[0] - t_big[0]).abs().max())}}
    lines.append(line)
    print(json.dumps(line), flush=True)
  if a.out:
    with open(a.out, 'w') as f:
      for line in lines:
        f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
  main()
