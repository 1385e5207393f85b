"""Q-network policies on the device: the eval-mode forward pass of the reference's QuantileNetwork and MLPNetwork (agents/networks.py).

The reference's QR-DQN agents (quantile, perciatelli44, finetune_perciatelli: configs/quantile.gin) and DQN agent (configs/dqn.gin)
act in eval mode (epsilon_eval = 0) by one forward pass, q = the mean of each action's atoms, argmax.  `QNetwork` holds the parameters
of such a network, packed once into the device image `ble_qnet_forward_f32` reads (csrc/ble_qnet.h); `VecQNetworkAgent` is the native
object -- [N, 1099] float32 device observations in, uint8 [N] device actions out, no host synchronisation, capturable in a graph.  The
kernel's reduction order depends on the network's shape only, so a row's q-values and action are the same bits at any batch size, at
any position and at any row stride: seed s of eval_agent_vec flies the same flight in any batch with a learned policy too.
"""
import ctypes
import re
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from balloon_learning_environment_amd import _abi
from balloon_learning_environment_amd import _lib
from balloon_learning_environment_amd import device as dev

NUM_ACTIONS = 3
_DENSE = re.compile(r'^Dense_(\d+)$')


def _dense_layers(params) -> Dict[int, dict]:
  tree = params.get('params', params) if hasattr(params, 'get') else params
  if not hasattr(tree, 'items'):
    raise ValueError('params: a {"params": {"Dense_i": {"kernel", "bias"}}} tree (or its inner dict)')
  layers = {}
  for name, leaf in tree.items():
    m = _DENSE.match(str(name))
    if m is None:
      raise ValueError(f'params: unexpected entry {name!r} (a QuantileNetwork / MLPNetwork holds Dense_0 .. Dense_L-1 only)')
    layers[int(m.group(1))] = leaf
  if not layers:
    raise ValueError('params: no Dense_i layer')
  missing = [i for i in range(max(layers) + 1) if i not in layers]
  if missing:
    raise ValueError(f'params: Dense_{missing[0]} is missing (layers {sorted(layers)})')
  return layers


class QNetwork:
  """The parameters of a QuantileNetwork (num_atoms > 1) or MLPNetwork (num_atoms == 1) with 3 actions and the 1099 features, in
  float32, and their packed device image.

  kernels[i]: [in, out] (flax's Dense kernel), biases[i]: [out].  Layer 0 maps 1099 features to hidden_units (or, with one layer, to
  3 * num_atoms), the last layer maps hidden_units to 3 * num_atoms."""

  def __init__(self, kernels, biases, num_atoms: int, device='cuda:0'):
    self.device = torch.device(device)
    self.kernels = [np.ascontiguousarray(k, np.float32) for k in kernels]
    self.biases = [np.ascontiguousarray(b, np.float32) for b in biases]
    self.num_layers = len(self.kernels)
    self.num_atoms = int(num_atoms)
    self.hidden_units = int(self.kernels[0].shape[1]) if self.num_layers > 1 else 0
    self._struct = _abi.BleQnetF32(self.num_layers, _lib.OBS_DIM, self.hidden_units, NUM_ACTIONS, self.num_atoms, 0, None)
    packed_floats = ctypes.c_int64()
    _lib.call('ble_qnet_workspace_f32', ctypes.byref(self._struct), 0, ctypes.byref(packed_floats), None)
    # the packed image, made once on the host (ble_qnet_pack_f32); it goes to the device on the first use there
    self.packed_host = np.zeros(packed_floats.value, np.float32)
    kp = (ctypes.c_void_p * self.num_layers)(*[k.ctypes.data for k in self.kernels])
    bp = (ctypes.c_void_p * self.num_layers)(*[b.ctypes.data for b in self.biases])
    _lib.call('ble_qnet_pack_f32', ctypes.byref(self._struct), kp, bp, self.packed_host.ctypes.data)
    self.packed: Optional[torch.Tensor] = None

  def to_device(self) -> 'QNetwork':
    """Copies the packed image to the network's device (once; not inside a graph capture)."""
    if self.packed is None:
      self.device = dev.require_gpu(self.device)
      with torch.cuda.device(self.device):
        self.packed = torch.from_numpy(self.packed_host).to(self.device)
      self._struct.weights = self.packed.data_ptr()
    return self

  @classmethod
  def from_params(cls, params, num_atoms: Optional[int] = None, device='cuda:0') -> 'QNetwork':
    """From the flax parameter tree the reference builds -- {'params': {'Dense_i': {'kernel': [in, out], 'bias': [out]}}}, or the
    inner dict -- whose leaves are anything np.asarray takes.  num_atoms: default out / 3 of the last layer (1: an MLPNetwork).

    Raises ValueError for a missing Dense_i, an input dimension other than 1099, layers whose widths do not chain, a last layer whose
    width is not a multiple of 3 * num_atoms, or a non-finite parameter."""
    layers = _dense_layers(params)
    kernels, biases = [], []
    for i in range(len(layers)):
      leaf = layers[i]
      try:
        with np.errstate(over='ignore'):         # (a value beyond float32's range becomes inf, refused below)
          k, b = np.asarray(leaf['kernel'], np.float32), np.asarray(leaf['bias'], np.float32)
      except (KeyError, TypeError) as e:
        raise ValueError(f'params: Dense_{i} needs a kernel and a bias') from e
      if k.ndim != 2 or b.shape != (k.shape[1],):
        raise ValueError(f'params: Dense_{i} kernel {k.shape} and bias {b.shape} are not [in, out] and [out]')
      want = _lib.OBS_DIM if i == 0 else kernels[-1].shape[1]
      if k.shape[0] != want:
        what = 'the input dimension' if i == 0 else f'the width of Dense_{i - 1}'
        raise ValueError(f'params: Dense_{i} takes {k.shape[0]} inputs, {what} is {want}')
      if not (np.isfinite(k).all() and np.isfinite(b).all()):
        raise ValueError(f'params: Dense_{i} has a non-finite value (in float32)')
      kernels.append(k)
      biases.append(b)
    n_out = kernels[-1].shape[1]
    atoms = n_out // NUM_ACTIONS if num_atoms is None else int(num_atoms)
    if atoms < 1 or n_out != NUM_ACTIONS * atoms:
      raise ValueError(f'params: the last layer has {n_out} outputs, not {NUM_ACTIONS} actions x {atoms} atoms')
    if len(kernels) > 1 and any(k.shape[1] != kernels[0].shape[1] for k in kernels[:-1]):
      raise ValueError('params: the hidden layers differ in width')
    return cls(kernels, biases, atoms, device=device)

  @classmethod
  def from_npz(cls, path, num_atoms: Optional[int] = None, device='cuda:0') -> 'QNetwork':
    """From save_npz's file (keys Dense_i/kernel and Dense_i/bias)."""
    with np.load(path) as z:
      tree = {}
      for key in z.files:
        layer, _, leaf = key.partition('/')
        tree.setdefault(layer, {})[leaf] = z[key]
    return cls.from_params(tree, num_atoms=num_atoms, device=device)

  def save_npz(self, path) -> None:
    arrays = {}
    for i, (k, b) in enumerate(zip(self.kernels, self.biases)):
      arrays[f'Dense_{i}/kernel'] = k
      arrays[f'Dense_{i}/bias'] = b
    np.savez(path, **arrays)

  def params(self) -> dict:
    """The flax-shaped tree of the float32 parameters."""
    return {'params': {f'Dense_{i}': {'kernel': k, 'bias': b} for i, (k, b) in enumerate(zip(self.kernels, self.biases))}}

  @property
  def shape(self) -> Tuple[int, int, int]:
    """(num_layers, hidden_units, num_atoms)."""
    return self.num_layers, self.hidden_units, self.num_atoms

  def flops_per_row(self) -> int:
    """2 x the multiply-adds of one forward pass (the reference's shapes, no padding)."""
    return sum(2 * k.shape[0] * k.shape[1] for k in self.kernels)


def init_params(kind: str, seed: int = 0, num_layers: int = 8, hidden_units: int = 600, num_atoms: int = 51) -> dict:
  """Parameters of the reference's initialisation with zero biases (flax Dense's bias_init): 'quantile' -- QuantileNetwork's
  variance_scaling(1 / sqrt(3), 'fan_in', 'uniform'), i.e. U(-l, l) with l = sqrt(3 scale / fan_in) = 3^(1/4) / sqrt(fan_in);
  'mlp' -- MLPNetwork's glorot_uniform, l = sqrt(6 / (fan_in + fan_out)), and num_atoms is ignored (one output per action).  The
  draws come from numpy's PCG64 with `seed`, not from JAX's PRNG: networks of the right scale, not the reference's bits."""
  if kind not in ('quantile', 'mlp'):
    raise ValueError(f"kind is 'quantile' or 'mlp', not {kind!r}")
  if num_layers < 1:
    raise ValueError('num_layers >= 1')
  atoms = num_atoms if kind == 'quantile' else 1
  rng = np.random.default_rng(seed)
  dims = [_lib.OBS_DIM] + [hidden_units] * (num_layers - 1) + [NUM_ACTIONS * atoms]
  tree = {}
  for i in range(num_layers):
    fan_in, fan_out = dims[i], dims[i + 1]
    limit = np.sqrt(3.0 / np.sqrt(3.0) / fan_in) if kind == 'quantile' else np.sqrt(6.0 / (fan_in + fan_out))
    tree[f'Dense_{i}'] = {'kernel': rng.uniform(-limit, limit, (fan_in, fan_out)).astype(np.float32),
                          'bias': np.zeros(fan_out, np.float32)}
  return {'params': tree}


class Forward:
  """ble_qnet_forward_f32 on a network descriptor whose image is on the device, with the scratch it needs: the activations of a batch
  size (2 x N x the widest padded layer, float32) are allocated on the first call at that size, which must not be inside a graph
  capture; later calls allocate nothing, so they can be captured.  `owner` names the caller's class in that refusal."""

  def __init__(self, struct: _abi.BleQnetF32, device: torch.device, owner: str):
    self.struct, self.device, self.owner = struct, device, owner
    self._scratch: Dict[int, torch.Tensor] = {}

  def _allocate(self, n: int) -> torch.Tensor:
    floats = ctypes.c_int64()
    _lib.call('ble_qnet_workspace_f32', ctypes.byref(self.struct), n, None, ctypes.byref(floats))
    return torch.empty(max(floats.value, 1), dtype=torch.float32, device=self.device)

  def __call__(self, obs: torch.Tensor, out: torch.Tensor, q_values: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch on the current stream of the network's device (no checks beyond the library's): the actions of obs's rows into out."""
    n = obs.shape[0]
    scratch = dev.first_use(self._scratch, n, lambda: self._allocate(n),
                            f'{self.owner}: call act once at batch size {n} before capturing it in a graph (scratch allocation)')
    stride = obs.stride(0) if n > 1 else max(obs.stride(0), _lib.OBS_DIM)      # (torch gives a one-row tensor any stride)
    _lib.call('ble_qnet_forward_f32', ctypes.byref(self.struct), obs.data_ptr(), stride, scratch.data_ptr(), out.data_ptr(),
              dev.ptr(q_values), n, dev.stream_ptr(self.device))
    return out


class VecQNetworkAgent:
  """A Q-network policy for N environments at once: act(obs [N, 1099] float32 device) -> uint8 [N] device.

  The scratch of a batch size is allocated on the first call at that size, which must not be inside a graph capture (Forward)."""

  def __init__(self, network: QNetwork):
    self.network = network.to_device()
    self.device = network.device
    self._forward = Forward(network._struct, self.device, 'VecQNetworkAgent')

  @dev.on_own_device
  def act(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None, q_values: Optional[torch.Tensor] = None) -> torch.Tensor:
    """obs: [N, >= 1099] float32 on this agent's device (rows may be padded: stride(0) >= 1099, stride(1) == 1); only the first 1099
    columns are read.  out: optional uint8 [N] for the actions; q_values: optional float32 [N, 3]."""
    assert obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] >= _lib.OBS_DIM and obs.stride(1) == 1, (obs.dtype, obs.shape)
    assert obs.device == self.device
    n = obs.shape[0]
    if out is None:
      out = torch.empty(n, dtype=torch.uint8, device=self.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n
    if q_values is not None:
      assert q_values.dtype == torch.float32 and q_values.is_contiguous() and q_values.numel() == n * NUM_ACTIONS
    if n == 0:
      return out
    return self._forward(obs, out, q_values)

  __call__ = act

  def get_name(self) -> str:
    return 'QuantileAgent' if self.network.num_atoms > 1 else 'DQNAgent'
