// ble_qnet.h -- the eval-mode forward pass of the reference's QuantileNetwork / MLPNetwork (agents/networks.py) on a batch of
// observations: Dense layers of fp32 weights on v_mfma_f32_32x32x2_f32, ReLU after every layer but the last, q[a] = the mean of action
// a's atoms, action = argmax q (jnp.argmax: the lowest index among equal maxima, the first NaN if one is NaN).
//
// Layout (made once by qnet_pack on the host).  Layer l maps K_l inputs to M_l outputs.  Kp = K rounded up to 8 (one
// K chunk), Mp = M rounded up to 64 (one workgroup's columns).  The layer's packed block is [Mp / 64 groups][Kp / 8 chunks][2 tiles]
// [64 lanes][4] floats, element (g, c, t, lane, j) = W[8c + 4(lane >> 5) + j][64g + 32t + (lane & 31)], zero outside W, followed by
// the bias padded with zeros to Mp.  Every block is a multiple of 64 floats, so every float4 read is aligned.
//
// Tiling: a workgroup is four independent waves over 128 rows x 64 columns, each wave 32 rows x 64 columns (two 32x32 accumulators).
// The K loop runs over the chunks in ascending order; in chunk c, MFMA step j sums k = 8c + j (lanes 0..31) and 8c + 4 + j (lanes
// 32..63).  Every output element is thus ONE fixed fma chain whose order depends on the layer's shape alone -- not on n, the row's
// position in the batch or the input's row stride: the batch-invariance contract.  Rows past n are loaded as row n - 1 (their results
// are not stored); input columns past K are loaded as 0.0, never read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ble {

constexpr int kQnetBlock = 256;        // four waves
constexpr int kQnetRows = 128;         // rows per workgroup, 32 per wave
constexpr int kQnetCols = 64;          // columns per workgroup (and per wave: two 32x32 tiles)
constexpr int kQnetChunk = 8;          // K per chunk: four MFMA steps of K = 2
constexpr int kQnetMaxLayers = 64;
constexpr int kQnetMaxHidden = 8192;
constexpr int kQnetMaxAtoms = 4096;
constexpr int kQnetHeadBlock = 256;

typedef float qnet_f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ inline int64_t qnet_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// Padded sizes of layer l of a network: inputs (Kp) and outputs (Mp) of the packed block.
struct QnetLayerDims {
  int k, m;            // the reference's in / out features
  int kp, mp;          // padded
  int64_t offset;      // of the layer's packed kernel, in floats from the start of the weights; its bias follows at offset + kp * mp
};

inline QnetLayerDims qnet_layer(int num_layers, int input_dim, int hidden, int num_actions, int num_atoms, int l) {
  QnetLayerDims d;
  d.offset = 0;
  for (int i = 0; i <= l; ++i) {
    d.k = i == 0 ? input_dim : hidden;
    d.m = i == num_layers - 1 ? num_actions * num_atoms : hidden;
    d.kp = (int)qnet_round_up(d.k, kQnetChunk);
    d.mp = (int)qnet_round_up(d.m, kQnetCols);
    if (i < l) d.offset += (int64_t)d.kp * d.mp + d.mp;
  }
  return d;
}

// The A operand of one chunk: x[k0 .. k0 + 3] of this lane's row.  kObs: the caller's observation rows (any stride, so no vector load;
// columns >= k are 0.0 and not read).  Otherwise the agent's own activation rows (stride a multiple of 64 floats, every column < kp
// written), one aligned float4.
template <bool kObs>
__device__ __forceinline__ float4 qnet_load_a(const float* __restrict__ xr, int k0, int k) {
  if (kObs) {
    float4 a;
    a.x = k0 + 0 < k ? xr[k0 + 0] : 0.0f;
    a.y = k0 + 1 < k ? xr[k0 + 1] : 0.0f;
    a.z = k0 + 2 < k ? xr[k0 + 2] : 0.0f;
    a.w = k0 + 3 < k ? xr[k0 + 3] : 0.0f;
    return a;
  }
  return *reinterpret_cast<const float4*>(xr + k0);
}

__device__ __forceinline__ void qnet_mfma4(const float4 a, const float4 b0, const float4 b1, qnet_f32x16& acc0, qnet_f32x16& acc1) {
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
}

// y[r][0 .. mp) = act(x[r][0 .. k) . W + b) for rows r < n: one Dense layer (+ ReLU unless it is the last).  Workgroup t covers column
// group t % groups and rows 128 (t / groups) ...: the groups of one row block are adjacent in dispatch order, so they read its rows
// while they are in cache.
template <bool kObs, bool kRelu>
__global__ __launch_bounds__(kQnetBlock) void ble_qnet_dense_kernel(const float* __restrict__ x, int64_t ldx, int k, int kp,
                                                                     const float* __restrict__ w, float* __restrict__ y, int64_t ldy,
                                                                     int groups, int64_t n) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t tile = blockIdx.x;
  const int g = (int)(tile % groups);
  const int64_t r0 = (tile / groups) * kQnetRows + (threadIdx.x >> 6) * 32;
  if (r0 >= n) return;                                       // (a whole wave; no barrier follows)
  const int half = lane >> 5;
  const int64_t row = min(r0 + (lane & 31), n - 1);
  const float* __restrict__ xr = x + row * ldx;
  const float4* __restrict__ wg = reinterpret_cast<const float4*>(w + (int64_t)g * kp * kQnetCols) + lane;
  const int chunks = kp / kQnetChunk;
  qnet_f32x16 acc0, acc1;
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
  // one chunk ahead in registers: its loads are in flight while this chunk's eight MFMAs (512 cycles) issue
  float4 a = qnet_load_a<kObs>(xr, 4 * half, k);
  float4 b0 = wg[0], b1 = wg[64];
  for (int c = 0; c < chunks; ++c) {
    const int cn = c + 1 < chunks ? c + 1 : c;
    const float4 an = qnet_load_a<kObs>(xr, cn * kQnetChunk + 4 * half, k);
    const float4 b0n = wg[(int64_t)cn * 128], b1n = wg[(int64_t)cn * 128 + 64];
    qnet_mfma4(a, b0, b1, acc0, acc1);
    a = an; b0 = b0n; b1 = b1n;
  }
  // epilogue: accumulator register r of tile t is row (r & 3) + 8 (r >> 2) + 4 half, column 32 t + (lane & 31)
  const float* __restrict__ bias = w + (int64_t)kp * (groups * kQnetCols) + g * kQnetCols;
  const int col = g * kQnetCols + (lane & 31);
  const float bias0 = bias[lane & 31], bias1 = bias[32 + (lane & 31)];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t rr = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (rr < n) {
      float v0 = acc0[r] + bias0, v1 = acc1[r] + bias1;
      if (kRelu) {                                          // nn.relu; a NaN stays NaN (fmaxf would drop it)
        v0 = v0 < 0.0f ? 0.0f : v0;
        v1 = v1 < 0.0f ? 0.0f : v1;
      }
      y[rr * ldy + col] = v0;
      y[rr * ldy + col + 32] = v1;
    }
  }
}

// q[a] = (logit[a * atoms] + ... + logit[a * atoms + atoms - 1]) / atoms in ascending atom order, fp32; the action is the first maximum,
// or the first NaN.  One lane per row.
__global__ __launch_bounds__(kQnetHeadBlock) void ble_qnet_head_kernel(const float* __restrict__ logits, int64_t ld, int actions,
                                                                       int atoms, uint8_t* __restrict__ action, float* __restrict__ q,
                                                                       int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kQnetHeadBlock + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ r = logits + i * ld;
  int best = 0;
  float qb = 0.0f;
  for (int a = 0; a < actions; ++a) {
    float s = 0.0f;
    for (int j = 0; j < atoms; ++j) s += r[a * atoms + j];
    const float qa = s / (float)atoms;
    if (q != nullptr) q[i * actions + a] = qa;
    if (a == 0 || (qb == qb && (qa != qa || qa > qb))) {
      best = a;
      qb = qa;
    }
  }
  action[i] = (uint8_t)best;
}

// Host: the packed image of a network (layout above) from its row-major kernels [k][m] and biases [m].
inline void qnet_pack(int num_layers, int input_dim, int hidden, int num_actions, int num_atoms, const float* const* kernel,
                      const float* const* bias, float* packed) {
  for (int l = 0; l < num_layers; ++l) {
    const QnetLayerDims d = qnet_layer(num_layers, input_dim, hidden, num_actions, num_atoms, l);
    float* p = packed + d.offset;
    const float* W = kernel[l];
    for (int g = 0; g < d.mp / kQnetCols; ++g)
      for (int c = 0; c < d.kp / kQnetChunk; ++c)
        for (int t = 0; t < 2; ++t)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 4; ++j) {
              const int kk = kQnetChunk * c + 4 * (lane >> 5) + j, mm = kQnetCols * g + 32 * t + (lane & 31);
              *p++ = (kk < d.k && mm < d.m) ? W[(int64_t)kk * d.m + mm] : 0.0f;
            }
    for (int mm = 0; mm < d.mp; ++mm) *p++ = mm < d.m ? bias[l][mm] : 0.0f;
  }
}

}  // namespace ble
