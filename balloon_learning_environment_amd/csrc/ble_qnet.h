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

// The per-layer shape of a network (the part of the shape table ble_adam_kernel takes by value): layer l maps k[l] inputs to m[l] outputs,
// padded to kp[l] and mp[l].
struct TrainDims {
  int layers;
  int64_t offset[kQnetMaxLayers + 1];        // packed block of layer l (its bias follows at + kp * mp); offset[layers] = the image's size
  int64_t toffset[kQnetMaxLayers];           // its transposed block in weights_t (l >= 1)
  int k[kQnetMaxLayers], m[kQnetMaxLayers], kp[kQnetMaxLayers], mp[kQnetMaxLayers];
};

// The shape table of a network: every size the host code needs, built once per entry-point call by qnet_shape.
struct QnetShape : TrainDims {
  int64_t ld;                  // floats per activation row: the widest mp
  int64_t max_block;           // the largest packed block (kernel + bias)
  int64_t transposed_floats;   // the size of weights_t
  int64_t block(int l) const { return offset[l + 1] - offset[l]; }
  // the transposed block of layer l >= 1 (W^T as a K' = M_l by M' = K_l layer, no bias): kp' = round8(M_l), mp' = round64(K_l) = mp[l - 1]
  int kpt(int l) const { return (int)qnet_round_up(m[l], kQnetChunk); }
  int mpt(int l) const { return mp[l - 1]; }
};

inline QnetShape qnet_shape(int num_layers, int input_dim, int hidden, int num_actions, int num_atoms) {
  QnetShape s{};
  s.layers = num_layers;
  for (int l = 0; l < num_layers; ++l) {
    s.k[l] = l == 0 ? input_dim : hidden;
    s.m[l] = l == num_layers - 1 ? num_actions * num_atoms : hidden;
    s.kp[l] = (int)qnet_round_up(s.k[l], kQnetChunk);
    s.mp[l] = (int)qnet_round_up(s.m[l], kQnetCols);
    s.offset[l + 1] = s.offset[l] + (int64_t)s.kp[l] * s.mp[l] + s.mp[l];
    s.toffset[l] = s.transposed_floats;
    if (l > 0) s.transposed_floats += (int64_t)s.kpt(l) * s.mpt(l);
    s.ld = s.ld > s.mp[l] ? s.ld : s.mp[l];
    s.max_block = s.max_block > s.block(l) ? s.max_block : s.block(l);
  }
  return s;
}

// The layout, stated once: float r of the packed kernel block ([groups][chunks][2 tiles][64 lanes][4]) of a layer with kp padded inputs
// holds W[*k][*m].
__host__ __device__ inline void qnet_slot_km(int64_t r, int kp, int* k, int* m) {
  const int j = (int)(r & 3), lane = (int)((r >> 2) & 63), t = (int)((r >> 8) & 1);
  const int64_t gc = r >> 9;
  const int chunks = kp / kQnetChunk;
  const int c = (int)(gc % chunks), g = (int)(gc / chunks);
  *k = kQnetChunk * c + 4 * (lane >> 5) + j;
  *m = kQnetCols * g + 32 * t + (lane & 31);
}

// Position of W^T[m][k] (= W[k][m]) in the transposed block of a layer with K inputs, M outputs: K' = M (kp' = round8(M)), M' = K.
__host__ __device__ inline int64_t qnet_transposed_index(int k, int m, int kpt) {
  const int c = m / kQnetChunk, j = m & 3, ln = (k & 31) + 32 * ((m & 7) >> 2), t = (k >> 5) & 1, g = k >> 6;
  return (((int64_t)g * (kpt / kQnetChunk) + c) * 2 + t) * 256 + ln * 4 + j;
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

// ------------------------------------------------------------------------------------------------------------ host: the packed images
// f(r, k, m, inside) for every float r of layer l's packed kernel block in storage order; inside: W has an element [k][m] (else padding).
template <class F>
inline void qnet_for_each_slot(const TrainDims& s, int l, F&& f) {
  for (int64_t r = 0; r < (int64_t)s.kp[l] * s.mp[l]; ++r) {
    int k, m;
    qnet_slot_km(r, s.kp[l], &k, &m);
    f(r, k, m, k < s.k[l] && m < s.m[l]);
  }
}

// The packed image of a network (layout above) from its row-major kernels [k][m] and biases [m].
inline void qnet_pack(const QnetShape& s, const float* const* kernel, const float* const* bias, float* packed) {
  for (int l = 0; l < s.layers; ++l) {
    float* p = packed + s.offset[l];
    qnet_for_each_slot(s, l, [&](int64_t r, int k, int m, bool inside) { p[r] = inside ? kernel[l][(int64_t)k * s.m[l] + m] : 0.0f; });
    p += (int64_t)s.kp[l] * s.mp[l];
    for (int m = 0; m < s.mp[l]; ++m) p[m] = m < s.m[l] ? bias[l][m] : 0.0f;
  }
}

// Its inverse: the kernels and biases of a packed image.
inline void qnet_unpack(const QnetShape& s, const float* packed, float* const* kernel, float* const* bias) {
  for (int l = 0; l < s.layers; ++l) {
    const float* p = packed + s.offset[l];
    qnet_for_each_slot(s, l, [&](int64_t r, int k, int m, bool inside) { if (inside) kernel[l][(int64_t)k * s.m[l] + m] = p[r]; });
    p += (int64_t)s.kp[l] * s.mp[l];
    for (int m = 0; m < s.m[l]; ++m) bias[l][m] = p[m];
  }
}

// weights_t of a packed image: the packed image of W^T of layers 1 .. L - 1, zero outside W^T (ble_train.h's dgrad reads it; the Adam
// kernel keeps it current).
inline void qnet_transpose(const QnetShape& s, const float* packed, float* packed_t) {
  for (int l = 1; l < s.layers; ++l) {
    const float* p = packed + s.offset[l];
    float* pt = packed_t + s.toffset[l];
    for (int64_t e = 0; e < (int64_t)s.kpt(l) * s.mpt(l); ++e) pt[e] = 0.0f;
    qnet_for_each_slot(s, l, [&](int64_t r, int k, int m, bool inside) { if (inside) pt[qnet_transposed_index(k, m, s.kpt(l))] = p[r]; });
  }
}

}  // namespace ble
