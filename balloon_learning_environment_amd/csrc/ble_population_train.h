// ble_population_train.h -- training a population by gradient: the kernels of ble_qnet_ppo_step_grouped_f32.  Rows
// [p B, (p + 1) B) of a batch of P B rows are member p's, and member p's part of every stage holds the bytes ble_qnet_ppo_step_f32
// gives member p's own trainer on those B rows: loss, dlogits, gradient, weights, weights_t and both Adam moments.
//
// Every kernel is a sibling of a plain one (ble_actor.h, ble_train.h) with one more coordinate, the member; the plain kernels keep
// their instructions.  What makes the bytes equal is what the siblings do NOT change: the statements of the loss in their order, the
// 8-row loop of dW with its row masking and MFMA order, the slabs (a function of B, the member's rows, alone) summed in slab order,
// dX's K loop over the member's own transposed image, Adam's statements.  No floating-point atomics; every sum runs in an order fixed by
// the shape and B.
#pragma once
#include "ble_actor.h"
#include "ble_population.h"
#include "ble_train.h"

namespace ble {

// ble_ppo_loss_kernel for a population, one wave per row b of the P B rows; member p = b / B.  The divisor is (float) B, the member's
// rows; clip, value_coef and entropy_coef are read at [p].  The arithmetic is the plain kernel's, statement for statement.
__global__ __launch_bounds__(kTrainLossBlock) void ble_ppo_loss_grouped_kernel(
    const float* __restrict__ logits, int64_t ld, const float* __restrict__ ret, const uint8_t* __restrict__ action,
    const float* __restrict__ old_logp, const float* __restrict__ advantage, const float* __restrict__ clip_of,
    const float* __restrict__ value_coef_of, const float* __restrict__ entropy_coef_of, int64_t rows_per_member, float* __restrict__ aux,
    float* __restrict__ dlogits, float* __restrict__ loss, uint32_t* __restrict__ err_flags) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  float* __restrict__ dl = dlogits + b * ld;
  for (int c = lane; c < ld; c += kTrainLossBlock) dl[c] = 0.0f;
  __syncthreads();
  if (lane != 0) return;
  const int act = action[b];
  if (act >= 3) {
    if (err_flags != nullptr) atomicOr(err_flags, kFlagTrainAction);
    loss[b] = 0.0f;
    aux[2 * b] = 0.0f; aux[2 * b + 1] = 0.0f;
    return;
  }
  const int64_t p = b / rows_per_member;
  const float clip = clip_of[p], value_coef = value_coef_of[p], entropy_coef = entropy_coef_of[p];
  const float* __restrict__ z = logits + b * ld;
  const AcSoftmax sm = ac_log_softmax(z[0], z[2], z[4]);
  const float t0 = sm.p[0] * sm.lp[0];
  const float t1 = sm.p[1] * sm.lp[1];
  const float t2 = sm.p[2] * sm.lp[2];
  const float t01 = t0 + t1;
  const float h = -(t01 + t2);
  const float lpa = act == 0 ? sm.lp[0] : (act == 1 ? sm.lp[1] : sm.lp[2]);
  const float adv = advantage[b];
  const float d = lpa - old_logp[b];
  const float rho = expf(d);
  const float s1 = rho * adv;
  const float lo = 1.0f - clip, hi = 1.0f + clip;
  const float rc = fminf(fmaxf(rho, lo), hi);
  const float s2 = rc * adv;
  const bool active = s1 <= s2;
  const float lpi = -(active ? s1 : s2);
  const float dv = z[1] - ret[b];
  const float dv2 = dv * dv;
  const float lv = value_coef * dv2;
  const float lsum = lpi + lv;
  const float eh = entropy_coef * h;
  loss[b] = lsum - eh;
  const float w = adv * rho;
  const float fb = (float)rows_per_member;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ind = a == act ? 1.0f : 0.0f;
    const float dp = ind - sm.p[a];
    const float wg = w * dp;
    const float g = active ? -wg : 0.0f;
    const float lh = sm.lp[a] + h;
    const float plh = sm.p[a] * lh;
    const float ha = entropy_coef * plh;
    const float gh = g + ha;
    dl[2 * a] = gh / fb;
  }
  const float c2 = 2.0f * value_coef;
  const float gv = c2 * dv;
  dl[1] = gv / fb;
  aux[2 * b] = lpa;
  aux[2 * b + 1] = h;
}

// ble_qnet_wgrad_kernel for a population: blockIdx.z = p slabs + slab.  The slab's rows are [p B + slab slab_rows, min(.., (p + 1) B));
// the block goes to out + p member_out_stride + slab slab_stride: member p's gradient image (slabs == 1: member_out_stride = the
// images' stride, out = grad + offset[l]) or that member's partial-sum slabs (member_out_stride = slabs slab_stride).  The 8-row loop,
// the rin masking, the MFMA order and the bias shuffle are the plain kernel's.
__global__ __launch_bounds__(64) void ble_qnet_wgrad_grouped_kernel(const float* __restrict__ x, int64_t ldx, int k_in, int kp,
                                                                    const float* __restrict__ dy, int64_t ldy, int m_out, int mp,
                                                                    int64_t rows_per_member, int64_t slab_rows, int slabs,
                                                                    float* __restrict__ out, int64_t member_out_stride,
                                                                    int64_t slab_stride) {
  const int lane = threadIdx.x, half = lane >> 5, l31 = lane & 31;
  const int k0 = blockIdx.x * 32, g = blockIdx.y;
  const int m0 = g * kQnetCols;
  const int64_t p = blockIdx.z / slabs, slab = blockIdx.z % slabs;
  const int64_t end = (p + 1) * rows_per_member;
  const int64_t rb = p * rows_per_member + slab * slab_rows;
  const int64_t re = rb + slab_rows < end ? rb + slab_rows : end;
  float* __restrict__ o = out + p * member_out_stride + slab * slab_stride;
  const int kk = k0 + l31;
  const bool kin = kk < k_in;
  qnet_f32x16 acc0, acc1;
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
  float sb0 = 0.0f, sb1 = 0.0f;
  const bool bias = blockIdx.x == 0;
  for (int64_t b = rb; b < re; b += 8) {
    float a[4], y0[4], y1[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t row = b + 2 * s + half;
      const bool rin = row < re;
      a[s] = rin && kin ? x[row * ldx + kk] : 0.0f;
      y0[s] = rin ? dy[row * ldy + m0 + l31] : 0.0f;
      y1[s] = rin ? dy[row * ldy + m0 + 32 + l31] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], y0[s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], y1[s], acc1, 0, 0, 0);
      if (bias) { sb0 += y0[s]; sb1 += y1[s]; }
    }
  }
  const int chunks = kp / kQnetChunk;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = k0 / kQnetChunk + q;
    if (c >= chunks) break;
    const int kb = kQnetChunk * c + 4 * half;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const qnet_f32x16& acc = t == 0 ? acc0 : acc1;
      const bool min_ = m0 + 32 * t + l31 < m_out;
      float4 v;
      v.x = min_ && kb + 0 < k_in ? acc[4 * q + 0] : 0.0f;
      v.y = min_ && kb + 1 < k_in ? acc[4 * q + 1] : 0.0f;
      v.z = min_ && kb + 2 < k_in ? acc[4 * q + 2] : 0.0f;
      v.w = min_ && kb + 3 < k_in ? acc[4 * q + 3] : 0.0f;
      reinterpret_cast<float4*>(o)[((int64_t)(g * chunks + c) * 2 + t) * 64 + lane] = v;
    }
  }
  if (bias) {                                  // db: even rows (lanes 0..31) + odd rows (lanes 32..63)
    const float o0 = __shfl_down(sb0, 32), o1 = __shfl_down(sb1, 32);
    if (half == 0) {
      float* __restrict__ ob = o + (int64_t)kp * mp + m0;
      ob[l31] = m0 + l31 < m_out ? sb0 + o0 : 0.0f;
      ob[32 + l31] = m0 + 32 + l31 < m_out ? sb1 + o1 : 0.0f;
    }
  }
}

// ble_wgrad_reduce_kernel per member (blockIdx.y = p): grad_p[e] = partial_p[0][e] + partial_p[1][e] + ... in slab order
__global__ __launch_bounds__(256) void ble_wgrad_reduce_grouped_kernel(const float* __restrict__ partial, int slabs, int64_t stride,
                                                                       int64_t n, float* __restrict__ grad, int64_t member_stride) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t p = blockIdx.y;
  const float* __restrict__ part = partial + p * slabs * stride;
  float s = part[e];
  for (int k = 1; k < slabs; ++k) s += part[k * stride + e];
  grad[p * member_stride + e] = s;
}

// ble_qnet_dgrad_kernel for a population, with ble_qnet_dense_grouped_kernel's tile coordinate (member p, row tile of the member, column
// group g; g fastest): a wave's 32 rows lie inside one member, rows past the member's end load the member's last row and store
// nothing, member p reads wt + p transposed_stride.
__global__ __launch_bounds__(kQnetBlock) void ble_qnet_dgrad_grouped_kernel(const float* __restrict__ dy, int64_t ld, int kp,
                                                                            const float* __restrict__ wt, int64_t transposed_stride,
                                                                            const float* __restrict__ xin, float* __restrict__ dx,
                                                                            int groups, int64_t rows_per_member,
                                                                            int64_t tiles_per_member) {
  const int lane = (int)(threadIdx.x & 63);
  const int64_t tile = blockIdx.x;
  const int g = (int)(tile % groups);
  const int64_t rt = tile / groups;
  const int64_t p = rt / tiles_per_member;
  const int64_t r0 = (rt % tiles_per_member) * kQnetRows + (threadIdx.x >> 6) * 32;      // the wave's first row, inside member p
  if (r0 >= rows_per_member) return;
  const int half = lane >> 5;
  const int64_t base = p * rows_per_member;
  const int64_t row = base + min(r0 + (lane & 31), rows_per_member - 1);
  const float* __restrict__ xr = dy + row * ld;
  const float4* __restrict__ wg = reinterpret_cast<const float4*>(wt + p * transposed_stride + (int64_t)g * kp * kQnetCols) + lane;
  const int chunks = kp / kQnetChunk;
  qnet_f32x16 acc0, acc1;
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
  float4 a = qnet_load_a<false>(xr, 4 * half, 0);
  float4 b0 = wg[0], b1 = wg[64];
  for (int c = 0; c < chunks; ++c) {
    const int cn = c + 1 < chunks ? c + 1 : c;
    const float4 an = qnet_load_a<false>(xr, cn * kQnetChunk + 4 * half, 0);
    const float4 b0n = wg[(int64_t)cn * 128], b1n = wg[(int64_t)cn * 128 + 64];
    qnet_mfma4(a, b0, b1, acc0, acc1);
    a = an; b0 = b0n; b1 = b1n;
  }
  const int col = g * kQnetCols + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t rl = r0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (rl < rows_per_member) {
      const int64_t rr = base + rl;
      dx[rr * ld + col] = xin[rr * ld + col] > 0.0f ? acc0[r] : 0.0f;
      dx[rr * ld + col + 32] = xin[rr * ld + col + 32] > 0.0f ? acc1[r] : 0.0f;
    }
  }
}

// ble_adam_kernel for a population (blockIdx.y = p): member p's image, gradient and moments at + p member_stride, its weights_t at
// + p transposed_stride, its learning rate lr_of[p].  corr is shared: one Adam step counter serves the whole population (the members
// update in lockstep).
__global__ __launch_bounds__(kAdamBlock) void ble_adam_grouped_kernel(float* __restrict__ w, float* __restrict__ wt,
                                                                      const float* __restrict__ grad, float* __restrict__ mom,
                                                                      float* __restrict__ vel, const float* __restrict__ corr,
                                                                      const float* __restrict__ lr_of, int64_t member_stride,
                                                                      int64_t transposed_stride, float b1, float omb1, float b2,
                                                                      float omb2, float eps, TrainDims dims) {
  const int64_t e = (int64_t)blockIdx.x * kAdamBlock + threadIdx.x;
  if (e >= dims.offset[dims.layers]) return;
  const int64_t p = blockIdx.y;
  const int64_t at = p * member_stride + e;
  const float lr = lr_of[p];
  const float g = grad[at];
  const float gg = g * g;
  const float m = omb1 * g + b1 * mom[at];
  const float v = omb2 * gg + b2 * vel[at];
  mom[at] = m;
  vel[at] = v;
  const float mh = m / corr[0], vh = v / corr[1];
  const float step = lr * (mh / (sqrtf(vh) + eps));
  const float nw = w[at] - step;
  w[at] = nw;
  mirror_weight_t(wt + p * transposed_stride, e, nw, dims);
}

}  // namespace ble
