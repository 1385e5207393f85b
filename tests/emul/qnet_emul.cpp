// The fma-chain twin of the Q-network kernels for tests/test_qnet_emul_host.py and tests/test_gpu_qnet_bits.py.  TEST
// TOOLING: never loaded by the package.
//
// Written from the documented summation order, not from the kernels: it includes no header of csrc/ and knows nothing of tiles, lanes,
// waves or the packed image.  It works on logical arrays -- W[k][m] row-major and bias[m], as ble_qnet_unpack_f32 hands them out --
// and on activation rows.  One v_mfma_f32_32x32x2_f32 step is fma(a_k1, b_k1, fma(a_k0, b_k0, C)), subnormals kept, so every output
// element of a Dense layer, of dX and of dW is one std::fmaf chain, and the twin walks that chain term by term, padded terms included.
// std::fmaf is correctly rounded with or without a hardware fma; -ffp-contract=off keeps every other statement one rounding.
//
// `order` names a MUTANT of the chain for the host test's sensitivity condition; order 0 is the contract:
//   1  ascending k (0, 1, 2, ... instead of 0, 4, 1, 5, 2, 6, 3, 7 within a chunk); the head: the atoms summed in descending order;
//   2  the halves swapped (8c + 4 + j before 8c + j; dW: the odd row of a step before the even one);
//   3  product and sum rounded apart (acc + a * w, two roundings);
//   4  one input column (`skip`) left out of a layer;
//   5  dW: within an 8-row step the even rows before the odd rows; db: ONE ascending chain instead of even-sum + odd-sum (swapping the
//      two partial sums would change nothing: a + b == b + a);
//   6  dW, db: the slabs reduced in descending order.
//
// Left out, because the device's bits are not derivable from the source there:
//   * Adam: `omb1 * g + b1 * mom[e]` is one expression under -ffp-contract=on and the compiler chooses which product fuses;
//   * the PPO, cloning and soft-cloning heads: expf / logf are the device library's;
//   * the replay return: the device's pow.
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

constexpr int kChunk = 8, kCols = 64, kStepRows = 8;

int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// One term of `cols` independent chains that share the A operand: acc[c] = fma(a, w[c], acc[c]).
void term(int order, float a, const float* w, float* acc, int cols) {
  if (order == 3) {
    for (int c = 0; c < cols; ++c) {
      const float p = a * w[c];
      acc[c] = acc[c] + p;
    }
  } else {
    for (int c = 0; c < cols; ++c) acc[c] = std::fmaf(a, w[c], acc[c]);
  }
}

// The k order of one chunk: the contract pairs k = 8c + j (first) with 8c + 4 + j (second) in step j.
void chunk_order(int order, int seq[kChunk]) {
  for (int j = 0; j < 4; ++j) {
    if (order == 1) { seq[2 * j] = 2 * j; seq[2 * j + 1] = 2 * j + 1; }
    else if (order == 2) { seq[2 * j] = 4 + j; seq[2 * j + 1] = j; }
    else { seq[2 * j] = j; seq[2 * j + 1] = 4 + j; }
  }
}

// acc[0 .. mp) = the chains over k = 0 .. kp - 1 of a(k) w[k][0 .. mp) in the chain's order; w: kp rows of mp floats, zero outside W.
template <class A>
void walk(int kp, int mp, int order, int skip, A&& a, const float* w, float* acc) {
  int seq[kChunk];
  chunk_order(order, seq);
  for (int c = 0; c < mp; ++c) acc[c] = 0.0f;
  for (int ch = 0; ch < kp / kChunk; ++ch)
    for (int i = 0; i < kChunk; ++i) {
      const int k = kChunk * ch + seq[i];
      if (order == 4 && k == skip) continue;
      term(order, a(k), w + (int64_t)k * mp, acc, mp);
    }
}

}  // namespace

extern "C" {

// One Dense layer: y [n][mp], mp = round64(m), from x [n] rows of stride ldx.  first != 0: the rows are observations, columns >= k are
// not read (a = 0.0 there); otherwise the rows are the previous layer's padded output and columns k .. kp - 1 are read as they are.
void emul_qnet_dense(const float* x, int64_t ldx, int64_t n, int k, int m, const float* w, const float* bias, int first, int relu,
                     int order, int skip, float* y) {
  const int kp = (int)round_up(k, kChunk), mp = (int)round_up(m, kCols);
  std::vector<float> wp((size_t)kp * mp, 0.0f), acc(mp);      // W with its zero padding: the padded terms are walked too
  for (int kk = 0; kk < k; ++kk)
    for (int c = 0; c < m; ++c) wp[(size_t)kk * mp + c] = w[(int64_t)kk * m + c];
  for (int64_t r = 0; r < n; ++r) {
    const float* xr = x + r * ldx;
    walk(kp, mp, order, skip, [&](int kk) { return kk < k || !first ? xr[kk] : 0.0f; }, wp.data(), acc.data());
    for (int c = 0; c < mp; ++c) {
      float v = acc[c] + (c < m ? bias[c] : 0.0f);
      if (relu) v = v < 0.0f ? 0.0f : v;
      y[r * mp + c] = v;
    }
  }
}

// q [n][actions] = (the atoms' sum, ascending from 0.0f) / (float)atoms; action = the first maximum, or the first NaN.
void emul_qnet_head(const float* logits, int64_t ld, int64_t n, int actions, int atoms, int order, float* q, uint8_t* action) {
  for (int64_t i = 0; i < n; ++i) {
    int best = 0;
    float qb = 0.0f;
    for (int a = 0; a < actions; ++a) {
      float s = 0.0f;
      for (int j = 0; j < atoms; ++j) s += logits[i * ld + a * atoms + (order == 1 ? atoms - 1 - j : j)];
      const float qa = s / (float)atoms;
      q[i * actions + a] = qa;
      const bool qb_nan = qb != qb, qa_nan = qa != qa;
      if (a == 0 || (!qb_nan && (qa_nan || qa > qb))) { best = a; qb = qa; }
    }
    action[i] = (uint8_t)best;
  }
}

// dX [n][round64(k)] of a layer l >= 1 with k inputs, m outputs: Dense's walk over W^T (K' = m, no bias) on the dY rows (stride ldy,
// columns m .. round8(m) - 1 read as they are), then 1{X > 0} from the layer's padded input X (stride ldx).
void emul_qnet_dgrad(const float* dy, int64_t ldy, int64_t n, int k, int m, const float* w, const float* xin, int64_t ldx, int order,
                     int skip, float* dx) {
  const int kpt = (int)round_up(m, kChunk), mpt = (int)round_up(k, kCols);
  std::vector<float> wt((size_t)kpt * mpt, 0.0f), acc(mpt);   // W^T with its zero padding
  for (int kk = 0; kk < k; ++kk)
    for (int c = 0; c < m; ++c) wt[(size_t)c * mpt + kk] = w[(int64_t)kk * m + c];
  for (int64_t r = 0; r < n; ++r) {
    walk(kpt, mpt, order, skip, [&](int mm) { return dy[r * ldy + mm]; }, wt.data(), acc.data());
    for (int c = 0; c < mpt; ++c) dx[r * mpt + c] = xin[r * ldx + c] > 0.0f ? acc[c] : 0.0f;
  }
}

// dW [k][m] and db [m] of one layer over batch rows 0 .. batch - 1 in `slabs` slabs of slab_rows rows: per slab [rb, re) one chain over
// rows rb, rb + 1, ... up to rb + 8 ceil((re - rb) / 8), rows >= re contributing fmaf(0, 0, acc); db = (even-offset rows' sum) +
// (odd-offset rows' sum), each from 0.0f and padded alike; then s = p[0]; s += p[1]; ... over the slabs.
void emul_qnet_wgrad(const float* x, int64_t ldx, int k, const float* dy, int64_t ldy, int m, int64_t batch, int slabs, int64_t slab_rows,
                     int order, float* dw, float* db) {
  int seq[kStepRows];
  for (int s = 0; s < 4; ++s) {
    if (order == 2) { seq[2 * s] = 2 * s + 1; seq[2 * s + 1] = 2 * s; }
    else if (order == 5) { seq[s] = 2 * s; seq[4 + s] = 2 * s + 1; }
    else { seq[2 * s] = 2 * s; seq[2 * s + 1] = 2 * s + 1; }
  }
  const size_t kern = (size_t)k * m, blk = kern + m;           // one slab's partial sums: dW then db
  std::vector<float> part((size_t)slabs * blk, 0.0f), zeros(m, 0.0f), even(m), odd(m), all(m);
  for (int z = 0; z < slabs; ++z) {
    const int64_t rb = (int64_t)z * slab_rows, re = rb + slab_rows < batch ? rb + slab_rows : batch;
    float* p = part.data() + (size_t)z * blk;
    for (int c = 0; c < m; ++c) even[c] = odd[c] = all[c] = 0.0f;
    for (int64_t b = rb; b < re; b += kStepRows) {
      for (int i = 0; i < kStepRows; ++i) {
        const int64_t row = b + seq[i];
        const float* yr = row < re ? dy + row * ldy : zeros.data();
        for (int kk = 0; kk < k; ++kk) term(order, row < re ? x[row * ldx + kk] : 0.0f, yr, p + (size_t)kk * m, m);
      }
      for (int i = 0; i < kStepRows; ++i) {
        const int64_t row = b + i;
        const float* yr = row < re ? dy + row * ldy : zeros.data();
        float* half = i & 1 ? odd.data() : even.data();
        for (int c = 0; c < m; ++c) { half[c] += yr[c]; all[c] += yr[c]; }
      }
    }
    for (int c = 0; c < m; ++c) p[kern + c] = order == 5 ? all[c] : even[c] + odd[c];
  }
  for (size_t e = 0; e < blk; ++e) {
    float s;
    if (order == 6) {
      s = part[(size_t)(slabs - 1) * blk + e];
      for (int z = slabs - 2; z >= 0; --z) s += part[(size_t)z * blk + e];
    } else {
      s = part[e];
      for (int z = 1; z < slabs; ++z) s += part[(size_t)z * blk + e];
    }
    (e < kern ? dw[e] : db[e - kern]) = s;
  }
}

// The quantile Huber loss of one batch (Dopamine's quantile_agent.train), every statement one rounding, sums in ascending j then i:
//   a* = the head's rule on the target logits, T_j = ret + (discount z'[a*, j]), u = T_j - theta_i, w = |tau_i - 1{u < 0}|,
//   tau_i = ((float)i + 0.5f) / (float)atoms, H = |u| <= kappa ? (0.5f u) u : kappa (|u| - 0.5f kappa), cl = clip(u, -kappa, kappa),
//   rho_i = (sum_j w H) / atoms, loss = sum_i rho_i, dlogits[action, i] = -(((sum_j w cl) / atoms) / batch), zero elsewhere up to ld.
// `|u| - 0.5f kappa` is the one expression the device build may contract; 0.5f kappa is exact for any normal kappa, so fused or not
// it is one rounding of the same real number.  An action >= actions zeroes the row and sets *flag.
void emul_qr_loss(const float* logits, const float* tlogits, int64_t ld, int actions, int atoms, const float* ret, const float* discount,
                  const uint8_t* action, float kappa, int64_t batch, float* targets, float* dlogits, float* loss, uint8_t* best_out,
                  int* flag) {
  std::vector<float> q(actions);
  for (int64_t b = 0; b < batch; ++b) {
    uint8_t best;
    emul_qnet_head(tlogits + b * ld, ld, 1, actions, atoms, 0, q.data(), &best);
    best_out[b] = best;
    const float* zt = tlogits + b * ld;
    const float* z = logits + b * ld;
    float* t = targets + b * atoms;
    for (int j = 0; j < atoms; ++j) {
      const float p = discount[b] * zt[best * atoms + j];
      t[j] = ret[b] + p;
    }
    float* dl = dlogits + b * ld;
    for (int64_t c = 0; c < ld; ++c) dl[c] = 0.0f;
    const int act = action[b];
    const bool valid = act < actions;
    if (!valid) *flag = 1;
    float l = 0.0f;
    for (int i = 0; i < atoms; ++i) {
      const float theta = valid ? z[act * atoms + i] : 0.0f;
      const float tau = ((float)i + 0.5f) / (float)atoms;
      float rho = 0.0f, grad = 0.0f;
      for (int j = 0; j < atoms; ++j) {
        const float u = t[j] - theta;
        const float w = std::fabs(tau - (u < 0.0f ? 1.0f : 0.0f));
        const float au = std::fabs(u);
        const float hk = 0.5f * kappa;
        const float hu = 0.5f * u;
        const float d = au - hk;
        const float h = au <= kappa ? hu * u : kappa * d;
        const float cl = au <= kappa ? u : (u < 0.0f ? -kappa : kappa);
        const float wh = w * h, wc = w * cl;
        rho += wh;
        grad += wc;
      }
      const float ri = valid ? rho / (float)atoms : 0.0f;
      l += ri;
      if (valid) {
        const float g = grad / (float)atoms;
        dl[act * atoms + i] = -(g / (float)batch);
      }
    }
    loss[b] = l;
  }
}

// DQN's TD losses on one-atom logits (Dopamine's dqn_agent.train): a* = the head's rule on the target network's row, T = ret +
// (discount q'[a*]), u = T - q[action]; kind 0 (mse): L = u u, dL/dq = -((2 u) / batch); kind 1 (huber): L = |u| <= 1 ? (0.5f u) u :
// |u| - 0.5f, dL/dq = -(clip(u, -1, 1) / batch).  An action >= actions zeroes the row and sets *flag; targets[b] = T either way.
void emul_td_loss(int kind, const float* logits, const float* other, int64_t ld, int actions, const float* ret, const float* discount,
                  const uint8_t* action, int64_t batch, float* targets, float* dlogits, float* loss, int* flag) {
  for (int64_t b = 0; b < batch; ++b) {
    const float* z = logits + b * ld;
    const float* zo = other + b * ld;
    float* dl = dlogits + b * ld;
    for (int64_t c = 0; c < ld; ++c) dl[c] = 0.0f;
    const int act = action[b];
    const bool valid = act < actions;
    if (!valid) *flag = 1;
    int best = 0;
    float qb = 0.0f;
    for (int a = 0; a < actions; ++a) {
      const float qa = zo[a];
      const bool qb_nan = qb != qb, qa_nan = qa != qa;
      if (a == 0 || (!qb_nan && (qa_nan || qa > qb))) { best = a; qb = qa; }
    }
    const float p = discount[b] * zo[best];
    const float t = ret[b] + p;
    targets[b] = t;
    float l = 0.0f;
    if (valid) {
      const float u = t - z[act];
      const float fb = (float)batch;
      if (kind == 0) {
        const float u2 = 2.0f * u;
        l = u * u;
        dl[act] = -(u2 / fb);
      } else {
        const float au = std::fabs(u);
        const float hu = 0.5f * u;
        l = au <= 1.0f ? hu * u : au - 0.5f;
        const float cl = au <= 1.0f ? u : (u < 0.0f ? -1.0f : 1.0f);
        dl[act] = -(cl / fb);
      }
    }
    loss[b] = l;
  }
}

}  // extern "C"
