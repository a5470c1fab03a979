// Fused loss kernels. Each produces the gradient w.r.t. the final
// layer's PRE-activation in one pass (log-softmax+NLL and sigmoid+BCE
// use their combined analytic forms), plus an optional per-node loss
// value (for the train-loss EMA metric) — no autograd, no separate
// softmax/log/clamp launches. Loss semantics follow the reference's
// problem layer: NLLLoss on log-softmax outputs (reference
// problems/dist_mnist_problem.py:65-98), BCELoss on sigmoid outputs
// and MSE/L1 regression (dist_dense_problem.py / experiments'
// make_loss choices).

#include "common.h"

namespace losses {

// log-softmax over rows: logp[m, c] = z[m, c] - logsumexp(z[m, :]).
// C is small (10 for MNIST); one thread per row.
template <typename T>
__global__ void logsoftmax_k(const T* __restrict__ Z, T* __restrict__ P,
                             long M, int C) {
  for (long m = blockIdx.x * 256L + threadIdx.x; m < M;
       m += (long)gridDim.x * 256L) {
    const T* z = Z + m * C;
    T* p = P + m * C;
    T mx = z[0];
    for (int c = 1; c < C; ++c) mx = z[c] > mx ? z[c] : mx;
    T s = T(0);
    for (int c = 0; c < C; ++c) s += ::exp(z[c] - mx);
    const T lse = mx + ::log(s);
    for (int c = 0; c < C; ++c) p[c] = z[c] - lse;
  }
}

// NLL backward through log-softmax: dZ = (exp(logp) - onehot(y)) * w,
// w = loss_scale / B (mean reduction per node, loss_scale folds the
// DiNNO pred-loss coefficient). loss[l] accumulates -mean logp[y].
template <typename T>
__global__ void nll_bwd_k(
    const T* __restrict__ logp, const long* __restrict__ y,
    T* __restrict__ dZ, T* __restrict__ loss,  // loss may be null, [L]
    long M, int C, int B, T loss_scale) {
  const T w = loss_scale / T(B);
  for (long m = blockIdx.x * 256L + threadIdx.x; m < M;
       m += (long)gridDim.x * 256L) {
    const T* p = logp + m * C;
    T* g = dZ + m * C;
    const int t = (int)y[m];
    for (int c = 0; c < C; ++c) {
      g[c] = (::exp(p[c]) - (c == t ? T(1) : T(0))) * w;
    }
    if (loss != nullptr) {
      atomicAdd(&loss[m / B], -p[t] / T(B));
    }
  }
}

// sigmoid+BCE combined backward (final density layer, O == 1):
// p = sigmoid(z) is the layer's stored output; dZ = (p - t)/B directly
// (the classic cancellation), loss[l] += BCE/B with clamped logs.
template <typename T>
__global__ void bce_bwd_k(
    const T* __restrict__ p, const T* __restrict__ tgt,
    T* __restrict__ dZ, T* __restrict__ loss, long M, int B,
    T loss_scale) {
  const T w = loss_scale / T(B);
  const T eps = T(1e-12);
  for (long m = blockIdx.x * 256L + threadIdx.x; m < M;
       m += (long)gridDim.x * 256L) {
    const T pm = p[m], t = tgt[m];
    dZ[m] = (pm - t) * w;
    if (loss != nullptr) {
      const T lp = ::log(pm > eps ? pm : eps);
      const T lq = ::log((T(1) - pm) > eps ? (T(1) - pm) : eps);
      atomicAdd(&loss[m / B], -(t * lp + (T(1) - t) * lq) / T(B));
    }
  }
}

// MSE / L1 backward w.r.t. the final ACTIVATION output (caller chains
// act_grad for the sigmoid). mode 0 = MSE, 1 = L1.
template <typename T, int MODE>
__global__ void regression_bwd_k(
    const T* __restrict__ yhat, const T* __restrict__ tgt,
    T* __restrict__ dY, T* __restrict__ loss, long M, int B,
    T loss_scale) {
  const T w = loss_scale / T(B);
  for (long m = blockIdx.x * 256L + threadIdx.x; m < M;
       m += (long)gridDim.x * 256L) {
    const T d = yhat[m] - tgt[m];
    if (MODE == 0) {
      dY[m] = T(2) * d * w;
      if (loss != nullptr) atomicAdd(&loss[m / B], d * d / T(B));
    } else {
      dY[m] = (d > T(0) ? w : (d < T(0) ? -w : T(0)));
      if (loss != nullptr) {
        atomicAdd(&loss[m / B], (d > T(0) ? d : -d) / T(B));
      }
    }
  }
}

// Fully fused classification backward: from the LOGITS, compute the
// row log-sum-exp, gather the target label from the resident dataset
// (via the index stream + offset — no separate target-gather kernel,
// no materialized log-probs in the training path), and write
// dZ = (softmax - onehot) * loss_scale / B. Offset comes from either
// the literal idx_off or slot `pit` of offs_dev (hipGraph mode).
template <typename T>
__global__ void nll_fused_k(
    const T* __restrict__ Z, const long* __restrict__ Y_all,
    const long* __restrict__ idx, T* __restrict__ dZ,
    T* __restrict__ loss,  // may be null, [L]
    const long* __restrict__ offs_dev, int pit,
    long maxlen, long idx_stride, long idx_off,
    long M, int C, int B, T loss_scale) {
  const T w = loss_scale / T(B);
  const long off = offs_dev ? offs_dev[pit] : idx_off;
  for (long m = blockIdx.x * 256L + threadIdx.x; m < M;
       m += (long)gridDim.x * 256L) {
    const long l = m / B;
    const long b = m - l * B;
    const long src = idx[l * idx_stride + off + b];
    const int t = (int)Y_all[l * maxlen + src];

    const T* z = Z + m * C;
    T* g = dZ + m * C;
    T mx = z[0];
    for (int c = 1; c < C; ++c) mx = z[c] > mx ? z[c] : mx;
    T sum = T(0);
    for (int c = 0; c < C; ++c) sum += ::exp(z[c] - mx);
    const T lse = mx + ::log(sum);
    for (int c = 0; c < C; ++c) {
      g[c] = (::exp(z[c] - lse) - (c == t ? T(1) : T(0))) * w;
    }
    if (loss != nullptr) {
      atomicAdd(&loss[l], -(z[t] - lse) / T(B));
    }
  }
}

// PPO clipped-surrogate + critic-MSE backward for a fixed-covariance
// Gaussian policy (covariance = cov * I), all nodes in one launch.
// Node l owns rows [l*B, (l+1)*B); mean reduction per node. Per row:
//   logp  = -0.5 * |a - mu|^2 / cov - logc,  logc = 0.5*A*log(2*pi*cov)
//   r     = exp(logp - old_logp)            (no eps, no exponent clamp:
//                                            the torch path has none)
//   actor = -min(r*adv, clamp(r, lo, hi)*adv),  critic = (v - rtg)^2
//   dmu_j = -loss_scale * g * r * (a_j - mu_j) / cov / B
//   dv    = loss_scale * critic_coef * 2 * (v - rtg) / B
// g is torch's subgradient of the min/clamp pair (minimum splits ties,
// clamp passes the gradient at its bounds): adv inside [lo, hi] and on
// the side where the unclipped term is the smaller one, else 0.
// lo/hi arrive already rounded to T, as torch rounds clamp's bounds.
// loss (may be null, [L, 2], zeroed by the caller) accumulates the
// per-node means (actor, critic), unscaled. A wave whose 64 rows all
// belong to one node shuffle-reduces and issues one atomic per term;
// a wave that straddles a node boundary or the end adds per lane.
// One thread per row; the row lives in registers (A <= PPO_MAX_A, the
// guarded full unroll keeps d[] out of scratch).
constexpr int PPO_MAX_A = 16;

template <typename T>
__global__ void ppo_loss_bwd_k(
    const T* __restrict__ mean, const T* __restrict__ acts,
    const T* __restrict__ old_logp, const T* __restrict__ adv,
    const T* __restrict__ v, const T* __restrict__ rtgs,
    T* __restrict__ dmean, T* __restrict__ dv,
    T* __restrict__ loss,  // may be null, [L, 2]
    long M, int A, int B, T inv_cov, T logc, T lo, T hi,
    T critic_coef, T loss_scale) {
  const T invB = T(1) / T(B);
  const int lane = threadIdx.x & 63;
  // wave-uniform trip count: every lane of a wave stays in the loop so
  // the shuffles below always see 64 active lanes
  for (long base = blockIdx.x * 256L + (threadIdx.x - lane); base < M;
       base += (long)gridDim.x * 256L) {
    const long m = base + lane;
    const bool valid = m < M;
    T la = T(0), lc = T(0);
    if (valid) {
      const T* mu = mean + m * A;
      const T* a = acts + m * A;
      T d[PPO_MAX_A];
      T sq = T(0);
#pragma unroll
      for (int j = 0; j < PPO_MAX_A; ++j) {
        d[j] = T(0);
        if (j < A) {
          d[j] = a[j] - mu[j];
          sq += d[j] * d[j];
        }
      }
      const T logp = T(-0.5) * sq * inv_cov - logc;
      const T r = ::exp(logp - old_logp[m]);
      const T ad = adv[m];
      const T rc = r < lo ? lo : (r > hi ? hi : r);
      const T s1 = r * ad, s2 = rc * ad;
      la = -(s1 < s2 ? s1 : s2) * invB;
      const bool pass = (r >= lo && r <= hi) ||
                        (ad > T(0) && r < lo) || (ad < T(0) && r > hi);
      const T g = pass ? ad : T(0);
      const T cm = -loss_scale * g * r * inv_cov * invB;
      T* dm = dmean + m * A;
#pragma unroll
      for (int j = 0; j < PPO_MAX_A; ++j) {
        if (j < A) dm[j] = cm * d[j];
      }
      const T e = v[m] - rtgs[m];
      lc = e * e * invB;
      dv[m] = loss_scale * critic_coef * T(2) * e * invB;
    }
    if (loss != nullptr) {
      const bool one_node =
          base + 63 < M && base / B == (base + 63) / B;
      if (one_node) {
        la = wave_reduce_sum(la);
        lc = wave_reduce_sum(lc);
        if (lane == 0) {
          atomicAdd(&loss[2 * (base / B)], la);
          atomicAdd(&loss[2 * (base / B) + 1], lc);
        }
      } else if (valid) {
        atomicAdd(&loss[2 * (m / B)], la);
        atomicAdd(&loss[2 * (m / B) + 1], lc);
      }
    }
  }
}

}  // namespace losses
