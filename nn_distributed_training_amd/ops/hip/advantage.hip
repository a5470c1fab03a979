// GAE(lambda) advantages of the multi-agent PPO tree (rl/advantages.py),
// all nodes in ONE launch: one block per node turns the node's critic
// values and rewards into the TD residuals, the per-episode reverse
// recurrence, the node's mean / unbiased std and the normalised
// advantages, plus the lambda-returns.
//
// Node l owns rows [l*M, (l+1)*M) in the layout of rl/device_rollout.py:
// uniform episodes of ep_len steps, the last one cut at M. A step s is
// the last of its episode when (s+1) % ep_len == 0 or s+1 == M. By
// default an episode's end is terminal (no bootstrap); with v_last
// ([L*E], E = ceil(M / ep_len), row l*E + e: the critic's value of the
// observation after episode e's last step) the end is a truncation and
// the return goes on with gamma * v_last. With k_s = gamma*lambda, or 0
// at an episode's last step,
//   delta_s = r_s + gamma * V_{s+1} - V_s             s not last
//   delta_s = r_s + gamma * v_last[l*E + e] - V_s     s last (0 if null)
//   A_s     = delta_s + k_s * A_{s+1}
//   ret_s   = A_s + V_s
//   adv_s   = (A_s - mean A) / (std A + 1e-10)       std over M-1
// so the whole row is ONE linear recurrence whose coefficient is exactly
// 0 across an episode boundary. It is split over the block: thread j owns
// the chunk [j*C, (j+1)*C), C = ceil(M / BLOCK), and
//   1  scans its chunk backwards from 0, which leaves the affine map
//      x -> a + p*x from the value after the chunk to the chunk's first
//      value (p = product of the chunk's k_s);
//   2  a Kogge-Stone suffix scan over the wave composes the maps, the
//      waves' totals go through LDS and every wave folds the later
//      waves' totals serially: each thread learns the value after its
//      chunk;
//   3  scans its chunk again from that value and keeps A_s.
// The serial length is C, not ep_len or M. All arithmetic is double for
// either T, the order of every sum is fixed (no atomics), the variance is
// two-pass; T appears in the loads of v and v_last and the final stores
// only.
//
// A_s stays in LDS for M <= LDS_MAX_M; above, `work` is a [L*M] double
// row in global memory (the adv output itself when T is double), so M is
// not bounded by the LDS.

#include "common.h"

namespace advantage {

constexpr int BLOCK = 256;
constexpr int NWAVE = BLOCK / WAVE;
constexpr int LDS_MAX_M = 16384;  // 128 KiB of doubles

// sum over the block in a fixed order, the same value in every thread
DEV_INLINE double block_sum_all(double x, double* s_part) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  x = wave_reduce_sum(x);
  __syncthreads();  // s_part may still be read from the call before
  if (lane == 0) s_part[wid] = x;
  __syncthreads();
  double tot = 0.0;
#pragma unroll
  for (int w = 0; w < NWAVE; ++w) tot += s_part[w];
  return tot;
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void ppo_gae_k(
    const T* __restrict__ v,            // [L*M]
    const double* __restrict__ rews,    // [M] (stride 0) or [L*M]
    long rew_stride,
    T* adv,                             // [L*M]
    T* ret,                             // [L*M], may be null
    double* work,                       // [L*M] or null: A_s in LDS
    int M, int ep_len, double gamma, double c,
    const T* __restrict__ v_last) {     // [L*E] or null: terminal ends
  __shared__ double s_a[NWAVE], s_p[NWAVE], s_part[NWAVE];
  extern __shared__ __align__(16) unsigned char gae_raw[];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const long row = (long)blockIdx.x * M;
  const T* vl = v + row;
  const double* rl = rews + (long)blockIdx.x * rew_stride;
  double* A = work != nullptr ? work + row
                              : reinterpret_cast<double*>(gae_raw);
  const int E = (M + ep_len - 1) / ep_len;
  const T* vend =
      v_last != nullptr ? v_last + (long)blockIdx.x * E : nullptr;

  // TD residuals, one coalesced sweep
  for (int s = tid; s < M; s += BLOCK) {
    const bool last = s + 1 == M || (s + 1) % ep_len == 0;
    const double vn =
        !last ? (double)vl[s + 1]
              : vend != nullptr ? (double)vend[s / ep_len] : 0.0;
    A[s] = rl[s] + gamma * vn - (double)vl[s];
  }
  __syncthreads();

  // 1: the chunk's map (a, p); an empty chunk is the identity (0, 1)
  const int C = (M + BLOCK - 1) / BLOCK;
  const long b0 = (long)tid * C;
  const int b = b0 < M ? (int)b0 : M;
  const int e = b0 + C < M ? (int)(b0 + C) : M;
  // t_end: position in its episode of the step after the chunk
  const int t_end = e % ep_len;
  double a = 0.0, p = 1.0;
  {
    int t = t_end;
    for (int s = e - 1; s >= b; --s) {
      const double k = (t == 0 || s + 1 == M) ? 0.0 : c;
      a = A[s] + k * a;
      p *= k;
      t = t == 0 ? ep_len - 1 : t - 1;
    }
  }
  // 2: suffix scan of the maps over the wave: lane j ends with the
  // composition of the chunks of lanes j..63
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const double a2 = __shfl_down(a, off, WAVE);
    const double p2 = __shfl_down(p, off, WAVE);
    if (lane + off < WAVE) {
      a += p * a2;
      p *= p2;
    }
  }
  if (lane == 0) {
    s_a[wid] = a;
    s_p[wid] = p;
  }
  __syncthreads();
  // value at the first step of the wave after this one
  double carry = 0.0;
  for (int w = NWAVE - 1; w > wid; --w) carry = s_a[w] + s_p[w] * carry;
  // the first value of lane j's chunk, then of its right neighbour's
  const double first = a + p * carry;
  double x = __shfl_down(first, 1, WAVE);
  if (lane == WAVE - 1) x = carry;
  // 3: the chunk again, from the value after it
  {
    int t = t_end;
    for (int s = e - 1; s >= b; --s) {
      const double k = (t == 0 || s + 1 == M) ? 0.0 : c;
      x = A[s] + k * x;
      A[s] = x;
      t = t == 0 ? ep_len - 1 : t - 1;
    }
  }
  __syncthreads();

  // mean, then the sum of squares about it
  double sum = 0.0;
  for (int s = tid; s < M; s += BLOCK) sum += A[s];
  const double mean = block_sum_all(sum, s_part) / (double)M;
  double sq = 0.0;
  for (int s = tid; s < M; s += BLOCK) {
    const double d = A[s] - mean;
    sq += d * d;
  }
  const double sd =
      ::sqrt(block_sum_all(sq, s_part) / (double)(M - 1));
  const double den = sd + 1e-10;

  // each thread reads A[s] before it writes adv[s]: `work` may be adv
  for (int s = tid; s < M; s += BLOCK) {
    const double As = A[s];
    if (ret != nullptr) ret[row + s] = (T)(As + (double)vl[s]);
    adv[row + s] = (T)((As - mean) / den);
  }
}

}  // namespace advantage
