// Decentralized-optimizer elementwise kernels, batched over the L node
// replicas of one rank (the reference's per-node, per-parameter Python
// loops — optimizers/dsgd.py:37-58, dinno.py:119-125, dsgt.py:58-105 —
// each become ONE launch here).
//
// Layout: parameter stacks are [L, n] row-major. Neighbor vectors live in
// a "table" [R, n] (R = L local snapshot rows + received remote rows);
// per-node neighbor lists are CSR int32 (offsets [L+1], indices into the
// table). All kernels are memory-bound grid-stride loops — the design
// goal is one pass over HBM per algorithm step with everything fused.

#include "common.h"

namespace ew {

constexpr int BLOCK = 256;

// Table rows: r < L -> local stack row, else -> received remote row.
// Avoids ever materializing a concatenated table (the local stack is
// read in place; remote rows land where irecv wrote them).
template <typename T>
DEV_INLINE const T* table_row(const T* local, const T* remote, long L,
                              long n, int r) {
  return r < L ? local + (long)r * n : remote + ((long)r - L) * n;
}

// ---------------------------------------------------------------------
// DiNNO round prologue (reference optimizers/dinno.py:119-124, fused):
//   S_i      = sum_{j in N(i)} th_j
//   dual_i  += rho * (deg_i * th_i - S_i)
//   s_i      = (deg_i * th_i + S_i) / 2     (= sum_j th_reg_j, the only
//                                            reduction the penalty
//                                            gradient needs)
template <typename T>
__global__ void dinno_dual_threg_k(
    const T* __restrict__ local,   // [L, n] round-start snapshot
    const T* __restrict__ remote,  // [R-L, n] received rows (may be null)
    const int* __restrict__ offs,  // [L+1]
    const int* __restrict__ idx,   // CSR neighbor rows
    T* __restrict__ duals,         // [L, n] in/out
    T* __restrict__ s_out,         // [L, n] out
    T rho, long n, long L) {
  const long total = L * n;
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long l = t / n;
    const long e = t - l * n;
    const int k0 = offs[l], k1 = offs[l + 1];
    T S = T(0);
    for (int k = k0; k < k1; ++k) {
      S += table_row(local, remote, L, n, idx[k])[e];
    }
    const T th = local[l * n + e];
    const T deg = T(k1 - k0);
    duals[t] += rho * (deg * th - S);
    s_out[t] = (deg * th + S) * T(0.5);
  }
}

// ---------------------------------------------------------------------
// Generic weighted row-combine (DSGD mixing, reference dsgd.py:37-46,
// made snapshot-synchronous):  out_l = sum_k w_k * table[idx_k]
// (the caller includes the self row with weight W_ll in the CSR).
template <typename T>
__global__ void mix_rows_k(
    const T* __restrict__ local, const T* __restrict__ remote,
    const int* __restrict__ offs, const int* __restrict__ idx,
    const T* __restrict__ w, T* __restrict__ out, long n, long L) {
  const long total = L * n;
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long l = t / n;
    const long e = t - l * n;
    const int k0 = offs[l], k1 = offs[l + 1];
    T acc = T(0);
    for (int k = k0; k < k1; ++k) {
      acc += w[k] * table_row(local, remote, L, n, idx[k])[e];
    }
    out[t] = acc;
  }
}

// ---------------------------------------------------------------------
// DSGT mixing (reference dsgt.py:58-75, synchronous):
//   p_out_l = sum_k w_k * (p_k - alpha * y_k)
//   y_mix_l = sum_k w_k * y_k
// The table rows bundle [p | y] as [R, 2n] so params and tracker ride
// one exchange (2x comm volume).
template <typename T>
__global__ void dsgt_mix_k(
    const T* __restrict__ p_loc,   // [L, n]
    const T* __restrict__ y_loc,   // [L, n]
    const T* __restrict__ remote,  // [R-L, 2n] bundles [p | y]
    const int* __restrict__ offs, const int* __restrict__ idx,
    const T* __restrict__ w, T* __restrict__ p_out,
    T* __restrict__ y_mix, T alpha, long n, long L) {
  const long total = L * n;
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long l = t / n;
    const long e = t - l * n;
    const int k0 = offs[l], k1 = offs[l + 1];
    T accp = T(0), accy = T(0);
    for (int k = k0; k < k1; ++k) {
      const int r = idx[k];
      T pj, yj;
      if (r < L) {
        pj = p_loc[(long)r * n + e];
        yj = y_loc[(long)r * n + e];
      } else {
        const T* row = remote + ((long)r - L) * (2 * n);
        pj = row[e];
        yj = row[n + e];
      }
      accp += w[k] * pj;
      accy += w[k] * yj;
    }
    p_out[t] = accp - alpha * accy;
    y_mix[t] = accy;
  }
}

// DSGT tracker update (reference dsgt.py:87-105):
//   y = y_mix + g_new - g_old ;  g_old = g_new
template <typename T>
__global__ void dsgt_y_update_k(
    const T* __restrict__ y_mix, const T* __restrict__ g_new,
    T* __restrict__ g_old, T* __restrict__ y, long total) {
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const T gn = g_new[t];
    y[t] = y_mix[t] + gn - g_old[t];
    g_old[t] = gn;
  }
}

// ---------------------------------------------------------------------
// Reduce per-tile gradient slabs [L, P, n] into [L, n] (consumers that
// are not the fused step: DSGD's axpy, DSGT's tracker update).
template <typename T>
__global__ void reduce_parts_k(const T* __restrict__ parts,
                               T* __restrict__ out, int nparts,
                               long n, long L) {
  const long total = L * n;
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long l = t / n;
    const long e = t - l * n;
    T acc = T(0);
    for (int p = 0; p < nparts; ++p) {
      acc += parts[(l * nparts + p) * n + e];
    }
    out[t] = acc;
  }
}

// ---------------------------------------------------------------------
// Fused primal step. The DiNNO penalty gradient is analytic
// (d/dth [ rho * sum_j ||th - th_reg_j||^2 ] = 2 rho (deg th - s), plus
// the dual term from <th, dual>), so it folds into the optimizer update
// and the autograd-visible loss never materializes (reference
// dinno.py:74-91 builds it through torch.cdist + autograd every primal
// iteration).  mode: 0=Adam 1=AdamW 2=SGD (matching dinno.py:55-72);
// with_penalty=false gives the plain local step (DSGD's dsgd.py:49-58).
// first_step: treat the Adam moments as zero without reading them —
// the per-round m/v zero-fill kernels of the non-persistent DiNNO mode
// fold away (reference recreates the Adam optimizer each round,
// dinno.py:57-72).
template <typename T, int MODE, bool WITH_PENALTY>
__global__ void fused_step_k(
    T* __restrict__ theta, T* __restrict__ grad,
    const T* __restrict__ dual,   // null unless WITH_PENALTY
    const T* __restrict__ s,      // null unless WITH_PENALTY
    const int* __restrict__ deg,  // [L], null unless WITH_PENALTY
    T* __restrict__ m, T* __restrict__ v,  // Adam state (null for SGD)
    T rho, T lr, T beta1, T beta2, T eps, T wd, T bc1, T bc2,
    int first_step, int nparts, long n, long L, int zero_grad) {
  const long total = L * n;
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long l = t / n;
    const long e = t - l * n;
    T g;
    if (nparts > 1) {  // per-tile slabs from the fused train step
      g = T(0);
      for (int p = 0; p < nparts; ++p) {
        const long gi = (l * nparts + p) * n + e;
        g += grad[gi];
        if (zero_grad) grad[gi] = T(0);  // next iter's atomics land
                                         // on a clean slate for free
      }
    } else {
      g = grad[t];
      if (zero_grad) grad[t] = T(0);
    }
    // isolated node under a dynamic graph: the golden engine skips the
    // whole primal update (the reference crashes on torch.stack of an
    // empty neighbor list, so "frozen" is this framework's defined
    // behavior) — freeze theta AND the Adam moments to match exactly
    if (WITH_PENALTY && deg[l] == 0) continue;
    T th = theta[t];
    if (WITH_PENALTY) {
      g += dual[t] + T(2) * rho * (T(deg[l]) * th - s[t]);
    }
    if (MODE == 2) {  // SGD
      theta[t] = th - lr * g;
      continue;
    }
    if (MODE == 1) {  // AdamW decoupled weight decay
      th -= lr * wd * th;
    } else if (wd != T(0)) {  // Adam L2
      g += wd * th;
    }
    const T m_prev = first_step ? T(0) : m[t];
    const T v_prev = first_step ? T(0) : v[t];
    const T mt = beta1 * m_prev + (T(1) - beta1) * g;
    const T vt = beta2 * v_prev + (T(1) - beta2) * g * g;
    m[t] = mt;
    v[t] = vt;
    // bc1 = 1-beta1^t, bc2 = 1-beta2^t (host-computed per step)
    theta[t] = th - lr * (mt / bc1) / (::sqrt(vt / bc2) + eps);
  }
}

// ---------------------------------------------------------------------
// The round's dual ascent folded into its first primal step: what
// dinno_dual_threg_k followed by fused_step_k<T, MODE, true> (nparts 1)
// compute, bit for bit, in one launch and without the round trip of
// duals and s through memory.
//
// fused_step_k updates theta in place with a thread per (node, e) and no
// order between them, so a neighbour's theta_j[e] may already be
// overwritten when thread (i, e) wants it. Here a BLOCK owns a strip of
// columns for all L local nodes (blockDim = (columns, L), thread (c, l)
// is node l of column e0 + c): every thread loads its theta into LDS,
// one barrier, and only then does anybody store theta. Nobody else
// touches the strip's columns, and remote rows are read-only. A
// neighbour that is a local row is read from LDS, which a runtime row
// number may index freely; th, the new dual and s stay in registers
// between the two phases. The grid has as many threads as
// fused_step_k's.
constexpr int STEP_DUAL_THREADS = 1024;  // columns * L at the most
constexpr int STEP_DUAL_LMAX = 16;

// a * b + c with the rounding fused_step_k's two Adam moment updates
// have as compiled: one fused multiply-add in fp64, a product and a sum
// in fp32 (the compiler pairs the two fp32 products into one packed
// multiply there). Bit-equality with fused_step_k needs the same here,
// whatever the surrounding code invites the compiler to contract;
// tests/test_step_dual_gpu.py holds the two kernels together.
template <typename T>
DEV_INLINE T step_mul_add(T a, T b, T c) {
#pragma clang fp contract(off)
  if (sizeof(T) == 8) return __builtin_fma(a, b, c);
  return a * b + c;
}

// ---------------------------------------------------------------------
// One element of a DiNNO primal step, written once for fused_step_dual_k
// and for the backward launch that carries the step
// (fused_mnist.hip dw_dx0_conv_bwd_k with STEP on). Three pieces, so a
// caller can put its own work (a barrier, a dot product) between them:
//   step_elem_load   the element's own loads;
//   step_nbr_sum     dinno_dual_threg_k's CSR walk, in its order, the
//                    neighbour's value coming from the caller's accessor
//                    nbr(table_row, q);
//   step_elem_apply  dual and s (DUAL), the penalty gradient, the
//                    SGD/Adam/AdamW update with step_mul_add's rounding,
//                    the isolated-node freeze, and every store.
// DUAL: the step carries the round's dual ascent (duals and s are
// written); otherwise both are read and the math is
// fused_step_k<T, MODE, true>'s at nparts 1. theta_in and theta_out may
// be one buffer (fused_step_dual_k, whose barrier orders the accesses)
// or two: then a frozen element is copied across.
template <typename T>
struct step_args_t {
  const T* theta_in;   // [L, n]
  T* theta_out;        // [L, n]
  const T* remote;     // [R-L, n] received rows (may be null)
  const int* offs;     // [L+1]
  const int* idx;      // CSR neighbor rows
  const int* deg;      // [L]
  T* duals;            // [L, n]
  T* s;                // [L, n]
  T* m;                // Adam state (null for SGD)
  T* v;
  T rho, lr, beta1, beta2, eps, wd, bc1, bc2;
  long n;
  int L;
};

template <typename T>
struct step_ld_t {
  T th, du, sv, m_prev, v_prev;
};

// load_mv false: the Adam moments count as zero and are not read
template <typename T, bool DUAL>
DEV_INLINE step_ld_t<T> step_elem_load(const step_args_t<T>& a, long t,
                                       bool load_mv) {
  step_ld_t<T> r;
  r.th = a.theta_in[t];
  r.du = a.duals[t];
  r.sv = DUAL ? T(0) : a.s[t];
  r.m_prev = T(0);
  r.v_prev = T(0);
  if (load_mv) {
    r.m_prev = a.m[t];
    r.v_prev = a.v[t];
  }
  return r;
}

// S[q] = sum over node l's neighbours, k ascending, of nbr(row, q), for
// NQ elements of the node at once. Four neighbours' loads go out
// together (clamped, and a clamped value is not added), so a node of
// degree <= 4 is one round trip however many elements the thread holds.
template <typename T, int NQ, typename NbrFn>
DEV_INLINE void step_nbr_sum(const step_args_t<T>& a, int l, NbrFn nbr,
                             T (&S)[NQ]) {
  const int k0 = a.offs[l], k1 = a.offs[l + 1];
#pragma unroll
  for (int q = 0; q < NQ; ++q) S[q] = T(0);
  for (int k = k0; k < k1; k += 4) {
    T nv[4][NQ];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = a.idx[min(k + j, k1 - 1)];
#pragma unroll
      for (int q = 0; q < NQ; ++q) nv[j][q] = nbr(r, q);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k + j < k1) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) S[q] += nv[j][q];
      }
    }
  }
}

// a neighbour's theta_in[e] from memory: a local row or a received one
template <typename T>
DEV_INLINE T step_nbr_global(const step_args_t<T>& a, int r, long e) {
  return table_row(a.theta_in, a.remote, (long)a.L, a.n, r)[e];
}

DEV_INLINE float step_fma(float a, float b, float c) {
  return __builtin_fmaf(a, b, c);
}
DEV_INLINE double step_fma(double a, double b, double c) {
  return __builtin_fma(a, b, c);
}

// S is step_nbr_sum's result (unused unless DUAL), g the loss gradient.
// Every rounding is written out, with contraction off: each fused
// multiply-add below is one that dinno_dual_threg_k and fused_step_k
// have as compiled, in fp32 and fp64. Left to the compiler the choice
// depends on the code around the call (in the backward launch it packed
// deg * th with 2 * rho into one two-wide fp32 multiply and left the
// subtraction of s unfused), and the callers must agree bit for bit.
template <typename T, int MODE, bool DUAL>
DEV_INLINE void step_elem_apply(const step_args_t<T>& a,
                                const step_ld_t<T>& in, T S, T g, int l,
                                long t) {
#pragma clang fp contract(off)
  T th = in.th, du = in.du, sv = in.sv;
  if (DUAL) {
    // dual += rho * (deg * th - S);  s = (deg * th + S) / 2
    const T dg = T(a.offs[l + 1] - a.offs[l]);
    du = step_fma(a.rho, step_fma(dg, th, -S), du);
    sv = step_fma(dg, th, S) * T(0.5);
    a.duals[t] = du;
    a.s[t] = sv;
  }
  // an isolated node is frozen, see fused_step_k
  const int dl = a.deg[l];
  if (dl == 0) {
    if (a.theta_out != a.theta_in) a.theta_out[t] = th;
    return;
  }
  // g += dual + 2 * rho * (deg * th - s)
  g = g + step_fma(T(2) * a.rho, step_fma(T(dl), th, -sv), du);
  if (MODE == 2) {  // SGD: th - lr * g
    a.theta_out[t] = step_fma(-a.lr, g, th);
    return;
  }
  if (MODE == 1) {  // AdamW decoupled weight decay: th -= lr * wd * th
    th = step_fma(-(a.lr * a.wd), th, th);
  } else if (a.wd != T(0)) {  // Adam L2: g += wd * th
    g = step_fma(a.wd, th, g);
  }
  const T mt = step_mul_add(T(1) - a.beta1, g, a.beta1 * in.m_prev);
  const T vt = step_mul_add(g, (T(1) - a.beta2) * g, a.beta2 * in.v_prev);
  a.m[t] = mt;
  a.v[t] = vt;
  a.theta_out[t] = th - a.lr * (mt / a.bc1) / (::sqrt(vt / a.bc2) + a.eps);
}

// f(mode_c): the optimizer mode as a compile-time constant, for a kernel
// that takes it as a run-time argument
template <typename F>
DEV_INLINE void step_mode_switch(int mode, F&& f) {
  if (mode == 0) f(std::integral_constant<int, 0>{});
  else if (mode == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 2>{});
}

template <typename T, int MODE, bool FIRST>
__global__ void __launch_bounds__(STEP_DUAL_THREADS) fused_step_dual_k(
    T* __restrict__ theta,         // [L, n] in/out (the round-start
                                   // snapshot on entry)
    T* __restrict__ grad,          // [L, n]
    const T* __restrict__ remote,  // [R-L, n] received rows (may be null)
    const int* __restrict__ offs,  // [L+1]
    const int* __restrict__ idx,   // CSR neighbor rows
    const int* __restrict__ deg,   // [L]
    T* __restrict__ duals,         // [L, n] in/out
    T* __restrict__ s_out,         // [L, n] out
    T* __restrict__ m, T* __restrict__ v,  // Adam state (null for SGD)
    T rho, T lr, T beta1, T beta2, T eps, T wd, T bc1, T bc2,
    long n, int L, int zero_grad) {
  // FIRST: the Adam moments count as zero and are not read
  constexpr bool LOAD_MV = MODE != 2 && !FIRST;
  __shared__ T th_s[STEP_DUAL_THREADS];  // [L][columns]
  const step_args_t<T> a{theta, theta, remote, offs, idx, deg, duals,
                         s_out, m, v, rho, lr, beta1, beta2, eps, wd,
                         bc1, bc2, n, L};
  const int cols = blockDim.x;
  const int c = threadIdx.x, l = threadIdx.y;
  for (long e0 = blockIdx.x * (long)cols; e0 < n;
       e0 += (long)gridDim.x * cols) {  // uniform over the block
    const long e = e0 + c;
    const bool live = e < n;
    const long t = (long)l * n + e;
    // all of the thread's loads go out before the barrier waits on th
    step_ld_t<T> in{T(0), T(0), T(0), T(0), T(0)};
    T g = T(0);
    if (live) {
      in = step_elem_load<T, true>(a, t, LOAD_MV);
      g = grad[t];
    }
    th_s[l * cols + c] = in.th;
    __syncthreads();  // the strip's theta is read; stores may follow
    if (live) {
      // a neighbour that is a local row comes from LDS
      T S[1];
      step_nbr_sum<T, 1>(a, l, [&](int r, int) {
        return r < L ? th_s[r * cols + c] : remote[((long)r - L) * n + e];
      }, S);
      if (zero_grad) grad[t] = T(0);
      step_elem_apply<T, MODE, true>(a, in, S[0], g, l, t);
    }
    __syncthreads();  // th_s is free for the next strip
  }
}

// Graph-capture variants: the round scalars (rho, lr, per-pit Adam
// bias corrections) live in a device buffer `sched` laid out as
// [rho, lr, bc1_pit0, bc2_pit0, bc1_pit1, ...] and batch offsets in an
// int64 buffer — the host updates them with one async pinned copy per
// round and replays a captured hipGraph with CONSTANT kernel args.
template <typename T>
__global__ void dinno_dual_threg_sched_k(
    const T* __restrict__ local, const T* __restrict__ remote,
    const int* __restrict__ offs, const int* __restrict__ idx,
    T* __restrict__ duals, T* __restrict__ s_out,
    const T* __restrict__ sched, long n, long L) {
  const T rho = sched[0];
  const long total = L * n;
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long l = t / n;
    const long e = t - l * n;
    const int k0 = offs[l], k1 = offs[l + 1];
    T S = T(0);
    for (int k = k0; k < k1; ++k) {
      S += table_row(local, remote, L, n, idx[k])[e];
    }
    const T th = local[l * n + e];
    const T deg = T(k1 - k0);
    duals[t] += rho * (deg * th - S);
    s_out[t] = (deg * th + S) * T(0.5);
  }
}

template <typename T, int MODE, bool WITH_PENALTY>
__global__ void fused_step_sched_k(
    T* __restrict__ theta, const T* __restrict__ grad,
    const T* __restrict__ dual, const T* __restrict__ s,
    const int* __restrict__ deg, T* __restrict__ m, T* __restrict__ v,
    const T* __restrict__ sched, int pit,
    T beta1, T beta2, T eps, T wd, int first_step, int nparts, long n, long L) {
  const T rho = sched[0];
  const T lr = sched[1];
  const T bc1 = sched[2 + 2 * pit];
  const T bc2 = sched[3 + 2 * pit];
  const long total = L * n;
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long l = t / n;
    const long e = t - l * n;
    // freeze isolated nodes (see fused_step_k)
    if (WITH_PENALTY && deg[l] == 0) continue;
    T th = theta[t];
    T g;
    if (nparts > 1) {  // per-tile slabs from the fused train step
      g = T(0);
      for (int p = 0; p < nparts; ++p) {
        g += grad[(l * nparts + p) * n + e];
      }
    } else {
      g = grad[t];
    }
    if (WITH_PENALTY) {
      g += dual[t] + T(2) * rho * (T(deg[l]) * th - s[t]);
    }
    if (MODE == 2) {
      theta[t] = th - lr * g;
      continue;
    }
    if (MODE == 1) {
      th -= lr * wd * th;
    } else if (wd != T(0)) {
      g += wd * th;
    }
    const T m_prev = first_step ? T(0) : m[t];
    const T v_prev = first_step ? T(0) : v[t];
    const T mt = beta1 * m_prev + (T(1) - beta1) * g;
    const T vt = beta2 * v_prev + (T(1) - beta2) * g * g;
    m[t] = mt;
    v[t] = vt;
    theta[t] = th - lr * (mt / bc1) / (::sqrt(vt / bc2) + eps);
  }
}

// Batch assembly: out[l*B + b, :] = X_all[l, idx[l, b], :] in one
// launch (replaces torch arange + advanced indexing + copies). idx rows
// may be strided views into a longer per-node index stream.
template <typename T>
__global__ void gather_batch_k(
    const T* __restrict__ X_all,       // [L, maxlen, F]
    const long* __restrict__ idx,      // [L, S] index stream
    T* __restrict__ out,               // [L*B, F]
    long maxlen, long Fdim, long B, long idx_stride, long idx_off,
    long total) {
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long f = t % Fdim;
    const long lb = t / Fdim;
    const long l = lb / B;
    const long b = lb - l * B;
    const long src = idx[l * idx_stride + idx_off + b];
    out[t] = X_all[(l * maxlen + src) * Fdim + f];
  }
}

// Same for targets (typed independently: long labels or T densities).
template <typename T>
__global__ void gather_targets_k(
    const T* __restrict__ Y_all, const long* __restrict__ idx,
    T* __restrict__ out, long maxlen, long B, long idx_stride,
    long idx_off, long total) {
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long l = t / B;
    const long b = t - l * B;
    out[t] = Y_all[l * maxlen + idx[l * idx_stride + idx_off + b]];
  }
}

// Gather with the batch offset read from a device buffer (slot `pit`
// of offs_dev) — hipGraph-replayable.
template <typename T>
__global__ void gather_batch_dev_k(
    const T* __restrict__ X_all, const long* __restrict__ idx,
    T* __restrict__ out, const long* __restrict__ offs_dev, int pit,
    long maxlen, long Fdim, long B, long idx_stride, long total) {
  const long idx_off = offs_dev[pit];
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    const long f = t % Fdim;
    const long lb = t / Fdim;
    const long l = lb / B;
    const long b = lb - l * B;
    const long src = idx[l * idx_stride + idx_off + b];
    out[t] = X_all[(l * maxlen + src) * Fdim + f];
  }
}

// Plain axpy: theta -= alpha * grad  (DSGD local step); zero_grad
// clears grad after consuming it (next iteration's atomic kernels
// then need no separate fill launch)
template <typename T>
__global__ void axpy_k(T* __restrict__ x, T* __restrict__ g,
                       T alpha, long total, int zero_grad) {
  for (long t = blockIdx.x * (long)BLOCK + threadIdx.x; t < total;
       t += (long)gridDim.x * BLOCK) {
    x[t] += alpha * g[t];
    if (zero_grad) g[t] = T(0);
  }
}

// Keyed Feistel permutation of [0, n): out[i] = lb + pi(i), pi a
// bijection. ONE elementwise launch replaces the device
// torch.randperm chain (rocprim radix sort + merges + arange/fill —
// ~245 us/round amortized in the online density workload, see
// profiles/dens_final_topk.txt). 4 Feistel rounds over the smallest
// 2^(2*hb) >= n, cycle-walking back into [0, n).
DEV_INLINE unsigned feistel_round_f(unsigned r, unsigned key) {
  unsigned f = r * 0x9E3779B9u + key;
  f ^= f >> 13;
  f *= 0x85EBCA6Bu;
  f ^= f >> 16;
  return f;
}

__global__ void feistel_perm_k(long* __restrict__ out, long n, long lb,
                               unsigned long long key, int half_bits) {
  const unsigned mask = (1u << half_bits) - 1u;
  for (long i = blockIdx.x * (long)BLOCK + threadIdx.x; i < n;
       i += (long)gridDim.x * BLOCK) {
    unsigned long long x = (unsigned long long)i;
    do {
      unsigned lhs = (unsigned)(x >> half_bits);
      unsigned rhs = (unsigned)x & mask;
#pragma unroll
      for (int rnd = 0; rnd < 4; ++rnd) {
        const unsigned f =
            feistel_round_f(rhs, (unsigned)(key >> (16 * rnd)) + rnd)
            & mask;
        const unsigned nl = rhs;
        rhs = lhs ^ f;
        lhs = nl;
      }
      x = ((unsigned long long)lhs << half_bits) | rhs;
    } while (x >= (unsigned long long)n);
    out[i] = lb + (long)x;
  }
}


// ---------------------------------------------------------------------
// Consensus-error metric kernels (eval-only; the one op that still ran
// through torch on the gathered stack — reference
// problems/dist_mnist_problem.py:152-175): row norms, pairwise
// normalized L2 distances, normalized mean vector, distances to mean.

template <typename T>
__global__ void row_norms_k(const T* __restrict__ stack,
                            T* __restrict__ norms, long n) {
  __shared__ T scratch[BLOCK / WAVE];
  const long i = blockIdx.x;
  T acc = T(0);
  for (long e = threadIdx.x; e < n; e += BLOCK) {
    const T v = stack[i * n + e];
    acc += v * v;
  }
  acc = block_reduce_sum<T, BLOCK>(acc, scratch);
  if (threadIdx.x == 0) norms[i] = ::sqrt(acc);
}

// D[i, j] = || stack_i/|stack_i| - stack_j/|stack_j| ||_2
template <typename T>
__global__ void pairwise_normed_dist_k(
    const T* __restrict__ stack, const T* __restrict__ norms,
    T* __restrict__ D, long N, long n) {
  __shared__ T scratch[BLOCK / WAVE];
  const long i = blockIdx.x / N;
  const long j = blockIdx.x % N;
  const T ri = T(1) / norms[i];
  const T rj = T(1) / norms[j];
  T acc = T(0);
  for (long e = threadIdx.x; e < n; e += BLOCK) {
    const T d = stack[i * n + e] * ri - stack[j * n + e] * rj;
    acc += d * d;
  }
  acc = block_reduce_sum<T, BLOCK>(acc, scratch);
  if (threadIdx.x == 0) D[i * N + j] = ::sqrt(acc);
}

template <typename T>
__global__ void normed_mean_k(const T* __restrict__ stack,
                              const T* __restrict__ norms,
                              T* __restrict__ mean, long N, long n) {
  for (long e = blockIdx.x * (long)BLOCK + threadIdx.x; e < n;
       e += (long)gridDim.x * BLOCK) {
    T acc = T(0);
    for (long i = 0; i < N; ++i) {
      acc += stack[i * n + e] / norms[i];
    }
    mean[e] = acc / T(N);
  }
}

template <typename T>
__global__ void dist_to_mean_k(const T* __restrict__ stack,
                               const T* __restrict__ norms,
                               const T* __restrict__ mean,
                               T* __restrict__ Dm, long n) {
  __shared__ T scratch[BLOCK / WAVE];
  const long i = blockIdx.x;
  const T ri = T(1) / norms[i];
  T acc = T(0);
  for (long e = threadIdx.x; e < n; e += BLOCK) {
    const T d = stack[i * n + e] * ri - mean[e];
    acc += d * d;
  }
  acc = block_reduce_sum<T, BLOCK>(acc, scratch);
  if (threadIdx.x == 0) Dm[i] = ::sqrt(acc);
}

}  // namespace ew
