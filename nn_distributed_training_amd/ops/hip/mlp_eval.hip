// Validation of the density MLPs in ONE launch (fused_validation).
//
// lift (in <= 4) -> trunk layers (out <= 64) -> tail (out <= 4) for all
// L local nodes over the whole validation set, in native precision (T =
// double / float; no bf16, so the metric does not depend on
// gemm_precision). The layered path runs one chunk of val_batch_size
// rows at a time: it copies the chunk L times, launches one kernel per
// layer with every hidden activation through memory and ends in eager
// torch. Here X_val [V, in] is stored once, the node index never enters
// an input address and no activation leaves the CU's LDS.
//
// Grid (ceil(V / R), L), 256 threads = 4 waves; R = 16 * NF rows, NF = 4
// (float) or 2 (double). A block owns R consecutive rows of one node:
//
//  lift   on VALU. The tile's inputs are staged in LDS xs[R][4]. Thread
//         t owns column t & (CP - 1), CP = ceil4(out) rounded up to a
//         power of two, and every 256 / CP-th row; its W0 row and bias
//         sit in registers, the inputs are LDS broadcasts. act(z) goes
//         to the wide image [R][ldw], ldw = ceil4(out) padded to 2 (mod
//         32); columns out..ceil4(out)-1 are zeros.
//  trunk  on MFMA (16x16x4 f64 / f32), evalk::mnist_eval_k's phase B:
//         wave w owns output columns [16w, 16w + 16) and all NF row
//         fragments, so one W fragment read feeds NF MFMAs. W streams
//         through two [64][34] LDS stages of 32 k; stage s+1's global
//         loads are issued before stage s's MFMAs and stored after them,
//         one barrier per stage. Rows of W past out and columns past in
//         are zeros, k-steps past ceil4(in) do not run. act(acc + b)
//         goes to one of two narrow images [R][66] that alternate as a
//         layer's input and output; columns out..63 are zeros.
//  tail   per-row dot product: thread t computes output t & 3 of row
//         t >> 2 from the last image and the weights in global memory.
//
// Predict mode (yv == nullptr) writes yhat[l, v, 0..out). Loss mode
// (head width 1) turns the row into its BCE (validate_all's clamp, eps =
// 1e-12 in T), squared or absolute error and weights it by 1 / c(v), c(v)
// = rows in v's chunk of Bv, so that the launch returns "sum over chunks
// of the chunk mean" whatever its own tiling. The block folds its rows
// in row order into part[l][tile] and draws node l's ticket; the last
// arriver sums the partials in tile order, overwrites loss_sum[l] and
// returns the ticket to zero (mnist_eval_k's hand-off): no block waits
// for another, no floating-point atomics, equal bits from every launch.
//
// Uses gmfma::mfma_t (gemm_mfma.hip) and fmnist::slab_store / slab_load
// (fused_mnist.hip): ext.hip includes this file after both.

#include "common.h"

namespace mlpe {

constexpr int MAXL = 8;        // linear layers of a chain
constexpr int LIFT_IN = 4;
constexpr int WIDE = 256;      // lift out
constexpr int NARROW = 64;     // trunk out, tail in
constexpr int TAIL_OUT = 4;
constexpr int WK = 32;         // k per W stage
constexpr int WS = WK + 2;     // stage row stride
constexpr int WLD = 64 * WK / 256;  // W loads per thread and stage
constexpr int NLD = NARROW + 2;     // narrow image row stride
constexpr int STAGE = 2 * 64 * WS;  // both stage buffers

// rows per block: 16-row MFMA fragments per wave
template <typename T>
constexpr int frags() { return sizeof(T) == 4 ? 4 : 2; }

// padded row stride of the wide image: ceil4(out) up to 2 (mod 32)
inline int wide_stride(int out) {
  const int o4 = (out + 3) / 4 * 4;
  return o4 + ((2 - o4 % 32) + 32) % 32;
}

struct Layer {
  long w_off, b_off;
  int in, out, act;
};

// written by ext.hip mlp_eval_plan, the only place that fills one
struct Plan {
  Layer ly[MAXL];
  double scale;   // the lift's activation scale
  int nl;
  int loss_kind;  // 0 predict, 1 BCE, 2 MSE, 3 L1
  int ldw;        // wide image row stride
  int cp;         // lift columns per row group, a power of two
  // LDS element offsets: the wide image at 0, then the two narrow
  // images, the W stages, the inputs [R][4] and the row losses [R]
  int off_nar, off_stage, off_x, off_rl;
};

template <typename T>
__global__ __launch_bounds__(256) void mlp_eval_k(
    const T* __restrict__ X,      // [V, in]
    const T* __restrict__ yv,     // [V] targets; null: predict mode
    const T* __restrict__ theta,  // [L, n]
    T* __restrict__ loss_sum,     // [L], overwritten (loss mode)
    T* __restrict__ yhat,         // [L, V, out] (predict mode)
    T* part,                      // [L, tiles] workspace
    int* tickets,                 // [L], zero between launches
    Plan p, long n, int V, int Bv) {
  using MF = gmfma::mfma_t<T>;
  using acc_t = typename MF::acc_t;
  constexpr int NF = frags<T>();
  constexpr int R = NF * 16;
  extern __shared__ __align__(16) unsigned char me_raw[];
  T* wide = reinterpret_cast<T*>(me_raw);
  T* nar = wide + p.off_nar;
  T* stg = wide + p.off_stage;
  T* xs = wide + p.off_x;
  T* rls = wide + p.off_rl;

  const int tile = blockIdx.x;
  const int tiles = gridDim.x;
  const long l = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int lo = lane & 15;
  const int lk = lane >> 4;
  const int v0 = tile * R;
  const T* th = theta + l * n;

  // ---- lift: act(x W0^T + b0) into the wide image --------------------
  {
    const Layer y = p.ly[0];
    // rows at or past V read row V - 1: finite values nobody uses
    for (int t = tid; t < R * LIFT_IN; t += 256) {
      const int r = t >> 2, j = t & 3;
      const long v = min(v0 + r, V - 1);
      xs[t] = j < y.in ? X[v * y.in + j] : T(0);
    }
    const int o = tid & (p.cp - 1);
    const int o4 = (y.out + 3) / 4 * 4;
    const int oc = min(o, y.out - 1);
    T w[LIFT_IN];
#pragma unroll
    for (int j = 0; j < LIFT_IN; ++j) {
      const T wv = th[y.w_off + (long)oc * y.in + min(j, y.in - 1)];
      w[j] = j < y.in ? wv : T(0);
    }
    const T b = th[y.b_off + oc];
    const T sc = (T)p.scale;
    __syncthreads();
    if (o < o4) {
      const int rstep = 256 / p.cp;
      for (int r = tid / p.cp; r < R; r += rstep) {
        T z = b;
#pragma unroll
        for (int j = 0; j < LIFT_IN; ++j) z += xs[r * LIFT_IN + j] * w[j];
        wide[r * p.ldw + o] = o < y.out ? act_fwd<T>(y.act, z, sc) : T(0);
      }
    }
  }

  // ---- trunk: act(cur W^T + b) on MFMA, image to image ---------------
  const T* cur = wide;
  int cs = p.ldw;
  for (int li = 1; li < p.nl - 1; ++li) {
    const Layer y = p.ly[li];
    const int I = y.in, O = y.out;
    const T* W = th + y.w_off;
    const T bv = th[y.b_off + min(wid * 16 + lo, O - 1)];
    acc_t acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = acc_t{};
    const int NS = (I + WK - 1) / WK;
    const int so = tid >> 5;  // W row of load 0; load q is row so + 8q
    const int sk = tid & 31;
    T wr[WLD];
    const auto ldstage = [&](int s) {
      const int k = s * WK + sk;
#pragma unroll
      for (int q = 0; q < WLD; ++q) {
        const int o = so + 8 * q;
        const T v = W[(long)min(o, O - 1) * I + min(k, I - 1)];
        wr[q] = (o < O && k < I) ? v : T(0);
      }
    };
    const auto ststage = [&](int buf) {
#pragma unroll
      for (int q = 0; q < WLD; ++q) {
        stg[buf * (64 * WS) + (so + 8 * q) * WS + sk] = wr[q];
      }
    };
    // the layer below ended in a barrier after its last MFMA, so both
    // stage buffers are free; this barrier also publishes its image
    ldstage(0);
    ststage(0);
    __syncthreads();
    for (int s = 0; s < NS; ++s) {
      if (s + 1 < NS) ldstage(s + 1);
      const T* Br = stg + (s & 1) * (64 * WS) + (wid * 16 + lo) * WS + lk;
      const T* Ar = cur + lo * cs + s * WK + lk;
      const int klim = min(WK, I - s * WK);
#pragma unroll
      for (int kk = 0; kk < WK; kk += 4) {
        if (kk < klim) {
          const T bw = Br[kk];
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            acc[f] = MF::mma(Ar[f * 16 * cs + kk], bw, acc[f]);
          }
        }
      }
      if (s + 1 < NS) ststage((s + 1) & 1);
      __syncthreads();
    }
    // the image this layer writes is the one the layer below read
    T* out = nar + (li & 1) * (R * NLD);
    const int o = wid * 16 + lo;
    const bool relu = y.act == ACT_RELU;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = f * 16 + MF::acc_row(lane, r);
        const T u = acc[f][r] + bv;
        out[row * NLD + o] = (o < O && !(relu && !(u > T(0)))) ? u : T(0);
      }
    }
    // sigmoid / tanh: a rolled second pass over the thread's own
    // elements, so that the unrolled one above carries no exp
    if (o < O && (y.act == ACT_SIGMOID || y.act == ACT_TANH)) {
#pragma unroll 1
      for (int e = 0; e < NF * 4; ++e) {
        T* q = out + ((e >> 2) * 16 + MF::acc_row(lane, e & 3)) * NLD + o;
        *q = act_fwd<T>(y.act, *q, T(1));
      }
    }
    cur = out;
    cs = NLD;
  }
  __syncthreads();

  // ---- tail: one thread per (row, output) ----------------------------
  {
    const Layer y = p.ly[p.nl - 1];
    const int r = tid >> 2, c = tid & 3;
    const int v = v0 + r;
    if (r < R && c < y.out) {
      const T* wt = th + y.w_off + (long)c * y.in;
      const T* a = cur + r * cs;
      T z = th[y.b_off + c];
      for (int k = 0; k < y.in; ++k) z += a[k] * wt[k];
      const T yh = act_fwd<T>(y.act, z, T(1));
      if (yv == nullptr) {
        if (v < V) yhat[(l * V + v) * y.out + c] = yh;
      } else if (v < V) {
        const T t = yv[v];
        T e;
        if (p.loss_kind == 1) {
          const T eps = T(1e-12);
          const T hi = T(1) - eps;
          const T pc = yh < eps ? eps : (yh > hi ? hi : yh);
          e = -(t * ::log(pc) + (T(1) - t) * ::log(T(1) - pc));
        } else if (p.loss_kind == 2) {
          e = (yh - t) * (yh - t);
        } else {
          e = ::fabs(yh - t);
        }
        const int cnt = min(Bv, V - (v / Bv) * Bv);  // rows in v's chunk
        rls[r] = e / T(cnt);
      } else {
        rls[r] = T(0);
      }
    }
  }
  if (yv == nullptr) return;
  __syncthreads();
  if (wid != 0) return;

  // ---- the block's partial, the node's ticket, the last one's sum ----
  {
    const T w = lane < R ? rls[lane] : T(0);
    T s = T(0);
#pragma unroll
    for (int i = 0; i < R; ++i) s += __shfl(w, i, WAVE);  // row order
    T* pl = part + l * tiles;
    int last = 0;
    if (lane == 0) {
      // the partial goes out write-through and has left the wave before
      // the ticket is drawn; the last block reads every partial past its
      // L1 (see mnist_eval_k for the same hand-off)
      fmnist::slab_store(&pl[tile], s);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int got = __hip_atomic_fetch_add(
          &tickets[l], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = got == tiles - 1;
      if (last) {
        __hip_atomic_store(&tickets[l], 0, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    last = __shfl(last, 0, WAVE);
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    T tot = T(0);
    for (int t0 = 0; t0 < tiles; t0 += WAVE) {
      const int t = t0 + lane;
      const T pv = fmnist::slab_load(&pl[min(t, tiles - 1)]);
      const T u = t < tiles ? pv : T(0);
#pragma unroll
      for (int i = 0; i < WAVE; ++i) tot += __shfl(u, i, WAVE);  // tile order
    }
    if (lane == 0) loss_sum[l] = tot;
  }
}

}  // namespace mlpe
