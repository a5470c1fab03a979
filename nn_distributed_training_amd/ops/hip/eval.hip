// Validation of the MNIST conv net in ONE launch (fused_validation).
//
// conv(1->F, K) + ReLU + 2x2 max-pool -> fc1 + ReLU -> fc2 -> log-softmax
// -> NLL and top-1 for all L local nodes over the whole validation set,
// in native precision (T = double / float; no bf16, so the metrics do
// not depend on gemm_precision). The layered path runs one chunk of
// val_batch_size rows at a time: it copies the chunk L times, launches
// four kernels that pass [L*Bv, I] activations through memory and ends
// in a handful of eager torch ops - about a thousand launches per
// evaluation at the paper shape. Here X_val [V, 784] is stored once and
// the node index never enters an image address.
//
// Grid (ceil(V / R), L), 256 threads = 4 waves. A block owns R (32, or
// 16 where 32 does not fit LDS) consecutive validation rows of one node
// and never leaves the CU's LDS between the image and the row's loss:
//
//  A  conv on VALU. Images are staged G = 4 at a time, so that the
//     pooled pixels of a group (4 x 144 at K = 5) keep all 256 lanes
//     busy where one image would leave 112 idle; the next group's loads
//     are in flight while this one is computed. K == KMAX runs one
//     thread per (image, pooled pixel) on the (K+1)x(K+1) register
//     window of conv::conv_pool_fwd_k, K < KMAX its guarded per-(filter,
//     pixel) loop, both in that kernel's order: bias first, taps
//     row-major, strict > for the pool, ReLU floor 0. The pooled
//     features go to the LDS tile x0[R][XS] only; no argmax index, no
//     global store. XS is ceil4(I) padded to 2 (mod 32), the stride
//     fc_fwd_split_k uses for bank-clean fragment reads.
//  B  fc1 on MFMA (16x16x4 f64 / f32). Wave w owns output columns
//     [16w, 16w + 16) and all R/16 row fragments: one W1 fragment read
//     feeds R/16 MFMAs. W1 streams through two [64][34] LDS stage
//     buffers, 32 k per stage; stage s+1's global loads are issued
//     before stage s's MFMAs and stored after them. The A operand is
//     read straight from x0. Rows H..63 and columns past I of a stage
//     are written as zeros, x0 columns I..ceil4(I)-1 likewise, and the
//     k-steps past ceil4(I) do not run. The image groups of phase A and
//     everything phase C keeps in LDS alias the stage buffers.
//  C  y1 = relu(z1 + b1) -> LDS; wave f < R/16 computes row fragment
//     f's logits as one 16x16 tile (W2 rows C..15 and y1 columns H..63
//     are zeros). A lane then holds class lane & 15 of four rows, so the
//     row max, sum, first-maximal class and the target's log-prob are
//     16-lane xor-shuffles on the accumulator registers, one exp per
//     element. correct[l, v] = (argmax == y_v) is one byte; rows at or
//     past V write nothing.
//
// Loss, in the reference's convention: validate_all returns the sum
// over chunks of the chunk-mean NLL (divided by V by the caller). Row v
// gets the weight 1 / c(v), c(v) = rows in v's chunk of Bv, which makes
// the launch independent of the chunking. A block folds its weighted
// row losses in row order into part[l][tile] and draws a ticket of node
// l (relaxed agent-scope atomics, as fc_fwd_split_k). The block that
// draws the last one sums the node's partials in tile order, overwrites
// loss_sum[l] and returns the ticket to zero: no block waits for
// another, and the result is bit-identical from launch to launch.
//
// Uses gmfma::mfma_t (gemm_mfma.hip) and fmnist::slab_store / slab_load
// / fc_w2_tile_load (fused_mnist.hip): ext.hip includes this file after
// both.

#include "common.h"

namespace evalk {

constexpr int IMG = 28;
constexpr int NPIX = IMG * IMG;
constexpr int G = 4;                          // images per conv group
constexpr int GLD = (G * NPIX + 255) / 256;   // image loads per thread
constexpr int WK = 32;                        // k per W1 stage
constexpr int WS = WK + 2;                    // stage row stride
constexpr int WLD = 64 * WK / 256;            // W1 loads per thread
constexpr int YS = 66;                        // y1 / W2 row stride
constexpr int STAGE = 2 * 64 * WS;            // both stage buffers
// what aliases the stage buffers
constexpr int C_Y1 = 0;                       // [32][YS]
constexpr int C_W2 = C_Y1 + 32 * YS;          // [16][YS] | b2 [16]
constexpr int C_RL = C_W2 + 16 * YS + 16;     // [32] weighted row losses
static_assert(G * NPIX <= STAGE, "image group must fit the W1 stages");
static_assert(C_RL + 32 <= STAGE, "tail must fit the W1 stages");

// padded row stride of the x0 tile: ceil4(I) up to 2 (mod 32)
inline int x0_stride(int I) {
  const int I4 = (I + 3) / 4 * 4;
  return I4 + ((2 - I4 % 32) + 32) % 32;
}

// written by ext.hip evalk_plan, the only place that fills one
struct Plan {
  long cw_off, cb_off, w1_off, b1_off, w2_off, b2_off;
  int F, K, P, I, H, C;
  int R;          // rows per block: 32 or 16
  int XS;         // x0 row stride
  int off_stage;  // LDS element offsets: x0 at 0, then the stage
  int off_wgt;    // buffers, then the conv weights and bias
};

template <typename T, int KMAX>
__global__ __launch_bounds__(256) void mnist_eval_k(
    const T* __restrict__ X,             // [V, 784]
    const long* __restrict__ yv,         // [V] targets
    const T* __restrict__ theta,         // [L, n]
    unsigned char* __restrict__ correct, // [L, V]
    T* __restrict__ loss_sum,            // [L], overwritten
    T* part,                             // [L, tiles] workspace
    int* tickets,                        // [L], zero between launches
    Plan p, long n, int V, int Bv) {
  using MF = gmfma::mfma_t<T>;
  using acc_t = typename MF::acc_t;
  extern __shared__ __align__(16) unsigned char ev_raw[];
  T* x0s = reinterpret_cast<T*>(ev_raw);
  T* stg = x0s + p.off_stage;
  T* wgt = x0s + p.off_wgt;
  T* imgs = stg;
  T* y1s = stg + C_Y1;
  T* w2s = stg + C_W2;
  T* rls = stg + C_RL;

  const int tile = blockIdx.x;
  const int tiles = gridDim.x;
  const long l = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int lo = lane & 15;
  const int lk = lane >> 4;
  const int F = p.F, K = p.K, P = p.P, I = p.I, H = p.H, C = p.C;
  const int R = p.R, XS = p.XS;
  const int NF = R / 16;
  const int v0 = tile * R;
  const T* th = theta + l * n;

  // what only the tail needs loads now, clamped not branched, and waits
  // in registers: W2, b2, b1 and the targets of the lane's four rows
  T w2v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w2v[j] = fmnist::fc_w2_tile_load(th + p.w2_off, tid + j * 256, H, C);
  }
  const T b2v = th[p.b2_off + min(tid, C - 1)];
  const T b1v = th[p.b1_off + min(wid * 16 + lo, H - 1)];
  int tg[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = (wid < NF ? wid : 0) * 16 + MF::acc_row(lane, r);
    tg[r] = (int)yv[min(v0 + row, V - 1)];
  }

  // ---- phase A: conv + ReLU + pool into x0 --------------------------
  const int nw = F * K * K;
  const int nwb = nw + F;
  for (int t = tid; t < nwb; t += 256) {
    wgt[t] = t < nw ? th[p.cw_off + t] : th[p.cb_off + t - nw];
  }
  {
    const int npad = (I + 3) / 4 * 4 - I;  // MFMA k-step tail: zeros
    for (int t = tid; t < R * npad; t += 256) {
      x0s[(t / npad) * XS + I + t % npad] = T(0);
    }
  }
  // rows at or past V read image V - 1: finite values nobody uses
  T pre[GLD];
  const auto ldgroup = [&](int g) {
#pragma unroll
    for (int j = 0; j < GLD; ++j) {
      const int t = min(j * 256 + tid, G * NPIX - 1);
      const int im = t / NPIX;
      const long v = min(v0 + g * G + im, V - 1);
      pre[j] = X[v * NPIX + (t - im * NPIX)];
    }
  };
  const int PP = P * P;
  const int NG = R / G;
  ldgroup(0);
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int j = 0; j < GLD; ++j) {
      const int t = j * 256 + tid;
      if (t < G * NPIX) imgs[t] = pre[j];
    }
    if (g + 1 < NG) ldgroup(g + 1);
    __syncthreads();
    if (K == KMAX) {
      constexpr int WN = KMAX + 1;
      for (int t = tid; t < G * PP; t += 256) {
        const int j = t / PP;
        const int pp = t - j * PP;
        const int py = pp / P;
        const int px = pp - py * P;
        const T* wbase = imgs + j * NPIX + (2 * py) * IMG + 2 * px;
        T win[WN * WN];
#pragma unroll
        for (int r = 0; r < WN; ++r) {
#pragma unroll
          for (int c = 0; c < WN; ++c) win[r * WN + c] = wbase[r * IMG + c];
        }
        T* xrow = x0s + (g * G + j) * XS + pp;
        for (int f = 0; f < F; ++f) {
          T w[KMAX * KMAX];
#pragma unroll
          for (int i = 0; i < KMAX * KMAX; ++i) {
            w[i] = wgt[f * KMAX * KMAX + i];
          }
          const T bias = wgt[nw + f];
          T best = T(0);  // ReLU floor
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            T acc = bias;
#pragma unroll
            for (int ky = 0; ky < KMAX; ++ky) {
#pragma unroll
              for (int kx = 0; kx < KMAX; ++kx) {
                acc += win[((d >> 1) + ky) * WN + (d & 1) + kx] *
                       w[ky * KMAX + kx];
              }
            }
            if (acc > best) best = acc;
          }
          xrow[f * PP] = best;
        }
      }
    } else {
      const int npool = F * PP;
      for (int t = tid; t < G * npool; t += 256) {
        const int j = t / npool;
        const int u = t - j * npool;
        const int f = u / PP;
        const int py = (u / P) % P;
        const int px = u % P;
        const T* img = imgs + j * NPIX;
        const T* wf = wgt + f * K * K;
        const T bias = wgt[nw + f];
        T best = T(0);  // ReLU floor
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int cy = 2 * py + (d >> 1);
          const int cx = 2 * px + (d & 1);
          T acc = bias;
#pragma unroll
          for (int ky = 0; ky < KMAX; ++ky) {
            if (ky >= K) break;
            const T* row = img + (cy + ky) * IMG + cx;
            const T* wr = wf + ky * K;
#pragma unroll
            for (int kx = 0; kx < KMAX; ++kx) {
              if (kx >= K) break;
              acc += row[kx] * wr[kx];
            }
          }
          if (acc > best) best = acc;
        }
        x0s[(g * G + j) * XS + u] = best;
      }
    }
    __syncthreads();  // group computed: imgs free, x0 rows visible
  }

  // ---- phase B: z1 = x0 @ W1^T on MFMA ------------------------------
  acc_t a0 = {}, a1 = {};
  {
    const T* W1 = th + p.w1_off;
    const int NS = (I + WK - 1) / WK;
    const int so = tid >> 5;  // W1 row of load 0; load q is row so + 8q
    const int sk = tid & 31;
    T wr[WLD];
    const auto ldstage = [&](int s) {
      const int k = s * WK + sk;
#pragma unroll
      for (int q = 0; q < WLD; ++q) {
        const int o = so + 8 * q;
        const T v = W1[(long)min(o, H - 1) * I + min(k, I - 1)];
        wr[q] = (o < H && k < I) ? v : T(0);
      }
    };
    const auto ststage = [&](int buf) {
#pragma unroll
      for (int q = 0; q < WLD; ++q) {
        stg[buf * (64 * WS) + (so + 8 * q) * WS + sk] = wr[q];
      }
    };
    ldstage(0);
    ststage(0);
    __syncthreads();
    for (int s = 0; s < NS; ++s) {
      if (s + 1 < NS) ldstage(s + 1);
      const T* Br = stg + (s & 1) * (64 * WS) + (wid * 16 + lo) * WS + lk;
      const T* A0 = x0s + lo * XS + s * WK + lk;
      const T* A1 = A0 + 16 * XS;
      const int klim = min(WK, I - s * WK);
#pragma unroll
      for (int kk = 0; kk < WK; kk += 4) {
        if (kk < klim) {
          const T b = Br[kk];
          a0 = MF::mma(A0[kk], b, a0);
          if (NF == 2) a1 = MF::mma(A1[kk], b, a1);
        }
      }
      if (s + 1 < NS) ststage((s + 1) & 1);
      __syncthreads();
    }
  }

  // ---- phase C: y1, logits, log-softmax, NLL, top-1 -----------------
  {
    const int o = wid * 16 + lo;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = MF::acc_row(lane, r);
      const T u0 = a0[r] + b1v;
      y1s[row * YS + o] = (o < H && u0 > T(0)) ? u0 : T(0);
      if (NF == 2) {
        const T u1 = a1[r] + b1v;
        y1s[(16 + row) * YS + o] = (o < H && u1 > T(0)) ? u1 : T(0);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = tid + j * 256;  // the zero-padded [16][64] tile
      w2s[(t >> 6) * YS + (t & 63)] = w2v[j];
    }
    if (tid < 16) w2s[16 * YS + tid] = tid < C ? b2v : T(0);
  }
  __syncthreads();

  if (wid < NF) {
    acc_t z = {};
    const T* Ar = y1s + (wid * 16 + lo) * YS + lk;  // y1[m = lo][h]
    const T* Br = w2s + lo * YS + lk;               // W2[c = lo][h]
#pragma unroll
    for (int kk = 0; kk < 64; kk += 4) z = MF::mma(Ar[kk], Br[kk], z);
    const int c = lo;
    const bool act = c < C;
    const T b2 = w2s[16 * YS + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wid * 16 + MF::acc_row(lane, r);
      const int v = v0 + row;
      const T zz = act ? z[r] + b2 : -INFINITY;
      T mx = zz;
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        const T ov = __shfl_xor(mx, off, 16);
        mx = ov > mx ? ov : mx;
      }
      T sum = act ? ::exp(zz - mx) : T(0);
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 16);
      }
      const T lp = zz - (mx + ::log(sum));  // -inf on pad classes
      // first maximal class: torch.argmax's tie rule
      T bv = lp;
      int bi = c;
      T nl = (act && c == tg[r]) ? -lp : T(0);
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) {
        const T ov = __shfl_xor(bv, off, 16);
        const int oi = __shfl_xor(bi, off, 16);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        nl += __shfl_xor(nl, off, 16);
      }
      if (lo == 0) {
        if (v < V) {
          const int cnt = min(Bv, V - (v / Bv) * Bv);  // rows in v's chunk
          rls[row] = nl / T(cnt);
          correct[l * V + v] = bi == tg[r] ? 1 : 0;
        } else {
          rls[row] = T(0);
        }
      }
    }
  }
  __syncthreads();
  if (wid != 0) return;

  // ---- the block's partial, the node's ticket, the last one's sum ---
  {
    const T w = lane < R ? rls[lane] : T(0);
    T s = T(0);
#pragma unroll
    for (int i = 0; i < 32; ++i) s += __shfl(w, i, WAVE);  // row order
    T* pl = part + l * tiles;
    int last = 0;
    if (lane == 0) {
      // the partial goes out write-through and has left the wave before
      // the ticket is drawn; the last block reads every partial past its
      // L1 (see fc_fwd_split_k for the same hand-off)
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

}  // namespace evalk
