// Every node's whole PPO gradient row in ONE launch (rl/stacked_ppo.py
// FusedPPOEngine, grad_engine "fused"): actor and critic forward, the
// clipped-surrogate / value loss of losses.hip ppo_loss_bwd_k and the
// full backward, for nets of a few layers of width <= 64 on a few
// hundred rows per node - the shape at which the layered path is two
// dozen launch-bound kernels.
//
// Work split. Grid (row tile, net, node), net 0 the actor and 1 the
// critic; a 256-thread block of 4 waves owns ONE net of ONE node on TM
// rows and never reads another block's activations.
//
// Residency. The block stages its net's weights from the [N, n] stack
// into LDS as [o][i] images with both extents zero-padded to multiples
// of 16, beside the zero-padded biases, the observation tile and every
// hidden layer's output tile; dZ ping-pongs between two more images
// (the head's output lands in one of them and the loss turns it into
// the head's dZ in place). Nothing is stashed to global memory. Rows at
// or past M are staged as zeros and get a zero dZ, so they add nothing
// to dW/db.
//
// Row stride. Every image of logical width w (a multiple of 16) has row
// stride w + 2 elements, i.e. 2 (mod 16) with an odd half. The forward
// reads both operands, and dX its dZ operand, "row-walking": lane
// (lo = lane & 15, lk = lane >> 4) reads row lo, column k + lk. With an
// even stride whose half is odd, lo * stride runs over 16 distinct even
// banks and lk in {0, 1} fills the odd ones: the 32 lanes the LDS
// serves together hit 32 distinct banks. dW's two operands and dX's
// weight operand are read "column-walking" (row k + lk, column lo); no
// stride clears both patterns (fused_mnist.hip's fc tail found the
// same) and this one leaves those a 2-way conflict.
//
// MFMA. v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 through
// gmfma::mfma_t (operand and accumulator maps in gemm_mfma.hip). The 4
// waves deal the 16x16 output fragments of each product round-robin;
// a fragment runs two accumulators to halve its dependency chain.
//   forward  Y[m][o]  = sum_i X[m][i]  W[o][i]   (+ b, relu below the head)
//   dW       dW[o][i] = sum_m dZ[m][o] X[m][i]   (the tile's rows)
//   dX       dX[m][i] = sum_o dZ[m][o] W[o][i]   masked with X[m][i] > 0
//   db       db[o] = sum_m dZ[m][o] * 1: the dW fragments of the first
//            i-column contract their dZ operand against ones as well
//
// Cross-tile reduction, deterministic and without floating-point
// atomics: the block writes its dW/db partials and its partial loss sum
// to a slab of its own, laid out like the net's slice of the row with
// the loss word behind it, then draws a ticket of its (node, net). The
// last arriver sums the slabs in tile order and OVERWRITES the net's
// slice of grad[l] and loss[l]: fused_mnist.hip fc_fwd_split_k's
// hand-off (write-through slab stores, relaxed agent-scope ticket that
// the reducer returns to zero, slab loads past L1). No block waits for
// another, two launches on the same inputs give the same bits, and the
// caller zeroes neither grad nor loss.
//
// Included by ext.hip after gemm_mfma.hip (mfma_t), losses.hip
// (PPO_MAX_A) and fused_mnist.hip (slab_store / slab_load). Compiled
// without packed fp32 VALU ops.

#include "common.h"

namespace ppof {

constexpr int MAXL = 8;     // linear layers per net
constexpr int MAX_W = 64;   // widest layer input / output
constexpr int LDZ = MAX_W + 2;
constexpr int LDS_BUDGET = 160 * 1024;
constexpr int STATIC_LDS = 64;  // the reducer flag, rounded up
constexpr int STG = 8;      // staging loads in flight per thread
constexpr int RED_U = 8;    // reducer: elements x tiles in flight
constexpr int RED_T = 4;

// rows per tile: the images of 12-64-64-64-5 take 132,544 B at 64 fp32
// rows; in fp64 176,000 B at 32 rows, over the budget, and 131,456 B at
// 16 rows
template <typename T>
struct tile_rows { static constexpr int value = 64; };
template <>
struct tile_rows<double> { static constexpr int value = 16; };

struct Net {
  int nl;
  int in_dim[MAXL], out_dim[MAXL];
  int w_off[MAXL], b_off[MAXL];  // in the node's parameter row
  int base, span;                // the net's slice [base, base + span)
  // LDS element offsets: weight image, bias, and the INPUT image of
  // each layer (the observation tile for layer 0)
  int wimg[MAXL], bimg[MAXL], aimg[MAXL];
};

struct Prog {
  Net net[2];   // actor, critic
  int dz[2];    // the dZ ping-pong images, TM x LDZ each
  int slab;     // elements between two slabs (>= span + 1 of both nets)
};

DEV_INLINE int pad16(int v) { return (v + 15) & ~15; }

// __syncthreads() written out: the HIP header's is not always_inline
// and a kernel compiled with its own target features (PPOF_KERNEL)
// would CALL it instead
DEV_INLINE void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Staging: rows x cols elements (cols a multiple of 16) of the
// row-major [R, C] source into an image of row stride cols + 2, zeros
// past R and C. Thread t walks elements t, t + 256, ... as (row, col)
// without a division per element; STG clamped loads are in flight
// before the first LDS store.
template <typename T>
DEV_INLINE void stage(T* img, const T* __restrict__ src, int R, int C,
                      int rows, int cols, int tid) {
  const int ld = cols + 2;
  const int dq = 256 / cols, dr = 256 - dq * cols;
  int r = tid / cols, c = tid - r * cols;
  while (r < rows) {
    T v[STG];
    int dst[STG];
#pragma unroll
    for (int j = 0; j < STG; ++j) {
      const T g = src[(long)min(r, R - 1) * C + min(c, C - 1)];
      v[j] = (r < R && c < C) ? g : T(0);
      dst[j] = r < rows ? r * ld + c : -1;
      c += dr;
      r += dq;
      if (c >= cols) { c -= cols; ++r; }
    }
#pragma unroll
    for (int j = 0; j < STG; ++j) {
      if (dst[j] >= 0) img[dst[j]] = v[j];
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#define PPOF_KERNEL \
  __attribute__((target("no-packed-fp32-ops"))) __global__
#else
#define PPOF_KERNEL __global__
#endif

template <typename T, int TM>
PPOF_KERNEL __launch_bounds__(256) void ppo_grad_fused_k(
    const T* __restrict__ theta,     // [N, n]
    const T* __restrict__ obs,       // [N*M, obs_dim]
    const T* __restrict__ acts,      // [N*M, A]
    const T* __restrict__ old_logp,  // [N*M]
    const T* __restrict__ adv,       // [N*M]
    const T* __restrict__ vtarg,     // [N*M]
    T* __restrict__ grad,            // [N, n]
    T* __restrict__ loss,            // [N, 2]
    T* slabs,                        // [N, 2, tiles, prog.slab]
    int* tickets,                    // [N, 2], zero between launches
    Prog prog, long n, int M, int A, T inv_cov, T logc, T clip_lo,
    T clip_hi, T critic_coef, T loss_scale) {
  using MF = gmfma::mfma_t<T>;
  using acc_t = typename MF::acc_t;
  static_assert(TM % 16 == 0 && TM <= 64, "one wave runs the loss");
  constexpr int TMF = TM / 16;
  extern __shared__ __align__(16) unsigned char ppof_raw[];
  __shared__ int lastf;
  T* lds = reinterpret_cast<T*>(ppof_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int lo = lane & 15;
  const int lk = lane >> 4;
  const int tile = blockIdx.x, tiles = gridDim.x;
  const int net = blockIdx.y;
  const long l = blockIdx.z;
  const int m0 = tile * TM;
  const Net& nt = prog.net[net];
  const int nl = nt.nl;
  const T* th = theta + l * n;
  T* slab = slabs + ((l * 2 + net) * tiles + tile) * (long)prog.slab;

  // ---- staging
  {
    const int I0 = nt.in_dim[0];
    stage(lds + nt.aimg[0], obs + (l * M + m0) * (long)I0,
          min(TM, M - m0), I0, TM, pad16(I0), tid);
    for (int li = 0; li < nl; ++li) {
      const int I = nt.in_dim[li], O = nt.out_dim[li];
      stage(lds + nt.wimg[li], th + nt.w_off[li], O, I, pad16(O),
            pad16(I), tid);
      stage(lds + nt.bimg[li], th + nt.b_off[li], 1, O, 1, pad16(O),
            tid);
    }
  }
  block_sync();

  // ---- forward: hidden outputs to their images, the head's to the dZ
  // image the backward starts from. Padded columns come out as
  // relu(0 + 0); rows past M hold relu(b) and are masked by the loss.
  for (int li = 0; li < nl; ++li) {
    const int Ip = pad16(nt.in_dim[li]), Op = pad16(nt.out_dim[li]);
    const int lda = Ip + 2, ldo = Op + 2;
    const bool head = li == nl - 1;
    const T* x = lds + nt.aimg[li];
    const T* w = lds + nt.wimg[li];
    const T* b = lds + nt.bimg[li];
    T* y = lds + (head ? prog.dz[li & 1] : nt.aimg[li + 1]);
    const int nf = TMF * (Op >> 4);
    for (int f = wid; f < nf; f += 4) {
      const int fm = f % TMF, fn = f / TMF;
      const T* xr = x + (fm * 16 + lo) * lda + lk;
      const T* wr = w + (fn * 16 + lo) * lda + lk;
      acc_t a0 = {}, a1 = {};
      for (int k = 0; k < Ip; k += 8) {
        a0 = MF::mma(xr[k], wr[k], a0);
        a1 = MF::mma(xr[k + 4], wr[k + 4], a1);
      }
      const T bv = b[fn * 16 + lo];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = fm * 16 + MF::acc_row(lane, r);
        T v = a0[r] + a1[r] + bv;
        if (!head) v = v > T(0) ? v : T(0);
        y[m * ldo + fn * 16 + lo] = v;
      }
    }
    block_sync();
  }

  // ---- loss, one lane of wave 0 per row, in place on the head's tile:
  // ppo_loss_bwd_k's formula (means over the node's M rows). Columns
  // past the head's width are already zero; rows past M become zero.
  if (wid == 0) {
    T* h = lds + prog.dz[(nl - 1) & 1];
    const int ldh = pad16(nt.out_dim[nl - 1]) + 2;
    const int m = lane;
    const bool valid = m < TM && m0 + m < M;
    const long row = l * M + m0 + m;
    const T invB = T(1) / T(M);
    T part = T(0);
    if (net == 0) {
      T d[losses::PPO_MAX_A];
      T cm = T(0);
      if (valid) {
        const T* a = acts + row * A;
        T sq = T(0);
#pragma unroll
        for (int j = 0; j < losses::PPO_MAX_A; ++j) {
          d[j] = T(0);
          if (j < A) {
            d[j] = a[j] - h[m * ldh + j];
            sq += d[j] * d[j];
          }
        }
        const T logp = T(-0.5) * sq * inv_cov - logc;
        const T r = ::exp(logp - old_logp[row]);
        const T ad = adv[row];
        const T rc = r < clip_lo ? clip_lo : (r > clip_hi ? clip_hi : r);
        const T s1 = r * ad, s2 = rc * ad;
        part = -(s1 < s2 ? s1 : s2) * invB;
        const bool pass = (r >= clip_lo && r <= clip_hi) ||
                          (ad > T(0) && r < clip_lo) ||
                          (ad < T(0) && r > clip_hi);
        const T g = pass ? ad : T(0);
        cm = -loss_scale * g * r * inv_cov * invB;
      } else {
#pragma unroll
        for (int j = 0; j < losses::PPO_MAX_A; ++j) d[j] = T(0);
      }
      if (m < TM) {
#pragma unroll
        for (int j = 0; j < losses::PPO_MAX_A; ++j) {
          if (j < A) h[m * ldh + j] = cm * d[j];
        }
      }
    } else if (m < TM) {
      T dv = T(0);
      if (valid) {
        const T e = h[m * ldh] - vtarg[row];
        part = e * e * invB;
        dv = loss_scale * critic_coef * T(2) * e * invB;
      }
      h[m * ldh] = dv;
    }
    part = wave_reduce_sum(part);
    if (lane == 0) fmnist::slab_store(&slab[nt.span], part);
  }
  block_sync();

  // ---- backward from the head down; one barrier per layer: dW (with
  // db) and dX of a layer read the same two images and dX writes the other dZ
  // image, which the layer above has finished with
  for (int li = nl - 1; li >= 0; --li) {
    const int I = nt.in_dim[li], O = nt.out_dim[li];
    const int Ip = pad16(I), Op = pad16(O);
    const int lda = Ip + 2, ldz = Op + 2;
    const T* dz = lds + prog.dz[li & 1];
    const T* x = lds + nt.aimg[li];
    const T* w = lds + nt.wimg[li];
    T* gw = slab + (nt.w_off[li] - nt.base);
    T* gb = slab + (nt.b_off[li] - nt.base);

    const int nfi = Ip >> 4;
    const int nfw = (Op >> 4) * nfi;
    for (int f = wid; f < nfw; f += 4) {
      const int fo = f / nfi, fi = f - fo * nfi;
      const T* ar = dz + lk * ldz + fo * 16 + lo;
      const T* br = x + lk * lda + fi * 16 + lo;
      acc_t a0 = {}, a1 = {}, ab = {};
      if (fi == 0) {  // wave-uniform: this fragment carries db as well
#pragma unroll
        for (int k = 0; k < TM; k += 8) {
          const T z0 = ar[k * ldz], z1 = ar[(k + 4) * ldz];
          a0 = MF::mma(z0, br[k * lda], a0);
          a1 = MF::mma(z1, br[(k + 4) * lda], a1);
          ab = MF::mma(z0, T(1), ab);
          ab = MF::mma(z1, T(1), ab);
        }
      } else {
#pragma unroll
        for (int k = 0; k < TM; k += 8) {
          a0 = MF::mma(ar[k * ldz], br[k * lda], a0);
          a1 = MF::mma(ar[(k + 4) * ldz], br[(k + 4) * lda], a1);
        }
      }
      const int i = fi * 16 + lo;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = fo * 16 + MF::acc_row(lane, r);
        if (o < O && i < I) {
          fmnist::slab_store(&gw[o * I + i], a0[r] + a1[r]);
        }
        if (fi == 0 && lo == 0 && o < O) {
          fmnist::slab_store(&gb[o], ab[r]);
        }
      }
    }

    if (li > 0) {  // the observations need no gradient
      T* dx = lds + prog.dz[(li - 1) & 1];
      const int nfx = TMF * nfi;
      for (int f = wid; f < nfx; f += 4) {
        const int fm = f % TMF, fi = f / TMF;
        const T* ar = dz + (fm * 16 + lo) * ldz + lk;
        const T* br = w + lk * lda + fi * 16 + lo;
        acc_t a0 = {}, a1 = {};
        for (int k = 0; k < Op; k += 8) {
          a0 = MF::mma(ar[k], br[k * lda], a0);
          a1 = MF::mma(ar[k + 4], br[(k + 4) * lda], a1);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int at =
              (fm * 16 + MF::acc_row(lane, r)) * lda + fi * 16 + lo;
          dx[at] = x[at] > T(0) ? a0[r] + a1[r] : T(0);
        }
      }
    }
    block_sync();
  }

  // ---- publish the slab and draw the (node, net)'s ticket, exactly as
  // fc_fwd_split_k does: the slab went out write-through, every wave
  // drains its stores, the block meets, one lane takes the ticket. The
  // block that draws the last one is the only one to touch the ticket
  // again and reads every slab word past its L1.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  block_sync();
  if (tid == 0) {
    int* tk = &tickets[l * 2 + net];
    const int got = __hip_atomic_fetch_add(tk, 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
    const int last = got == tiles - 1;
    if (last) {
      __hip_atomic_store(tk, 0, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    lastf = last;
  }
  block_sync();
  if (!lastf) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- reducer: every word of the net's slice and the loss word,
  // summed over the tiles in tile order whatever order they arrived in;
  // RED_U x RED_T clamped loads in flight per thread
  const T* sl = slabs + (l * 2 + net) * tiles * (long)prog.slab;
  const int P = nt.span + 1;
  T* gl = grad + l * n + nt.base;
  for (int j0 = tid; j0 < P; j0 += 256 * RED_U) {
    T s[RED_U] = {};
    for (int t0 = 0; t0 < tiles; t0 += RED_T) {
      T v[RED_T][RED_U];
#pragma unroll
      for (int q = 0; q < RED_T; ++q) {
        const T* p = sl + (long)min(t0 + q, tiles - 1) * prog.slab;
#pragma unroll
        for (int u = 0; u < RED_U; ++u) {
          v[q][u] = fmnist::slab_load(&p[min(j0 + 256 * u, P - 1)]);
        }
      }
#pragma unroll
      for (int q = 0; q < RED_T; ++q) {
        if (t0 + q < tiles) {
#pragma unroll
          for (int u = 0; u < RED_U; ++u) s[u] += v[q][u];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RED_U; ++u) {
      const int j = j0 + 256 * u;
      if (j < nt.span) gl[j] = s[u];
      else if (j == nt.span) loss[l * 2 + net] = s[u];
    }
  }
}

}  // namespace ppof
