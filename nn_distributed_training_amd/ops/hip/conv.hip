// MNISTConvNet head: Conv2d(1, F, k) + ReLU + MaxPool2d(2), fused
// forward and backward, batched over node replicas.
//
// The conv is the first layer, so backward only needs dW/db (no dX) —
// the whole layer costs two kernels per direction. Images are staged in
// LDS (28*28 doubles = 6.3 KB) so each of the k*k taps reads on-chip.

#include "common.h"

#include <type_traits>

namespace conv {

// X: [L*B, 28*28]; theta: [L, n] flat stack, W at w_off ([F,1,k,k]
// row-major = [F, k*k]), b at b_off; Y: [L*B, F*P*P] pooled+ReLU output;
// idx: [L*B, F*P*P] argmax position (0..3) for pool backward.
// Grid: one block per image, 256 threads (the launch bound). KMAX bounds
// the tap loops at compile time (K<=KMAX checked by the caller) so they
// fully unroll.
// src_idx != null: the image rows GATHER straight from the resident
// dataset (X = X_all [L, maxlen, IMG*IMG], row = src_idx[l*idx_stride
// + idx_off + b]) — the separate gather_batch launch and the xb
// buffer round-trip disappear from the fused-fc train path.
//
// Staging: the weight/bias loads do not depend on the index stream, so
// their first batch is issued BEFORE the src_idx -> image-row two-hop
// and lands under it; the image then loads in batches of four
// independent elements per thread (one L2 round trip for a 28x28 image
// on 256 threads, not one per 256 elements).
//
// Two block-uniform compute paths, chosen from the runtime K:
//  * K == KMAX (the model's K=5; K=7): one thread per POOLED PIXEL. It
//    reads the pixel's (K+1)x(K+1) image window from LDS into registers
//    once; the four pool positions are the four KxK sub-windows of it.
//    Per filter the K*K weights are read into registers (wave-uniform
//    LDS reads) and 4*K*K FMAs run back to back: no runtime tap guards,
//    so no branch or LDS wait between taps.
//  * K < KMAX (K=3, 4, 6): one thread per (filter, pooled pixel) with
//    runtime `break` guards in the unrolled tap loops. Every tap is then
//    its own LDS read -> wait -> FMA -> branch, which is why the
//    model's shape does not run here.
// Both sum each conv position as bias first, then taps row-major, one
// FMA each; ties keep the first pool position (strict >), and a window
// with no positive position gives Y=0, idx=0.
template <typename T, int KMAX>
__global__ __launch_bounds__(256) void conv_pool_fwd_k(
    const T* __restrict__ X, const T* __restrict__ theta,
    T* __restrict__ Y, unsigned char* __restrict__ idx,
    long n, long w_off, long b_off, int B, int F, int K, int IMG,
    const long* __restrict__ src_idx, long idx_stride, long idx_off,
    long maxlen) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  T* img = reinterpret_cast<T*>(smem_raw);             // [IMG*IMG]
  T* wgt = img + IMG * IMG;                            // [F*K*K + F]

  const long lb = blockIdx.x;           // image index in [0, L*B)
  const long l = lb / B;
  const int conv_out = IMG - (K - 1);
  const int P = conv_out / 2;
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;

  // this node's conv weights then bias, as one [F*K*K + F] image; the
  // first nthr elements (all 78 at the model's shape) load now
  const T* Wg = theta + l * n + w_off;
  const T* bg = theta + l * n + b_off;
  const int nw = F * K * K;
  const int nwb = nw + F;
  const auto wload = [&](int t) { return t < nw ? Wg[t] : bg[t - nw]; };
  const T w_first = tid < nwb ? wload(tid) : T(0);

  const long src_row =
      src_idx ? l * maxlen + src_idx[l * idx_stride + idx_off + lb % B]
              : lb;
  const T* src = X + src_row * IMG * IMG;
  const int npix = IMG * IMG;
  // clamped addresses: the four loads of a batch issue unconditionally,
  // back to back; only the LDS writes are bounds-guarded
  const auto ldbatch = [&](int t0, T (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + j * nthr + tid;
      v[j] = src[t < npix ? t : npix - 1];
    }
  };
  const auto stbatch = [&](int t0, const T (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + j * nthr + tid;
      if (t < npix) img[t] = v[j];
    }
  };
  {
    T v[4];
    ldbatch(0, v);
    if (tid < nwb) wgt[tid] = w_first;
    stbatch(0, v);
  }
  for (int t0 = 4 * nthr; t0 < npix; t0 += 4 * nthr) {
    T v[4];
    ldbatch(t0, v);
    stbatch(t0, v);
  }
  for (int t = nthr + tid; t < nwb; t += nthr) wgt[t] = wload(t);
  __syncthreads();

  const int PP = P * P;
  const int npool = F * PP;
  if (K == KMAX) {
    constexpr int WN = KMAX + 1;
    for (int t = tid; t < PP; t += nthr) {
      const int py = t / P;
      const int px = t % P;
      const T* wbase = img + (2 * py) * IMG + 2 * px;
      T win[WN * WN];
#pragma unroll
      for (int r = 0; r < WN; ++r) {
#pragma unroll
        for (int c = 0; c < WN; ++c) win[r * WN + c] = wbase[r * IMG + c];
      }
      for (int f = 0; f < F; ++f) {
        T w[KMAX * KMAX];
#pragma unroll
        for (int i = 0; i < KMAX * KMAX; ++i) {
          w[i] = wgt[f * KMAX * KMAX + i];
        }
        const T bias = wgt[nw + f];
        T best = T(0);       // ReLU floor: max(0, .) pooled
        int best_i = 0;
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
          if (acc > best) { best = acc; best_i = d; }
        }
        Y[lb * npool + f * PP + t] = best;
        idx[lb * npool + f * PP + t] = (unsigned char)best_i;
      }
    }
    return;
  }

  for (int t = tid; t < npool; t += nthr) {
    const int f = t / PP;
    const int py = (t / P) % P;
    const int px = t % P;
    const T* wf = wgt + f * K * K;
    const T bias = wgt[nw + f];

    T best = T(0);       // ReLU floor: max(0, .) pooled
    int best_i = 0;
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
      if (acc > best) { best = acc; best_i = d; }
    }
    Y[lb * npool + t] = best;          // relu(max pre-act) == max(relu)
    idx[lb * npool + t] = (unsigned char)best_i;
  }
}

// One level of the multi-value wave reduction below: N partials per
// lane become N/2. Lanes whose bit D is clear keep the even slot of
// each pair and send the odd one to lane^D; lanes with the bit set do
// the opposite; each adds what it receives. Slots at or past NREAL are
// compile-time zeros: a pair of two such slots needs no exchange. All
// subscripts are compile-time (the lane bit only drives selects), so
// the partials stay in registers.
template <typename T, int S, int N, int NREAL, int D>
DEV_INLINE void wave_halve_slots(T (&v)[S], bool hi) {
  constexpr int NX = (NREAL + 1) / 2;  // exchanges at this level
  T recv[NX];
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    const T a = v[2 * j];
    const T b = (2 * j + 1 < NREAL) ? v[2 * j + 1] : T(0);
    recv[j] = __shfl_xor(hi ? a : b, D, WAVE);
  }
  // every exchange of the level is issued before the first add waits
  // on one (left alone the scheduler pairs them up, and the level
  // becomes NX/2 dependent LDS-crossbar round trips instead of one)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    const T a = v[2 * j];
    const T b = (2 * j + 1 < NREAL) ? v[2 * j + 1] : T(0);
    v[j] = (hi ? b : a) + recv[j];
  }
}

template <typename T, int S, int N, int NREAL, int D>
DEV_INLINE void wave_reduce_slots_from(T (&v)[S], int lane) {
  if constexpr (D >= 1) {
    if constexpr (N > 1) {
      wave_halve_slots<T, S, N, NREAL, D>(v, (lane & D) != 0);
      wave_reduce_slots_from<T, S, N / 2, (NREAL + 1) / 2, D / 2>(v, lane);
    } else {
      v[0] += __shfl_xor(v[0], D, WAVE);
      wave_reduce_slots_from<T, S, 1, 1, D / 2>(v, lane);
    }
  }
}

// Wave-wide sums of NREAL per-lane partials v[0..NREAL) at once, as a
// halving butterfly: S (a power of two, NREAL <= S <= WAVE) slots are
// halved at xor distances 32, 16, ... until one is left, and any
// distances that remain are plain xor adds. That is S-1 exchanges (fewer
// with padding) in a dependent chain log2(WAVE) deep, where one
// wave_reduce_sum per slot is 6*NREAL exchanges in a chain as long.
// Returns the wave total of slot wave_slot_of<S>(lane) in every lane.
template <typename T, int S, int NREAL>
DEV_INLINE T wave_reduce_slots(T (&v)[S], int lane) {
  static_assert(S >= 2 && S <= WAVE && (S & (S - 1)) == 0, "bad S");
  static_assert(NREAL >= 1 && NREAL <= S, "bad NREAL");
  wave_reduce_slots_from<T, S, S, NREAL, WAVE / 2>(v, lane);
  return v[0];
}

// The slot whose total wave_reduce_slots leaves in `lane`: the first
// level hands slot parity to lane bit 5, the next one to bit 4, ..., so
// the slot number is the lane's top log2(S) bits reversed (lanes that
// differ only in the bits below hold the same total).
template <int S>
DEV_INLINE int wave_slot_of(int lane) {
  int s = 0;
#pragma unroll
  for (int bit = 1, d = WAVE / 2; bit < S; bit <<= 1, d >>= 1) {
    if (lane & d) s |= bit;
  }
  return s;
}

constexpr int pow2_at_least(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

// defined after conv_pool_bwd_body, whose end it is
template <typename T, int KMAX>
DEV_INLINE void conv_bwd_reduce_tail(
    T (&acc)[pow2_at_least(KMAX * KMAX + 1)], T* __restrict__ gstack,
    long n, long w_off, long b_off, int l, int f, int K, int tid,
    int nthr, T* __restrict__ red);

// Backward to weights/bias: route each pooled grad to its argmax conv
// position, multiply by the image window. dY is the grad AFTER the relu
// mask (pooled output > 0), applied by the caller via act_grad.
//
// Grid: (l, f, batch-chunk) so the chip fills (the v1 one-block-per-
// (l,f) version was 24 blocks on 256 CUs and 41% of round time);
// each thread accumulates a private dW[K*K]+db over its strided share
// of the chunk, each wave reduces its K*K+1 partials with one halving
// butterfly (wave_reduce_slots), the lanes left holding a total park it
// in LDS, and after ONE barrier the first KMAX*KMAX+1 threads combine
// the waves and atomically add into the grad stack (the caller zeroes
// the conv slice first).
//
// Two block-uniform compute paths, chosen from the runtime K:
//  * K == KMAX: no zero-grad skip and no runtime breaks, so the K*K
//    image loads of an item issue back to back. An item is two
//    dependent round trips: its (g, argmax) header together with its
//    source-row index, then its taps.
//  * K < KMAX: one item at a time with a zero-grad skip and runtime
//    `break` guards in the unrolled tap loops.
//
// The body takes its block index `bid`, thread index `tid`, block size
// `nthr` (a multiple of 64, at most 256) and its LDS scratch `red`
// ([(KMAX*KMAX+1)*4]) as arguments, so the merged backward launch
// (fused_mnist.hip dw_conv_bwd_k) can run it as one role of a flat grid.
template <typename T, int KMAX>
DEV_INLINE void conv_pool_bwd_body(
    const T* __restrict__ dY, const unsigned char* __restrict__ idx,
    const T* __restrict__ X, T* __restrict__ gstack,
    long n, long w_off, long b_off, int B, int F, int K, int IMG,
    int nchunk,
    const long* __restrict__ src_idx, long idx_stride, long idx_off,
    long maxlen, int bid, int tid, int nthr, T* __restrict__ red) {
  constexpr int NTAP = KMAX * KMAX;
  constexpr int NSLOT = pow2_at_least(NTAP + 1);
  const int chunk = bid % nchunk;
  const int f = (bid / nchunk) % F;
  const int l = bid / (nchunk * F);
  const int conv_out = IMG - (K - 1);
  const int P = conv_out / 2;
  const int npool = F * P * P;
  const int cb = (B + nchunk - 1) / nchunk;       // images per chunk
  const int b0 = chunk * cb;
  const int b1 = min(B, b0 + cb);

  // acc[0..NTAP) = dW taps (KMAX-strided), acc[NTAP] = db; the rest is
  // the butterfly's padding and is never read
  T acc[NSLOT];
#pragma unroll
  for (int i = 0; i <= NTAP; ++i) acc[i] = T(0);

  const int work = (b1 - b0) * P * P;
  if (K == KMAX) {
    // no per-element zero-skip branch and no runtime breaks inside the
    // unrolled GLOBAL-load chain — both forced per-element branch +
    // vmcnt waits around the K*K img loads (trap 4c); unconditional
    // taps pipeline (g = 0 contributes 0).
    // An item's header (g, argmax) and its source-row index load
    // together; the K*K taps follow as the second round trip. The
    // src_idx test is hoisted around the whole loop: as a branch inside
    // the iteration it puts a vmcnt(0) wait between the header loads.
    const auto run = [&](auto indexed) {
      for (int t = tid; t < work; t += nthr) {
        const int b = b0 + t / (P * P);
        const int pyx = t % (P * P);
        const long lb = (long)l * B + b;
        const long o = lb * npool + f * P * P + pyx;
        const T g = dY[o];
        const int d = idx[o];
        long row = lb;
        if constexpr (decltype(indexed)::value) {
          row = l * maxlen + src_idx[l * idx_stride + idx_off + b];
        }
        const int cy = 2 * (pyx / P) + (d >> 1);
        const int cx = 2 * (pyx % P) + (d & 1);
        const T* img = X + row * IMG * IMG + cy * IMG + cx;
        acc[NTAP] += g;
#pragma unroll
        for (int ky = 0; ky < KMAX; ++ky) {
#pragma unroll
          for (int kx = 0; kx < KMAX; ++kx) {
            acc[ky * KMAX + kx] += g * img[ky * IMG + kx];
          }
        }
      }
    };
    if (src_idx) {
      run(std::true_type{});
    } else {
      run(std::false_type{});
    }
  } else {
    for (int t = tid; t < work; t += nthr) {
      const int b = b0 + t / (P * P);
      const int py = (t / P) % P;
      const int px = t % P;
      const long lb = (long)l * B + b;
      const long o = lb * npool + f * P * P + py * P + px;
      const T g = dY[o];
      if (g == T(0)) continue;
      const int d = idx[o];
      const int cy = 2 * py + (d >> 1);
      const int cx = 2 * px + (d & 1);
      const long src_row =
          src_idx ? l * maxlen + src_idx[l * idx_stride + idx_off + b]
                  : lb;
      const T* img = X + src_row * IMG * IMG;
      acc[NTAP] += g;
      // compile-time bounds + KMAX-strided indices: a runtime
      // `ky*K+kx` subscript makes acc[] dynamically indexed and the
      // compiler spills the whole accumulator to scratch (rule 20)
#pragma unroll
      for (int ky = 0; ky < KMAX; ++ky) {
        if (ky >= K) break;
        const T* row = img + (cy + ky) * IMG + cx;
#pragma unroll
        for (int kx = 0; kx < KMAX; ++kx) {
          if (kx >= K) break;
          acc[ky * KMAX + kx] += g * row[kx];
        }
      }
    }
  }

  conv_bwd_reduce_tail<T, KMAX>(acc, gstack, n, w_off, b_off, l, f, K,
                                tid, nthr, red);
}

// The end of a conv-backward block: acc[0..KMAX*KMAX) are the thread's
// dW tap partials (KMAX-strided), acc[KMAX*KMAX] its db partial, all for
// filter f of node l.
// Reduce the K*K+1 partials: one butterfly per wave (no barriers; a
// lane without items, a wave without items and a tap skipped because
// K < KMAX all carry exact zeros), the lane that ends up with a
// slot's wave total parks it in LDS, then ONE barrier and the first
// KMAX*KMAX+1 threads finish their tap in parallel. Skipped taps are
// neither parked nor added. Every thread of the block must arrive.
// red: [tap][wave]
template <typename T, int KMAX>
DEV_INLINE void conv_bwd_reduce_tail(
    T (&acc)[pow2_at_least(KMAX * KMAX + 1)], T* __restrict__ gstack,
    long n, long w_off, long b_off, int l, int f, int K, int tid,
    int nthr, T* __restrict__ red) {
  constexpr int NTAP = KMAX * KMAX;
  constexpr int NSLOT = pow2_at_least(NTAP + 1);
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  T* wslice = gstack + (long)l * n + w_off + (long)f * K * K;
  const auto live = [&](int i) {
    return i == NTAP || (i < NTAP && i / KMAX < K && i % KMAX < K);
  };
  {
    const T tot = wave_reduce_slots<T, NSLOT, NTAP + 1>(acc, lane);
    const int i = wave_slot_of<NSLOT>(lane);
    const bool owner = (lane & (WAVE / NSLOT - 1)) == 0;
    if (owner && live(i)) red[i * 4 + wid] = tot;
  }
  __syncthreads();
  for (int i = tid; i < NTAP + 1; i += nthr) {
    if (!live(i)) continue;
    const T tot =
        red[i * 4] + red[i * 4 + 1] + red[i * 4 + 2] + red[i * 4 + 3];
    if (i == NTAP) {
      atomicAdd(&gstack[(long)l * n + b_off + f], tot);
    } else {
      atomicAdd(&wslice[(i / KMAX) * K + i % KMAX], tot);
    }
  }
}

template <typename T, int KMAX>
__global__ void conv_pool_bwd_k(
    const T* __restrict__ dY, const unsigned char* __restrict__ idx,
    const T* __restrict__ X, T* __restrict__ gstack,
    long n, long w_off, long b_off, int B, int F, int K, int IMG,
    int nchunk,
    const long* __restrict__ src_idx, long idx_stride, long idx_off,
    long maxlen) {
  __shared__ T red[(KMAX * KMAX + 1) * 4];
  conv_pool_bwd_body<T, KMAX>(
      dY, idx, X, gstack, n, w_off, b_off, B, F, K, IMG, nchunk,
      src_idx, idx_stride, idx_off, maxlen, blockIdx.x, threadIdx.x,
      blockDim.x, red);
}

}  // namespace conv
