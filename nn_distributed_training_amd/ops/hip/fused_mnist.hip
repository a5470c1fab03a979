// Fully fused MNIST train step (CDNA4).
//
// One kernel performs, per tile of T images of one node replica:
//   gather (index stream) -> conv+ReLU+maxpool -> fc1+ReLU ->
//   fc2 logits -> log-sum-exp + NLL dZ (targets read from the resident
//   label array) -> fc2 dW/db -> dh1 -> fc1 dW/db -> dpool ->
//   conv dW/db
// with every intermediate living in LDS. The layered engine ran this
// as ~12 launches per primal iteration with every activation making an
// HBM round trip; at n=28,440 the work per launch is tiny and the round
// is kernel-boundary-bound (profiles/README.md), so fusing the chain is
// the lever the per-kernel optimizations could not reach.
//
// Gradients accumulate ATOMICALLY into the [L, n] grad stack (caller
// zeroes it); blocks are independent (one per (l, image-tile)), so no
// inter-workgroup ordering is assumed anywhere. fc1's 27,648 weights
// stay in L2 (221 KB fp64 — larger than LDS); each block streams them
// for fc1-forward and once more for dpool.
//
// LDS budget at T=8, fp64: img 50.2KB + pool 27.6KB + h1/dh1 8KB +
// W2 5.2KB + W1 tile 8.3KB + small ~ 104KB -> 1 block/CU; T is a
// launch parameter (dynamic LDS).

#include "common.h"

namespace fmnist {

template <typename T>
__global__ __launch_bounds__(256) void mnist_train_step_k(
    const T* __restrict__ X_all,      // [L, maxlen, IMG*IMG]
    const long* __restrict__ Y_all,   // [L, maxlen]
    const long* __restrict__ idx,     // [L, S] index stream
    const long* __restrict__ offs_dev,  // nullable; slot `pit`
    const T* __restrict__ theta,      // [L, n]
    T* __restrict__ gparts,           // [L, NT, n] per-tile slabs
    T* __restrict__ loss,             // nullable [L]
    int pit, long idx_off, long idx_stride, long maxlen, long n,
    long wc_off, long bc_off, long w1_off, long b1_off, long w2_off,
    long b2_off,
    int B, int F, int K, int IMG, int H, int C, int TI, int NT,
    T loss_scale) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int conv_out = IMG - (K - 1);
  const int P = conv_out / 2;
  const int PF = F * P * P;          // pooled features (432)

  T* img = reinterpret_cast<T*>(smem_raw);        // [TI][IMG*IMG]
  T* pool = img + (long)TI * IMG * IMG;           // [TI][PF]
  T* h1 = pool + (long)TI * PF;                   // [TI][H]
  T* dh1 = h1 + (long)TI * H;                     // [TI][H]
  T* dz2 = dh1 + (long)TI * H;                    // [TI][C]
  T* wconv = dz2 + (long)TI * C;                  // [F*K*K + F]
  T* w2s = wconv + F * K * K + F;                 // [C*H + C]
  T* wt = w2s + (long)C * H + C;                  // [16][65] W1 tiles
  unsigned char* pidx =
      reinterpret_cast<unsigned char*>(wt + 16 * 65);
  long* src = reinterpret_cast<long*>(
      pidx + ((long)TI * PF + 15) / 16 * 16);     // [TI]

  const long l = blockIdx.z;
  const int tile = blockIdx.x;
  const int t0 = tile * TI;                       // first image index
  const int tcnt = min(TI, B - t0);
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);

  const T* th = theta + l * n;
  // this block's private gradient slab: every weight entry is written
  // exactly once by one thread (plain stores — the atomic version
  // serialized ~1.8M f64 atomics per launch); the fused optimizer step
  // reduces the NT slabs on the fly.
  T* gr = gparts + (l * (long)NT + tile) * n;
  const long off = offs_dev ? offs_dev[pit] : idx_off;

  // ---- P0: resolve sources, stage images + conv weights ----
  if (tid < tcnt) {
    src[tid] = idx[l * idx_stride + off + t0 + tid];
  }
  for (int t = tid; t < F * K * K + F; t += 256) {
    wconv[t] = th[wc_off + t];  // wc..|bc.. contiguous in the layout
  }
  for (int t = tid; t < C * H; t += 256) w2s[t] = th[w2_off + t];
  for (int t = tid; t < C; t += 256) w2s[C * H + t] = th[b2_off + t];
  __syncthreads();
  for (int u = tid; u < tcnt * IMG * IMG; u += 256) {
    const int t = u / (IMG * IMG);
    img[u] = X_all[(l * maxlen + src[t]) * IMG * IMG
                   + (u - t * IMG * IMG)];
  }
  __syncthreads();

  // ---- P1: conv + ReLU + maxpool forward ----
  for (int u = tid; u < tcnt * PF; u += 256) {
    const int t = u / PF;
    const int r = u - t * PF;
    const int f = r / (P * P);
    const int py = (r / P) % P;
    const int px = r % P;
    const T* wf = wconv + f * K * K;
    const T bias = wconv[F * K * K + f];
    const T* im = img + (long)t * IMG * IMG;
    T best = T(0);
    int best_i = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int cy = 2 * py + (d >> 1);
      const int cx = 2 * px + (d & 1);
      T acc = bias;
      for (int ky = 0; ky < K; ++ky) {
        const T* row = im + (cy + ky) * IMG + cx;
        const T* wr = wf + ky * K;
        for (int kx = 0; kx < K; ++kx) acc += row[kx] * wr[kx];
      }
      if (acc > best) { best = acc; best_i = d; }
    }
    pool[u] = best;
    pidx[u] = (unsigned char)best_i;
  }
  __syncthreads();

  // ---- P2: fc1 + ReLU as an LDS-tiled mini-GEMM. Per 16-deep
  // K-tile: stage wt[k][o] = W1[o][k0+k] with consecutive threads
  // reading consecutive W1-row elements (the v1 per-thread serial dot
  // walked W1 with a 3.5KB stride across lanes — the dominant cost of
  // the first fused version), then accumulate (t, o) outputs.
  const T* W1 = th + w1_off;
  {
    T acc[2] = {};  // (t, o) outputs per thread: TI*H/256 <= 2 at TI=8
    for (int k0 = 0; k0 < PF; k0 += 16) {
      for (int u = tid; u < H * 16; u += 256) {
        const int o = u / 16, k = u & 15;
        wt[k * 65 + o] =
            (k0 + k < PF) ? W1[(long)o * PF + k0 + k] : T(0);
      }
      __syncthreads();
      const int kmax = min(16, PF - k0);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int u = tid + a * 256;
        if (u < tcnt * H) {
          const int t = u / H;
          const int o = u - t * H;
          const T* x = pool + (long)t * PF + k0;
          T sacc = T(0);
          for (int k = 0; k < kmax; ++k) {
            sacc += x[k] * wt[k * 65 + o];
          }
          acc[a] += sacc;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int u = tid + a * 256;
      if (u < tcnt * H) {
        const T z = acc[a] + th[b1_off + (u % H)];
        h1[u] = z > T(0) ? z : T(0);
      }
    }
  }
  __syncthreads();

  // ---- P3: fc2 logits (W2 is LDS-resident) + LSE + NLL dZ ----
  for (int u = tid; u < tcnt * C; u += 256) {
    const int t = u / C;
    const int o = u - t * C;
    const T* w = w2s + (long)o * H;
    const T* x = h1 + (long)t * H;
    T acc = w2s[C * H + o];
    for (int i = 0; i < H; ++i) acc += x[i] * w[i];
    dz2[u] = acc;  // logits, converted in place below
  }
  __syncthreads();
  const T wmean = loss_scale / T(B);
  if (tid < tcnt) {
    T* z = dz2 + (long)tid * C;
    const int y = (int)Y_all[l * maxlen + src[tid]];
    T mx = z[0];
    for (int c = 1; c < C; ++c) mx = z[c] > mx ? z[c] : mx;
    T sum = T(0);
    for (int c = 0; c < C; ++c) sum += ::exp(z[c] - mx);
    const T lse = mx + ::log(sum);
    if (loss != nullptr) {
      atomicAdd(&loss[l], -(z[y] - lse) / T(B));
    }
    for (int c = 0; c < C; ++c) {
      z[c] = (::exp(z[c] - lse) - (c == y ? T(1) : T(0))) * wmean;
    }
  }
  __syncthreads();

  // ---- P4: fc2 dW/db ----
  for (int u = tid; u < C * H + C; u += 256) {
    T acc = T(0);
    if (u < C * H) {
      const int o = u / H;
      const int i = u - o * H;
      for (int t = 0; t < tcnt; ++t) {
        acc += dz2[(long)t * C + o] * h1[(long)t * H + i];
      }
      gr[w2_off + u] = acc;
    } else {
      const int o = u - C * H;
      for (int t = 0; t < tcnt; ++t) acc += dz2[(long)t * C + o];
      gr[b2_off + o] = acc;
    }
  }

  // ---- P5: dh1 = dz2 @ W2, ReLU' ----
  for (int u = tid; u < tcnt * H; u += 256) {
    const int t = u / H;
    const int i = u - t * H;
    T acc = T(0);
    for (int o = 0; o < C; ++o) {
      acc += dz2[(long)t * C + o] * w2s[(long)o * H + i];
    }
    dh1[u] = (h1[u] > T(0)) ? acc : T(0);
  }
  __syncthreads();

  // ---- P6: fc1 dW/db ----
  for (int u = tid; u < H * PF; u += 256) {
    const int o = u / PF;
    const int i = u - o * PF;
    T acc = T(0);
    for (int t = 0; t < tcnt; ++t) {
      acc += dh1[(long)t * H + o] * pool[(long)t * PF + i];
    }
    gr[w1_off + u] = acc;
  }
  for (int u = tid; u < H; u += 256) {
    T acc = T(0);
    for (int t = 0; t < tcnt; ++t) acc += dh1[(long)t * H + u];
    gr[b1_off + u] = acc;
  }
  __syncthreads();

  // ---- P7: dpool = dh1 @ W1 as a tiled GEMM over 64-wide i-tiles and
  // 16-deep o-tiles: wt[o][i] staged with consecutive threads reading
  // consecutive W1 elements (coalesced), accumulators in registers.
  // pool is reused as dpool (safe: P6's readers hit the barrier above;
  // the ReLU' mask is applied from the saved sign via a fresh read of
  // pool BEFORE overwrite within the same thread's element).
  {
    for (int i0 = 0; i0 < PF; i0 += 64) {
      const int imax = min(64, PF - i0);
      T acc[2] = {};  // (t, ii) outputs: TI*64/256 = 2 at TI = 8
      for (int o0 = 0; o0 < H; o0 += 16) {
        // wt[o][ii] = W1[o0+o][i0+ii]; thread u: o = u/64, ii = u%64
        for (int u = tid; u < 16 * 64; u += 256) {
          const int o = u / 64, ii = u & 63;
          wt[o * 65 + ii] = (ii < imax)
                                ? W1[(long)(o0 + o) * PF + i0 + ii]
                                : T(0);
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          const int u = tid + a * 256;
          const int t = u / 64;
          const int ii = u & 63;
          if (t < tcnt) {
            const T* g = dh1 + (long)t * H + o0;
            T sacc = T(0);
            for (int o = 0; o < 16; ++o) {
              sacc += g[o] * wt[o * 65 + ii];
            }
            acc[a] += sacc;
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int u = tid + a * 256;
        const int t = u / 64;
        const int ii = u & 63;
        if (t < tcnt && ii < imax) {
          const long e = (long)t * PF + i0 + ii;
          pool[e] = (pool[e] > T(0)) ? acc[a] : T(0);
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- P8: conv dW/db via argmax routing ----
  for (int f = 0; f < F; ++f) {
    T dw[7 * 7];
    T db = T(0);
#pragma unroll
    for (int i = 0; i < 7 * 7; ++i) dw[i] = T(0);
    for (int u = tid; u < tcnt * P * P; u += 256) {
      const int t = u / (P * P);
      const int py = (u / P) % P;
      const int px = u % P;
      const long e = (long)t * PF + f * P * P + py * P + px;
      const T g = pool[e];
      if (g == T(0)) continue;
      const int d = pidx[e];
      const int cy = 2 * py + (d >> 1);
      const int cx = 2 * px + (d & 1);
      const T* im = img + (long)t * IMG * IMG;
      db += g;
      for (int ky = 0; ky < K; ++ky) {
        const T* row = im + (cy + ky) * IMG + cx;
        for (int kx = 0; kx < K; ++kx) dw[ky * K + kx] += g * row[kx];
      }
    }
    T* red = wt;  // W1-tile buffer is free in P8; [4] per value
    const int wid = tid / WAVE;
    for (int i = 0; i < K * K + 1; ++i) {
      T v = (i < K * K) ? dw[i] : db;
      v = wave_reduce_sum(v);
      if (lane == 0) red[wid] = v;
      __syncthreads();
      if (tid == 0) {
        const T tot = red[0] + red[1] + red[2] + red[3];
        if (i < K * K) {
          gr[wc_off + (long)f * K * K + i] = tot;
        } else {
          gr[bc_off + f] = tot;
        }
      }
      __syncthreads();
    }
  }
}


// ---------------------------------------------------------------------
// Fused fc BLOCK: fc1+ReLU -> fc2 logits -> log-softmax+NLL -> fc2
// dW/db -> dz1 -> dX0 (replaces 7 small kernels: 2x linear_fwd,
// nll_fused, 2x linear_bwd_dw, 2x linear_bwd_dx — each near the ~5 us
// kernel floor, ~65 us/iteration of GPU time at the MNIST bench shapes,
// profiles/mnist_r2d_topk.txt). The conv layer stays separate (its
// kernels are not floor-bound); fc1 dW/db run on the store-path dw
// kernel from the exported dz1.
//
// The big contractions run on the f64/f32 MFMA matrix cores: fc1 fwd
// (K = I) and dX0 (K = H); y1 is LDS-resident and never touches HBM.
// A row tile is RT(16) rows of one node. Requires H <= 64, C <= 16;
// the fc2 grad slices accumulate atomically (caller zeroes the whole
// grad stack).
//
// Two chip-filling launches. As one launch of one block per row tile
// this was 32 blocks at the MNIST shape (8 nodes x 64 rows): each
// pulled all of W1 through one CU for the fc1 forward and again for
// dX0 while 7/8 of the chip idled. Here the fc1 forward is split over K
// (fc_fwd_split_k: row tiles x S slices, the last slice block to
// arrive runs the tail) and dX0 is a grid of its own (fc_dx0_k: one
// block per 16-column strip of I). No block ever waits for another.
constexpr int FC_RT = 16;
constexpr int FC_W2S = 65;  // padded LDS row stride of W2

// Diagnostic phase clock (compiled out unless the extension is built
// with NDTA_BUILD_DEFINES=-DNDTA_FC_PHASE_CLOCK): thread 0 of each
// block stamps wall_clock64() (100 MHz) at the phase boundaries into
// fc_phase_stamps[block][slot]; ext.fc_phase_clock() reads them back.
// The diagnostic build adds one barrier before the last stamp so slot 5
// is the block's end, not wave 0's. fc_block_k: slots 0-5 bound P0..P4.
// fc_fwd_split_k: 0 staged, 1 MFMA loop and slab stores issued, 2
// ticket drawn (reducers only), 3 slabs summed and y1 in LDS, 4 P2
// done, 5 P3 done.
#ifdef NDTA_FC_PHASE_CLOCK
constexpr int FC_CLK_BLOCKS = 256;
__device__ unsigned long long fc_phase_stamps[FC_CLK_BLOCKS * 8];
#define FC_STAMP(slot)                                              \
  do {                                                              \
    if (threadIdx.x == 0) {                                         \
      const int b_ = blockIdx.z * gridDim.x + blockIdx.x;           \
      if (b_ < FC_CLK_BLOCKS) {                                     \
        fc_phase_stamps[b_ * 8 + (slot)] = wall_clock64();          \
      }                                                             \
    }                                                               \
  } while (0)
// a block that runs no tail (fc_fwd_split_k's non-reducers) zeroes its
// slot 2, so that the reader can tell this launch's reducers
#define FC_STAMP_NONE(slot)                                         \
  do {                                                              \
    const int b_ = blockIdx.z * gridDim.x + blockIdx.x;             \
    if (b_ < FC_CLK_BLOCKS) fc_phase_stamps[b_ * 8 + (slot)] = 0;   \
  } while (0)
#else
#define FC_STAMP(slot) do {} while (0)
#define FC_STAMP_NONE(slot) do {} while (0)
#endif
// W2 into its LDS image [16][FC_W2S] for the tail below: element t of
// the [16 c][64 h] tile, a real zero where c >= C or h >= H (the tail's
// MFMA operands sweep the whole tile, and 0 x stale LDS could be NaN).
// The load is clamped, not branched, so it can sit in a batch of loads.
template <typename T>
DEV_INLINE T fc_w2_tile_load(const T* __restrict__ W2, int t, int H,
                             int C) {
  const int c = t >> 6, h = t & 63;
  const T v = W2[min(c, C - 1) * H + min(h, H - 1)];
  return (c < C && h < H) ? v : T(0);
}

// The fc2 tail of a 16-row tile, written once for fc_block_k and
// fc_fwd_split_k: from y1 in LDS through the logits, log-softmax + NLL
// and dZ2 (P2) to the dz1 store and the fc2 dW/db atomics (P3). Every
// thread of the block calls it (it holds two barriers); waves 0-3 work.
//
// The three products are one 16x16 MFMA tile each per wave, 4 k-steps:
//   logits Z[m][c]  = y1[m][:] . W2[c][:]   wave w sums h in [16w, 16w+16)
//   dz1[m][h]       = dZ2[m][:] . W2[:][h]  wave w owns h-fragment 16w
//   fc2 dW[c][h]    = dZ2[:][c] . y1[:][h]  wave w owns h-fragment 16w
// The four partial logit tiles meet in zps and are added to b2 in wave
// order, so the sum does not depend on timing. The operands sweep pad
// rows and columns, which must be real zeros: W2 rows C..15 and columns
// H..63 (fc_w2_tile_load), y1 columns H..63 (the caller's y1 store),
// dZ2 columns C..15 (written here). Rows at or past M have dZ2 = 0, so
// they add nothing to dW/db.
//
// LDS strides stay 65 (W2, y1) and 17 (dZ2, zps). A fragment read is
// either lo * stride + lk (16 rows x 4 k) or lk * stride + lo (4 k x 16
// columns), banked over 32 lanes (lk in {0,1} or {2,3}). With 17 both
// forms have one colliding pair; with 65 both are 2-way (2 extra LDS
// cycles per read, ~28 reads per wave). No stride clears both forms
// (the first wants 2 mod 32, the second 16 mod 32), and 66 would only
// move the conflict from the logits to the other two products.
//
// tgt_of(m) is row m's target; it is called only for rows below M.
template <typename T, bool KEEP_DZ1, int SLOT_P2, typename TgtFn>
DEV_INLINE void fc_tail(
    const T* w2s,            // [16][FC_W2S] | b2 at [16 * FC_W2S]
    const T* y1s,            // [16][65]
    T* dz2s,                 // [16][17]
    T* zps,                  // [4][16][17] scratch
    T* dz1s,                 // [16][65] dz1 kept in LDS (KEEP_DZ1)
    TgtFn tgt_of,
    T* __restrict__ grad_l,  // the node's grad slice
    T* __restrict__ dz1t,    // the tile's first dz1 row
    T* __restrict__ loss_l,  // nullable
    long w2_off, long b2_off, int m0, int M, int H, int C,
    T loss_scale) {
  using MF = gmfma::mfma_t<T>;
  using acc_t = typename MF::acc_t;
  constexpr int RT = FC_RT;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int lo = lane & 15;
  const int lk = lane >> 4;
  const bool work = wid < 4;  // wave-uniform
  const int h0 = wid * 16;

  // P2: fc2 logits, this wave's quarter of the contraction
  if (work) {
    acc_t z = {};
    const T* Ar = y1s + lo * 65 + h0 + lk;      // y1[m = lo][h]
    const T* Br = w2s + lo * FC_W2S + h0 + lk;  // W2[c = lo][h]
#pragma unroll
    for (int kk = 0; kk < 16; kk += 4) z = MF::mma(Ar[kk], Br[kk], z);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      zps[wid * (RT * 17) + MF::acc_row(lane, r) * 17 + lo] = z[r];
    }
  }
  __syncthreads();

  // log-softmax + NLL dZ2, one (row, class) per thread: row m's classes
  // sit in 16 adjacent lanes, so the row max and the row sum are 4
  // xor-shuffles each and every exp runs once.
  if (work) {
    const int m = tid >> 4, c = tid & 15;
    const bool act = c < C;
    const bool rowok = (m0 + m) < M;
    T z = -INFINITY;
    if (act) {
      z = w2s[16 * FC_W2S + c];  // b2
#pragma unroll
      for (int w = 0; w < 4; ++w) z += zps[w * (RT * 17) + m * 17 + c];
    }
    T mx = z;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      const T o = __shfl_xor(mx, off, 16);
      mx = o > mx ? o : mx;
    }
    const T e = act ? ::exp(z - mx) : T(0);
    T sum = e;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      sum += __shfl_xor(sum, off, 16);
    }
    T dz = T(0);
    if (act && rowok) {
      const int tgt = tgt_of(m);
      dz = (e / sum - (c == tgt ? T(1) : T(0))) * (loss_scale / T(M));
      if (c == tgt && loss_l != nullptr) {
        const T lse = mx + ::log(sum);
        atomicAdd(loss_l, -(z - lse) / T(M));
      }
    }
    dz2s[m * 17 + c] = dz;  // pad classes too: an MFMA operand
  }
  __syncthreads();
  FC_STAMP(SLOT_P2);

  // P3: dz1 = (dZ2 @ W2) * relu'(y1) -> global (and LDS for a caller
  // that goes on to dX0); fc2 dW/db
  if (work) {
    acc_t d1 = {}, dw = {};
    const T* A1 = dz2s + lo * 17 + lk;           // dZ2[m = lo][c]
    const T* B1 = w2s + lk * FC_W2S + h0 + lo;   // W2[c][h]
    const T* A2 = dz2s + lk * 17 + lo;           // dZ2[m][c = lo]
    const T* B2 = y1s + lk * 65 + h0 + lo;       // y1[m][h]
#pragma unroll
    for (int kk = 0; kk < 16; kk += 4) {
      d1 = MF::mma(A1[kk], B1[kk * FC_W2S], d1);
      dw = MF::mma(A2[kk * 17], B2[kk * 65], dw);
    }
    const int h = h0 + lo;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = MF::acc_row(lane, r);  // m of d1, c of dw
      const T v = y1s[row * 65 + h] > T(0) ? d1[r] : T(0);
      if (KEEP_DZ1) dz1s[row * 65 + h] = v;  // 0 where h >= H
      if (m0 + row < M && h < H) dz1t[(long)row * H + h] = v;
      if (row < C && h < H) {
        atomicAdd(&grad_l[w2_off + row * H + h], dw[r]);
      }
    }
  }
  if (tid >= 32 && tid < 32 + C) {
    const int c = tid - 32;
    T s = T(0);
    for (int m = 0; m < RT; ++m) s += dz2s[m * 17 + c];
    atomicAdd(&grad_l[b2_off + c], s);
  }
}

// fc_block_k: the whole block as ONE launch, one 512-thread block per
// row tile. Kept for stacks with so many row tiles that the split
// forward's grid would pass the CU count (ext.hip fc_kernel_for).
// one 16-column strip of the dX0 pass: W1[0:64, ix:ix+16] as 16 MFMA B
// operands plus the x0 values that carry the conv relu' mask for the
// lane's four output elements
template <typename T>
struct fc_strip_t {
  T w[16];
  T xm[4];
};

template <typename T>
__global__ __launch_bounds__(512) void fc_block_k(
    const T* __restrict__ x0,        // [L*M, I] conv/pool output
    const T* __restrict__ theta,     // [L, n]
    const long* __restrict__ Y_all,  // [L, maxlen] targets
    const long* __restrict__ idx,    // index stream
    long idx_stride, long idx_off, long maxlen,
    T* __restrict__ grad,            // [L, n]
    T* __restrict__ dx0,             // [L*M, I]
    T* __restrict__ dz1g,            // [L*M, H] dz1 out (fc1 dW/db
                                     // run on the store-path dw
                                     // kernel: the in-kernel atomic dW1
                                     // was ~884K f64 atomics/launch)
    T* __restrict__ loss,            // nullable [L]
    long n, long w1_off, long b1_off, long w2_off, long b2_off,
    int M, int I, int H, int C, T loss_scale, int mask_dx0) {
  // 512 threads = 4 CONSUMER waves (MFMA) + 4 PRODUCER waves (HBM ->
  // double-buffered LDS) for the fc1 forward: W1's 221 KB/block stream
  // was the serial chain of the 256-thread version (stage, barrier,
  // MFMA, barrier x14); wave specialization keeps the stream off the
  // compute path. All 8 waves then share the log-softmax (one (row,
  // class) per thread) and the dX0 strips, whose first W1 loads are
  // issued before the fc2 phases so they land under them.
  using MF = gmfma::mfma_t<T>;
  using acc_t = typename MF::acc_t;
  using strip_t = fc_strip_t<T>;
  typedef T vec2 __attribute__((ext_vector_type(2)));
  constexpr int RT = FC_RT;

  // single LDS arena (trap 4a)
  __shared__ T lds[2 * 32 * (RT + 1) + 2 * 32 * 65 + 2 * RT * 65 +
                   RT * 17 + 16 * FC_W2S + 16];
  T* As = lds;                             // [2][32][RT+1]
  T* Bs = As + 2 * 32 * (RT + 1);          // [2][32][65]
  T* y1s = Bs + 2 * 32 * 65;               // [RT][65]
  T* dz1s = y1s + RT * 65;                 // [RT][65]
  T* dz2s = dz1s + RT * 65;                // [RT][17]
  T* w2s = dz2s + RT * 17;                 // [C][65] | b2 at [16*65]

  const long l = blockIdx.z;
  const int m0 = blockIdx.x * RT;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;                // 0-3 consume, 4-7 produce
  const bool producer = wid >= 4;
  const T* th = theta + l * n;
  const T* W1 = th + w1_off;
  const T* b1 = th + b1_off;
  const int lo = lane & 15;
  const int lk = lane >> 4;
  const bool fullm = (m0 + RT) <= M;
  const int nst = (I + 31) / 32;
  const T* x0b = x0 + (long)(l * (long)M + m0) * I;  // block's rows

  FC_STAMP(0);
  // P0: W2 as the tail's zero-padded [16][64] tile (row stride 65) + b2
  for (int t = tid; t < 16 * 64; t += 512) {
    w2s[(t >> 6) * FC_W2S + (t & 63)] =
        fc_w2_tile_load(th + w2_off, t, H, C);
  }
  for (int t = tid; t < C; t += 512) {
    w2s[16 * FC_W2S + t] = th[b2_off + t];
  }
  FC_STAMP(1);

  // producer staging: 256 threads cover the [32 k][RT m] x0 image
  // (1 vec2 pair each) and the [32 k][64 o] W1 image (4 pairs)
  const int ptid = tid - 256;
  const int am = producer ? ptid / 16 : 0;
  const int akp = producer ? ptid % 16 : 0;
  const auto stage = [&](int buf, int k0) {
    T* Ab = As + buf * 32 * (RT + 1);
    T* Bb = Bs + buf * 32 * 65;
    if (fullm && (k0 + 32) <= I && H == 64) {  // guard-free (trap 4c)
      const vec2 va = *reinterpret_cast<const vec2*>(
          &x0[(long)(l * (long)M + m0 + am) * I + k0 + 2 * akp]);
      Ab[(2 * akp) * (RT + 1) + am] = va.x;
      Ab[(2 * akp + 1) * (RT + 1) + am] = va.y;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const vec2 vb = *reinterpret_cast<const vec2*>(
            &W1[(long)(am + q * 16) * I + k0 + 2 * akp]);
        Bb[(2 * akp) * 65 + am + q * 16] = vb.x;
        Bb[(2 * akp + 1) * 65 + am + q * 16] = vb.y;
      }
    } else {
      const int k_ = k0 + 2 * akp;
      vec2 va = vec2{0, 0};
      if (m0 + am < M) {
        if (k_ + 1 < I) {
          va = *reinterpret_cast<const vec2*>(
              &x0[(long)(l * (long)M + m0 + am) * I + k_]);
        } else if (k_ < I) {
          va.x = x0[(long)(l * (long)M + m0 + am) * I + k_];
        }
      }
      Ab[(2 * akp) * (RT + 1) + am] = va.x;
      Ab[(2 * akp + 1) * (RT + 1) + am] = va.y;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = am + q * 16;
        vec2 vb = vec2{0, 0};
        if (o < H) {
          if (k_ + 1 < I) {
            vb = *reinterpret_cast<const vec2*>(&W1[(long)o * I + k_]);
          } else if (k_ < I) {
            vb.x = W1[(long)o * I + k_];
          }
        }
        Bb[(2 * akp) * 65 + o] = vb.x;
        Bb[(2 * akp + 1) * 65 + o] = vb.y;
      }
    }
  };

  // P1: fc1 forward on MFMA (consumer waves: one 16-wide o-fragment
  // each) while producers fill the next stage's buffers
  acc_t a1 = {};
  const int o0w = wid * 16;  // consumers: 0..48
  if (producer) stage(0, 0);
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    if (producer) {
      if (st + 1 < nst) stage((st + 1) & 1, (st + 1) * 32);
    } else {
      const T* Ab = As + (st & 1) * 32 * (RT + 1);
      const T* Bb = Bs + (st & 1) * 32 * 65;
#pragma unroll
      for (int kk = 0; kk < 32; kk += 4) {
        const int ka = kk + lk;
        const T a = Ab[ka * (RT + 1) + lo];
        const T b = Bb[ka * 65 + o0w + lo];
        a1 = MF::mma(a, b, a1);
      }
    }
    __syncthreads();
  }

  // dX0 strips (P4) are dealt round-robin to the waves as well; the
  // first two strips' W1 columns and x0 mask values do not depend on
  // anything computed here, so they load now and land under P2/P3.
  const int nstrip = (I + 15) / 16;
  const auto ldstrip = [&](int s, strip_t& st) {
    if (s >= nstrip) return;  // wave-uniform
    const int i = s * 16 + lo;
    if (H == 64 && s * 16 + 16 <= I && fullm) {  // guard-free (4c)
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        st.w[t] = W1[(long)(4 * t + lk) * I + i];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st.xm[r] = mask_dx0
                       ? x0b[(long)MF::acc_row(lane, r) * I + i]
                       : T(1);
      }
    } else {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        st.w[t] = ((4 * t + lk) < H && i < I)
                      ? W1[(long)(4 * t + lk) * I + i]
                      : T(0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = MF::acc_row(lane, r);
        st.xm[r] = !mask_dx0 ? T(1)
                   : (m0 + m < M && i < I) ? x0b[(long)m * I + i]
                                           : T(0);
      }
    }
  };
  strip_t sa, sb;
  ldstrip(wid, sa);
  ldstrip(wid + 8, sb);

  // y1 = relu(z1 + b1) into LDS (never stored to HBM), a real zero in
  // the columns past H: the tail's MFMA operands sweep all 64
  if (!producer) {
    const int o = o0w + lo;
    const T bo = b1[min(o, H - 1)];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = MF::acc_row(lane, r);
      const T z = a1[r] + bo;
      y1s[m * 65 + o] = (o < H && z > T(0)) ? z : T(0);
    }
  }
  __syncthreads();
  FC_STAMP(2);

  // P2 + P3: the shared fc2 tail (waves 0-3); its logit partials use
  // the stream's B buffers, free since P1's last barrier. dz1 stays in
  // LDS for P4, zero in the pad columns the dX0 MFMA sweeps over.
  fc_tail<T, true, 3>(
      w2s, y1s, dz2s, Bs, dz1s,
      [&](int m) {
        return (int)
            Y_all[l * maxlen + idx[l * idx_stride + idx_off + m0 + m]];
      },
      grad + l * n, dz1g + (long)(l * (long)M + m0) * H,
      loss != nullptr ? loss + l : nullptr, w2_off, b2_off, m0, M, H, C,
      loss_scale);
  __syncthreads();
  FC_STAMP(4);

  // P4: dX0 = dz1 @ W1 with the conv relu' mask. A[m][k=o] from LDS,
  // B[k=o][i] = the strip's W1 columns, already in registers. Wave w
  // owns strips w, w+8, ...; as soon as a slot's MFMAs have issued it
  // reloads with the strip two ahead, so a wave always has its next
  // strip complete or in flight. Two accumulators halve the MFMA
  // dependency chain.
  const auto dx_strip = [&](int s, const strip_t& st) {
    acc_t ax0 = {}, ax1 = {};
#pragma unroll
    for (int t = 0; t < 16; t += 2) {
      ax0 = MF::mma(dz1s[lo * 65 + 4 * t + lk], st.w[t], ax0);
      ax1 = MF::mma(dz1s[lo * 65 + 4 * t + 4 + lk], st.w[t + 1], ax1);
    }
    const int i = s * 16 + lo;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = MF::acc_row(lane, r);
      if (m0 + m < M && i < I) {
        // conv relu' mask: x0 IS the conv block's relu output
        dx0[(long)(l * (long)M + m0 + m) * I + i] =
            st.xm[r] > T(0) ? ax0[r] + ax1[r] : T(0);
      }
    }
  };
  for (int s = wid; s < nstrip; s += 16) {
    dx_strip(s, sa);
    ldstrip(s + 16, sa);
    if (s + 8 < nstrip) dx_strip(s + 8, sb);
    ldstrip(s + 24, sb);
  }
#ifdef NDTA_FC_PHASE_CLOCK
  __syncthreads();
  FC_STAMP(5);
#endif
}

//
// fc_fwd_split_k LDS arena (one dynamic array): the fixed tail arenas
// first, then the [80][KSP] operand image: rows 0-15 the x0 tile slice,
// rows 16-79 the W1 slice, both row-major in k exactly as they sit in
// memory, so staging is 16-byte loads and 16-byte LDS stores. KSP = 2
// (mod 32) keeps the MFMA fragment reads (16 rows x 4 k per wave) off
// each other's banks in fp64 and fp32.
constexpr int FCS_W2 = 0;                          // [17][65] W2 | b2
constexpr int FCS_Y1 = FCS_W2 + 17 * FC_W2S;       // [16][65]
constexpr int FCS_DZ2 = FCS_Y1 + FC_RT * 65;       // [16][17]
constexpr int FCS_FLAG = FCS_DZ2 + FC_RT * 17;     // "I am last" word
constexpr int FCS_STG = 2424;                      // 16-byte multiple
static_assert(FCS_FLAG + 2 <= FCS_STG, "fc split arena overlap");
// the tail's logit partials reuse the operand image (KSP >= 34)
static_assert(4 * FC_RT * 17 <= (FC_RT + 64) * 34, "fc split zps");
constexpr int FCS_ROWS = FC_RT + 64;               // image rows
constexpr int FCS_NLD = 18;  // staging loads in flight per thread

// padded row length of the operand image for a KS-wide slice
inline int fc_split_ksp(int KS) {
  return KS + ((2 - KS % 32) + 32) % 32;
}

// elements of dynamic LDS fc_fwd_split_k needs for a KS-wide slice
inline long fc_split_lds_elems(int KS) {
  return FCS_STG + (long)FCS_ROWS * fc_split_ksp(KS);
}

// A slab word crosses from its slice block to the tile's reducer inside
// one launch. Relaxed agent-scope atomic accesses of the word's bits
// are the write-through store and the L1-bypassing load that such a
// hand-off needs (the .s shows both with the sc1 bit).
template <typename T>
struct slab_bits { using type = unsigned long long; };
template <>
struct slab_bits<float> { using type = unsigned; };

template <typename T>
DEV_INLINE void slab_store(T* p, T v) {
  using U = typename slab_bits<T>::type;
  __hip_atomic_store(reinterpret_cast<U*>(p), __builtin_bit_cast(U, v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T>
DEV_INLINE T slab_load(const T* p) {
  using U = typename slab_bits<T>::type;
  return __builtin_bit_cast(
      T, __hip_atomic_load(reinterpret_cast<const U*>(p),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

template <typename T>
__global__ __launch_bounds__(256) void fc_fwd_split_k(
    const T* __restrict__ x0,        // [L*M, I] conv/pool output
    const T* __restrict__ theta,     // [L, n]
    const long* __restrict__ Y_all,  // [L, maxlen] targets
    const long* __restrict__ idx,    // index stream
    long idx_stride, long idx_off, long maxlen,
    T* __restrict__ grad,            // [L, n]
    T* __restrict__ dz1g,            // [L*M, H] dz1 out
    T* __restrict__ loss,            // nullable [L]
    T* slabs,                        // [tiles, S, 16, 64] partial z1
    int* tickets,                    // [tiles], zero between launches
    long n, long w1_off, long b1_off, long w2_off, long b2_off,
    int M, int I, int H, int C, T loss_scale, int mtiles, int S, int KS,
    int KSP) {
  using MF = gmfma::mfma_t<T>;
  using acc_t = typename MF::acc_t;
  typedef T vec2 __attribute__((ext_vector_type(2)));
  constexpr int RT = FC_RT;
  extern __shared__ __align__(16) unsigned char fcs_raw[];
  T* lds = reinterpret_cast<T*>(fcs_raw);
  T* w2s = lds + FCS_W2;
  T* y1s = lds + FCS_Y1;
  T* dz2s = lds + FCS_DZ2;
  int* lastf = reinterpret_cast<int*>(lds + FCS_FLAG);
  T* stg = lds + FCS_STG;

  const int tile = blockIdx.x / S;
  const int slice = blockIdx.x - tile * S;
  const long l = tile / mtiles;
  const int m0 = (tile - (int)l * mtiles) * RT;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int lo = lane & 15;
  const int lk = lane >> 4;
  const T* th = theta + l * n;
  const T* W1 = th + w1_off;
  const T* x0b = x0 + (long)(l * (long)M + m0) * I;
  const int kb = slice * KS;
  const int klen = min(KS, I - kb);  // <= 0: an empty slice

  // what only the reducer's tail needs still loads in every block, in
  // the staging round trip and clamped not branched, so that the tail
  // starts no load chain of its own: the row's index-stream entry (its
  // target is fetched below, once this has landed), W2, b2 and b1
  const long trow =
      idx[l * idx_stride + idx_off + min(m0 + (tid >> 4), M - 1)];
  T w2v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w2v[j] = fc_w2_tile_load(th + w2_off, tid + j * 256, H, C);
  }
  const T b2v = th[b2_off + min(tid, C - 1)];
  const T b1v = th[b1_off + min(tid & 63, H - 1)];

  if (klen == KS && m0 + RT <= M && H == 64) {
    // full slice: guard-free 16-byte loads, FCS_NLD per thread in
    // flight, then 16-byte LDS stores. (row, kp) walk the image in
    // steps of 256 pairs without a division per load.
    const int kph = KS / 2;
    const int dq = 256 / kph, dr = 256 - dq * kph;
    int row = tid / kph, kp = tid - row * kph;
    while (row < FCS_ROWS) {
      vec2 v[FCS_NLD];
      int dst[FCS_NLD];
#pragma unroll
      for (int j = 0; j < FCS_NLD; ++j) {
        const int rc = min(row, FCS_ROWS - 1);
        const T* src = rc < RT ? x0b + (long)rc * I
                               : W1 + (long)(rc - RT) * I;
        v[j] = *reinterpret_cast<const vec2*>(src + kb + 2 * kp);
        dst[j] = row < FCS_ROWS ? rc * KSP + 2 * kp : -1;
        kp += dr;
        row += dq;
        if (kp >= kph) { kp -= kph; ++row; }
      }
#pragma unroll
      for (int j = 0; j < FCS_NLD; ++j) {
        if (dst[j] >= 0) *reinterpret_cast<vec2*>(stg + dst[j]) = v[j];
      }
    }
  } else {
    // K tail, M tail, H < 64 or an empty slice: guarded scalar loads,
    // zeros where the slice, the row tile or W1 ends
    for (int u = tid; u < FCS_ROWS * KS; u += 256) {
      const int r = u / KS, k = u - r * KS;
      T v = T(0);
      if (k < klen) {
        if (r < RT) {
          if (m0 + r < M) v = x0b[(long)r * I + kb + k];
        } else if (r - RT < H) {
          v = W1[(long)(r - RT) * I + kb + k];
        }
      }
      stg[r * KSP + k] = v;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = tid + j * 256;  // the zero-padded [16][64] tile
    w2s[(t >> 6) * FC_W2S + (t & 63)] = w2v[j];
  }
  if (tid < C) w2s[16 * FC_W2S + tid] = b2v;
  const int tgt = (int)Y_all[l * maxlen + trow];
  __syncthreads();
  FC_STAMP(0);

  // this slice's share of z1: wave w owns o-fragment [16w, 16w+16);
  // two accumulators halve the MFMA dependency chain
  {
    acc_t a0 = {}, a1 = {};
    const T* Ar = stg + lo * KSP + lk;
    const T* Br = stg + (RT + wid * 16 + lo) * KSP + lk;
    int kk = 0;
#pragma unroll 4
    for (; kk + 8 <= KS; kk += 8) {
      a0 = MF::mma(Ar[kk], Br[kk], a0);
      a1 = MF::mma(Ar[kk + 4], Br[kk + 4], a1);
    }
    if (kk < KS) a0 = MF::mma(Ar[kk], Br[kk], a0);
    T* slab = slabs + ((long)tile * S + slice) * (RT * 64);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      slab_store(&slab[MF::acc_row(lane, r) * 64 + wid * 16 + lo],
                 a0[r] + a1[r]);
    }
  }
  FC_STAMP(1);

  // publish the slab and draw a ticket. The slab went out write-through
  // (slab_store), so there is no release fence: every wave drains its
  // stores, the block meets, one lane adds to the tile's ticket. The
  // block that draws S - 1 is the reducer, the only one to touch the
  // ticket again, and reads every slab word past its L1 (slab_load), so
  // it needs no acquire either; the wavefront fence only keeps the
  // compiler from moving those loads up.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int got = __hip_atomic_fetch_add(
        &tickets[tile], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = got == S - 1;
    if (last) {
      __hip_atomic_store(&tickets[tile], 0, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    *lastf = last;
    if (!last) FC_STAMP_NONE(2);
  }
  __syncthreads();
  if (!*lastf) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  FC_STAMP(2);

  // reducer: z1 = slabs summed in slice order (independent of arrival
  // order), y1 = relu(z1 + b1) into LDS (never stored to HBM)
  {
    const T* sl = slabs + (long)tile * S * (RT * 64);
    T z[4] = {};
    for (int s0 = 0; s0 < S; s0 += 4) {  // 16 loads in flight, clamped
      T v[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long so = (long)min(s0 + q, S - 1) * (RT * 64) + tid;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[q][j] = slab_load(&sl[so + j * 256]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (s0 + q < S) {
#pragma unroll
          for (int j = 0; j < 4; ++j) z[j] += v[q][j];
        }
      }
    }
    const int o = tid & 63;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = (tid >> 6) + 4 * j;
      const T v = z[j] + b1v;
      y1s[m * 65 + o] = (o < H && v > T(0)) ? v : T(0);
    }
  }
  __syncthreads();
  FC_STAMP(3);

  // P2 + P3: the shared fc2 tail; its logit partials use the operand
  // image, which no wave reads after the barrier before the ticket
  fc_tail<T, false, 4>(
      w2s, y1s, dz2s, stg, static_cast<T*>(nullptr),
      [&](int) { return tgt; },
      grad + l * n, dz1g + (long)(l * (long)M + m0) * H,
      loss != nullptr ? loss + l : nullptr, w2_off, b2_off, m0, M, H, C,
      loss_scale);
#ifdef NDTA_FC_PHASE_CLOCK
  __syncthreads();
  FC_STAMP(5);
#endif
}

// dX0 = dz1 @ W1 with the conv relu' mask, one block per (16-column
// strip of I, 64-row group of M, node): wave w takes rows [16w, 16w+16)
// of the group. A lane's operands are 16 dz1 values (A), 16 W1 values
// (B) and the 4 x0 values that carry the mask: 36 independent loads
// issued together, clamped rather than branched at the M/I/H tails (a
// clamped load reads valid memory and its value is replaced by 0), so
// the kernel is one load round trip, 16 MFMAs and a masked store, with
// no LDS and no barrier.
//
// fc_dx0_tile is one wave's [16 rows from m0][16 columns from i0] tile
// of that product (m0 < M): it leaves in g[r] the lane's masked value
// for row m0 + acc_row(lane, r) and column i0 + (lane & 15). Rows past
// M and columns past I hold values that mean nothing; the caller masks
// them. fc_dx0_k stores the tile; the fused backward
// (dw_dx0_conv_bwd_k) feeds it to the conv dW taps without a trip
// through memory.
template <typename T>
DEV_INLINE void fc_dx0_tile(
    const T* __restrict__ x0, const T* __restrict__ theta,
    const T* __restrict__ dz1g, long n, long w1_off, int M, int I, int H,
    int mask_dx0, long l, int m0, int i0, int lane, T (&g)[4]) {
  using MF = gmfma::mfma_t<T>;
  using acc_t = typename MF::acc_t;
  const int lo = lane & 15;
  const int lk = lane >> 4;
  const int i = i0 + lo;
  const int ic = min(i, I - 1);
  const T* W1 = theta + l * n + w1_off;
  const T* dzr = dz1g + (long)(l * (long)M + min(m0 + lo, M - 1)) * H;

  T a[16], w[16], xm[4];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int h = min(4 * t + lk, H - 1);
    a[t] = dzr[h];
    w[t] = W1[(long)h * I + ic];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = min(m0 + MF::acc_row(lane, r), M - 1);
    xm[r] = mask_dx0 ? x0[(long)(l * (long)M + m) * I + ic] : T(1);
  }
  // zero what the clamps stood in for: rows past M, columns past I and
  // the H < 64 padding of the contraction
  const bool aok = m0 + lo < M;
  const bool wok = i < I;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const bool hok = 4 * t + lk < H;
    a[t] = (aok && hok) ? a[t] : T(0);
    w[t] = (wok && hok) ? w[t] : T(0);
  }
  acc_t ax0 = {}, ax1 = {};
#pragma unroll
  for (int t = 0; t < 16; t += 2) {
    ax0 = MF::mma(a[t], w[t], ax0);
    ax1 = MF::mma(a[t + 1], w[t + 1], ax1);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    // conv relu' mask: x0 IS the conv block's relu output
    g[r] = xm[r] > T(0) ? ax0[r] + ax1[r] : T(0);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fc_dx0_k(
    const T* __restrict__ x0,     // [L*M, I]
    const T* __restrict__ theta,  // [L, n]
    const T* __restrict__ dz1g,   // [L*M, H]
    T* __restrict__ dx0,          // [L*M, I]
    long n, long w1_off, int M, int I, int H, int mask_dx0) {
  using MF = gmfma::mfma_t<T>;
  const long l = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int m0 = blockIdx.y * 64 + wid * 16;
  if (m0 >= M) return;  // wave-uniform; the kernel has no barrier
  const int i = blockIdx.x * 16 + (lane & 15);
  T g[4];
  fc_dx0_tile<T>(x0, theta, dz1g, n, w1_off, M, I, H, mask_dx0, l, m0,
                 blockIdx.x * 16, lane, g);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + MF::acc_row(lane, r);
    if (m < M && i < I) dx0[(long)(l * (long)M + m) * I + i] = g[r];
  }
}

// ---------------------------------------------------------------------
// Merged backward launch: fc1 dW/db (gemm::linear_bwd_dw_body) and the
// gather-sourced conv dW/db (conv::conv_pool_bwd_body) as two roles of
// one flat grid of 256-thread blocks. Both only read what the fc block
// produced (dz1 + x0 for one, dx0 + the pool argmax for the other) and
// write disjoint slices of the grad stack, so as separate launches the
// 7.8 us dW kernel sat in a serial slot of its own; in one grid the 864
// dW blocks of the MNIST shape share the chip with the 768 conv blocks.
// Blocks [0, n_dw) decode to the dW kernel's (bx, by, bz) grid, the
// rest to the conv kernel's block index; the role branch is
// block-uniform and the LDS arena is the larger of the two needs
// (two [64][17] dW tiles, or the conv role's [K*K+1][4] wave sums).
// No occupancy bound beyond the block size: the conv role needs ~110
// VGPRs in fp64 (4 blocks/CU) and forcing 8 waves/SIMD spills its dW
// accumulators to scratch. The short dW blocks (one load round trip
// and one barrier at M = 64) come first in the grid and retire
// quickly, so the conv blocks fill in behind them.
template <typename T, int KMAX>
__global__ __launch_bounds__(256) void dw_conv_bwd_k(
    // dW role
    const T* __restrict__ dZ, const T* __restrict__ X,
    long w_off, long b_off, int M, int I, int O, int dw_gx, int dw_gy,
    int n_dw,
    // conv role
    const T* __restrict__ dY, const unsigned char* __restrict__ pidx,
    const T* __restrict__ X_all, long cw_off, long cb_off, int F, int K,
    int IMG, int nchunk, const long* __restrict__ src_idx,
    long idx_stride, long idx_off, long maxlen,
    T* __restrict__ gstack, long n) {
  constexpr int DW_LDS = 2 * gemm::DW_ROWS * (gemm::TILE + 1);
  constexpr int CV_LDS = (KMAX * KMAX + 1) * 4;
  __shared__ T smem[DW_LDS > CV_LDS ? DW_LDS : CV_LDS];
  const int bid = blockIdx.x;
  const int tid = threadIdx.x;
  if (bid < n_dw) {
    const int bx = bid % dw_gx;
    const int by = (bid / dw_gx) % dw_gy;
    const long bz = bid / (dw_gx * dw_gy);
    gemm::linear_bwd_dw_body<T>(
        dZ, X, gstack, n, w_off, b_off, M, I, O, bx, by, bz,
        tid / gemm::TILE, tid % gemm::TILE, smem,
        smem + gemm::DW_ROWS * (gemm::TILE + 1));
  } else {
    conv::conv_pool_bwd_body<T, KMAX>(
        dY, pidx, X_all, gstack, n, cw_off, cb_off, M, F, K, IMG,
        nchunk, src_idx, idx_stride, idx_off, maxlen, bid - n_dw, tid,
        256, smem);
  }
}

// ---------------------------------------------------------------------
// The merged backward with dX0 folded in. fc_dx0_k existed only to
// write dX0 to memory for the conv role above, which read each value
// back once, as the multiplier g of one item's taps. Here the conv role
// takes fc_dx0_k's decomposition instead: one block per (16-column
// strip of I, 64-row group of M, node), wave w on rows [16w, 16w+16),
// and computes the strip's dX0 tile itself (fc_dx0_tile: the same
// operand loads and MFMA order, so every g is bit-equal to what
// fc_dx0_k stored). A lane then holds four items (m, i), m = m0 +
// acc_row(lane, r), i its column: it runs their K*K taps into the same
// private acc[] as conv_pool_bwd_body and ends in the same tail.
//
// Requires P*P % 16 == 0 (a strip lies inside one filter, so f is
// block-uniform, and I = F*P*P has no column tail) and K == KMAX (the
// guard-free tap path); ext.hip bwd_dx0_fused is where that is decided.
//
// One load round trip brings the tile's operands, the lane's four
// argmax bytes and its rows' source indices; the taps are the next. The
// tap addresses do not wait for g, so the compiler issues all four
// items' tap loads (60 at K = 5) under the tile's last MFMAs; that
// takes about 240 VGPRs in fp64, hence the two-waves-per-SIMD bound on
// the kernel below. NFL is how many items' taps may be in flight at
// once: 4 wherever that fits 256 VGPRs, 1 for fp64 at K = 7 (4 spills
// there). Rows past M are clamped for every address and carry g = 0. A wave whose rows are all past M loads nothing but
// still runs the tail with exact-zero partials: the tail has a barrier.
template <typename T, int KMAX>
DEV_INLINE void dx0_conv_bwd_body(
    const T* __restrict__ x0, const T* __restrict__ theta,
    const T* __restrict__ dz1g, long w1_off, int H,
    const unsigned char* __restrict__ pidx, const T* __restrict__ X_all,
    T* __restrict__ gstack, long n, long cw_off, long cb_off, int M,
    int I, int IMG, const long* __restrict__ src_idx, long idx_stride,
    long idx_off, long maxlen, int sx, int gy, int l, int tid,
    T* __restrict__ red) {
  using MF = gmfma::mfma_t<T>;
  constexpr int NTAP = KMAX * KMAX;
  constexpr int NSLOT = conv::pow2_at_least(NTAP + 1);
  constexpr int NFL = (sizeof(T) == 8 && KMAX > 5) ? 1 : 4;
  const int P = (IMG - (KMAX - 1)) / 2;
  const int PP = P * P;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int m0 = gy * 64 + wid * 16;
  const int i = sx * 16 + (lane & 15);
  const int f = (sx * 16) / PP;
  const int pyx = i - f * PP;

  T acc[NSLOT];
#pragma unroll
  for (int t = 0; t <= NTAP; ++t) acc[t] = T(0);

  if (m0 < M) {  // wave-uniform
    int d[4];
    long srow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = min(m0 + MF::acc_row(lane, r), M - 1);
      d[r] = pidx[((long)l * M + m) * I + i];
      srow[r] = src_idx[l * idx_stride + idx_off + m];
    }
    // the tap addresses hang on these eight loads alone: they stay in
    // front of the tile's 36 (left alone the scheduler sinks them behind
    // the first waits of the tile, a round trip of their own)
    __builtin_amdgcn_sched_barrier(0);
    T g[4];
    fc_dx0_tile<T>(x0, theta, dz1g, n, w1_off, M, I, H, 1, l, m0,
                   sx * 16, lane, g);
    const int py2 = 2 * (pyx / P), px2 = 2 * (pyx % P);
    const T* img[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (m0 + MF::acc_row(lane, r) >= M) g[r] = T(0);
      const int cy = py2 + ((d[r] >> 1) & 1);
      const int cx = px2 + (d[r] & 1);
      img[r] = X_all + ((long)l * maxlen + srow[r]) * IMG * IMG +
               cy * IMG + cx;
    }
#pragma unroll
    for (int r0 = 0; r0 < 4; r0 += NFL) {
      T tap[NFL][NTAP];
#pragma unroll
      for (int q = 0; q < NFL; ++q) {
#pragma unroll
        for (int ky = 0; ky < KMAX; ++ky) {
#pragma unroll
          for (int kx = 0; kx < KMAX; ++kx) {
            tap[q][ky * KMAX + kx] = img[r0 + q][ky * IMG + kx];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < NFL; ++q) {
        acc[NTAP] += g[r0 + q];
#pragma unroll
        for (int t = 0; t < NTAP; ++t) acc[t] += g[r0 + q] * tap[q][t];
      }
      // the next group's loads stay behind this group's FMAs
      if (r0 + NFL < 4) __builtin_amdgcn_sched_barrier(0);
    }
  }
  conv::conv_bwd_reduce_tail<T, KMAX>(acc, gstack, n, cw_off, cb_off, l,
                                      f, KMAX, tid, 256, red);
}

// Flat grid: the n_cv conv blocks first, then the dW kernel's (bx, by,
// bz) grid; same LDS arena and block-uniform role branch as
// dw_conv_bwd_k. The order is the reverse of dw_conv_bwd_k's, whose 768
// conv blocks were about as short as its dW blocks. Here the 216 conv
// blocks of the MNIST shape are the launch's critical path (two
// dependent load round trips, 100 tap loads per thread) and the 864 dW blocks one
// round trip each: started first, the conv blocks take a CU each and
// the dW blocks fill in around and after them (12.6 us per call);
// started last they wait for dW blocks to retire at two blocks per CU
// and the launch is 16.9 us (profiles/README.md).
//
// STEP != 0: the launch also takes the DiNNO primal step that followed
// it (ew::fused_step_dual_k, STEP_DUAL, or ew::fused_step_k with the
// penalty, STEP_PLAIN), element for element what those kernels compute
// (ew::step_elem_*). The step reads theta_in, which is `theta` here, and
// writes theta_out, another buffer: nothing in the launch writes
// theta_in, so the conv role's W1 reads and the dual ascent's reads of
// the neighbours' round-start theta race with no store.
//  * dW role: the thread that owns dW[o][i] (and the bias block's row 0
//    for db[o]) never stores it. Its step loads go out with the staging
//    loads, before the barrier; after the dot product it steps its
//    element with g = acc. The fc1 slice of the grad stack is not
//    touched and stays zero.
//  * conv role: its atomics, and the fc block's for fc2 in the launch
//    before, leave F*K*K + F + C*H + C sums in the grad stack. Every
//    conv block drains its atomics, meets, and one lane draws a ticket
//    for the node (fc_fwd_split_k's hand-off: relaxed agent-scope
//    atomics, no spin-wait). The block that draws the node's last ticket
//    reads those sums past its L1, zeroes them, steps their elements and
//    returns the ticket to zero. No block waits for another.
constexpr int STEP_NONE = 0, STEP_PLAIN = 1, STEP_DUAL = 2;

template <typename T>
struct bwd_step_t {
  ew::step_args_t<T> a;
  int mode;      // 0 Adam, 1 AdamW, 2 SGD
  int load_mv;   // 0: the moments count as zero and are not read
  long w2_off, b2_off;
  int C, F;
  int* tickets;  // [L], zero between launches
};

// the dW role's sink (gemm::linear_bwd_dw_sink_body) on the step path
template <typename T, bool DUAL>
struct dw_step_sink {
  const bwd_step_t<T>& p;
  long w_off, b_off;
  int l, I;
  ew::step_ld_t<T> in;
  T S[1];

  DEV_INLINE void fetch(long e) {
    in = ew::step_elem_load<T, DUAL>(p.a, (long)l * p.a.n + e,
                                     p.load_mv != 0);
    if (DUAL) {
      ew::step_nbr_sum<T, 1>(p.a, l, [&](int r, int) {
        return ew::step_nbr_global(p.a, r, e);
      }, S);
    }
  }
  DEV_INLINE void apply(long e, T g) {
    ew::step_mode_switch(p.mode, [&](auto mode_c) {
      ew::step_elem_apply<T, decltype(mode_c)::value, DUAL>(
          p.a, in, S[0], g, l, (long)l * p.a.n + e);
    });
  }
  DEV_INLINE void prefetch(int o, int i, bool live) {
    if (live) fetch(w_off + (long)o * I + i);
  }
  DEV_INLINE void weight(int o, int i, T acc) {
    apply(w_off + (long)o * I + i, acc);
  }
  // one thread row of one block in gx: its loads are a trip of their own
  DEV_INLINE void bias(int o, T s) {
    fetch(b_off + o);
    apply(b_off + o, s);
  }
};

// The end of a conv-role block on the step path; every thread of the
// block arrives. `flag` is an LDS word. H is fc1's width, so fc2's W is
// [C][H].
template <typename T, bool DUAL>
DEV_INLINE void bwd_step_ticket_tail(
    const bwd_step_t<T>& p, T* gstack, long cw_off, long cb_off, int KK,
    int H, int l, int per_node, int tid, int* flag) {
  constexpr int NQ = 3;  // elements per thread and trip: 728 at MNIST
  // the atomics are out of this wave when vmcnt drains; see
  // fc_fwd_split_k for why no fence is needed on either side
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int got = __hip_atomic_fetch_add(
        &p.tickets[l], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = got == per_node - 1;
    if (last) {
      __hip_atomic_store(&p.tickets[l], 0, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    *flag = last;
  }
  __syncthreads();
  if (!*flag) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  const int n0 = p.F * KK, n1 = n0 + p.F, n2 = n1 + p.C * H;
  const int total = n2 + p.C;
  const long n = p.a.n;
  for (int u0 = tid; u0 < total; u0 += 256 * NQ) {
    long e[NQ];
    T g[NQ], S[NQ];
    ew::step_ld_t<T> in[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int u = min(u0 + q * 256, total - 1);
      e[q] = u < n0   ? cw_off + u
             : u < n1 ? cb_off + (u - n0)
             : u < n2 ? p.w2_off + (u - n1)
                      : p.b2_off + (u - n2);
      g[q] = slab_load(&gstack[(long)l * n + e[q]]);
      in[q] = ew::step_elem_load<T, DUAL>(p.a, (long)l * n + e[q],
                                          p.load_mv != 0);
    }
    if (DUAL) {
      ew::step_nbr_sum<T, NQ>(p.a, l, [&](int r, int q) {
        return ew::step_nbr_global(p.a, r, e[q]);
      }, S);
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (u0 + q * 256 < total) {
        const long t = (long)l * n + e[q];
        gstack[t] = T(0);  // the next launch's atomics start from zero
        ew::step_mode_switch(p.mode, [&](auto mode_c) {
          ew::step_elem_apply<T, decltype(mode_c)::value, DUAL>(
              p.a, in[q], S[q], g[q], l, t);
        });
      }
    }
  }
}

template <typename T, int KMAX, int STEP = STEP_NONE>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(2, 2))) void dw_dx0_conv_bwd_k(
    // dW role (and the tile's operands: dZ = dz1, X = x0)
    const T* __restrict__ dZ, const T* __restrict__ X,
    long w_off, long b_off, int M, int I, int O, int dw_gx, int dw_gy,
    // conv role
    const T* __restrict__ theta, const unsigned char* __restrict__ pidx,
    const T* __restrict__ X_all, long cw_off, long cb_off, int IMG,
    int cv_gx, int cv_gy, int n_cv, const long* __restrict__ src_idx,
    long idx_stride, long idx_off, long maxlen,
    T* __restrict__ gstack, long n,
    bwd_step_t<T> sp) {  // read only where STEP != STEP_NONE
  constexpr int DW_LDS = 2 * gemm::DW_ROWS * (gemm::TILE + 1);
  constexpr int CV_LDS = (KMAX * KMAX + 1) * 4;
  static_assert(STEP == STEP_NONE || CV_LDS + 2 <= DW_LDS,
                "the ticket flag sits behind the conv role's wave sums");
  __shared__ T smem[DW_LDS > CV_LDS ? DW_LDS : CV_LDS];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < n_cv) {
    const int bid = blockIdx.x;
    const int l = bid / (cv_gx * cv_gy);
    dx0_conv_bwd_body<T, KMAX>(
        X, theta, dZ, w_off, O, pidx, X_all, gstack, n, cw_off, cb_off,
        M, I, IMG, src_idx, idx_stride, idx_off, maxlen, bid % cv_gx,
        (bid / cv_gx) % cv_gy, l, tid, smem);
    if constexpr (STEP != STEP_NONE) {
      bwd_step_ticket_tail<T, STEP == STEP_DUAL>(
          sp, gstack, cw_off, cb_off, KMAX * KMAX, O, l, cv_gx * cv_gy,
          tid, reinterpret_cast<int*>(smem + CV_LDS));
    }
  } else {
    const int bid = blockIdx.x - n_cv;
    const int bx = bid % dw_gx;
    const int by = (bid / dw_gx) % dw_gy;
    const long bz = bid / (dw_gx * dw_gy);
    if constexpr (STEP != STEP_NONE) {
      dw_step_sink<T, STEP == STEP_DUAL> sink{
          sp, w_off, b_off, (int)bz, I, {}, {}};
      gemm::linear_bwd_dw_sink_body<T>(
          dZ, X, M, I, O, bx, by, bz, tid / gemm::TILE, tid % gemm::TILE,
          smem, smem + gemm::DW_ROWS * (gemm::TILE + 1), sink);
    } else {
      gemm::linear_bwd_dw_body<T>(
          dZ, X, gstack, n, w_off, b_off, M, I, O, bx, by, bz,
          tid / gemm::TILE, tid % gemm::TILE, smem,
          smem + gemm::DW_ROWS * (gemm::TILE + 1));
    }
  }
}

}  // namespace fmnist
