// Every node's whole gradient row of a small regression MLP in ONE
// launch (CDNA4 gfx950; ops/stacked.py fused_train): forward, loss and
// backward of a (node, 64-row tile) run inside one block with every
// activation in LDS and every dW/db partial in registers. Global memory
// sees the input rows, the targets and one gradient slab per (block,
// node); no activation, stash or dZ goes out.
//
// Chains (ext.hip mlp_grad_plan decides): a lift (layer 0, in <= 4,
// out <= 256, sin_relu / relu / none), one or more trunk layers
// (in <= 256, out <= 64, relu / none) and a tail (out <= 4, none /
// sigmoid / tanh) under BCE, MSE or L1.
//
// Work split. Persistent 256-thread blocks (4 waves), at most one per
// CU. The (node, tile) pairs are numbered node-major and block b owns
// the contiguous range [b*T/G, (b+1)*T/G) like mlp_fwd_fused_k. The
// block's gradient partials stay in registers across ALL its tiles of a
// node and leave once per (block, node):
//   first trunk layer  dW [64 o][256 i]: wave w owns i in [64w, 64w+64),
//                      4x4 fragments, 64 registers per lane
//   later trunk layers dW [64 o][64 i]: waves 2x2, 2x2 fragments each,
//                      16 registers per lane and layer
//   lift dW/db         in + 1 registers for each of the 4 lift columns
//                      a lane meets in the first trunk layer's dX
//   trunk db, tail dW/db, loss: one register each per thread
//
// Forward. The phases of mlp_fused.hip, called: stage_params,
// lift_tile<false>, trunk_tile<false> and tail_out, so every activation
// image holds the bits mlp_fwd_fused_k<true> stashes (rounded to bf16
// where that kernel rounds). Unlike the forward kernel's ping-pong, each
// trunk output keeps an image of its own: the backward reads them all.
//
// Backward, the rounding points of the layered bf16 path. With dZ of
// layer li as a bf16 image Z[m][o] and, unrounded, as an fp32 image
// F[m][o] (the tail image's storage, free once the tail is done):
//   db[o]     = sum_m F[m][o]                       VALU, unrounded
//   dW[o][i]  = sum_m bf(dZ[m][o]) bf(A[m][i])      MFMA over the rows
//   dX[m][i]  = sum_o bf(dZ[m][o]) bf(W[o][i])      MFMA over o
// on v_mfma_f32_16x16x32_bf16 (fragment maps in gemm_bf16.hip). dW is
// taken as D[i][o] (A operand = A^T, B operand = dZ), so a lane ends
// with 4 consecutive i of one o: one 16-byte slab store. dX of a narrow
// layer is taken as D[i][m] (A operand = W^T, B operand = dZ^T read
// row-wise), so the masked result leaves as one 8-byte bf16 and one
// 16-byte fp32 LDS write, as in trunk_tile. dX of the first trunk layer
// is taken as D[m][i]: a lane holds 16 rows of ONE lift column per
// fragment, multiplies by the lift's activation factor with z recomputed
// from the <= 4 inputs (act_bwd, unrounded fp32) and adds dz * x[k] and
// dz into the column's registers; no [64][256] dZ image exists.
// The tail's forward, loss, dW, db and dX are unrounded fp32 VALU; loss
// and head dZ are the device functions of losses.hip.
//
// Transposed operands. dW contracts over the rows and dX over o, so A^T,
// dZ (as a B operand) and W^T want 8 consecutive elements of a COLUMN of
// images laid out row-major for the forward. Second, transposed images
// do not fit 160 KB at 64-row tiles, so gather8 builds such a fragment
// from eight 16-bit LDS reads at immediate row offsets. The gfx950
// transposed read (ds_read_b64_tr_b16) would make it two reads; its lane
// map is not pinned in this project and nothing here depends on it.
//
// Cross-block reduction, deterministic and without floating-point
// atomics. A block writes its partials for node l to slab (l, j), j its
// rank among the blocks that own tiles of l, laid out like the gradient
// row with the loss word behind; the layers' slices tile [0, n), so the
// slab is written whole. Each wave releases its stores at agent scope,
// the block meets, one lane draws the node's ticket (a vector atomic).
// The block that draws the last one acquires, sums the slabs in rank
// order and OVERWRITES grad[l] and loss[l], and returns the ticket to
// zero. No block waits for another; two launches give the same bits;
// the caller zeroes nothing.
//
// Barriers order LDS only (mlpf::lds_barrier). Compiled without packed
// fp32 VALU ops. The one asm statement is empty (see the tile loop).

#include "common.h"

namespace mlpg {

using gbf16::bf16x4;
using gbf16::bf16x8;
using gbf16::f32x4;
using mlpf::lds_barrier;
using mlpf::LDN;
using mlpf::LDT;
using mlpf::LDW;
using mlpf::r32;
using mlpf::TM;

constexpr int MAXT = mlpf::MAXL - 2;  // trunk layers
constexpr int IMG_N = TM * LDN * 2;   // bytes of a narrow bf16 image
constexpr int RED_FLOATS = 272;       // 4 x 64 fold, 4 loss words, flag
constexpr int RED_U = 8;              // reducer: words in flight

struct Prog {
  mlpf::Prog f;  // the forward phases' program; f.off_tail is F as well
  int nt;        // trunk layers: 1 .. nt, the tail is nt + 1
  int off_act;   // output image of trunk layer li < nt at (li-1)*IMG_N
  int off_dz;    // two bf16 dZ images; layer li reads image li & 1
  int off_x;     // fp32 [TM][4] input rows
  int off_hz;    // fp32 [TM][4] dZ of the head
  int off_red;   // fp32 [RED_FLOATS]
  int vec[mlpf::MAXL];  // the layer's dW rows take 16-byte slab stores
  int loss_kind;        // 1 sigmoid+BCE, 2 MSE, 3 L1
  int slab;             // floats between two slabs, >= n + 1
  int J;                // slabs per node
  float w;              // loss_scale / M
};

// 8 consecutive rows k0 .. k0+7 of column col: a fragment whose
// contraction index runs down the image
DEV_INLINE bf16x8 gather8(const __bf16* img, int stride, int k0, int col) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = img[(k0 + j) * stride + col];
  return v;
}

// the block that owns tile t
DEV_INLINE int owner(long t, long total, int G) {
  int b = (int)(t * G / total);
  while (total * (b + 1) / G <= t) ++b;
  while (total * b / G > t) --b;
  return b;
}

// column sums of the unrounded dZ: thread (wid, lane) takes 16 rows
DEV_INLINE float db_part(const float* F, int wid, int lane) {
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += F[(wid * 16 + r) * LDT + lane];
  return s;
}

// trunk layer li >= 2 on the tile: db, dW into acc, dZ of layer li - 1
DEV_INLINE void narrow_bwd(const Prog& p, int li, unsigned char* lds,
                           int lane, int wid, f32x4 (&acc)[2][2],
                           float& db) {
  const mlpf::Layer& y = p.f.ly[li];
  const __bf16* Wi = reinterpret_cast<const __bf16*>(lds + y.img);
  const __bf16* Ab = reinterpret_cast<const __bf16*>(
      lds + p.off_act + (li - 2) * IMG_N);
  const __bf16* Zb = reinterpret_cast<const __bf16*>(
      lds + p.off_dz + (li & 1) * IMG_N);
  __bf16* Zo = reinterpret_cast<__bf16*>(
      lds + p.off_dz + ((li - 1) & 1) * IMG_N);
  float* F = reinterpret_cast<float*>(lds + p.f.off_tail);
  const int lo = lane & 15, lk = lane >> 4;
  const int w1 = (wid >> 1) * 32, w0 = (wid & 1) * 32;
  const int kp = r32(y.in), sw = kp + 8;

  db += db_part(F, wid, lane);

  f32x4 x[2][2] = {};  // dX as [fi][fm]: rows i, cols m
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int k0 = ks * 32 + 8 * lk;
    bf16x8 a[2], z[2], wt[2], zr[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      a[f] = gather8(Ab, LDN, k0, w1 + f * 16 + lo);   // A^T, rows i
      z[f] = gather8(Zb, LDN, k0, w0 + f * 16 + lo);   // dZ, cols o
      wt[f] = bf16x8{};
      if (w1 + f * 16 < kp) {
        wt[f] = gather8(Wi, sw, k0, w1 + f * 16 + lo);  // W^T, rows i
      }
      zr[f] = *reinterpret_cast<const bf16x8*>(
          &Zb[(w0 + f * 16 + lo) * LDN + k0]);          // dZ^T, cols m
    }
#pragma unroll
    for (int fi = 0; fi < 2; ++fi) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        acc[fi][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[fi], z[g], acc[fi][g], 0, 0, 0);
        x[fi][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wt[fi], zr[g], x[fi][g], 0, 0, 0);
      }
    }
  }
  lds_barrier();  // every wave is done with F and with Zb's reader Zo

  const int act_b = p.f.ly[li - 1].act;
#pragma unroll
  for (int fi = 0; fi < 2; ++fi) {
    const int i4 = w1 + fi * 16 + lk * 4;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
      const int mr = w0 + fm * 16 + lo;
      const bf16x4 ab = *reinterpret_cast<const bf16x4*>(&Ab[mr * LDN + i4]);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool pass = act_b != ACT_RELU || (float)ab[r] > 0.f;
        v[r] = (i4 + r < y.in && pass) ? x[fi][fm][r] : 0.f;
      }
      *reinterpret_cast<f32x4*>(&F[mr * LDT + i4]) = v;
      *reinterpret_cast<bf16x4*>(&Zo[mr * LDN + i4]) =
          __builtin_convertvector(v, bf16x4);
    }
  }
  lds_barrier();
}

// trunk layer 1 on the tile: db, dW into aw, and the lift's dW/db into
// lw straight from the dX accumulators
DEV_INLINE void wide_bwd(const Prog& p, unsigned char* lds, int lane,
                         int wid, f32x4 (&aw)[4][4], float& db,
                         float (&lw)[4][5]) {
  const mlpf::Layer& y = p.f.ly[1];
  const mlpf::Layer& y0 = p.f.ly[0];
  const __bf16* Wi = reinterpret_cast<const __bf16*>(lds + y.img);
  const __bf16* A0 = reinterpret_cast<const __bf16*>(lds + p.f.off_wide);
  const __bf16* Zb = reinterpret_cast<const __bf16*>(
      lds + p.off_dz + IMG_N);
  const float* F = reinterpret_cast<const float*>(lds + p.f.off_tail);
  const float* par0 =
      reinterpret_cast<const float*>(lds + p.f.off_par) + y0.par;
  const float* xs = reinterpret_cast<const float*>(lds + p.off_x);
  const int lo = lane & 15, lk = lane >> 4;
  const int ic = wid * 64;
  const int kp = r32(y.in), sw = kp + 8;  // kp is the lift's padded out

  db += db_part(F, wid, lane);

  {
    bf16x8 z[2][4];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
      for (int fo = 0; fo < 4; ++fo) {
        z[ks][fo] = gather8(Zb, LDN, ks * 32 + 8 * lk, fo * 16 + lo);
      }
    }
#pragma unroll
    for (int fi = 0; fi < 4; ++fi) {
      if (ic + fi * 16 < kp) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 a =
              gather8(A0, LDW, ks * 32 + 8 * lk, ic + fi * 16 + lo);
#pragma unroll
          for (int fo = 0; fo < 4; ++fo) {
            aw[fi][fo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, z[ks][fo], aw[fi][fo], 0, 0, 0);
          }
        }
      }
    }
  }

  // dX one 16-row fragment at a time (the fm loop is NOT unrolled: the
  // activation factor's sin / cos would be inlined 64 times and its
  // temporaries spill): dZ row-wise is the A operand, rows m
#pragma unroll
  for (int fi = 0; fi < 4; ++fi) {
    if (ic + fi * 16 < kp) {
      const int i = ic + fi * 16 + lo;
      const bf16x8 wt0 = gather8(Wi, sw, 8 * lk, i);
      const bf16x8 wt1 = gather8(Wi, sw, 32 + 8 * lk, i);
      const f32x4 wl = *reinterpret_cast<const f32x4*>(&par0[i * 4]);
      const float bl = par0[kp * 4 + i];
      const bool live = i < y0.out;
#pragma unroll 1
      for (int fm = 0; fm < 4; ++fm) {
        const __bf16* zp = &Zb[(fm * 16 + lo) * LDN + 8 * lk];
        f32x4 x = {};  // rows m = fm*16 + lk*4 + r of column i
        x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            *reinterpret_cast<const bf16x8*>(zp), wt0, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            *reinterpret_cast<const bf16x8*>(zp + 32), wt1, x, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f32x4 xv = *reinterpret_cast<const f32x4*>(
              &xs[(fm * 16 + lk * 4 + r) * 4]);
          float z = bl;
#pragma unroll
          for (int k = 0; k < 4; ++k) z += xv[k] * wl[k];
          const float dz =
              live ? x[r] * act_bwd(y0.act, z, z, y0.scale) : 0.f;
#pragma unroll
          for (int k = 0; k < 4; ++k) lw[fi][k] += dz * xv[k];
          lw[fi][4] += dz;
        }
      }
    }
  }
}

// one db vector of the node: fold the four waves' partials, in order
DEV_INLINE void flush_db(float* red, float* dst, int out, float v, int tid) {
  red[tid] = v;
  lds_barrier();
  if (tid < out) {
    dst[tid] = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
  }
  lds_barrier();
}

// X [L*M, in0], Y [L*M, out_tail], theta / grad [L, n], loss [L] or
// null; slabs [L, J, p.slab], tickets [L] zero between launches
GBF16_KERNEL __launch_bounds__(256) void mlp_grad_fused_k(
    const float* __restrict__ X, const float* __restrict__ Y,
    const float* __restrict__ theta, float* __restrict__ grad,
    float* __restrict__ loss, float* slabs, int* tickets, const Prog p,
    long n, int M, int L) {
  extern __shared__ __align__(16) unsigned char mlpg_raw[];
  unsigned char* lds = mlpg_raw;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = gridDim.x;
  const int tpn = (M + TM - 1) / TM;
  const long total = (long)L * tpn;
  const long t0 = total * blockIdx.x / G;
  const long t1 = total * (blockIdx.x + 1) / G;
  const int nt = p.nt;
  const mlpf::Layer& yt = p.f.ly[nt + 1];  // the tail
  const mlpf::Layer& yn = p.f.ly[nt];      // the last trunk layer

  __bf16* wide = reinterpret_cast<__bf16*>(lds + p.f.off_wide);
  float* T = reinterpret_cast<float*>(lds + p.f.off_tail);
  float* xs = reinterpret_cast<float*>(lds + p.off_x);
  float* hz = reinterpret_cast<float*>(lds + p.off_hz);
  float* red = reinterpret_cast<float*>(lds + p.off_red);
  int* lastf = reinterpret_cast<int*>(red + 260);
  const float* part =
      reinterpret_cast<const float*>(lds + p.f.off_par) + yt.par;

  // the node's partials, in registers over all its tiles
  f32x4 aw[4][4] = {};
  f32x4 an[MAXT - 1][2][2] = {};
  float lw[4][5] = {};
  float db[MAXT] = {};
  float tw = 0.f, tb = 0.f, lossp = 0.f;

  long cur_l = -1;
  for (long t = t0; t < t1; ++t) {
    const long l = t / tpn;
    const int m0 = (int)(t - l * tpn) * TM;
    const long grow0 = l * (long)M;
    // The lane id is made opaque once per tile. Every phase's per-lane
    // LDS addresses are invariant over the tile loop; hoisted out of it
    // they outnumber the registers and spill to scratch, recomputed per
    // tile they are a few VALU ops.
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    const int tid = wid * 64 + lane;
    const int lo = lane & 15, lk = lane >> 4;
    if (l != cur_l) {
      mlpf::stage_params(p.f, theta + l * n, lds, tid);
      cur_l = l;
    }
    if (wid == 0) {
      const float* xr = X + (grow0 + min(m0 + tid, M - 1)) * p.f.ly[0].in;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xs[tid * 4 + k] = k < p.f.ly[0].in ? xr[k] : 0.f;
      }
    }
    lds_barrier();

    // ---- forward: trunk li < nt writes image li - 1, the last trunk
    // layer the fp32 tail image (its bf16 copy lands in a dZ image
    // that the head overwrites)
    mlpf::lift_tile<false>(p.f, X, lds, grow0, m0, M, tid);
    lds_barrier();
    for (int li = 1; li <= nt; ++li) {
      const __bf16* S = li == 1 ? wide : reinterpret_cast<const __bf16*>(
                                      lds + p.off_act + (li - 2) * IMG_N);
      __bf16* D = reinterpret_cast<__bf16*>(
          li < nt ? lds + p.off_act + (li - 1) * IMG_N
                  : lds + p.off_dz + (nt & 1) * IMG_N);
      mlpf::trunk_tile<false>(p.f, li, lds, S, li == 1 ? LDW : LDN, D, LDN,
                              grow0, m0, M, tid);
      lds_barrier();
    }

    // ---- tail forward, loss, head dZ: thread (row, q)
    {
      const int row = tid >> 2, q = tid & 3;
      const float yh = mlpf::tail_out(p.f, lds, tid);
      const bool valid = q < yt.out && m0 + row < M;
      float dz = 0.f;
      if (valid) {
        const float tg = Y[(grow0 + m0 + row) * yt.out + q];
        if (p.loss_kind == 1) {
          dz = losses::bce_dz(yh, tg, p.w);
          lossp += losses::bce_term(yh, tg, M);
        } else {
          const float d = yh - tg;
          const float dy = p.loss_kind == 2
                               ? losses::regression_dy<float, 0>(d, p.w)
                               : losses::regression_dy<float, 1>(d, p.w);
          lossp += p.loss_kind == 2
                       ? losses::regression_term<float, 0>(d, M)
                       : losses::regression_term<float, 1>(d, M);
          dz = dy * act_bwd(yt.act, 0.f, yh, yt.scale);
        }
      }
      hz[tid] = dz;
    }
    lds_barrier();

    // ---- tail dW / db: thread (t, c) walks the rows
    {
      const int tt = wid, c = lane;
#pragma unroll 8
      for (int r = 0; r < TM; ++r) {
        const float g = hz[r * 4 + tt];
        tw += g * T[r * LDT + c];
        tb += g;
      }
    }
    lds_barrier();

    // ---- tail dX -> dZ of the last trunk layer, in place over T
    {
      const int row = tid >> 2, q = tid & 3;
      __bf16* Zo = reinterpret_cast<__bf16*>(lds + p.off_dz + (nt & 1) * IMG_N);
      const f32x4 g = *reinterpret_cast<const f32x4*>(&hz[row * 4]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c0 = 4 * q + 16 * j;
        const f32x4 a = *reinterpret_cast<const f32x4*>(&T[row * LDT + c0]);
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = 0.f;
#pragma unroll
          for (int k = 0; k < mlpf::TAIL_OUT; ++k) {
            s += g[k] * part[k * 64 + c0 + r];
          }
          const bool pass = yn.act != ACT_RELU || a[r] > 0.f;
          v[r] = (c0 + r < yn.out && pass) ? s : 0.f;
        }
        *reinterpret_cast<f32x4*>(&T[row * LDT + c0]) = v;
        *reinterpret_cast<bf16x4*>(&Zo[row * LDN + c0]) =
            __builtin_convertvector(v, bf16x4);
      }
    }
    lds_barrier();

    // ---- trunk backward, top down
    // ONE copy of the layer's code on a runtime li (unrolled per layer,
    // every copy's lane addresses are hoisted out of the tile loop and
    // spill); only the add into the layer's registers is selected
#pragma unroll 1
    for (int li = nt; li >= 2; --li) {
      f32x4 d[2][2] = {};
      float s = 0.f;
      narrow_bwd(p, li, lds, lane, wid, d, s);
#pragma unroll
      for (int c = 2; c <= MAXT; ++c) {
        if (c == li) {
          db[c - 1] += s;
#pragma unroll
          for (int f = 0; f < 4; ++f) an[c - 2][f >> 1][f & 1] += d[f >> 1][f & 1];
        }
      }
    }
    wide_bwd(p, lds, lane, wid, aw, db[0], lw);
    lds_barrier();  // the next tile's lift may write

    if (t + 1 < t1 && (t + 1) / tpn == l) continue;

    // ---- the node is done here: partials -> slab (l, rank)
    const int bfirst = owner(l * tpn, total, G);
    const int cnt = owner((l + 1) * (long)tpn - 1, total, G) - bfirst + 1;
    float* slab =
        slabs + (l * p.J + ((int)blockIdx.x - bfirst)) * (long)p.slab;
    {
      const mlpf::Layer& y = p.f.ly[1];
#pragma unroll
      for (int fi = 0; fi < 4; ++fi) {
        const int i4 = wid * 64 + fi * 16 + lk * 4;
#pragma unroll
        for (int fo = 0; fo < 4; ++fo) {
          const int o = fo * 16 + lo;
          if (o < y.out) {
            mlpf::store4(slab + y.w_off + (long)o * y.in, i4, y.in,
                         p.vec[1] != 0, aw[fi][fo]);
          }
          aw[fi][fo] = f32x4{};
        }
      }
      flush_db(red, slab + y.b_off, y.out, db[0], tid);
      db[0] = 0.f;
    }
#pragma unroll
    for (int li = 2; li <= MAXT; ++li) {
      if (li <= nt) {
        const mlpf::Layer& y = p.f.ly[li];
#pragma unroll
        for (int fi = 0; fi < 2; ++fi) {
          const int i4 = (wid >> 1) * 32 + fi * 16 + lk * 4;
#pragma unroll
          for (int fo = 0; fo < 2; ++fo) {
            const int o = (wid & 1) * 32 + fo * 16 + lo;
            if (o < y.out) {
              mlpf::store4(slab + y.w_off + (long)o * y.in, i4, y.in,
                           p.vec[li] != 0, an[li - 2][fi][fo]);
            }
            an[li - 2][fi][fo] = f32x4{};
          }
        }
        flush_db(red, slab + y.b_off, y.out, db[li - 1], tid);
        db[li - 1] = 0.f;
      }
    }
    {
      const int tt = wid, c = lane;
      if (tt < yt.out && c < yt.in) slab[yt.w_off + tt * yt.in + c] = tw;
      if (tt < yt.out && c == 0) slab[yt.b_off + tt] = tb;
      tw = tb = 0.f;
    }
    {
      const mlpf::Layer& y0 = p.f.ly[0];
#pragma unroll
      for (int fi = 0; fi < 4; ++fi) {
        const int i = wid * 64 + fi * 16 + lo;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          float v = lw[fi][k];
          v += __shfl_xor(v, 16, WAVE);
          v += __shfl_xor(v, 32, WAVE);
          if (lk == 0 && i < y0.out) {
            if (k < 4) {
              if (k < y0.in) slab[y0.w_off + (long)i * y0.in + k] = v;
            } else {
              slab[y0.b_off + i] = v;
            }
          }
          lw[fi][k] = 0.f;
        }
      }
    }
    {
      const float s = wave_reduce_sum(lossp);
      lossp = 0.f;
      if (lane == 0) red[256 + wid] = s;
    }

    // ---- publish and draw the node's ticket
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    lds_barrier();
    if (tid == 0) {
      slab[n] = (red[256] + red[257]) + (red[258] + red[259]);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const int got = __hip_atomic_fetch_add(
          &tickets[l], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = got == cnt - 1;
      if (last) {
        __hip_atomic_store(&tickets[l], 0, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      *lastf = last;
    }
    lds_barrier();
    if (*lastf) {
      // ---- reducer: every word of the row and the loss word, summed
      // over the node's slabs in rank order
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const float* sl = slabs + l * p.J * (long)p.slab;
      for (long e0 = tid; e0 <= n; e0 += 256 * RED_U) {
        float s[RED_U] = {};
        for (int j = 0; j < cnt; ++j) {
          const float* pj = sl + (long)j * p.slab;
#pragma unroll
          for (int u = 0; u < RED_U; ++u) {
            const long e = e0 + 256 * u;
            s[u] += pj[e < n ? e : n];
          }
        }
#pragma unroll
        for (int u = 0; u < RED_U; ++u) {
          const long e = e0 + 256 * u;
          if (e < n) grad[l * n + e] = s[u];
          else if (e == n && loss != nullptr) loss[l] = s[u];
        }
      }
    }
    lds_barrier();  // lastf and red are free again
  }
}

}  // namespace mlpg
