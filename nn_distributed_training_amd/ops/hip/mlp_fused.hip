// Whole-MLP forward in one launch (CDNA4 gfx950): the chain of stacked
// linear layers of a small MLP runs per 64-row tile inside one block,
// with the node's whole weight set resident in LDS. Between layers the
// activation exists only as the bf16 LDS image that the next layer's
// MFMA reads; global memory sees the input rows, and either every
// layer's fp32 output once (STASH: what bwd_chain reads) or the last
// layer's only (inference).
//
// Work split: persistent 256-thread blocks (4 waves). The (node l,
// 64-row tile) pairs are numbered node-major and block b owns the
// contiguous range [b*T/G, (b+1)*T/G), so it stages a node's weights
// once and again only when l changes (at most L-1 more times over the
// whole grid). One block per CU: the flagship chain takes ~117 KB of
// the 160 KB LDS.
//
// Three roles, by position in the chain (ext.hip mlp_plan decides):
//   lift  (layer 0, in <= 4, out <= 256): fp32 VALU like encode_fwd_k.
//     Thread (row = tid>>2, k-octet = (tid&3) + 4j) computes 8 outputs
//     from the row's <= 4 inputs and a 16-byte W row read from the fp32
//     parameter image, writes them as ONE 16-byte store into the wide
//     bf16 activation image and (STASH) as 32 contiguous bytes to the
//     fp32 stash: four neighbouring threads write 128 contiguous bytes
//     of a row.
//   trunk (in <= 256, out <= 64): v_mfma_f32_16x16x32_bf16, 4 waves 2x2
//     over the 64(m) x 64(o) tile, each 2x2 fragments, both operand
//     images k-contiguous with the fragment maps of gemm_bf16.hip. The
//     product is taken TRANSPOSED (A operand = W image [o][k], B operand
//     = activation image [m][k]), so the accumulator of a lane holds 4
//     consecutive o of one row m: the epilogue act(acc + b) leaves as
//     one 8-byte bf16 LDS write into the next layer's image, one 16-byte
//     fp32 global store to the stash, and one 16-byte fp32 LDS write
//     where a tail follows.
//     Activation images ping-pong between a wide buffer (row stride 264
//     bf16 = 132 dwords = 4 mod 64) and a narrow one (stride 72 = 36
//     dwords); a weight image has stride roundup32(in) + 8, which is
//     4 * odd dwords as well, so the 16 rows of a fragment read cover
//     all 64 banks once. Weights are rounded fp32 -> bf16 (RNE) once, at
//     staging. Rows o >= out and columns k >= in of a weight image, and
//     columns >= out of an activation image up to the next multiple of
//     32, are zeros: the MFMA loop never tests an element. Rows past M
//     repeat row M-1 on load and are guarded on store.
//   tail  (last layer, out <= 4): fp32 contraction of the UNROUNDED fp32
//     output of the last trunk layer (a [64][68] fp32 LDS image) with
//     fp32 weights: thread (row = tid>>2, q = tid&3) sums columns
//     q + 4j, two lane exchanges fold the four quarters. This is the
//     precision the layered path gives such a layer, which never takes
//     the bf16 kernel.
//
// No atomics, no cross-block hand-off, no inline assembly; compiled
// without packed fp32 VALU ops like gemm_bf16.hip, whose vector types,
// pack8 and kernel attribute it reuses.

#include "common.h"

namespace mlpf {

using gbf16::bf16x4;
using gbf16::bf16x8;
using gbf16::f32x4;

constexpr int TM = 64;        // rows per tile
constexpr int MAXL = 8;       // layers per chain
constexpr int LDW = 264;      // wide activation image stride (bf16)
constexpr int LDN = 72;       // narrow activation image stride (bf16)
constexpr int LDT = 68;       // fp32 tail image stride (floats)
constexpr int LIFT_IN = 4, LIFT_OUT = 256;
constexpr int TRUNK_IN = 256, TRUNK_OUT = 64;
constexpr int TAIL_OUT = 4;
constexpr long LDS_BUDGET = 160 * 1024;

struct Layer {
  long w_off, b_off;
  int in, out, act;
  float scale;
  int img;   // byte offset of the bf16 weight image (trunk)
  int par;   // float offset into the fp32 parameter image
  int vec;   // stash rows take 16-byte stores
};

struct Prog {
  int nl, has_tail;
  int off_wide, off_narrow, off_tail, off_par;  // byte offsets
  Layer ly[MAXL];
  float* stash[MAXL];
};

DEV_INLINE int r32(int v) { return (v + 31) & ~31; }

// Block barrier that orders LDS traffic only. Threads of a block hand
// data to each other through LDS alone here, so the stash stores need
// not have landed when the next phase starts; __syncthreads() would
// drain them (vmcnt(0)) at each of the tile's barriers, and with one
// wave per SIMD nothing else runs while it waits.
DEV_INLINE void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// node l's parameters -> LDS: bf16 [o][k] images for the trunk layers,
// zero-padded fp32 for the lift (W as [o][4], then b), the trunk biases
// ([64]) and the tail (W as [4][64], then b[4])
DEV_INLINE void stage_params(const Prog& p, const float* __restrict__ th,
                             unsigned char* lds, int tid) {
  float* par = reinterpret_cast<float*>(lds + p.off_par);
  for (int li = 0; li < p.nl; ++li) {
    const Layer& y = p.ly[li];
    const float* W = th + y.w_off;
    const float* b = th + y.b_off;
    float* pp = par + y.par;
    if (li == 0) {
      const int op = r32(y.out);
      for (int i = tid; i < op * 4; i += 256) {
        const int o = i >> 2, k = i & 3;
        pp[i] = (o < y.out && k < y.in) ? W[(long)o * y.in + k] : 0.f;
      }
      for (int i = tid; i < op; i += 256) {
        pp[op * 4 + i] = i < y.out ? b[i] : 0.f;
      }
    } else if (p.has_tail && li == p.nl - 1) {
      {
        const int t = tid >> 6, k = tid & 63;  // 256 threads = [4][64]
        pp[tid] = (t < y.out && k < y.in) ? W[(long)t * y.in + k] : 0.f;
      }
      if (tid < TAIL_OUT) pp[TAIL_OUT * 64 + tid] = tid < y.out ? b[tid] : 0.f;
    } else {
      __bf16* img = reinterpret_cast<__bf16*>(lds + y.img);
      const int kp = r32(y.in), sw = kp + 8, noct = kp >> 3;
      for (int i = tid; i < TRUNK_OUT * noct; i += 256) {
        const int o = i / noct, k0 = (i - o * noct) * 8;
        f32x4 v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * h + j;
            v[h][j] = (o < y.out && k < y.in) ? W[(long)o * y.in + k] : 0.f;
          }
        }
        *reinterpret_cast<bf16x8*>(&img[o * sw + k0]) =
            gbf16::pack8(v[0], v[1]);
      }
      if (tid < TRUNK_OUT) pp[tid] = tid < y.out ? b[tid] : 0.f;
    }
  }
}

// 4 consecutive fp32 of one stash row, o0 a multiple of 4
DEV_INLINE void store4(float* __restrict__ row, int o0, int out, bool vec,
                       f32x4 v) {
  if (vec && o0 + 4 <= out) {
    *reinterpret_cast<f32x4*>(row + o0) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (o0 + j < out) row[o0 + j] = v[j];
    }
  }
}

template <bool STASH>
DEV_INLINE void lift_tile(const Prog& p, const float* __restrict__ X,
                          unsigned char* lds, long grow0, int m0, int M,
                          int tid) {
  const Layer& y = p.ly[0];
  const float* par = reinterpret_cast<const float*>(lds + p.off_par) + y.par;
  __bf16* img = reinterpret_cast<__bf16*>(lds + p.off_wide);
  const int op = r32(y.out);
  const float* pb = par + op * 4;
  const int row = tid >> 2;
  const int m = min(m0 + row, M - 1);  // M tail: clamp on load
  const float* xr = X + (grow0 + m) * y.in;
  float x[LIFT_IN];
#pragma unroll
  for (int i = 0; i < LIFT_IN; ++i) x[i] = i < y.in ? xr[i] : 0.f;
  float* srow = STASH ? p.stash[0] + (grow0 + m) * y.out : nullptr;
  const bool live = m0 + row < M;
  for (int oc = tid & 3; oc < (op >> 3); oc += 4) {
    f32x4 v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = oc * 8 + 4 * h + j;
        const f32x4 w = *reinterpret_cast<const f32x4*>(&par[o * 4]);
        float z = pb[o];
#pragma unroll
        for (int i = 0; i < LIFT_IN; ++i) z += x[i] * w[i];
        v[h][j] = o < y.out ? act_fwd(y.act, z, y.scale) : 0.f;
      }
    }
    *reinterpret_cast<bf16x8*>(&img[row * LDW + oc * 8]) =
        gbf16::pack8(v[0], v[1]);
    if (STASH && live) {
      store4(srow, oc * 8, y.out, y.vec != 0, v[0]);
      store4(srow, oc * 8 + 4, y.out, y.vec != 0, v[1]);
    }
  }
}

// one trunk layer on the tile: S (stride ss) -> D (stride sd)
template <bool STASH>
DEV_INLINE void trunk_tile(const Prog& p, int li, unsigned char* lds,
                           const __bf16* S, int ss, __bf16* D, int sd,
                           long grow0, int m0, int M, int tid) {
  const Layer& y = p.ly[li];
  const __bf16* Wi = reinterpret_cast<const __bf16*>(lds + y.img);
  const float* bias =
      reinterpret_cast<const float*>(lds + p.off_par) + y.par;
  float* T = reinterpret_cast<float*>(lds + p.off_tail);
  const int lane = tid & 63, wid = tid >> 6;
  const int wm = (wid >> 1) * 32, wo = (wid & 1) * 32;
  const int kp = r32(y.in), sw = kp + 8;
  const bool last = li == p.nl - 1;
  const bool feeds_tail = p.has_tail && li == p.nl - 2;

  f32x4 acc[2][2] = {};  // [fo][fm]; rows o, cols m
  for (int kk = 0; kk < kp; kk += 32) {
    const int ko = kk + 8 * (lane >> 4);
    bf16x8 w[2], a[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      w[f] = *reinterpret_cast<const bf16x8*>(
          &Wi[(wo + f * 16 + (lane & 15)) * sw + ko]);
      a[f] = *reinterpret_cast<const bf16x8*>(
          &S[(wm + f * 16 + (lane & 15)) * ss + ko]);
    }
#pragma unroll
    for (int fo = 0; fo < 2; ++fo) {
#pragma unroll
      for (int fm = 0; fm < 2; ++fm) {
        acc[fo][fm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            w[fo], a[fm], acc[fo][fm], 0, 0, 0);
      }
    }
  }

  const bool to_global = STASH || last;
#pragma unroll
  for (int fo = 0; fo < 2; ++fo) {
    const int o4 = wo + fo * 16 + (lane >> 4) * 4;
    const f32x4 b = *reinterpret_cast<const f32x4*>(&bias[o4]);
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
      const int mr = wm + fm * 16 + (lane & 15);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = o4 + r < y.out
                   ? act_fwd(y.act, acc[fo][fm][r] + b[r], y.scale)
                   : 0.f;
      }
      if (!last) {
        *reinterpret_cast<bf16x4*>(&D[mr * sd + o4]) =
            __builtin_convertvector(v, bf16x4);
      }
      if (feeds_tail) {
        *reinterpret_cast<f32x4*>(&T[mr * LDT + o4]) = v;
      }
      if (to_global && m0 + mr < M) {
        store4(p.stash[li] + (grow0 + m0 + mr) * y.out, o4, y.out,
               y.vec != 0, v);
      }
    }
  }
}

// the tail's output (row = tid>>2, q = tid&3) of the tile; every thread
// of the block calls it (lane exchanges), q >= out gets padding
DEV_INLINE float tail_out(const Prog& p, unsigned char* lds, int tid) {
  const Layer& y = p.ly[p.nl - 1];
  const float* par =
      reinterpret_cast<const float*>(lds + p.off_par) + y.par;
  const float* T = reinterpret_cast<const float*>(lds + p.off_tail);
  const int row = tid >> 2, q = tid & 3;
  float s[TAIL_OUT] = {};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = q + 4 * j;
    const float v = T[row * LDT + c];
#pragma unroll
    for (int t = 0; t < TAIL_OUT; ++t) s[t] += v * par[t * 64 + c];
  }
#pragma unroll
  for (int t = 0; t < TAIL_OUT; ++t) {
    s[t] += __shfl_xor(s[t], 1, WAVE);
    s[t] += __shfl_xor(s[t], 2, WAVE);
  }
  const float z = (q == 0 ? s[0] : q == 1 ? s[1] : q == 2 ? s[2] : s[3])
                  + par[TAIL_OUT * 64 + q];
  return act_fwd(y.act, z, y.scale);
}

DEV_INLINE void tail_tile(const Prog& p, unsigned char* lds, long grow0,
                          int m0, int M, int tid) {
  const Layer& y = p.ly[p.nl - 1];
  const int row = tid >> 2, q = tid & 3;
  const float v = tail_out(p, lds, tid);
  if (q < y.out && m0 + row < M) {
    p.stash[p.nl - 1][(grow0 + m0 + row) * y.out + q] = v;
  }
}

// X [L*M, in0] fp32, theta [L, n] fp32; p.stash[li] [L*M, out_li] fp32,
// all of them with STASH, the last one only without.
template <bool STASH>
GBF16_KERNEL __launch_bounds__(256) void mlp_fwd_fused_k(
    const float* __restrict__ X, const float* __restrict__ theta,
    const Prog p, long n, int M, int L) {
  extern __shared__ __align__(16) unsigned char mlpf_raw[];
  const int tid = threadIdx.x;
  const int tpn = (M + TM - 1) / TM;
  const long total = (long)L * tpn;
  const long t0 = total * blockIdx.x / gridDim.x;
  const long t1 = total * (blockIdx.x + 1) / gridDim.x;
  __bf16* wide = reinterpret_cast<__bf16*>(mlpf_raw + p.off_wide);
  __bf16* narrow = reinterpret_cast<__bf16*>(mlpf_raw + p.off_narrow);
  const int ntrunk_end = p.has_tail ? p.nl - 1 : p.nl;

  long cur_l = -1;
  for (long t = t0; t < t1; ++t) {
    const long l = t / tpn;
    const int m0 = (int)(t - l * tpn) * TM;
    const long grow0 = l * (long)M;
    if (l != cur_l) {
      lds_barrier();  // the previous tile's tail is done with them
      stage_params(p, theta + l * n, mlpf_raw, tid);
      cur_l = l;
      lds_barrier();
    }
    lift_tile<STASH>(p, X, mlpf_raw, grow0, m0, M, tid);
    lds_barrier();
    for (int li = 1; li < ntrunk_end; ++li) {
      if (li & 1) {
        trunk_tile<STASH>(p, li, mlpf_raw, wide, LDW, narrow, LDN, grow0,
                          m0, M, tid);
      } else {
        trunk_tile<STASH>(p, li, mlpf_raw, narrow, LDN, wide, LDW, grow0,
                          m0, M, tid);
      }
      lds_barrier();
    }
    if (p.has_tail) tail_tile(p, mlpf_raw, grow0, m0, M, tid);
  }
}

}  // namespace mlpf
