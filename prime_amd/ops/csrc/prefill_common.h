// What the chunked ragged prefill kernels share (prefill_ragged.hip over the
// bf16 cache, prefill_ragged_paged.hip over the paged bf16 cache,
// prefill_ragged_fp8.hip over the fp8 cache): the tile constants, the
// (lens, n_new) clamp, the swizzles of the two LDS images with the fragment
// reads that undo them, the MFMA / pack helpers, the empty-split and
// epilogue stores, the merge kernel, the argument checks and the dispatch;
// and, for the two bf16 files, the LDS-DMA stage and the whole kernel body
// (pf_body) over a tile-source policy. The library is one non-RDC compile
// per file, so the kernels here are `static`: each file gets its own copy,
// and the swizzle a file stages with cannot drift from the XOR the fragment
// reads apply.
//
// All including files are compiled without the packed fp32 VALU
// instructions (ops/build.py, NO_PACKED_FP32).
#pragma once
#include <type_traits>

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) short4v lds_short4;
typedef __attribute__((address_space(1))) const void g_void;

#define PF_THREADS 256
#define PF_Q_ROWS 128    // query rows (t*G + g) per workgroup, 32 per wave
#define PF_KEY_TILE 64   // keys per step
#define PF_NEG (-1e30f)

// Clamped (L0, n) of slot b, the same in every kernel.
__device__ __forceinline__ void pf_live(const int* __restrict__ lens,
                                        const int* __restrict__ n_new, int b,
                                        int T, int Smax, int& L0, int& n) {
  L0 = min(max(lens[b], 0), Smax);
  n = L0 == 0 ? 0 : min(max(n_new[b], 0), min(T, Smax - L0 + 1));
}

// ---- LDS images -----------------------------------------------------------
// Both tiles are [64 keys][D] bf16, linear, with an XOR on the byte offset
// inside the row. K: the 16 B slot XOR of attention.hip's swz16 (a 16 B
// fragment read of 32 rows x 2 slots is conflict-free). V: the transposing
// read takes, per 16 lanes, 4 consecutive rows x 32 contiguous bytes, and
// the two 16-lane groups of a half wave sit side by side (64 B); XORing the
// 64 B block index with the row's position among its 4 puts the four rows
// in four different quarters of the 256 B bank line (D = 64: two rows share
// a line, so the row pair's parity picks the block).
template <int D>
__device__ __forceinline__ int pf_kswz(int row) {
  return (D == 128 ? (row & 15) : ((row >> 1) & 7)) << 4;
}
template <int D>
__device__ __forceinline__ int pf_vswz(int row) {
  return (D == 128 ? (row & 3) : ((row >> 1) & 1)) << 6;
}

template <int D>
__device__ __forceinline__ short8 pf_kfrag(const bf16* tile, int row, int colb) {
  return *reinterpret_cast<const short8*>(reinterpret_cast<const char*>(tile) +
                                          row * (D * 2) +
                                          (colb ^ pf_kswz<D>(row)));
}

// V^T fragment of the 32x32x16 MFMA from the [key][d] tile: the lane gets
// V[key = ks*16 + hi*8 + j][d = dt*32 + lo], j = 0..7.
// ds_read_b64_tr_b16, per group of 16 lanes (i = lane & 15): lane i gives the
// address of 4 contiguous bf16; the 16 x 4 values are the 4 x 16 matrix
// M[e][c] = (lane 4*e + c/4, element c%4), and lane i receives column i,
// M[0..3][i]. So lanes 4e..4e+3 point at row (key) e, 16 consecutive d, and
// every lane comes back with 4 consecutive keys at d = i. Two reads give the
// 8 keys. HW-verified by tests/test_prefill_ragged_gpu.py::
// test_transposing_read_probe with asymmetric data.
template <int D>
__device__ __forceinline__ short8 pf_vfrag(const bf16* tile, int ks, int dt,
                                           int lane) {
  const int i = lane & 15, g1 = (lane >> 4) & 1, hi = lane >> 5;
  const int colb = (dt * 32 + g1 * 16 + (i & 3) * 4) * 2;
  short4v x[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = ks * 16 + hi * 8 + h * 4 + (i >> 2);
    const lds_char* p =
        (const lds_char*)tile + row * (D * 2) + (colb ^ pf_vswz<D>(row));
    x[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)p);
  }
  return short8{x[0][0], x[0][1], x[0][2], x[0][3],
                x[1][0], x[1][1], x[1][2], x[1][3]};
}

__device__ __forceinline__ f32x16 pf_mfma(short8 a, short8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// two f32 -> one dword of 2 bf16, round to nearest even
__device__ __forceinline__ unsigned pf_cvt_pk(float lo_, float hi_) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo_), "v"(hi_));
  return r;
}

// v_permlane32_swap_b32 a, b: a's lanes >= 32 swap with b's lanes < 32
__device__ __forceinline__ void pf_swap32(unsigned& a, unsigned& b) {
  asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// P^T fragment of 16 keys from the two 4-value r-groups g0, g0 + 4 of a score
// tile: pack, then swap halves with the partner lane: lanes < 32 end with
// keys 0..7, lanes >= 32 with keys 8..15 of the slice.
__device__ __forceinline__ short8 pf_pfrag(float xa, float xb, float xc,
                                           float xd, float ya, float yb,
                                           float yc, float yd) {
  unsigned x0 = pf_cvt_pk(xa, xb);
  unsigned x1 = pf_cvt_pk(xc, xd);
  unsigned y0 = pf_cvt_pk(ya, yb);
  unsigned y1 = pf_cvt_pk(yc, yd);
  pf_swap32(x0, y0);
  pf_swap32(x1, y1);
  short8 frag;
  reinterpret_cast<unsigned*>(&frag)[0] = x0;
  reinterpret_cast<unsigned*>(&frag)[1] = x1;
  reinterpret_cast<unsigned*>(&frag)[2] = y0;
  reinterpret_cast<unsigned*>(&frag)[3] = y1;
  return frag;
}

// A (q-tile, split) with nothing live: zeros (one split) or the neutral
// partials (0, -1e30, 0). No cache row is touched.
template <int D, int GSH>
__device__ __forceinline__ void pf_write_empty(bf16* __restrict__ O,
                                               float* ws_o, float* ws_ml,
                                               int row0, int M, int nsplit,
                                               int b, int hkv, int T, int H,
                                               int tid) {
  constexpr int G = 1 << GSH;
  for (int i = tid; i < PF_Q_ROWS * (D / 8); i += PF_THREADS) {
    const int row = row0 + i / (D / 8), c8 = (i % (D / 8)) * 8;
    if (row >= M) break;
    if (nsplit == 1) {
      const int t = row >> GSH, g = row & (G - 1);
      *reinterpret_cast<short8*>(
          O + (((int64_t)b * T + t) * H + hkv * G + g) * D + c8) =
          short8{0, 0, 0, 0, 0, 0, 0, 0};
    } else {
      float* p = ws_o + (int64_t)row * D + c8;
      *reinterpret_cast<f32x4*>(p) = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(p + 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c8 == 0) {
        ws_ml[row * 2] = PF_NEG;
        ws_ml[row * 2 + 1] = 0.f;
      }
    }
  }
}

// o_acc[dt][r] is d = dt*32 + (r&3) + 8*(r>>2) + 4*hi of query row lo;
// l_run is already reduced over the lane pair.
template <int D>
__device__ __forceinline__ void pf_epilogue(const f32x16 (&o_acc)[D / 32],
                                            float m_run, float l_run,
                                            bool live, bf16* orow, float* ws_o,
                                            float* ws_ml, int myrow,
                                            int nsplit, int hi) {
  if (nsplit == 1) {
    const float inv = (live && l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        bf16x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          y.v[j] = f2bf(live ? o_acc[dt][rg * 4 + j] * inv : 0.f);
        *reinterpret_cast<bf16x4*>(orow + dt * 32 + 8 * rg + 4 * hi) = y;
      }
  } else {
    float* prow_o = ws_o + (int64_t)myrow * D;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg)
        *reinterpret_cast<f32x4*>(prow_o + dt * 32 + 8 * rg + 4 * hi) =
            f32x4{o_acc[dt][rg * 4], o_acc[dt][rg * 4 + 1],
                  o_acc[dt][rg * 4 + 2], o_acc[dt][rg * 4 + 3]};
    if (hi == 0) {
      ws_ml[myrow * 2] = m_run;
      ws_ml[myrow * 2 + 1] = l_run;
    }
  }
}

// Stage keys [kb, kb + 64) of one (b, kv head) into `tile`; rows past `last`
// re-read row `last`. `gbase` is the (block-uniform) address logical row 0 of
// the tile's source has: the slab of a contiguous cache, or, for a page, its
// base minus its first logical row; every row read is in [kb, max(kb, last)].
// 256 lanes, 16 B each, D/32 rounds. The swizzle of the image is applied
// through the SOURCE address: LDS-DMA writes linearly.
template <int D, bool VTILE>
__device__ __forceinline__ void pf_stage(const bf16* __restrict__ gbase,
                                         int64_t row_stride, int kb, int last,
                                         bf16* tile, int tid) {
  constexpr int UPR = D / 8;  // 16 B units per row
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int u = i * PF_THREADS + tid;
    const int row = u / UPR;
    const int colb =
        ((u % UPR) * 16) ^ (VTILE ? pf_vswz<D>(row) : pf_kswz<D>(row));
    const bf16* src =
        gbase + (int64_t)min(kb + row, last) * row_stride + colb / 2;
    // linear destination: wave-uniform base + lane * 16
    lds_char* dst = (lds_char*)tile + i * (PF_THREADS * 16) + (tid >> 6) * 1024;
    __builtin_amdgcn_global_load_lds((g_void*)src, (lds_void*)dst, 16, 0, 0);
  }
}

// s_waitcnt vmcnt(0): this wave's loads, LDS-DMA included, have landed
__device__ __forceinline__ void pf_wait_loads() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

// The bf16 prefill kernel (the structure is described in prefill_ragged.hip).
// Where a key tile comes from is asked of a `Src` policy, a small struct
// built by the __global__ wrapper from its kernel arguments:
//   src.open(b, col, stride, r0, r1)  once, behind the empty-split return
//   src.off(kb, first)                element offset, from src.Kb / src.Vb, of
//                                     the pf_stage base of tile kb; `first`:
//                                     the split's first tile
//   src.prefetch(kb, r1)              behind the stage of the tile before kb
// so the contiguous and the paged kernel are one text.
template <int D, int GSH, class Src>
__device__ __forceinline__ void pf_body(
    const bf16* __restrict__ Q, bf16* __restrict__ O, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ n_new, int T, int H,
    int Hkv, int Smax, int split_rows, float scale, Src src) {
  constexpr int G = 1 << GSH;
  constexpr int QT = PF_Q_ROWS / G;  // tokens per q-tile
  constexpr int DSL = D / 16;        // k-steps of the score MFMA
  constexpr int DT32 = D / 32;       // 32-wide d tiles of O^T
  const int qt = gridDim.x - 1 - blockIdx.x;  // longest trips first
  const int bk = blockIdx.y;
  const int b = bk / Hkv, hkv = bk - b * Hkv;
  const int sp = blockIdx.z, nsplit = gridDim.z;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int lo = lane & 31, hi = lane >> 5;
  const int M = T * G;
  int L0, n;
  pf_live(lens, n_new, b, T, Smax, L0, n);

  const int t0 = qt * QT;                 // first token of the tile
  const int tl = min(t0 + QT, n) - 1;     // its last LIVE token
  const int row0 = qt * PF_Q_ROWS;
  const int r0 = sp * split_rows;
  const int r1 = tl >= t0 ? min(r0 + split_rows, L0 + tl) : 0;
  // partials of this (b, kv head, split)
  const int64_t prow = ((int64_t)bk * nsplit + sp) * M;
  float* ws_o = ws + prow * D;
  float* ws_ml = ws + (int64_t)gridDim.y * nsplit * M * D + prow * 2;

  if (r0 >= r1) {  // block-uniform: nothing live here; no cache row touched
    pf_write_empty<D, GSH>(O, ws_o, ws_ml, row0, M, nsplit, b, hkv, T, H, tid);
    return;
  }

  __shared__ __attribute__((aligned(1024))) bf16 k_lds[2][PF_KEY_TILE * D];
  __shared__ __attribute__((aligned(1024))) bf16 v_lds[2][PF_KEY_TILE * D];

  const int64_t row_stride = (int64_t)Hkv * D;
  src.open(b, (int64_t)hkv * D, row_stride, r0, r1);
  const int last = r1 - 1;  // tile loads past the range re-read this row

  // ---- this lane's query row; rows of dead tokens run on zeros
  const int myrow = row0 + wid * 32 + lo;
  const int my_t = myrow >> GSH, my_g = myrow & (G - 1);
  const bool live = my_t < n;
  const int64_t qo_off =
      (((int64_t)b * T + my_t) * H + hkv * G + my_g) * D;  // used if my_t < T
  short8 qf[DSL];
#pragma unroll
  for (int ds = 0; ds < DSL; ++ds) {
    qf[ds] = short8{0, 0, 0, 0, 0, 0, 0, 0};
    if (live)
      qf[ds] = *reinterpret_cast<const short8*>(Q + qo_off + ds * 16 + hi * 8);
  }
  const int lim = min(r1, L0 + my_t);  // first key this row may NOT see
  // wave-uniform: first / last live token of the wave
  const int tw0 = (row0 + wid * 32) >> GSH;
  const int twl = min((row0 + wid * 32 + 31) >> GSH, tl);
  const int kend_w = tw0 < n ? min(r1, L0 + twl) : 0;
  const int lim_min = min(r1, L0 + tw0);

  float m_run = PF_NEG, l_run = 0.f;
  f32x16 o_acc[DT32];
#pragma unroll
  for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[dt][r] = 0.f;

  {
    const int64_t off = src.off(r0, true);
    pf_stage<D, false>(src.Kb + off, row_stride, r0, last, k_lds[0], tid);
    pf_stage<D, true>(src.Vb + off, row_stride, r0, last, v_lds[0], tid);
  }
  for (int kb = r0, it = 0; kb < r1; kb += PF_KEY_TILE, ++it) {
    const int buf = it & 1;
    // tile boundary, reached by every wave on every path: this wave's share
    // of tile `it` has landed; behind the barrier everyone's has, and tile
    // it - 1 is consumed
    pf_wait_loads();
    __syncthreads();
    if (kb + PF_KEY_TILE < r1) {
      const int64_t off = src.off(kb + PF_KEY_TILE, false);
      pf_stage<D, false>(src.Kb + off, row_stride, kb + PF_KEY_TILE, last,
                         k_lds[buf ^ 1], tid);
      pf_stage<D, true>(src.Vb + off, row_stride, kb + PF_KEY_TILE, last,
                        v_lds[buf ^ 1], tid);
    }
    src.prefetch(kb + 2 * PF_KEY_TILE, r1);
    if (kb >= kend_w) continue;  // past this wave's last live row

    // ---- St = K . Q^T: two 32-key C tiles
    f32x16 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[t][r] = 0.f;
#pragma unroll
      for (int ds = 0; ds < DSL; ++ds)
        st[t] = pf_mfma(pf_kfrag<D>(k_lds[buf], t * 32 + lo, ds * 32 + hi * 16),
                        qf[ds], st[t]);
    }
    // ---- online softmax, lane-local: st[t][r] is key kb + t*32 + (r&3) +
    // 8*(r>>2) + 4*hi of query row lo
    if (kb + PF_KEY_TILE > lim_min) {  // wave-uniform: a step the mask bites
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kg = kb + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          st[t][r] = kg < lim ? st[t][r] * scale : PF_NEG;
        }
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) st[t][r] *= scale;
    }
    float tmax = PF_NEG;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, st[t][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mnew = fmaxf(m_run, tmax);
    if (__ballot(mnew > m_run)) {  // some row of the wave grew
      const float alpha = __expf(m_run - mnew);  // 1 for rows that did not
      l_run *= alpha;
#pragma unroll
      for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[dt][r] *= alpha;
      m_run = mnew;
    }
    // a row with no visible key yet subtracts 0: exp(-1e30) = 0 exactly
    const float msub = m_run == PF_NEG ? 0.f : m_run;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __expf(st[t][r] - msub);
        st[t][r] = p;
        psum += p;
      }
    l_run += psum;  // this lane's half of the row; pair-reduced at the end

    // ---- P^T fragments (pf_pfrag): 16 keys each, natural key order
    short8 pa[4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kst = 0; kst < 2; ++kst) {
        const int g0 = 8 * kst, g1 = 8 * kst + 4;
        pa[t * 2 + kst] = pf_pfrag(st[t][g0], st[t][g0 + 1], st[t][g0 + 2],
                                   st[t][g0 + 3], st[t][g1], st[t][g1 + 1],
                                   st[t][g1 + 2], st[t][g1 + 3]);
      }
    // ---- O^T += V^T . P^T
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        o_acc[dt] = pf_mfma(pf_vfrag<D>(v_lds[buf], ks, dt, lane), pa[ks],
                            o_acc[dt]);
  }

  l_run += __shfl_xor(l_run, 32, 64);
  if (myrow >= M) return;
  pf_epilogue<D>(o_acc, m_run, l_run, live, O + qo_off, ws_o, ws_ml, myrow,
                 nsplit, hi);
}

// grid B*T*H, D threads: splits combined in index order; dead queries
// (t >= n, idle slots) are written as exact zeros.
static __global__ void attn_prefill_merge_kernel(
    const float* __restrict__ ws, bf16* __restrict__ O,
    const int* __restrict__ lens, const int* __restrict__ n_new, int B, int T,
    int H, int Hkv, int D, int Smax, int nsplit) {
  const int bth = blockIdx.x;
  const int b = bth / (T * H);
  const int th = bth - b * (T * H);
  const int t = th / H, h = th - t * H;
  const int G = H / Hkv, M = T * G;
  const int hkv = h / G, row = t * G + (h - hkv * G);
  const int d = threadIdx.x;
  int L0, n;
  pf_live(lens, n_new, b, T, Smax, L0, n);
  bf16* o = O + (int64_t)bth * D + d;
  if (t >= n) {
    *o = f2bf(0.f);
    return;
  }
  const int64_t p0 = ((int64_t)b * Hkv + hkv) * nsplit * M + row;
  const float* po = ws + p0 * D + d;
  const float* pml = ws + (int64_t)B * Hkv * nsplit * M * D + p0 * 2;
  float mx = PF_NEG;
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, pml[(int64_t)s * M * 2]);
  float num = 0.f, den = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float w = __expf(pml[(int64_t)s * M * 2] - mx);
    den += w * pml[(int64_t)s * M * 2 + 1];
    num += w * po[(int64_t)s * M * D];
  }
  *o = f2bf(num / fmaxf(den, 1e-30f));
}

// The argument checks of both entry points; 0 or hipErrorInvalidValue.
static inline int pf_check_args(int64_t B, int64_t T, int64_t H, int64_t Hkv,
                                int64_t Smax, int64_t D, int64_t split_rows,
                                const void* ws, const void* lens,
                                const void* n_new) {
  if ((D != 64 && D != 128) || B < 1 || T < 1 || H < 1 || Hkv < 1 ||
      Smax < 1 || T > Smax || H % Hkv != 0 || split_rows < PF_KEY_TILE ||
      split_rows % PF_KEY_TILE != 0 || !lens || !n_new)
    return hipErrorInvalidValue;
  const int64_t G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return hipErrorInvalidValue;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  if (nsplit > 65535 || B * Hkv > 65535 || B * T * H > 0x7fffffff ||
      Smax > 0x7fffffff - split_rows - PF_Q_ROWS || (nsplit > 1 && !ws))
    return hipErrorInvalidValue;
  return 0;
}

// Calls launch(D, GSH, grid) with the checked D in {64, 128} and GSH = log2 G
// as integral constants; grid is (q-tiles, B*Hkv, nsplit). Callers must have
// run pf_check_args: any other G lands on the G = 8 instantiation.
template <class F>
static void pf_dispatch(int64_t B, int64_t T, int64_t H, int64_t Hkv,
                        int64_t D, int64_t nsplit, F launch) {
  const int64_t G = H / Hkv;
  const dim3 grid((unsigned)((T * G + PF_Q_ROWS - 1) / PF_Q_ROWS),
                  (unsigned)(B * Hkv), (unsigned)nsplit);
  auto with_d = [&](auto d) {
    switch (G) {
      case 1: launch(d, std::integral_constant<int, 0>{}, grid); break;
      case 2: launch(d, std::integral_constant<int, 1>{}, grid); break;
      case 4: launch(d, std::integral_constant<int, 2>{}, grid); break;
      default: launch(d, std::integral_constant<int, 3>{}, grid); break;
    }
  };
  if (D == 128)
    with_d(std::integral_constant<int, 128>{});
  else
    with_d(std::integral_constant<int, 64>{});
}

// The merge launch (when there is something to merge) and the status of
// every prefill entry point.
static inline int pf_launch_merge(hipStream_t stream, const void* ws, void* O,
                                  const void* lens, const void* n_new,
                                  int64_t B, int64_t T, int64_t H, int64_t Hkv,
                                  int64_t D, int64_t Smax, int64_t nsplit) {
  if (nsplit > 1)
    hipLaunchKernelGGL(attn_prefill_merge_kernel, dim3((unsigned)(B * T * H)),
                       dim3((unsigned)D), 0, stream, (const float*)ws, (bf16*)O,
                       (const int*)lens, (const int*)n_new, (int)B, (int)T,
                       (int)H, (int)Hkv, (int)D, (int)Smax, (int)nsplit);
  return (int)hipGetLastError();
}
