// What the chunked ragged prefill kernels share (prefill_ragged.hip over the
// bf16 cache, prefill_ragged_fp8.hip over the fp8 cache): the tile constants,
// the (lens, n_new) clamp, the swizzles of the two LDS images with the
// fragment reads that undo them, the MFMA / pack helpers, the empty-split
// and epilogue stores and the merge kernel. The library is one non-RDC
// compile per file, so the kernels here are `static`: each file gets its own
// copy, and the swizzle a file stages with cannot drift from the XOR the
// fragment reads apply.
//
// Both including files are compiled without the packed fp32 VALU
// instructions (ops/build.py, NO_PACKED_FP32).
#pragma once
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
