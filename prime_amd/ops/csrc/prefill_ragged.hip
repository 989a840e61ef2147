// Chunked ragged prefill for gfx950: a block of T new tokens per sequence
// attends to a KV cache that already holds a prefix (and the new rows).
//
// Contract (that of attn_decode_ragged_multi, without the T limit): lens[b]
// is the number of cache rows the FIRST new token attends to, n_new[b] the
// live new tokens; int32 DEVICE vectors read inside the kernels, clamped:
//   L0 = clamp(lens[b], 0, Smax);  n = L0 ? clamp(n_new[b], 0,
//   min(T, Smax - L0 + 1)) : 0.
// Query t < n attends to rows [0, L0 + t); query t >= n gives exact zeros.
// No cache row at or beyond L0 + n - 1 is loaded.
//
// Work split. Grid (q-tiles, B*Hkv, nsplit), heaviest (last) q-tile first.
// A workgroup of 4 waves owns PF_Q_ROWS = 128 rows r = t*G + g of one
// (b, kv head): 128/G consecutive tokens with all their heads, 32 rows per
// wave. It walks the keys [0, L0 + t_last) of its tile, intersected with its
// split range, in PF_KEY_TILE = 64-key steps. Each K and V tile is staged
// ONCE per workgroup into LDS, straight from the cache rows (row stride
// Hkv*D, 16 B LDS-DMA pieces, tracked loads), double-buffered: the next
// tile's loads are issued behind the tile-boundary barrier.
//
// Per wave and step, on mfma_f32_32x32x16_bf16 (maps of attention.hip):
//   St[key][row] = K . Q^T   A = K fragment, one 16 B LDS read at the
//                            swizzled address; B = Q^T fragment, in
//                            registers for the whole key loop. The
//                            accumulator holds St[key = (r&3) + 8*(r>>2) +
//                            4*hi][row = lo]: a row's scores are lane-local
//                            (the lane pair (l, l^32) splits the 64 keys).
//   softmax                  in registers + one __shfl_xor 32.
//   P                        packed to bf16 pairs, one permlane32 swap per
//                            pair: the B fragment P^T[k = hi*8 + j][row =
//                            lo] in natural key order. No LDS bounce.
//   O^T[d][row] = V^T . P^T  the mirrored form keeps the query row on lo
//                            in the O accumulator too, so the online-softmax
//                            rescale is a lane-local multiply. A = V^T
//                            fragment: lane needs V[key = hi*8 + j][d = lo],
//                            8 keys at one d, from a tile that has d
//                            contiguous. Two ds_read_b64_tr_b16 do that
//                            transpose on the LDS read (pf_vfrag): no V^T
//                            workspace, no transposing pass over the cache.
// Masks only where they bite: the select key < L0 + t(row) runs in steps that
// reach rows >= L0 + t_first of the wave (wave-uniform); a wave skips the
// steps past its last live row. Masked scores are the finite -1e30; a row
// whose running max is still -1e30 subtracts 0. Tile loads past the live
// range re-read its last row.
//
// nsplit == 1: the kernel normalises and stores bf16 itself, no workspace.
// Otherwise each split writes fp32 partials, o [B*Hkv, nsplit, M, D] followed
// by (m, l) [B*Hkv, nsplit, M, 2] with M = T*G (neutral (0, -1e30, 0) when
// empty), and attn_prefill_merge_kernel combines them in index order: no
// float atomics, bit-reproducible.
//
// Q, O [B,T,H,D]; K/V cache [B,Smax,Hkv,D] contiguous; D in {64,128},
// G = H/Hkv in {1,2,4,8}, 1 <= T <= Smax.
//
// This file is compiled without the packed fp32 VALU instructions
// (ops/build.py, NO_PACKED_FP32).
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

// Clamped (L0, n) of slot b, the same in both kernels.
__device__ __forceinline__ void pf_live(const int* __restrict__ lens,
                                        const int* __restrict__ n_new, int b,
                                        int T, int Smax, int& L0, int& n) {
  L0 = min(max(lens[b], 0), Smax);
  n = L0 == 0 ? 0 : min(max(n_new[b], 0), min(T, Smax - L0 + 1));
}

// ---- LDS images -----------------------------------------------------------
// Both tiles are [64 keys][D] bf16, linear, with an XOR on the byte offset
// inside the row, applied through the pre-swizzled SOURCE address (LDS-DMA
// writes linearly). K: the 16 B slot XOR of attention.hip's swz16 (a 16 B
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

// Stage keys [kb, kb + 64) of one (b, kv head) into `tile`; rows past `last`
// re-read row `last`. 256 lanes, 16 B each, D/32 rounds.
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

template <int D, int GSH>
__global__ __launch_bounds__(PF_THREADS, 2) void attn_prefill_ragged_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, bf16* __restrict__ O, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ n_new, int T, int H,
    int Hkv, int Smax, int split_rows, float scale) {
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
    return;
  }

  __shared__ __attribute__((aligned(1024))) bf16 k_lds[2][PF_KEY_TILE * D];
  __shared__ __attribute__((aligned(1024))) bf16 v_lds[2][PF_KEY_TILE * D];

  const int64_t row_stride = (int64_t)Hkv * D;
  const bf16* Kb = K + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const bf16* Vb = V + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
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

  pf_stage<D, false>(Kb, row_stride, r0, last, k_lds[0], tid);
  pf_stage<D, true>(Vb, row_stride, r0, last, v_lds[0], tid);
  for (int kb = r0, it = 0; kb < r1; kb += PF_KEY_TILE, ++it) {
    const int buf = it & 1;
    // tile boundary, reached by every wave on every path: this wave's share
    // of tile `it` has landed; behind the barrier everyone's has, and tile
    // it - 1 is consumed
    pf_wait_loads();
    __syncthreads();
    if (kb + PF_KEY_TILE < r1) {
      pf_stage<D, false>(Kb, row_stride, kb + PF_KEY_TILE, last, k_lds[buf ^ 1], tid);
      pf_stage<D, true>(Vb, row_stride, kb + PF_KEY_TILE, last, v_lds[buf ^ 1], tid);
    }
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

    // ---- P^T fragments: per 16 keys, pack the two 4-value r-groups and
    // swap halves with the partner lane: lanes < 32 end with keys 0..7,
    // lanes >= 32 with keys 8..15 of the slice
    short8 pa[4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kst = 0; kst < 2; ++kst) {
        const int g0 = 8 * kst, g1 = 8 * kst + 4;
        unsigned x0 = pf_cvt_pk(st[t][g0 + 0], st[t][g0 + 1]);
        unsigned x1 = pf_cvt_pk(st[t][g0 + 2], st[t][g0 + 3]);
        unsigned y0 = pf_cvt_pk(st[t][g1 + 0], st[t][g1 + 1]);
        unsigned y1 = pf_cvt_pk(st[t][g1 + 2], st[t][g1 + 3]);
        pf_swap32(x0, y0);
        pf_swap32(x1, y1);
        short8 frag;
        reinterpret_cast<unsigned*>(&frag)[0] = x0;
        reinterpret_cast<unsigned*>(&frag)[1] = x1;
        reinterpret_cast<unsigned*>(&frag)[2] = y0;
        reinterpret_cast<unsigned*>(&frag)[3] = y1;
        pa[t * 2 + kst] = frag;
      }
    // ---- O^T += V^T . P^T
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        o_acc[dt] = pf_mfma(pf_vfrag<D>(v_lds[buf], ks, dt, lane), pa[ks],
                            o_acc[dt]);
  }

  // ---- epilogue: o_acc[dt][r] is d = dt*32 + (r&3) + 8*(r>>2) + 4*hi of
  // query row lo
  l_run += __shfl_xor(l_run, 32, 64);
  if (myrow >= M) return;
  if (nsplit == 1) {
    const float inv = (live && l_run > 0.f) ? 1.f / l_run : 0.f;
    bf16* orow = O + qo_off;
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
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
    for (int dt = 0; dt < DT32; ++dt)
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
__global__ void attn_prefill_merge_kernel(
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

template <int D, int GSH>
static void pf_launch(hipStream_t stream, dim3 grid, const void* Q,
                      const void* K, const void* V, void* O, void* ws,
                      const void* lens, const void* n_new, int T, int H,
                      int Hkv, int Smax, int split_rows, float scale) {
  hipLaunchKernelGGL((attn_prefill_ragged_kernel<D, GSH>), grid,
                     dim3(PF_THREADS), 0, stream, (const bf16*)Q,
                     (const bf16*)K, (const bf16*)V, (bf16*)O, (float*)ws,
                     (const int*)lens, (const int*)n_new, T, H, Hkv, Smax,
                     split_rows, scale);
}

template <int D>
static void pf_launch_g(int gsh, hipStream_t stream, dim3 grid, const void* Q,
                        const void* K, const void* V, void* O, void* ws,
                        const void* lens, const void* n_new, int T, int H,
                        int Hkv, int Smax, int split_rows, float scale) {
  switch (gsh) {
    case 0: pf_launch<D, 0>(stream, grid, Q, K, V, O, ws, lens, n_new, T, H, Hkv, Smax, split_rows, scale); break;
    case 1: pf_launch<D, 1>(stream, grid, Q, K, V, O, ws, lens, n_new, T, H, Hkv, Smax, split_rows, scale); break;
    case 2: pf_launch<D, 2>(stream, grid, Q, K, V, O, ws, lens, n_new, T, H, Hkv, Smax, split_rows, scale); break;
    default: pf_launch<D, 3>(stream, grid, Q, K, V, O, ws, lens, n_new, T, H, Hkv, Smax, split_rows, scale); break;
  }
}

// Tile constants (ops.PREFILL_Q_ROWS / ops.PREFILL_KEY_TILE mirror them).
PRIME_API int prime_prefill_q_rows(void) { return PF_Q_ROWS; }
PRIME_API int prime_prefill_key_tile(void) { return PF_KEY_TILE; }

// split_rows: a positive multiple of PF_KEY_TILE chosen from the launch shape
// only. nsplit = ceil(Smax / split_rows); with nsplit == 1 ws is not used,
// otherwise ws is fp32 [B*Hkv * nsplit * T*(H/Hkv) * (D + 2)].
PRIME_API int prime_attn_prefill_ragged(
    hipStream_t stream, const void* Q, const void* K, const void* V, void* O,
    void* ws, const void* lens, const void* n_new, int64_t B, int64_t T,
    int64_t H, int64_t Hkv, int64_t Smax, int64_t D, int64_t split_rows,
    double scale) {
  if ((D != 64 && D != 128) || B < 1 || T < 1 || H < 1 || Hkv < 1 ||
      Smax < 1 || T > Smax || H % Hkv != 0 || split_rows < PF_KEY_TILE ||
      split_rows % PF_KEY_TILE != 0 || !lens || !n_new)
    return hipErrorInvalidValue;
  const int64_t G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return hipErrorInvalidValue;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  const int64_t nqt = (T * G + PF_Q_ROWS - 1) / PF_Q_ROWS;
  if (nsplit > 65535 || B * Hkv > 65535 || B * T * H > 0x7fffffff ||
      Smax > 0x7fffffff - split_rows - PF_Q_ROWS || (nsplit > 1 && !ws))
    return hipErrorInvalidValue;
  const int gsh = G == 1 ? 0 : (G == 2 ? 1 : (G == 4 ? 2 : 3));
  const dim3 grid((unsigned)nqt, (unsigned)(B * Hkv), (unsigned)nsplit);
  if (D == 128)
    pf_launch_g<128>(gsh, stream, grid, Q, K, V, O, ws, lens, n_new, (int)T,
                     (int)H, (int)Hkv, (int)Smax, (int)split_rows, (float)scale);
  else
    pf_launch_g<64>(gsh, stream, grid, Q, K, V, O, ws, lens, n_new, (int)T,
                    (int)H, (int)Hkv, (int)Smax, (int)split_rows, (float)scale);
  if (nsplit > 1)
    hipLaunchKernelGGL(attn_prefill_merge_kernel, dim3((unsigned)(B * T * H)),
                       dim3((unsigned)D), 0, stream, (const float*)ws, (bf16*)O,
                       (const int*)lens, (const int*)n_new, (int)B, (int)T,
                       (int)H, (int)Hkv, (int)D, (int)Smax, (int)nsplit);
  return (int)hipGetLastError();
}

// ---- probe of the transposing LDS read --------------------------------
// src [64][64] bf16 -> dst = src^T, through the kernel's own V path: the
// swizzled stage of a 64-key D = 64 tile, then pf_vfrag. Wave w transposes
// keys [16w, 16w + 16).
__global__ __launch_bounds__(PF_THREADS) void tr16_probe_kernel(
    const bf16* __restrict__ src, bf16* __restrict__ dst) {
  __shared__ __attribute__((aligned(1024))) bf16 tile[PF_KEY_TILE * 64];
  const int tid = threadIdx.x, lane = tid & 63, ks = tid >> 6;
  pf_stage<64, true>(src, 64, 0, PF_KEY_TILE - 1, tile, tid);
  pf_wait_loads();
  __syncthreads();
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
    *reinterpret_cast<short8*>(dst + (dt * 32 + (lane & 31)) * 64 + ks * 16 +
                               (lane >> 5) * 8) = pf_vfrag<64>(tile, ks, dt, lane);
}

PRIME_API int prime_tr16_probe(hipStream_t stream, const void* src, void* dst) {
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(PF_THREADS), 0, stream,
                     (const bf16*)src, (bf16*)dst);
  return (int)hipGetLastError();
}
