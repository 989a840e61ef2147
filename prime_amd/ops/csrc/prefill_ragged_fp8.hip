// Chunked ragged prefill over the fp8 (OCP e4m3fn) KV cache for gfx950: the
// contract of prefill_ragged.hip word for word (grid, q-tile / split ranges,
// lens / n_new clamp, dead rows, empty splits, workspace layout, index-order
// merge) with the cache format of decode_fp8kv.hip (k, v bytes
// [B,Smax,Hkv,D]; k_scale, v_scale fp32 [B,Smax,Hkv], value = float(byte) *
// scale). The values attended to are kv_cache_dequant(cache); q, the scores,
// P and the accumulators are not quantised. No byte and no scale at or
// beyond row L0 + n - 1 is loaded.
//
// Both products, the fragment maps, the register softmax and the P pack are
// those of attn_prefill_ragged_kernel; what differs is how a tile reaches
// LDS. LDS-DMA cannot convert and the transposing V read needs 16-bit
// elements, so the bytes are DECODED ONCE PER WORKGROUP ON THE WAY INTO LDS,
// into the very bf16 images (pf_kswz / pf_vswz) the bf16 kernel reads:
//
//   load     tile it + 1, right behind the tile-boundary barrier: per lane
//            D/64 16 B loads of K, D/64 of V (a 64 x D byte tile is 256
//            lanes x D/64 units of 16 bytes; unit u = i*256 + tid is row
//            u / (D/16), bytes 16*(u % (D/16))..), and one 4 B scale: lanes
//            0..63 k_scale of the 64 keys, lanes 64..127 v_scale. Ordinary
//            tracked loads that stay in registers (8 + 1 VGPRs at D = 128)
//            through tile it's MFMAs: their first use is the decode below,
//            so the vmcnt wait lands behind the compute.
//   decode   after the PV MFMAs of tile it: cvt_pk_f32_fp8, then the upper
//            16 bits of each fp32 with one v_perm_b32 per pair (exact: a
//            finite e4m3 value has at most 4 significant bits and an
//            exponent inside the bf16 range).
//   store    two ds_write_b128 per 16 loaded bytes into buffer buf ^ 1. The
//            K XOR moves whole 16 B slots and the V XOR whole 64 B blocks,
//            so a unit's 32 decoded bytes stay two whole slots. Bank
//            conflicts (64 banks, a b128 store served per 16 lanes, which
//            here are D=128: 2 rows x 8 units, D=64: 4 rows x 4 units): the K
//            XOR differs in its low bit between the rows that share a slot
//            column, so 16 lanes hit 16 slots: none. The V XOR leaves the low
//            slot bit alone, which would put two rows on the same 8 even
//            slots (2-way on every V store); the lanes of the odd row (D=64:
//            odd row pair) therefore store their upper 8 elements first:
//            none either. The swap is 4 v_cndmask on the loaded dwords.
//   scales   two [2][64] float arrays; a lane's 16 keys of a 32-key score
//            tile are t*32 + 8*(r>>2) + 4*hi + (r&3), four consecutive per
//            r>>2: one ds_read_b128 each, 8 for k_scale and 8 for v_scale
//            per step, two addresses per wave (broadcast).
// Buffer rule: buf ^ 1 is written only behind the barrier that ended its last
// read and read only behind the next barrier; one barrier per tile. A wave
// that skips a step (past its last live row) still loads, decodes and stores
// its share. The prologue loads, decodes and stores tile 0.
//
// k_scale enters at the score, x = st * (k_scale[key] * scale), before mask,
// max and exp; the product in brackets is taken once, at the LDS store.
// v_scale enters at P before rounding: the fragment is bf16(p * v_scale[key])
// while the row sum keeps the unscaled fp32 p (the rule of both other fp8
// attention kernels). A masked p is exactly 0 and the clamped scale of row
// `last` is finite.
//
// This file is compiled without the packed fp32 VALU instructions
// (ops/build.py, NO_PACKED_FP32).
#include "prefill_common.h"

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef unsigned char u8;

// Eight e4m3 bytes (two dwords, element j in byte j) -> eight bf16: the upper
// half of each fp32 IS the bf16 (see the head).
__device__ __forceinline__ short8 pf8_dec8(unsigned w0, unsigned w1) {
  u32x4 d;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const unsigned w = h ? w1 : w0;
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    d[2 * h] = __builtin_amdgcn_perm(__float_as_uint(a.y), __float_as_uint(a.x),
                                     0x07060302u);
    d[2 * h + 1] = __builtin_amdgcn_perm(__float_as_uint(c.y),
                                         __float_as_uint(c.x), 0x07060302u);
  }
  return __builtin_bit_cast(short8, d);
}

// One tile in flight: this lane's units of K and V and its scale.
template <int D>
struct Pf8Regs {
  u32x4 k[D / 64], v[D / 64];
  float s;
};

// Issue the loads of keys [kb, kb + 64); rows and scales past `last` re-read
// row `last`. Waves 2 and 3 load no scale.
template <int D>
__device__ __forceinline__ void pf8_load(
    const u8* __restrict__ Kb, const u8* __restrict__ Vb,
    const float* __restrict__ Ksb, const float* __restrict__ Vsb,
    int64_t row_stride, int Hkv, int kb, int last, int tid, Pf8Regs<D>& x) {
  constexpr int UPR = D / 16;  // 16-byte units per row
#pragma unroll
  for (int i = 0; i < D / 64; ++i) {
    const int u = i * PF_THREADS + tid;
    const int64_t off =
        (int64_t)min(kb + u / UPR, last) * row_stride + (u % UPR) * 16;
    x.k[i] = *reinterpret_cast<const u32x4*>(Kb + off);
    x.v[i] = *reinterpret_cast<const u32x4*>(Vb + off);
  }
  x.s = 0.f;
  if (tid < 2 * PF_KEY_TILE) {  // wave-uniform
    const int64_t key = min(kb + (tid & (PF_KEY_TILE - 1)), last);
    x.s = (tid < PF_KEY_TILE ? Ksb : Vsb)[key * Hkv];
  }
}

// Decode one unit into its two 16 B slots of row `rowp`; `first` is the half
// (0: elements 0..7) that the first store carries.
__device__ __forceinline__ void pf8_store_unit(char* rowp, int colb, int swz,
                                               int first, u32x4 w) {
  const unsigned a0 = first ? w[2] : w[0], a1 = first ? w[3] : w[1];
  const unsigned b0 = first ? w[0] : w[2], b1 = first ? w[1] : w[3];
  *reinterpret_cast<short8*>(rowp + ((colb + first * 16) ^ swz)) =
      pf8_dec8(a0, a1);
  *reinterpret_cast<short8*>(rowp + ((colb + 16 - first * 16) ^ swz)) =
      pf8_dec8(b0, b1);
}

// Decode a loaded tile into the bf16 images and the scale arrays of one
// buffer; ks gets k_scale * scale.
template <int D>
__device__ __forceinline__ void pf8_store(const Pf8Regs<D>& x, bf16* ktile,
                                          bf16* vtile, float* ks, float* vs,
                                          float scale, int tid) {
  constexpr int UPR = D / 16;
#pragma unroll
  for (int i = 0; i < D / 64; ++i) {
    const int u = i * PF_THREADS + tid;
    const int row = u / UPR, colb = (u % UPR) * 32;
    // K: in natural order; V: the odd row (pair) leads with its upper half
    pf8_store_unit(reinterpret_cast<char*>(ktile) + row * (D * 2), colb,
                   pf_kswz<D>(row), 0, x.k[i]);
    pf8_store_unit(reinterpret_cast<char*>(vtile) + row * (D * 2), colb,
                   pf_vswz<D>(row), (D == 128 ? row : row >> 1) & 1, x.v[i]);
  }
  if (tid < PF_KEY_TILE)
    ks[tid] = x.s * scale;  // the softmax scale rides on k_scale
  else if (tid < 2 * PF_KEY_TILE)
    vs[tid - PF_KEY_TILE] = x.s;
}

// Workgroups per CU (= waves per SIMD) the register allocator is held to:
// D = 128 the bf16 kernel's 2; D = 64 fits 3 without scratch when asked
// (docs/KERNELS.md).
template <int D, int GSH>
__global__ __launch_bounds__(PF_THREADS, D == 128 ? 2 : 3) void
attn_prefill_ragged_fp8_kernel(
    const bf16* __restrict__ Q, const u8* __restrict__ K,
    const u8* __restrict__ V, const float* __restrict__ Ks,
    const float* __restrict__ Vs, bf16* __restrict__ O, float* __restrict__ ws,
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
    pf_write_empty<D, GSH>(O, ws_o, ws_ml, row0, M, nsplit, b, hkv, T, H, tid);
    return;
  }

  __shared__ __attribute__((aligned(1024))) bf16 k_lds[2][PF_KEY_TILE * D];
  __shared__ __attribute__((aligned(1024))) bf16 v_lds[2][PF_KEY_TILE * D];
  __shared__ __attribute__((aligned(16))) float ks_lds[2][PF_KEY_TILE];
  __shared__ __attribute__((aligned(16))) float vs_lds[2][PF_KEY_TILE];

  const int64_t row_stride = (int64_t)Hkv * D;  // bytes = elements
  const u8* Kb = K + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const u8* Vb = V + (int64_t)b * Smax * row_stride + (int64_t)hkv * D;
  const float* Ksb = Ks + (int64_t)b * Smax * Hkv + hkv;
  const float* Vsb = Vs + (int64_t)b * Smax * Hkv + hkv;
  const int last = r1 - 1;  // loads past the range re-read this row

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

  Pf8Regs<D> nx;
  pf8_load<D>(Kb, Vb, Ksb, Vsb, row_stride, Hkv, r0, last, tid, nx);
  pf8_store<D>(nx, k_lds[0], v_lds[0], ks_lds[0], vs_lds[0], scale, tid);
  for (int kb = r0, it = 0; kb < r1; kb += PF_KEY_TILE, ++it) {
    const int buf = it & 1;
    // tile boundary, reached by every wave on every path: behind the barrier
    // everyone's stores of tile `it` are visible and tile it - 1 is consumed
    __syncthreads();
    const bool more = kb + PF_KEY_TILE < r1;  // block-uniform
    if (more)
      pf8_load<D>(Kb, Vb, Ksb, Vsb, row_stride, Hkv, kb + PF_KEY_TILE, last,
                  tid, nx);
    if (kb < kend_w) {  // not past this wave's last live row
      // ---- St = K . Q^T: two 32-key C tiles
      f32x16 st[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[t][r] = 0.f;
#pragma unroll
        for (int ds = 0; ds < DSL; ++ds)
          st[t] = pf_mfma(
              pf_kfrag<D>(k_lds[buf], t * 32 + lo, ds * 32 + hi * 16), qf[ds],
              st[t]);
      }
      // ---- online softmax, lane-local: st[t][r] is key kb + t*32 + (r&3) +
      // 8*(r>>2) + 4*hi of query row lo; ks_lds holds k_scale * scale
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const f32x4 sc = *reinterpret_cast<const f32x4*>(
              &ks_lds[buf][t * 32 + 8 * rg + 4 * hi]);
#pragma unroll
          for (int j = 0; j < 4; ++j) st[t][rg * 4 + j] *= sc[j];
        }
      if (kb + PF_KEY_TILE > lim_min) {  // wave-uniform: a step the mask bites
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kg = kb + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            st[t][r] = kg < lim ? st[t][r] : PF_NEG;
          }
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
          psum += p;  // the row sum keeps the unscaled weight
        }
      l_run += psum;  // this lane's half of the row; pair-reduced at the end

      // ---- P^T fragments (pf_pfrag) of p * v_scale: 16 keys each, natural
      // key order
      short8 pa[4];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kst = 0; kst < 2; ++kst) {
          const int g0 = 8 * kst, g1 = 8 * kst + 4;
          const f32x4 s0 = *reinterpret_cast<const f32x4*>(
              &vs_lds[buf][t * 32 + 2 * g0 + 4 * hi]);
          const f32x4 s1 = *reinterpret_cast<const f32x4*>(
              &vs_lds[buf][t * 32 + 2 * g1 + 4 * hi]);
          pa[t * 2 + kst] = pf_pfrag(
              st[t][g0] * s0[0], st[t][g0 + 1] * s0[1], st[t][g0 + 2] * s0[2],
              st[t][g0 + 3] * s0[3], st[t][g1] * s1[0], st[t][g1 + 1] * s1[1],
              st[t][g1 + 2] * s1[2], st[t][g1 + 3] * s1[3]);
        }
      // ---- O^T += V^T . P^T
#pragma unroll
      for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          o_acc[dt] = pf_mfma(pf_vfrag<D>(v_lds[buf], ks, dt, lane), pa[ks],
                              o_acc[dt]);
    }
    // tile it + 1 into the other buffer: its last readers passed the barrier
    // above, its next ones wait behind the barrier below
    if (more)
      pf8_store<D>(nx, k_lds[buf ^ 1], v_lds[buf ^ 1], ks_lds[buf ^ 1],
                   vs_lds[buf ^ 1], scale, tid);
  }

  l_run += __shfl_xor(l_run, 32, 64);
  if (myrow >= M) return;
  pf_epilogue<D>(o_acc, m_run, l_run, live, O + qo_off, ws_o, ws_ml, myrow,
                 nsplit, hi);
}

// The contract of prime_attn_prefill_ragged (split_rows, ws layout), with the
// cache as e4m3 bytes K/V [B,Smax,Hkv,D] + fp32 k_scale/v_scale [B,Smax,Hkv].
PRIME_API int prime_attn_prefill_ragged_fp8(
    hipStream_t stream, const void* Q, const void* K, const void* V,
    const void* k_scale, const void* v_scale, void* O, void* ws,
    const void* lens, const void* n_new, int64_t B, int64_t T, int64_t H,
    int64_t Hkv, int64_t Smax, int64_t D, int64_t split_rows, double scale) {
  if (pf_check_args(B, T, H, Hkv, Smax, D, split_rows, ws, lens, n_new) ||
      !k_scale || !v_scale)
    return hipErrorInvalidValue;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  pf_dispatch(B, T, H, Hkv, D, nsplit, [&](auto d, auto gsh, dim3 grid) {
    hipLaunchKernelGGL((attn_prefill_ragged_fp8_kernel<d(), gsh()>), grid,
                       dim3(PF_THREADS), 0, stream, (const bf16*)Q,
                       (const u8*)K, (const u8*)V, (const float*)k_scale,
                       (const float*)v_scale, (bf16*)O, (float*)ws,
                       (const int*)lens, (const int*)n_new, (int)T, (int)H,
                       (int)Hkv, (int)Smax, (int)split_rows, (float)scale);
  });
  return pf_launch_merge(stream, ws, O, lens, n_new, B, T, H, Hkv, D, Smax,
                         nsplit);
}
