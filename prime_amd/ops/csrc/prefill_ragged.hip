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
#include "prefill_common.h"

// Stage keys [kb, kb + 64) of one (b, kv head) into `tile`; rows past `last`
// re-read row `last`. 256 lanes, 16 B each, D/32 rounds. The swizzle of the
// image (prefill_common.h) is applied through the SOURCE address: LDS-DMA
// writes linearly.
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
    pf_write_empty<D, GSH>(O, ws_o, ws_ml, row0, M, nsplit, b, hkv, T, H, tid);
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
  if (pf_check_args(B, T, H, Hkv, Smax, D, split_rows, ws, lens, n_new))
    return hipErrorInvalidValue;
  const int64_t G = H / Hkv;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  const int64_t nqt = (T * G + PF_Q_ROWS - 1) / PF_Q_ROWS;
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
