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

// The tile source of pf_body: every tile of sequence b comes from slab b.
struct PfContiguous {
  const bf16 *Kb, *Vb;
  int Smax;
  __device__ __forceinline__ void open(int b, int64_t col, int64_t row_stride,
                                       int, int) {
    Kb += (int64_t)b * Smax * row_stride + col;
    Vb += (int64_t)b * Smax * row_stride + col;
  }
  __device__ __forceinline__ int64_t off(int, bool) const { return 0; }
  __device__ __forceinline__ void prefetch(int, int) {}
};

template <int D, int GSH>
__global__ __launch_bounds__(PF_THREADS, 2) void attn_prefill_ragged_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, bf16* __restrict__ O, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ n_new, int T, int H,
    int Hkv, int Smax, int split_rows, float scale) {
  pf_body<D, GSH>(Q, O, ws, lens, n_new, T, H, Hkv, Smax, split_rows, scale,
                  PfContiguous{K, V, Smax});
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
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  pf_dispatch(B, T, H, Hkv, D, nsplit, [&](auto d, auto gsh, dim3 grid) {
    hipLaunchKernelGGL((attn_prefill_ragged_kernel<d(), gsh()>), grid,
                       dim3(PF_THREADS), 0, stream, (const bf16*)Q,
                       (const bf16*)K, (const bf16*)V, (bf16*)O, (float*)ws,
                       (const int*)lens, (const int*)n_new, (int)T, (int)H,
                       (int)Hkv, (int)Smax, (int)split_rows, (float)scale);
  });
  return pf_launch_merge(stream, ws, O, lens, n_new, B, T, H, Hkv, D, Smax,
                         nsplit);
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
