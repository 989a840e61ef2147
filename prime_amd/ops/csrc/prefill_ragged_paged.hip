// Chunked ragged prefill over a PAGED bf16 KV cache (gfx950): a block of T
// new tokens per sequence attends to a cache that already holds a prefix
// (and the new rows), stored as a pool of pages K/V [n_pages, P, Hkv, D]
// with an int32 block table [B, max_pages] read inside the kernel. Logical
// row r of sequence b is pool row table[b, r / P] * P + r % P; Smax =
// max_pages * P takes the place of the contiguous Smax in the (lens, n_new)
// clamp, the splits and the workspace.
//
// Contract and structure are those of prefill_ragged.hip (128-row q-tiles,
// 64-key tiles, both 32x32x16 products, register softmax, the transposing V
// read, the swizzles, the double-buffered LDS-DMA stage, split + merge):
// both kernels are pf_body of prefill_common.h, so for the same rows the
// result is bit-identical. The address path, the tile source PfPaged below:
//
//  - P is a multiple of the key tile and tiles are aligned, so a staged tile
//    lies in ONE page: the stage takes one block-uniform page base per tile.
//    "Rows past `last` re-read row `last`" is unchanged: last >= the tile's
//    first row, so it is in the tile's page.
//  - Page ids are a two-deep scalar pipeline: pid0 (the split's first tile),
//    pid_nxt (tile staged behind this barrier). The id of the tile AFTER
//    next is loaded right after that stage is issued, a whole tile of
//    compute before its first use, so the prefetch issue behind the
//    tile-boundary barrier never waits on a table load.
//
// Safety: an entry is read only for a tile with kb < r1 <= L0 + n - 1, i.e.
// for a page holding a row below the live end, and is clamped to
// [0, n_pages); entries of other pages are never read. Table rows may share
// pages (read-only prefix sharing).
//
// Q, O [B,T,H,D]; D in {64,128}, G = H/Hkv in {1,2,4,8}, P in {64,128,256},
// 1 <= T <= Smax.
//
// Compiled without the packed fp32 VALU instructions (ops/build.py,
// NO_PACKED_FP32).
#include "prefill_common.h"

// Clamped id of the page under tile kb (block-uniform: a scalar load).
__device__ __forceinline__ int pfp_page(const int* __restrict__ tb, int kb,
                                        int psh, int n_pages) {
  const int id = tb[__builtin_amdgcn_readfirstlane(kb >> psh)];
  return __builtin_amdgcn_readfirstlane(min(max(id, 0), n_pages - 1));
}

// Element offset that turns logical row numbers of tile kb's page into pool
// rows: (pid * P - first logical row of the page) * row_stride.
__device__ __forceinline__ int64_t pfp_off(int pid, int kb, int psh,
                                           int64_t row_stride) {
  return (((int64_t)pid << psh) - (int64_t)((kb >> psh) << psh)) * row_stride;
}

// The tile source of pf_body: the page-id pipeline described above.
struct PfPaged {
  const bf16 *Kb, *Vb;  // pool bases, + the kv head's column after open()
  const int* tb;        // the table; this sequence's row after open()
  int psh, n_pages, max_pages;
  int64_t row_stride;
  int pid0, pid_nxt;
  // page ids of the first two tiles; the first is the one table wait
  __device__ __forceinline__ void open(int b, int64_t col, int64_t stride,
                                       int r0, int r1) {
    row_stride = stride;
    Kb += col;
    Vb += col;
    tb += (int64_t)b * max_pages;
    pid0 = pfp_page(tb, r0, psh, n_pages);
    pid_nxt = 0;
    if (r0 + PF_KEY_TILE < r1)
      pid_nxt = pfp_page(tb, r0 + PF_KEY_TILE, psh, n_pages);
  }
  // pid_nxt was loaded a tile ago: no stage waits on the table
  __device__ __forceinline__ int64_t off(int kb, bool first) const {
    return pfp_off(first ? pid0 : pid_nxt, kb, psh, row_stride);
  }
  // id of the tile after next, used behind the NEXT barrier
  __device__ __forceinline__ void prefetch(int kb, int r1) {
    if (kb < r1) pid_nxt = pfp_page(tb, kb, psh, n_pages);
  }
};

template <int D, int GSH>
__global__ __launch_bounds__(PF_THREADS, 2) void attn_prefill_ragged_paged_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, bf16* __restrict__ O, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ n_new,
    const int* __restrict__ table, int T, int H, int Hkv, int psh, int n_pages,
    int max_pages, int split_rows, float scale) {
  pf_body<D, GSH>(Q, O, ws, lens, n_new, T, H, Hkv, max_pages << psh,
                  split_rows, scale,
                  PfPaged{K, V, table, psh, n_pages, max_pages, 0, 0, 0});
}

// K, V: pools [n_pages, P, Hkv, D]; table: int32 [B, max_pages] on the device;
// Smax = max_pages * P. split_rows: a positive multiple of PF_KEY_TILE chosen
// from the launch shape only. nsplit = ceil(Smax / split_rows); with
// nsplit == 1 ws is not used, otherwise ws is fp32
// [B*Hkv * nsplit * T*(H/Hkv) * (D + 2)].
PRIME_API int prime_attn_prefill_ragged_paged(
    hipStream_t stream, const void* Q, const void* K, const void* V, void* O,
    void* ws, const void* lens, const void* n_new, const void* table,
    int64_t B, int64_t T, int64_t H, int64_t Hkv, int64_t P, int64_t n_pages,
    int64_t max_pages, int64_t D, int64_t split_rows, double scale) {
  if ((P != 64 && P != 128 && P != 256) || n_pages < 1 || max_pages < 1 ||
      max_pages > 0x7fffffff / P || n_pages > 0x7fffffff / P || !table)
    return hipErrorInvalidValue;
  const int64_t Smax = max_pages * P;
  if (pf_check_args(B, T, H, Hkv, Smax, D, split_rows, ws, lens, n_new))
    return hipErrorInvalidValue;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  const int psh = P == 64 ? 6 : (P == 128 ? 7 : 8);
  pf_dispatch(B, T, H, Hkv, D, nsplit, [&](auto d, auto gsh, dim3 grid) {
    hipLaunchKernelGGL((attn_prefill_ragged_paged_kernel<d(), gsh()>), grid,
                       dim3(PF_THREADS), 0, stream, (const bf16*)Q,
                       (const bf16*)K, (const bf16*)V, (bf16*)O, (float*)ws,
                       (const int*)lens, (const int*)n_new, (const int*)table,
                       (int)T, (int)H, (int)Hkv, psh, (int)n_pages,
                       (int)max_pages, (int)split_rows, (float)scale);
  });
  return pf_launch_merge(stream, ws, O, lens, n_new, B, T, H, Hkv, D, Smax,
                         nsplit);
}
