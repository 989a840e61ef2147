// Ragged single-token decode attention over a PAGED bf16 KV cache (gfx950).
//
// The cache is a pool of pages, K/V [n_pages, P, Hkv, D] (row stride Hkv*D,
// as in the contiguous cache), plus an int32 block table [B, max_pages] read
// inside the kernel: logical row r of sequence b is pool row
// table[b, r / P] * P + r % P. Smax = max_pages * P takes the place of the
// contiguous Smax everywhere (the lens clamp, the splits, the workspace).
//
// Contract, work split, chunking, the K and V phases, the summation order,
// the workspace layout and the merge are those of decode_ragged.hip: both
// kernels are dr_body of decode_ragged_common.h, so for the same rows the
// result is bit-identical. What differs is the address path, the row policy
// DrPaged below:
//
//  - A chunk is DR_CHUNK = 256 ALIGNED logical rows (r0 is a multiple of the
//    chunk) and P >= 64, so a chunk lies in at most 256 / P <= 4 pages, whose
//    ids are workgroup-uniform. They live in four scalar values (DrpPages).
//  - The ids of chunk c + 1 are fetched with wave-uniform loads at the top of
//    chunk c, before its K loads are issued, and are first used one iteration
//    later: no K or V row load sits behind a table load of its own chunk.
//    Only the first chunk of a split waits for its ids (once per workgroup).
//  - A lane picks its row's page from the four values with selects on
//    (row in chunk) >> log2(P): address = (pg * P + row % P) * row_stride.
//    The V phase keeps the VU-deep run-ahead of the contiguous kernel; its
//    row indices are known before any load, so the selects are, too.
//
// Safety: a table entry is read and used only for a page that holds a row
// below min(r1, lens[b]); such an entry is clamped to [0, n_pages), so no
// table content can move a load out of the pool. Entries of other pages are
// never read. Two table rows may name the same page (read-only sharing).
//
// Q [B,H,D], O [B,H,D], ws fp32 [B*Hkv, nsplit, G*(D+2)]. D in {64,128},
// G in {1,2,4,8}, P in {64,128,256}.
//
// Compiled without the packed fp32 VALU instructions (ops/build.py,
// NO_PACKED_FP32).
#include "decode_ragged_common.h"

// The ids of the (at most four) pages under a chunk. Four named scalars, not
// an array: the values stay in scalar registers and a lane's pick is a chain
// of selects, never an indexed stack object.
struct DrpPages {
  int p0, p1, p2, p3;
};

// The (clamped) ids of the pages under chunk [c0, c0 + cn), cn >= 1: entry j
// is read iff page j of the chunk holds a live row. tb is workgroup-uniform,
// so these are scalar loads.
__device__ __forceinline__ int drp_id(const int* __restrict__ tb, int idx,
                                      bool used, int n_pages) {
  int id = 0;
  if (used) id = tb[idx];
  return __builtin_amdgcn_readfirstlane(min(max(id, 0), n_pages - 1));
}

__device__ __forceinline__ DrpPages drp_fetch(const int* __restrict__ tb,
                                              int c0, int cn, int psh,
                                              int n_pages) {
  const int i0 = c0 >> psh;
  DrpPages pg;
  pg.p0 = drp_id(tb, i0, true, n_pages);
  pg.p1 = drp_id(tb, i0 + 1, (1 << psh) < cn, n_pages);
  pg.p2 = drp_id(tb, i0 + 2, (2 << psh) < cn, n_pages);
  pg.p3 = drp_id(tb, i0 + 3, (3 << psh) < cn, n_pages);
  return pg;
}

// Pool row of row `rc` (0..255) of the chunk whose page ids are pg.
// (n_pages * P fits an int: checked at the entry point.)
__device__ __forceinline__ int drp_row(DrpPages pg, int rc, int psh) {
  const int j = rc >> psh;
  int id = pg.p0;
  if (j == 1) id = pg.p1;
  if (j == 2) id = pg.p2;
  if (j == 3) id = pg.p3;
  return (id << psh) + (rc & ((1 << psh) - 1));
}

// The row policy of dr_body: owns the page ids of the chunk being computed
// (pg) and of the next one (pgn).
struct DrPaged {
  const bf16 *Kb, *Vb;  // pool bases, + the kv head's column after open()
  const int* tb;        // the table; this sequence's row after open()
  int psh, n_pages, max_pages;
  int64_t row_stride;
  DrpPages pg, pgn;
  // ids of the first chunk: the one table wait of the workgroup, overlapped
  // with the q load
  __device__ __forceinline__ void open(int b, int64_t col, int64_t stride,
                                       int r0, int r1) {
    row_stride = stride;
    Kb += col;
    Vb += col;
    tb += (int64_t)b * max_pages;
    pg = drp_fetch(tb, r0, min(DR_CHUNK, r1 - r0), psh, n_pages);
  }
  // page ids of the NEXT chunk, issued before this chunk's loads and first
  // used an iteration later
  __device__ __forceinline__ void begin_chunk(int c0, int r1) {
    pgn = pg;
    if (c0 + DR_CHUNK < r1)
      pgn = drp_fetch(tb, c0 + DR_CHUNK, min(DR_CHUNK, r1 - c0 - DR_CHUNK),
                      psh, n_pages);
  }
  __device__ __forceinline__ int64_t off(int rc) const {
    return drp_row(pg, rc, psh) * row_stride;
  }
  __device__ __forceinline__ void end_chunk() { pg = pgn; }
};

template <int D, int G>
__global__ __launch_bounds__(DR_THREADS) void attn_decode_ragged_paged_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ table, int H,
    int Hkv, int psh, int n_pages, int max_pages, int split_rows,
    float scale) {
  dr_body<D, G>(Q, ws, lens, H, Hkv, max_pages << psh, split_rows, scale,
                DrPaged{K, V, table, psh, n_pages, max_pages, 0, {}, {}});
}

// K, V: pools [n_pages, P, Hkv, D]; table: int32 [B, max_pages] on the device.
// ws, split_rows: see dr_check_args, with Smax = max_pages * P.
PRIME_API int prime_attn_decode_ragged_paged(
    hipStream_t stream, const void* Q, const void* K, const void* V, void* O,
    void* ws, const void* lens, const void* table, int64_t B, int64_t H,
    int64_t Hkv, int64_t P, int64_t n_pages, int64_t max_pages, int64_t D,
    int64_t split_rows, double scale) {
  if ((P != 64 && P != 128 && P != 256) || n_pages < 1 || max_pages < 1 ||
      n_pages * P > 0x7fffffff || !table ||
      dr_check_args(B, H, Hkv, max_pages * P, D, split_rows, ws, lens))
    return hipErrorInvalidValue;
  const int64_t nsplit = (max_pages * P + split_rows - 1) / split_rows;
  const int psh = P == 64 ? 6 : (P == 128 ? 7 : 8);
  dr_dispatch(D, H / Hkv, [&](auto d, auto g) {
    hipLaunchKernelGGL((attn_decode_ragged_paged_kernel<d(), g()>),
                       dim3((int)(B * Hkv), (int)nsplit), dim3(DR_THREADS), 0,
                       stream, (const bf16*)Q, (const bf16*)K, (const bf16*)V,
                       (float*)ws, (const int*)lens, (const int*)table, (int)H,
                       (int)Hkv, psh, (int)n_pages, (int)max_pages,
                       (int)split_rows, (float)scale);
  });
  return dr_launch_merge(stream, ws, O, B, H, Hkv, D, nsplit);
}
