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
// read, the swizzles, the double-buffered LDS-DMA stage, split + merge);
// for the same rows the result is bit-identical. The address path:
//
//  - P is a multiple of the key tile and tiles are aligned, so a staged tile
//    lies in ONE page: the stage takes one block-uniform page base per tile.
//    "Rows past `last` re-read row `last`" is unchanged: last >= the tile's
//    first row, so it is in the tile's page.
//  - Page ids are a two-deep scalar pipeline: pid_cur (tile being computed),
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

// Stage keys [kb, kb + 64) into `tile` from `gpage`, the address logical row
// 0 WOULD have if the tile's page were laid out at its logical position (page
// base minus the page's first logical row): rows past `last` re-read row
// `last`; every row read is in [kb, max(kb, last)], inside the page. The
// image swizzle is applied through the source address, as in pf_stage.
template <int D, bool VTILE>
__device__ __forceinline__ void pfp_stage(const bf16* __restrict__ gpage,
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
        gpage + (int64_t)min(kb + row, last) * row_stride + colb / 2;
    lds_char* dst = (lds_char*)tile + i * (PF_THREADS * 16) + (tid >> 6) * 1024;
    __builtin_amdgcn_global_load_lds((g_void*)src, (lds_void*)dst, 16, 0, 0);
  }
}

// s_waitcnt vmcnt(0): this wave's loads, LDS-DMA included, have landed
__device__ __forceinline__ void pfp_wait_loads() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

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

template <int D, int GSH>
__global__ __launch_bounds__(PF_THREADS, 2) void attn_prefill_ragged_paged_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, bf16* __restrict__ O, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ n_new,
    const int* __restrict__ table, int T, int H, int Hkv, int psh, int n_pages,
    int max_pages, int split_rows, float scale) {
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
  const int Smax = max_pages << psh;
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
  const bf16* Kb = K + (int64_t)hkv * D;
  const bf16* Vb = V + (int64_t)hkv * D;
  const int* tb = table + (int64_t)b * max_pages;
  const int last = r1 - 1;  // tile loads past the range re-read this row

  // page ids of the first two tiles; the first is the one table wait
  const int pid0 = pfp_page(tb, r0, psh, n_pages);
  int pid_nxt = 0;
  if (r0 + PF_KEY_TILE < r1)
    pid_nxt = pfp_page(tb, r0 + PF_KEY_TILE, psh, n_pages);

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
    const int64_t off = pfp_off(pid0, r0, psh, row_stride);
    pfp_stage<D, false>(Kb + off, row_stride, r0, last, k_lds[0], tid);
    pfp_stage<D, true>(Vb + off, row_stride, r0, last, v_lds[0], tid);
  }
  for (int kb = r0, it = 0; kb < r1; kb += PF_KEY_TILE, ++it) {
    const int buf = it & 1;
    // tile boundary, reached by every wave on every path: this wave's share
    // of tile `it` has landed; behind the barrier everyone's has, and tile
    // it - 1 is consumed
    pfp_wait_loads();
    __syncthreads();
    if (kb + PF_KEY_TILE < r1) {
      // pid_nxt was loaded a tile ago: nothing here waits on the table
      const int64_t off = pfp_off(pid_nxt, kb + PF_KEY_TILE, psh, row_stride);
      pfp_stage<D, false>(Kb + off, row_stride, kb + PF_KEY_TILE, last,
                          k_lds[buf ^ 1], tid);
      pfp_stage<D, true>(Vb + off, row_stride, kb + PF_KEY_TILE, last,
                         v_lds[buf ^ 1], tid);
    }
    // id of the tile after next, used behind the NEXT barrier
    if (kb + 2 * PF_KEY_TILE < r1)
      pid_nxt = pfp_page(tb, kb + 2 * PF_KEY_TILE, psh, n_pages);
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

struct PfpArgs {
  hipStream_t stream;
  dim3 grid;
  const void *Q, *K, *V, *lens, *n_new, *table;
  void *O, *ws;
  int T, H, Hkv, psh, n_pages, max_pages, split_rows;
  float scale;
};

template <int D, int GSH>
static void pfp_launch(const PfpArgs& a) {
  hipLaunchKernelGGL((attn_prefill_ragged_paged_kernel<D, GSH>), a.grid,
                     dim3(PF_THREADS), 0, a.stream, (const bf16*)a.Q,
                     (const bf16*)a.K, (const bf16*)a.V, (bf16*)a.O,
                     (float*)a.ws, (const int*)a.lens, (const int*)a.n_new,
                     (const int*)a.table, a.T, a.H, a.Hkv, a.psh, a.n_pages,
                     a.max_pages, a.split_rows, a.scale);
}

template <int D>
static void pfp_launch_g(int gsh, const PfpArgs& a) {
  switch (gsh) {
    case 0: pfp_launch<D, 0>(a); break;
    case 1: pfp_launch<D, 1>(a); break;
    case 2: pfp_launch<D, 2>(a); break;
    default: pfp_launch<D, 3>(a); break;
  }
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
  const int64_t G = H / Hkv;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  const int64_t nqt = (T * G + PF_Q_ROWS - 1) / PF_Q_ROWS;
  const int gsh = G == 1 ? 0 : (G == 2 ? 1 : (G == 4 ? 2 : 3));
  const PfpArgs a{stream,
                  dim3((unsigned)nqt, (unsigned)(B * Hkv), (unsigned)nsplit),
                  Q, K, V, lens, n_new, table, O, ws, (int)T, (int)H, (int)Hkv,
                  P == 64 ? 6 : (P == 128 ? 7 : 8), (int)n_pages,
                  (int)max_pages, (int)split_rows, (float)scale};
  if (D == 128)
    pfp_launch_g<128>(gsh, a);
  else
    pfp_launch_g<64>(gsh, a);
  if (nsplit > 1)
    hipLaunchKernelGGL(attn_prefill_merge_kernel, dim3((unsigned)(B * T * H)),
                       dim3((unsigned)D), 0, stream, (const float*)ws, (bf16*)O,
                       (const int*)lens, (const int*)n_new, (int)B, (int)T,
                       (int)H, (int)Hkv, (int)D, (int)Smax, (int)nsplit);
  return (int)hipGetLastError();
}
