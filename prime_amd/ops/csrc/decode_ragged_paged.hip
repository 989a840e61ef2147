// Ragged single-token decode attention over a PAGED bf16 KV cache (gfx950).
//
// The cache is a pool of pages, K/V [n_pages, P, Hkv, D] (row stride Hkv*D,
// as in the contiguous cache), plus an int32 block table [B, max_pages] read
// inside the kernel: logical row r of sequence b is pool row
// table[b, r / P] * P + r % P. Smax = max_pages * P takes the place of the
// contiguous Smax everywhere (the lens clamp, the splits, the workspace).
//
// Contract, work split, chunking, the K and V phases, the summation order,
// the workspace layout and the merge are those of decode_ragged.hip; for the
// same rows the result is bit-identical. What differs is the address path:
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
#include "common.h"

#define DR_CHUNK 256    // keys per online-softmax chunk (= block size)
#define DR_THREADS 256

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

template <int D, int G>
__global__ __launch_bounds__(DR_THREADS) void attn_decode_ragged_paged_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, float* __restrict__ ws,
    const int* __restrict__ lens, const int* __restrict__ table, int H,
    int Hkv, int psh, int n_pages, int max_pages, int split_rows,
    float scale) {
  constexpr int PART = G * (D + 2);  // floats per (b, kv head, split)
  constexpr int LPR = D / 4;         // lanes per V row (8 B each)
  constexpr int RG = DR_THREADS / LPR;  // V rows in flight
  constexpr int NW = DR_THREADS / 64;
  constexpr int KU = G >= 8 ? 2 : (G >= 4 ? 4 : D / 8);
  constexpr int VU = G >= 4 ? 4 : 8;  // V row steps in flight per thread
  const int bk = blockIdx.x;
  const int b = bk / Hkv, hkv = bk - b * Hkv;
  const int sp = blockIdx.y, nsplit = gridDim.y;
  const int t = threadIdx.x;
  const int lane = t & 63, wid = t >> 6;
  const int Smax = max_pages << psh;
  const int L = min(max(lens[b], 0), Smax);
  const int r0 = sp * split_rows;
  const int r1 = min(r0 + split_rows, L);
  float* wsp = ws + ((int64_t)bk * nsplit + sp) * PART;

  if (r0 >= r1) {  // block-uniform: empty split (or idle slot)
    for (int i = t; i < PART; i += DR_THREADS)
      wsp[i] = (i >= G * D && i < G * D + G) ? -1e30f : 0.f;
    return;
  }

  __shared__ float q_lds[G * D];
  __shared__ float p_lds[G][DR_CHUNK];
  __shared__ float red_m[NW][G];
  __shared__ float red_s[NW][G];
  __shared__ __attribute__((aligned(16))) float part[RG * D];

  const int64_t row_stride = (int64_t)Hkv * D;
  const bf16* qp = Q + ((int64_t)b * H + (int64_t)hkv * G) * D;
  const bf16* Kb = K + (int64_t)hkv * D;
  const bf16* Vb = V + (int64_t)hkv * D;
  const int* tb = table + (int64_t)b * max_pages;

  // ids of the first chunk: the one table wait of the workgroup, overlapped
  // with the q load
  DrpPages pg = drp_fetch(tb, r0, min(DR_CHUNK, r1 - r0), psh, n_pages);

  for (int i = t; i < G * D; i += DR_THREADS) q_lds[i] = bf2f(qp[i]);
  __syncthreads();

  float m[G], lsum[G], acc[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -1e30f;
    lsum[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[g][j] = 0.f;
  }
  const int vr = t / LPR, vd = (t - vr * LPR) * 4;

  for (int c0 = r0; c0 < r1; c0 += DR_CHUNK) {
    const int cn = min(DR_CHUNK, r1 - c0);
    // ---- page ids of the NEXT chunk, issued before this chunk's loads and
    // first used an iteration later
    DrpPages pgn = pg;
    if (c0 + DR_CHUNK < r1)
      pgn = drp_fetch(tb, c0 + DR_CHUNK, min(DR_CHUNK, r1 - c0 - DR_CHUNK),
                      psh, n_pages);
    // ---- scores: key c0 + t against the G queries
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = -1e30f;
    if (t < cn) {
      const bf16x8* kr = reinterpret_cast<const bf16x8*>(
          Kb + drp_row(pg, t, psh) * row_stride);
      float dot[G];
#pragma unroll
      for (int g = 0; g < G; ++g) dot[g] = 0.f;
#pragma unroll KU
      for (int j = 0; j < D / 8; ++j) {
        const bf16x8 kv8 = kr[j];
        float kf[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) kf[u] = bf2f(kv8.v[u]);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int u = 0; u < 8; ++u) dot[g] += q_lds[g * D + j * 8 + u] * kf[u];
      }
#pragma unroll
      for (int g = 0; g < G; ++g) s[g] = dot[g] * scale;
    }
    // ---- chunk max of each head (all lanes get the wave result)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float x = s[g];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
      if (lane == 0) red_m[wid][g] = x;
    }
    __syncthreads();
    float alpha[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mx = red_m[0][g];
#pragma unroll
      for (int w = 1; w < NW; ++w) mx = fmaxf(mx, red_m[w][g]);
      const float mnew = fmaxf(m[g], mx);
      alpha[g] = __expf(m[g] - mnew);
      m[g] = mnew;
      const float p = (t < cn) ? __expf(s[g] - mnew) : 0.f;
      p_lds[g][t] = p;
      float x = p;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
      if (lane == 0) red_s[wid][g] = x;
    }
    __syncthreads();  // p_lds and red_s ready
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float ps = red_s[0][g];
#pragma unroll
      for (int w = 1; w < NW; ++w) ps += red_s[w][g];
      lsum[g] = lsum[g] * alpha[g] + ps;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[g][j] *= alpha[g];
    }
    // ---- V rows, coalesced, VU steps of loads issued before their FMAs. A
    // step past the chunk re-reads the chunk's last live row with weight 0
    // (a row of a used page), so no row at or beyond the length is touched.
    for (int l0 = vr; l0 < cn; l0 += RG * VU) {
      bf16x4 v4[VU];
#pragma unroll
      for (int k = 0; k < VU; ++k) {
        const int lc = min(l0 + k * RG, cn - 1);
        v4[k] = *reinterpret_cast<const bf16x4*>(
            Vb + drp_row(pg, lc, psh) * row_stride + vd);
      }
#pragma unroll
      for (int k = 0; k < VU; ++k) {
        const int l = l0 + k * RG;
        const int lc = min(l, cn - 1);
        float vf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) vf[j] = bf2f(v4[k].v[j]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float p = (l < cn) ? p_lds[g][lc] : 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[g][j] += p * vf[j];
        }
      }
    }
    pg = pgn;
    __syncthreads();  // p_lds / red_* reused by the next chunk
  }

  // ---- combine the RG row groups in a fixed order, one head at a time
#pragma unroll
  for (int g = 0; g < G; ++g) {
    f32x4v a;
#pragma unroll
    for (int j = 0; j < 4; ++j) a.v[j] = acc[g][j];
    *reinterpret_cast<f32x4v*>(&part[vr * D + vd]) = a;
    __syncthreads();
    if (t < D) {
      float o = part[t];
#pragma unroll
      for (int r = 1; r < RG; ++r) o += part[r * D + t];
      wsp[g * D + t] = o;
    }
    if (t == 0) {
      wsp[G * D + g] = m[g];
      wsp[G * D + G + g] = lsum[g];
    }
    __syncthreads();
  }
}

// The merge of decode_ragged.hip (the library is one non-RDC compile per
// file, so this file carries its own copy): splits in index order.
static __global__ void attn_decode_paged_merge_kernel(
    const float* __restrict__ ws, bf16* __restrict__ O, int H, int Hkv, int D,
    int nsplit) {
  const int bh = blockIdx.x;
  const int b = bh / H, h = bh - b * H;
  const int G = H / Hkv;
  const int hkv = h / G, g = h - hkv * G;
  const int d = threadIdx.x;
  const int part = G * (D + 2);
  const float* base = ws + ((int64_t)b * Hkv + hkv) * nsplit * part;
  float M = -1e30f;
  for (int s = 0; s < nsplit; ++s)
    M = fmaxf(M, base[(int64_t)s * part + G * D + g]);
  float num = 0.f, den = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* ps = base + (int64_t)s * part;
    const float w = __expf(ps[G * D + g] - M);
    den += w * ps[G * D + G + g];
    num += w * ps[g * D + d];
  }
  // every split empty (idle slot): num = den = 0 -> exactly zero
  O[((int64_t)b * H + h) * D + d] = f2bf(num / fmaxf(den, 1e-30f));
}

struct DrpArgs {
  hipStream_t stream;
  const void *Q, *K, *V, *lens, *table;
  void* ws;
  int B, H, Hkv, psh, n_pages, max_pages, split_rows, nsplit;
  float scale;
};

template <int D, int G>
static void drp_launch(const DrpArgs& a) {
  hipLaunchKernelGGL((attn_decode_ragged_paged_kernel<D, G>),
                     dim3(a.B * a.Hkv, a.nsplit), dim3(DR_THREADS), 0,
                     a.stream, (const bf16*)a.Q, (const bf16*)a.K,
                     (const bf16*)a.V, (float*)a.ws, (const int*)a.lens,
                     (const int*)a.table, a.H, a.Hkv, a.psh, a.n_pages,
                     a.max_pages, a.split_rows, a.scale);
}

template <int D>
static int drp_launch_g(int G, const DrpArgs& a) {
  switch (G) {
    case 1: drp_launch<D, 1>(a); break;
    case 2: drp_launch<D, 2>(a); break;
    case 4: drp_launch<D, 4>(a); break;
    case 8: drp_launch<D, 8>(a); break;
    default: return hipErrorInvalidValue;
  }
  return hipSuccess;
}

// K, V: pools [n_pages, P, Hkv, D]; table: int32 [B, max_pages] on the device.
// ws: fp32 [B*Hkv, ceil(Smax/split_rows), (H/Hkv)*(D+2)] with Smax =
// max_pages * P. split_rows: a positive multiple of DR_CHUNK chosen from the
// launch shape only.
PRIME_API int prime_attn_decode_ragged_paged(
    hipStream_t stream, const void* Q, const void* K, const void* V, void* O,
    void* ws, const void* lens, const void* table, int64_t B, int64_t H,
    int64_t Hkv, int64_t P, int64_t n_pages, int64_t max_pages, int64_t D,
    int64_t split_rows, double scale) {
  if ((D != 64 && D != 128) || (P != 64 && P != 128 && P != 256) || B < 1 ||
      H < 1 || Hkv < 1 || n_pages < 1 || max_pages < 1 || H % Hkv != 0 ||
      split_rows < DR_CHUNK || split_rows % DR_CHUNK != 0 || !ws || !lens ||
      !table)
    return hipErrorInvalidValue;
  const int64_t G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return hipErrorInvalidValue;
  const int64_t Smax = max_pages * P;
  const int64_t nsplit = (Smax + split_rows - 1) / split_rows;
  if (nsplit > 65535 || B * Hkv > 0x7fffffff || B * H > 0x7fffffff ||
      Smax > 0x7fffffff - split_rows || n_pages * P > 0x7fffffff)
    return hipErrorInvalidValue;
  const DrpArgs a{stream, Q, K, V, lens, table, ws, (int)B, (int)H, (int)Hkv,
                  P == 64 ? 6 : (P == 128 ? 7 : 8), (int)n_pages,
                  (int)max_pages, (int)split_rows, (int)nsplit, (float)scale};
  const int rc = D == 128 ? drp_launch_g<128>((int)G, a)
                          : drp_launch_g<64>((int)G, a);
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(attn_decode_paged_merge_kernel, dim3((int)(B * H)),
                     dim3((int)D), 0, stream, (const float*)ws, (bf16*)O,
                     (int)H, (int)Hkv, (int)D, (int)nsplit);
  return (int)hipGetLastError();
}
