// Flash attention (causal/non-causal, GQA) for gfx950 — MFMA
// v_mfma_f32_16x16x32_bf16 tiles, online softmax, FA2-style split backward
// (dQ q-outer; dK/dV kv-outer with a grid-split q loop + fp32 partial
// workspaces). A 32x32 swapped-operand forward (flash_fwd32_kernel) is
// kept behind PRIME_ATTN_V4=1 — measured occupancy-bound (see profiles).
//
// Design (profiled v1 at ~70 TF: redundant per-wave global reads and
// unswizzled LDS dominated; measured after fixes: fwd ~240 TF / bwd ~168
// TF at the 10B shape):
//  - K/V(+transposed) tiles are staged COOPERATIVELY once per block with
//    __builtin_amdgcn_global_load_lds width-16 (no VGPR round trip), with
//    the T2 XOR-16B swizzle applied via the pre-swizzled SOURCE address
//    (global_load_lds writes linearly: guide §5.5 T2 + rule 21).
//  - all operand-fragment LDS reads are ld8 (16 B) at the swizzled address:
//    2-way bank aliasing max (free on CDNA4).
//  - per-wave P / dS buffers are swizzled the same way (v1 left a 16-way
//    conflict on the PV A-fragment reads).
//  - kernels are STRIDE-AWARE over [B,S,H,D] inputs: q/k/v are consumed
//    directly as views into the packed qkv GEMM output, no transposes or
//    .contiguous() copies (v1 spent 8% of step time in copyBuffer).
//  - lse/delta layout [B,S,H] (contiguous with the row order of bshd).
//
// Fragment maps for mfma_f32_16x16x32_bf16 (HW-verified by
// tests/test_ops_gpu.py::test_mfma_layout_vs_matmul, asymmetric inputs):
//   A[16][32]: lane l holds A[l%16][(l/16)*8 + j]          j = 0..7
//   B[32][16]: lane l holds B[(l/16)*8 + j][l%16]
//   C[16][16]: lane l holds C[(l/16)*4 + r][l%16]          r = 0..3
//
// Workgroup = 4 waves; each wave owns 16 q-rows (fwd/dQ) or 16 k-rows
// (dK/dV); tile = 64 x 64. S % 64 == 0 (checked host-side), D in {64,128}.
#include "common.h"
#include <stdlib.h>

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void g_void;

__device__ __forceinline__ short8 ld8(const bf16* p) {
  return *reinterpret_cast<const short8*>(p);
}

__device__ __forceinline__ f32x4 mfma16(short8 a, short8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float grp16_max(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}
__device__ __forceinline__ float grp16_sum(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off, 64);
  return x;
}

#define NEG_INF (-1e30f)

#ifndef PRIME_FWD_SETPRIO
#define PRIME_FWD_SETPRIO 0
#endif
#if PRIME_FWD_SETPRIO
#define FWD_PRIO(x) __builtin_amdgcn_s_setprio(x)
#else
#define FWD_PRIO(x)
#endif

// ---- swizzled-tile helpers --------------------------------------------
// A [ROWS][COLS] bf16 tile lives linearly in LDS; byte (row, colb) is
// stored at row*COLS*2 + (colb ^ ((row&7)<<4)). Stage from a strided
// global matrix; read 8-element fragments at the same swizzle.

template <int ROWS, int COLS, int NT = 256>
__device__ __forceinline__ void stage_tile(const bf16* __restrict__ gbase,
                                           int64_t row_stride, bf16* lds_tile,
                                           int tid) {
  constexpr int UNITS = ROWS * COLS / 8;  // 16 B units
  constexpr int UPR = COLS / 8;           // units per row
  static_assert(UNITS % NT == 0, "tile not divisible by block lanes");
#pragma unroll
  for (int i = 0; i < UNITS / NT; ++i) {
    const int u = i * NT + tid;
    const int row = u / UPR;
    const int colb = ((u % UPR) * 16) ^ ((row & 7) << 4);  // pre-swizzle src
    const bf16* src = gbase + (int64_t)row * row_stride + colb / 2;
    // linear dest: wave-uniform base + lane*16 (global_load_lds contract)
    const int wid = tid >> 6;
    lds_void* dst = (lds_void*)((lds_char*)lds_tile + i * (NT * 16) + wid * 1024);
    __builtin_amdgcn_global_load_lds((g_void*)src, dst, 16, 0, 0);
  }
}

template <int COLS>
__device__ __forceinline__ short8 ld8_swz(const bf16* lds_tile, int row,
                                          int colb) {
  return *reinterpret_cast<const short8*>(
      reinterpret_cast<const char*>(lds_tile) + row * (COLS * 2) +
      (colb ^ ((row & 7) << 4)));
}

template <int COLS>
__device__ __forceinline__ void st16_swz(bf16* lds_tile, int row, int col,
                                         bf16 v) {
  *reinterpret_cast<bf16*>(reinterpret_cast<char*>(lds_tile) + row * (COLS * 2) +
                           ((col * 2) ^ ((row & 7) << 4))) = v;
}

// wave-local fence: P/dS LDS writes must land before same-wave ld8 reads
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// ---- document mask ------------------------------------------------------
// doc_start[B][S] int32: index of the first token of the document that
// token i belongs to (0 <= doc_start[i] <= i, non-decreasing in i). Query
// i sees key j iff doc_start[i] <= j <= i. The dK/dV kernel uses the
// mirror array doc_end[B][S] (exclusive end of key j's document): query i
// sees key j iff j <= i < doc_end[j]. Every loop bound taken from either
// array goes through doc_clamp, so an out-of-contract array can give wrong
// numbers but never an out-of-range tile address.
__device__ __forceinline__ int doc_clamp(int v, int hi) {
  return v < 0 ? 0 : (v > hi ? hi : v);
}

// ---------------------------------------------------------------- forward
// Q[B,S,H,D] (strided), K[B,S,Hkv,D] (strided), Vt[B,Hkv,D,S] (contiguous)
// -> O[B,S,H,D] (contiguous), lse[B,S,H] fp32.
// DOC: document mask (see "document mask" above doc_clamp) — a separate
// instantiation; DOC=false compiles to the code it was before the mask.
template <int D, int NW, bool DOC = false>  // NW waves x 16 q-rows per block
__global__ __launch_bounds__(512) void flash_fwd_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ Vt, bf16* __restrict__ O, float* __restrict__ lse,
    int B, int H, int Hkv, int S, float scale, int causal,
    int64_t sqb, int64_t sqs, int64_t sqh,
    int64_t skb, int64_t sks, int64_t skh,
    const int* __restrict__ doc) {
  constexpr int DS = D / 32;
  constexpr int DT = D / 16;
  constexpr int QT = NW * 16;  // q rows per block
  // NW=8: one K/Vt stage feeds 2x the compute of the 4-wave version
  // (halves staging traffic, +50% waves/CU at 48 KB LDS)
  const int n_qt = S / QT;
  const int bh = blockIdx.x / n_qt;
  // longest-trip q-tiles first: causal trip count grows with qt
  const int qt = n_qt - 1 - (blockIdx.x - bh * n_qt);
  const int b = bh / H, h = bh - b * H;
  const int hkv = h / (H / Hkv);
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lg = lane >> 4, li = lane & 15;
  const int q0 = qt * QT + wid * 16;

  const bf16* Qb = Q + b * sqb + h * sqh;
  const bf16* Kb = K + b * skb + hkv * skh;
  const bf16* Vtb = Vt + ((int64_t)(b * Hkv + hkv) * D) * S;

  __shared__ bf16 k_lds[64 * D];
  __shared__ bf16 vt_lds[D * 64];
  __shared__ bf16 p_lds_all[NW][16 * 64];
  bf16* p_lds = p_lds_all[wid];

  short8 qf[DS];
#pragma unroll
  for (int ds = 0; ds < DS; ++ds)
    qf[ds] = ld8(Qb + (int64_t)(q0 + li) * sqs + ds * 32 + lg * 8);

  float m[4], l[4];
  f32x4 o_acc[DT];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = NEG_INF; l[r] = 0.f; }
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kv_end = causal ? (qt * QT + QT) : S;
  // DOC: the block's first row has its smallest doc_start, so the k/v loop
  // starts at that tile (block-uniform: all waves co-stage); a wave whose
  // own first row starts later skips the leading tiles' compute
  int kv_begin = 0, my_kv_begin = 0, row_ds[4];
  if (DOC) {
    const int* doc_b = doc + (int64_t)b * S;
    kv_begin = doc_clamp(doc_b[qt * QT], qt * QT) & ~63;
    my_kv_begin = doc_clamp(doc_b[q0], q0) & ~63;
#pragma unroll
    for (int r = 0; r < 4; ++r) row_ds[r] = doc_b[q0 + lg * 4 + r];
  }
  for (int kv = kv_begin; kv < kv_end; kv += 64) {
    __syncthreads();  // all waves done reading the previous tile
    stage_tile<64, D, NW * 64>(Kb + (int64_t)kv * sks, sks, k_lds, threadIdx.x);
    // Vt tile: rows d (stride S), cols k in [kv, kv+64)
    stage_tile<D, 64, NW * 64>(Vtb + kv, S, vt_lds, threadIdx.x);
    __syncthreads();  // staged (syncthreads drains vmcnt)
    if (DOC && kv < my_kv_begin) continue;  // before this wave's documents

    // ---- S = scale * Q K^T
    f32x4 s[4];
    FWD_PRIO(1);
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      f32x4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < DS; ++ds)
        acc = mfma16(qf[ds], ld8_swz<D>(k_lds, sub * 16 + li, ds * 64 + lg * 16), acc);
      s[sub] = acc;
    }
    FWD_PRIO(0);
    // ---- online softmax per q-row (reg r), row owned by 16-lane group
    float alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qg = q0 + lg * 4 + r;
      float tmax = NEG_INF;
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        float v = s[sub][r] * scale;
        if (causal && (kv + sub * 16 + li) > qg) v = NEG_INF;
        if (DOC && (kv + sub * 16 + li) < row_ds[r]) v = NEG_INF;
        s[sub][r] = v;
        tmax = fmaxf(tmax, v);
      }
      tmax = grp16_max(tmax);
      // defer-max (guide T13): if this tile's max does not exceed the
      // running max by more than THR, keep the old max — P values stay
      // bounded by e^THR (fp32 accumulates fine) and the O-wide rescale
      // pass is skipped (alpha == 1)
// A/B on MI355X (3x interleaved): defer-max = 230 TF vs plain 240 TF —
// our per-tile rescale is only 32 muls/lane, cheaper than the added
// branches. Off by default; kept for structures with wider O state.
#ifndef PRIME_DEFER_MAX
#define PRIME_DEFER_MAX 0
#endif
#if PRIME_DEFER_MAX
      const float THR = 8.f;
      float mnew = m[r];
      if (tmax > m[r] + 0.f) mnew = (tmax - m[r] <= THR && m[r] > NEG_INF)
                                        ? m[r] : fmaxf(m[r], tmax);
#else
      const float mnew = fmaxf(m[r], tmax);
#endif
      alpha[r] = (mnew == m[r]) ? 1.f : __expf(m[r] - mnew);
      float psum = 0.f;
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        // DOC: a row can meet a tile that lies wholly before its document
        // (m, mnew and s all NEG_INF): exp(0) = 1 there, so masked scores
        // are zeroed explicitly
        const float p = (DOC && s[sub][r] <= NEG_INF)
                            ? 0.f : __expf(s[sub][r] - mnew);
        s[sub][r] = p;
        psum += p;
      }
      l[r] = l[r] * alpha[r] + grp16_sum(psum);
      m[r] = mnew;
    }
    float amin = 1.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) amin = fminf(amin, alpha[r]);
    if (__ballot(amin < 1.f)) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o_acc[dt][r] *= alpha[r];
    }
    // ---- P (C-layout) -> swizzled per-wave LDS (A-layout source)
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        st16_swz<64>(p_lds, lg * 4 + r, sub * 16 + li, f2bf(s[sub][r]));
    wave_lds_fence();
    // ---- O += P V
    FWD_PRIO(1);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        o_acc[dt] = mfma16(ld8_swz<64>(p_lds, li, ks * 64 + lg * 16),
                           ld8_swz<64>(vt_lds, dt * 16 + li, ks * 64 + lg * 16),
                           o_acc[dt]);
    FWD_PRIO(0);
  }
  // ---- epilogue
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = (l[r] > 0.f) ? 1.f / l[r] : 0.f;
    const int qg = q0 + lg * 4 + r;
    bf16* orow = O + (((int64_t)(b * S + qg)) * H + h) * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      orow[dt * 16 + li] = f2bf(o_acc[dt][r] * inv);
    if (li == 0)
      lse[((int64_t)(b * S + qg)) * H + h] = m[r] + __logf(fmaxf(l[r], 1e-30f));
  }
}


// ------------------------------------------------- forward v5 (32x32 MFMA)
// 8-wave swapped-operand structure (guide §B attn, 8-warp 32x32 ladder):
// St = K·Q^T with v_mfma_f32_32x32x16_bf16 puts each q-row's scores
// LANE-LOCAL (lane pair (l, l^32) splits the row), so the online softmax
// is fully in-register and P feeds the PV A-fragment after one lane-pair
// exchange (v_cvt_pk_bf16_f32 pack + v_permlane32_swap_b32 — guide T12).
// 8 waves x 32 q-rows = 256-row q tiles sharing one K/Vt stage (vs the
// 16x16 kernel's per-wave P LDS bounce + 4x staging traffic). The round-1
// v4 (4-wave, shfl-based exchange, always-rescale) measured 130 TF; the
// deltas here are the rest of the technique stack: defer-max rescale
// skipping (T13), cheap P exchange, per-wave causal trip clipping, and
// setprio around the MFMA clusters (T5).
//
// 32x32x16 fragment maps (HW-verified, test_mfma32_layout_vs_matmul):
//   A[32][16]: lane holds A[lane&31][(lane>>5)*8 + j]
//   B[16][32]: lane holds B[(lane>>5)*8 + j][lane&31]
//   C[32][32]: lane holds C[(r&3) + 8*(r>>2) + 4*(lane>>5)][lane&31]
typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ f32x16 mfma32(short8 a, short8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// pack two f32 into one dword of 2 bf16 (no builtin on gfx950 — guide T12)
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo_, float hi_) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo_), "v"(hi_));
  return r;
}

// v_permlane32_swap_b32 a, b: a's lanes>=32 swap with b's lanes<32 —
// after the swap, lane l<32 sees (a_l, a_{l+32}) and lane l>=32 sees
// (b_{l-32}, b_l) in (a, b)
__device__ __forceinline__ void permlane32_swap(unsigned& a, unsigned& b) {
  asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// FLAGS bits: 1 = setprio around MFMA clusters, 2 = defer-max (THR=8),
// 4 = 3-buffer deep prefetch with counted vmcnt at the tile boundary
// (guide T4: __syncthreads' vmcnt(0) drain waits on the JUST-issued
// stage; with 2 tiles of lookahead the boundary only needs the oldest
// in-flight tile, so vmcnt(4) leaves the newest 4 loads flying)
template <int D, int FLAGS, bool DOC = false>
__global__ __launch_bounds__(512, 2) void flash_fwd_v5_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ Vt, bf16* __restrict__ O, float* __restrict__ lse,
    int B, int H, int Hkv, int S, float scale, int causal,
    int64_t sqb, int64_t sqs, int64_t sqh,
    int64_t skb, int64_t sks, int64_t skh,
    const int* __restrict__ doc) {
  constexpr int DSL = D / 16;   // 16-wide d slices for the K dim
  constexpr int DT32 = D / 32;  // 32-wide output d tiles
  const int n_qt = S / 256;
  // XCD-aware bijective remap (guide T1): consecutive qt-tiles of one
  // (b,h) land on ONE XCD's L2, which then reuses the same K/V stream
  const int nwg = gridDim.x;
  int vb = blockIdx.x;
  if ((nwg & 7) == 0) vb = (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  const int bh = vb / n_qt;
  const int qt = n_qt - 1 - (vb - bh * n_qt);  // longest trips first
  const int b = bh / H, h = bh - b * H;
  const int hkv = h / (H / Hkv);
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lo = lane & 31, hi = lane >> 5;
  const int q0w = qt * 256 + wid * 32;  // this wave's first q row

  const bf16* Qb = Q + b * sqb + h * sqh;
  const bf16* Kb = K + b * skb + hkv * skh;
  const bf16* Vtb = Vt + ((int64_t)(b * Hkv + hkv) * D) * S;

  constexpr int NBUF = (FLAGS & 4) ? 3 : 2;
  __shared__ bf16 k_lds[NBUF][64 * D];
  __shared__ bf16 vt_lds[NBUF][D * 64];
  __shared__ float bcast_all[8][32];  // per-wave alpha / inv-l broadcast
  float* bcast = bcast_all[wid];

  // Q^T B-fragments, pre-scaled: lane holds Q[q0w+lo][ds*16+hi*8+j]
  short8 qf[DSL];
#pragma unroll
  for (int ds = 0; ds < DSL; ++ds) {
    const bf16* src = Qb + (int64_t)(q0w + lo) * sqs + ds * 16 + hi * 8;
    short8 raw = ld8(src);
    short8 sc;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bf16 v = reinterpret_cast<const bf16*>(&raw)[j];
      reinterpret_cast<bf16*>(&sc)[j] = f2bf(bf2f(v) * scale);
    }
    qf[ds] = sc;
  }

  float m_run = NEG_INF, l_run = 0.f;
  f32x16 o_acc[DT32];
#pragma unroll
  for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[dt][r] = 0.f;

  const int kv_end = causal ? (qt * 256 + 256) : S;
  // per-wave causal clip: this wave's rows end at q0w+31, so tiles past
  // q0w+32 are fully masked — skip their compute (they still stage+sync)
  const int my_kv_end = causal ? (q0w + 32) : S;
  // DOC: block-uniform loop start at the tile of the block's smallest
  // doc_start (its first row's); per-wave start for the compute skip; the
  // lane's own row start for the element mask, which only tiles that
  // begin before the wave's LAST row's start (its largest) need. The
  // prologue stages and the prefetch distance are relative to kv_begin.
  int kv_begin = 0, my_kv_begin = 0, my_ds = 0, my_ds_last = 0;
  if (DOC) {
    const int* doc_b = doc + (int64_t)b * S;
    kv_begin = doc_clamp(doc_b[qt * 256], qt * 256) & ~63;
    my_kv_begin = doc_clamp(doc_b[q0w], q0w) & ~63;
    my_ds = doc_b[q0w + lo];
    my_ds_last = doc_b[q0w + 31];
  }
  stage_tile<64, D, 512>(Kb + (int64_t)kv_begin * sks, sks, k_lds[0], threadIdx.x);
  stage_tile<D, 64, 512>(Vtb + kv_begin, S, vt_lds[0], threadIdx.x);
  if (FLAGS & 4) {  // 2-deep prologue
    if (kv_begin + 64 < kv_end) {
      stage_tile<64, D, 512>(Kb + (int64_t)(kv_begin + 64) * sks, sks, k_lds[1], threadIdx.x);
      stage_tile<D, 64, 512>(Vtb + kv_begin + 64, S, vt_lds[1], threadIdx.x);
    }
  }
  int idx = 0;
  for (int kv = kv_begin, kt = 0; kv < kv_end; kv += 64, ++kt) {
    idx = kt % NBUF;
    if (FLAGS & 4) {
      // tile kv's stages are >=1 full tile old: only the newest tile's
      // 4 loads may still fly across this rendezvous
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      const int pre = kv + 2 * 64;
      if (pre < kv_end) {
        stage_tile<64, D, 512>(Kb + (int64_t)pre * sks, sks,
                               k_lds[(kt + 2) % NBUF], threadIdx.x);
        stage_tile<D, 64, 512>(Vtb + pre, S, vt_lds[(kt + 2) % NBUF],
                               threadIdx.x);
      }
    } else {
      __syncthreads();  // prev tile consumed + this tile's stage drained
      if (kv + 64 < kv_end) {
        // prefetch-behind-barrier: these loads get the whole tile's
        // compute to land (the next syncthreads drains them)
        stage_tile<64, D, 512>(Kb + (int64_t)(kv + 64) * sks, sks,
                               k_lds[(kt + 1) % NBUF], threadIdx.x);
        stage_tile<D, 64, 512>(Vtb + kv + 64, S, vt_lds[(kt + 1) % NBUF],
                               threadIdx.x);
      }
    }
    if (kv >= my_kv_end) continue;  // fully-masked tile for this wave
    if (DOC && kv < my_kv_begin) continue;  // before this wave's documents

    // ---- St = (K q^T): two 32x32 C tiles over the 64-key block
    f32x16 st[2];
    if (FLAGS & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[t][r] = 0.f;
#pragma unroll
      for (int ds = 0; ds < DSL; ++ds) {
        const short8 kf = ld8_swz<D>(k_lds[idx], t * 32 + lo, ds * 32 + hi * 16);
        st[t] = mfma32(kf, qf[ds], st[t]);
      }
    }
    if (FLAGS & 1) __builtin_amdgcn_s_setprio(0);
    // ---- online softmax: st[t][r] is k = kv + t*32 + crow(r,hi) for
    // q row q0w+lo; lane pair (l, l^32) splits the row's 64 scores
    float tmax = NEG_INF;
    if (DOC && kv < my_ds_last) {  // wave-uniform: a boundary tile
      // a row still wholly masked keeps m_run = NEG_INF through the
      // per-wave rescale below (alpha = exp(0) = 1 on o = l = 0) and
      // p = 0 through the <= NEG_INF guard, so nothing leaks
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kg = kv + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (kg < my_ds) st[t][r] = NEG_INF;
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kg = kv + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (causal && kg > q0w + lo) st[t][r] = NEG_INF;
        tmax = fmaxf(tmax, st[t][r]);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    // defer-max (guide T13): skip the O-wide rescale while the running
    // max still bounds P by e^THR (fp32 accumulation tolerates it)
    const float thr = (FLAGS & 2) ? 8.f : 0.f;
    float alpha = 1.f;
    if (__ballot(tmax > m_run + thr)) {
      const float mnew = fmaxf(m_run, tmax);
      alpha = __expf(m_run - mnew);  // 1 for rows that did not grow
      m_run = mnew;
      if (hi == 0) bcast[lo] = alpha;
      wave_lds_fence();
#pragma unroll
      for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          o_acc[dt][r] *= bcast[(r & 3) + 8 * (r >> 2) + 4 * hi];
    }
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = (st[t][r] <= NEG_INF) ? 0.f : __expf(st[t][r] - m_run);
        st[t][r] = pv;
        psum += pv;
      }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;

    // ---- P -> PV A-fragments (guide T12): per 16-k slice, pack the two
    // 4-value r-groups to bf16 dwords and permlane32_swap — lane l<32
    // keeps x and receives partner's x; lane>=32 receives partner's y and
    // keeps y. Result is branch-free and identical on both halves.
    short8 pa[2 * 2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int kst = 0; kst < 2; ++kst) {
        const int g0 = 4 * (2 * kst), g1 = 4 * (2 * kst + 1);
        unsigned x0 = cvt_pk_bf16(st[t][g0 + 0], st[t][g0 + 1]);
        unsigned x1 = cvt_pk_bf16(st[t][g0 + 2], st[t][g0 + 3]);
        unsigned y0 = cvt_pk_bf16(st[t][g1 + 0], st[t][g1 + 1]);
        unsigned y1 = cvt_pk_bf16(st[t][g1 + 2], st[t][g1 + 3]);
        permlane32_swap(x0, y0);
        permlane32_swap(x1, y1);
        short8 frag;
        reinterpret_cast<unsigned*>(&frag)[0] = x0;
        reinterpret_cast<unsigned*>(&frag)[1] = x1;
        reinterpret_cast<unsigned*>(&frag)[2] = y0;
        reinterpret_cast<unsigned*>(&frag)[3] = y1;
        pa[t * 2 + kst] = frag;
      }
    }
    // ---- O += P V  (B-frags from swizzled Vt LDS)
    if (FLAGS & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        o_acc[dt] = mfma32(pa[ks],
                           ld8_swz<64>(vt_lds[idx], dt * 32 + lo, ks * 32 + hi * 16),
                           o_acc[dt]);
    if (FLAGS & 1) __builtin_amdgcn_s_setprio(0);
  }
  // ---- epilogue: O /= l (per-row broadcast), write + lse
  if (hi == 0) bcast[lo] = (l_run > 0.f) ? 1.f / l_run : 0.f;
  wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float inv = bcast[qr];
    bf16* orow = O + (((int64_t)(b * S + q0w + qr)) * H + h) * D;
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
      orow[dt * 32 + lo] = f2bf(o_acc[dt][r] * inv);
  }
  if (hi == 0)
    lse[((int64_t)(b * S + q0w + lo)) * H + h] = m_run + __logf(fmaxf(l_run, 1e-30f));
}

// ------------------------------------------------------- delta = rowsum(dO*O)
// dO, O: contiguous [B,S,H,D] -> delta [B,S,H] (row-ordered, contiguous)
// rowc_t (nullable): also writes lse and delta in [B,H,S] order, as
// rowc_t[0] = lse^T and rowc_t[1] = delta^T, for the dK/dV kernel, whose
// lanes then read four consecutive queries of one head as one 16-byte load.
__global__ void attn_delta_kernel(const bf16* __restrict__ dO,
                                  const bf16* __restrict__ O,
                                  float* __restrict__ delta, int64_t rows,
                                  int D, const float* __restrict__ lse,
                                  float* __restrict__ rowc_t, int S, int H) {
  const int64_t row0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  for (int64_t r = row0; r < rows; r += (int64_t)gridDim.x * (blockDim.x >> 6)) {
    float acc = 0.f;
    for (int i = lane * 2; i < D; i += 128) {
      acc += bf2f(dO[r * D + i]) * bf2f(O[r * D + i]);
      acc += bf2f(dO[r * D + i + 1]) * bf2f(O[r * D + i + 1]);
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) {
      delta[r] = acc;
      if (rowc_t) {
        const int64_t bs = r / H;  // r = (b*S + s)*H + h
        const int h = (int)(r - bs * H);
        const int64_t bb = bs / S;
        const int s = (int)(bs - bb * S);
        const int64_t t = (bb * H + h) * S + s;
        rowc_t[t] = lse[r];
        rowc_t[rows + t] = acc;
      }
    }
  }
}

// ------------------------------------------------ backward dQ v5 (32x32)
// Same 8-wave swapped-operand structure as the v5 forward: St = K·Q^T and
// dPt = V·dO^T give lane-local q-rows (q = lane&31), so lse/delta are one
// scalar per lane and dS never touches LDS — it is packed straight into
// the dQ-accumulation A-fragments with cvt_pk + permlane32_swap.
template <int D, int FLAGS, bool DOC = false>
__global__ __launch_bounds__(512, 2) void flash_bwd_dq_v5_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ Kt,
    const bf16* __restrict__ dO, const float* __restrict__ lse,
    const float* __restrict__ delta, bf16* __restrict__ dQ, int B, int H,
    int Hkv, int S, float scale, int causal,
    int64_t sqb, int64_t sqs, int64_t sqh,
    int64_t skb, int64_t sks, int64_t skh,
    int64_t svb, int64_t svs, int64_t svh,
    const int* __restrict__ doc) {
  constexpr int DSL = D / 16;
  constexpr int DT32 = D / 32;
  const int n_qt = S / 256;
  const int nwg = gridDim.x;
  int vb = blockIdx.x;
  if ((nwg & 7) == 0) vb = (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  const int bh = vb / n_qt;
  const int qt = n_qt - 1 - (vb - bh * n_qt);
  const int b = bh / H, h = bh - b * H;
  const int hkv = h / (H / Hkv);
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lo = lane & 31, hi = lane >> 5;
  const int q0w = qt * 256 + wid * 32;

  const bf16* Qb = Q + b * sqb + h * sqh;
  const bf16* Kb = K + b * skb + hkv * skh;
  const bf16* Vb = V + b * svb + hkv * svh;
  const bf16* Ktb = Kt + ((int64_t)(b * Hkv + hkv) * D) * S;
  const bf16* dOb = dO + ((int64_t)b * S * H + h) * D;  // row stride H*D
  const float* lse_b = lse + (int64_t)b * S * H + h;    // stride H
  const float* dl_b = delta + (int64_t)b * S * H + h;

  __shared__ bf16 k_lds[2][64 * D];
  __shared__ bf16 v_lds[2][64 * D];
  __shared__ bf16 kt_lds[2][D * 64];

  // Q^T / dO^T B-fragments for this wave's 32 q rows (q = lo)
  short8 qf[DSL], dof[DSL];
#pragma unroll
  for (int ds = 0; ds < DSL; ++ds) {
    const bf16* src = Qb + (int64_t)(q0w + lo) * sqs + ds * 16 + hi * 8;
    short8 raw = ld8(src);
    short8 sc;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bf16 v = reinterpret_cast<const bf16*>(&raw)[j];
      reinterpret_cast<bf16*>(&sc)[j] = f2bf(bf2f(v) * scale);
    }
    qf[ds] = sc;
    dof[ds] = ld8(dOb + (int64_t)(q0w + lo) * H * D + ds * 16 + hi * 8);
  }
  const float lse_q = lse_b[(int64_t)(q0w + lo) * H];
  const float dl_q = dl_b[(int64_t)(q0w + lo) * H];

  f32x16 dq_acc[DT32];
#pragma unroll
  for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[dt][r] = 0.f;

  const int kv_end = causal ? (qt * 256 + 256) : S;
  const int my_kv_end = causal ? (q0w + 32) : S;
  // DOC: as in the v5 forward. The element mask stays inline on every
  // tile here: hoisting it behind a boundary-tile branch, as the forward
  // does, pushed this kernel to 256 VGPRs plus scratch.
  int kv_begin = 0, my_kv_begin = 0, my_ds = 0;
  if (DOC) {
    const int* doc_b = doc + (int64_t)b * S;
    kv_begin = doc_clamp(doc_b[qt * 256], qt * 256) & ~63;
    my_kv_begin = doc_clamp(doc_b[q0w], q0w) & ~63;
    my_ds = doc_b[q0w + lo];
  }
  stage_tile<64, D, 512>(Kb + (int64_t)kv_begin * sks, sks, k_lds[0], threadIdx.x);
  stage_tile<64, D, 512>(Vb + (int64_t)kv_begin * svs, svs, v_lds[0], threadIdx.x);
  stage_tile<D, 64, 512>(Ktb + kv_begin, S, kt_lds[0], threadIdx.x);
  int idx = 0;
  for (int kv = kv_begin; kv < kv_end; kv += 64, idx ^= 1) {
    __syncthreads();
    if (kv + 64 < kv_end) {
      stage_tile<64, D, 512>(Kb + (int64_t)(kv + 64) * sks, sks,
                             k_lds[idx ^ 1], threadIdx.x);
      stage_tile<64, D, 512>(Vb + (int64_t)(kv + 64) * svs, svs,
                             v_lds[idx ^ 1], threadIdx.x);
      stage_tile<D, 64, 512>(Ktb + kv + 64, S, kt_lds[idx ^ 1], threadIdx.x);
    }
    if (kv >= my_kv_end) continue;
    if (DOC && kv < my_kv_begin) continue;

    // ---- St = K·Q^T (pre-scaled), dPt = V·dO^T: C[k][q], q = lo
    f32x16 st[2], dpt[2];
    if (FLAGS & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { st[t][r] = 0.f; dpt[t][r] = 0.f; }
#pragma unroll
      for (int ds = 0; ds < DSL; ++ds) {
        const short8 kf = ld8_swz<D>(k_lds[idx], t * 32 + lo, ds * 32 + hi * 16);
        const short8 vf = ld8_swz<D>(v_lds[idx], t * 32 + lo, ds * 32 + hi * 16);
        st[t] = mfma32(kf, qf[ds], st[t]);
        dpt[t] = mfma32(vf, dof[ds], dpt[t]);
      }
    }
    if (FLAGS & 1) __builtin_amdgcn_s_setprio(0);
    // ---- dS = P * (dP - delta) * scale, all in-register (q = lo)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kg = kv + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        float p = __expf(st[t][r] - lse_q);
        if (causal && kg > q0w + lo) p = 0.f;
        if (DOC && kg < my_ds) p = 0.f;
        st[t][r] = p * (dpt[t][r] - dl_q) * scale;
      }
    // ---- dS -> A-fragments (same lane-pair exchange as the fwd P)
    short8 da[2 * 2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int kst = 0; kst < 2; ++kst) {
        const int g0 = 4 * (2 * kst), g1 = 4 * (2 * kst + 1);
        unsigned x0 = cvt_pk_bf16(st[t][g0 + 0], st[t][g0 + 1]);
        unsigned x1 = cvt_pk_bf16(st[t][g0 + 2], st[t][g0 + 3]);
        unsigned y0 = cvt_pk_bf16(st[t][g1 + 0], st[t][g1 + 1]);
        unsigned y1 = cvt_pk_bf16(st[t][g1 + 2], st[t][g1 + 3]);
        permlane32_swap(x0, y0);
        permlane32_swap(x1, y1);
        short8 frag;
        reinterpret_cast<unsigned*>(&frag)[0] = x0;
        reinterpret_cast<unsigned*>(&frag)[1] = x1;
        reinterpret_cast<unsigned*>(&frag)[2] = y0;
        reinterpret_cast<unsigned*>(&frag)[3] = y1;
        da[t * 2 + kst] = frag;
      }
    }
    // ---- dQ += dS·K (B-frags from swizzled Kt LDS)
    if (FLAGS & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        dq_acc[dt] = mfma32(da[ks],
                            ld8_swz<64>(kt_lds[idx], dt * 32 + lo, ks * 32 + hi * 16),
                            dq_acc[dt]);
    if (FLAGS & 1) __builtin_amdgcn_s_setprio(0);
  }
  // ---- epilogue: C[q][d] rows q = crow(r,hi)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = (r & 3) + 8 * (r >> 2) + 4 * hi;
    bf16* row = dQ + (((int64_t)(b * S + q0w + qr)) * H + h) * D;
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
      row[dt * 32 + lo] = f2bf(dq_acc[dt][r]);
  }
}

// ----------------------------------------------------------- backward dQ
// Stages K[64][D], V[64][D] (B-operands for S and dP) and Kt[D][64]
// (B-operand for dQ += dS*K). dO is contiguous [B,S,H,D].
template <int D, bool DOC = false>
__global__ __launch_bounds__(256) void flash_bwd_dq_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ Kt,
    const bf16* __restrict__ dO, const float* __restrict__ lse,
    const float* __restrict__ delta, bf16* __restrict__ dQ, int B, int H,
    int Hkv, int S, float scale, int causal,
    int64_t sqb, int64_t sqs, int64_t sqh,
    int64_t skb, int64_t sks, int64_t skh,
    int64_t svb, int64_t svs, int64_t svh,
    const int* __restrict__ doc) {
  constexpr int DS = D / 32;
  constexpr int DT = D / 16;
  const int n_qt = S / 64;
  const int bh = blockIdx.x / n_qt;
  const int qt = n_qt - 1 - (blockIdx.x - bh * n_qt);  // longest trips first
  const int b = bh / H, h = bh - b * H;
  const int hkv = h / (H / Hkv);
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lg = lane >> 4, li = lane & 15;
  const int q0 = qt * 64 + wid * 16;

  const bf16* Qb = Q + b * sqb + h * sqh;
  const bf16* Kb = K + b * skb + hkv * skh;
  const bf16* Vb = V + b * svb + hkv * svh;
  const bf16* Ktb = Kt + ((int64_t)(b * Hkv + hkv) * D) * S;
  const bf16* dOb = dO + ((int64_t)b * S * H + h) * D;  // row stride H*D
  const float* lse_b = lse + (int64_t)b * S * H + h;    // stride H
  const float* dl_b = delta + (int64_t)b * S * H + h;

  __shared__ bf16 k_lds[64 * D];
  __shared__ bf16 v_lds[64 * D];
  __shared__ bf16 kt_lds[D * 64];
  __shared__ bf16 ds_lds_all[4][16 * 64];
  bf16* ds_lds = ds_lds_all[wid];

  short8 qf[DS], dof[DS];
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) {
    qf[ds] = ld8(Qb + (int64_t)(q0 + li) * sqs + ds * 32 + lg * 8);
    dof[ds] = ld8(dOb + (int64_t)(q0 + li) * H * D + ds * 32 + lg * 8);
  }
  float lse_r[4], dl_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lse_r[r] = lse_b[(int64_t)(q0 + lg * 4 + r) * H];
    dl_r[r] = dl_b[(int64_t)(q0 + lg * 4 + r) * H];
  }
  f32x4 dq_acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kv_end = causal ? (qt * 64 + 64) : S;
  int kv_begin = 0, my_kv_begin = 0, row_ds[4];  // DOC: as in flash_fwd_kernel
  if (DOC) {
    const int* doc_b = doc + (int64_t)b * S;
    kv_begin = doc_clamp(doc_b[qt * 64], qt * 64) & ~63;
    my_kv_begin = doc_clamp(doc_b[q0], q0) & ~63;
#pragma unroll
    for (int r = 0; r < 4; ++r) row_ds[r] = doc_b[q0 + lg * 4 + r];
  }
  for (int kv = kv_begin; kv < kv_end; kv += 64) {
    __syncthreads();
    stage_tile<64, D>(Kb + (int64_t)kv * sks, sks, k_lds, threadIdx.x);
    stage_tile<64, D>(Vb + (int64_t)kv * svs, svs, v_lds, threadIdx.x);
    stage_tile<D, 64>(Ktb + kv, S, kt_lds, threadIdx.x);
    __syncthreads();
    if (DOC && kv < my_kv_begin) continue;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      f32x4 s_acc{0.f, 0.f, 0.f, 0.f}, dp_acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < DS; ++ds) {
        s_acc = mfma16(qf[ds], ld8_swz<D>(k_lds, sub * 16 + li, ds * 64 + lg * 16), s_acc);
        dp_acc = mfma16(dof[ds], ld8_swz<D>(v_lds, sub * 16 + li, ds * 64 + lg * 16), dp_acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qg = q0 + lg * 4 + r;
        const int kg = kv + sub * 16 + li;
        float p = __expf(s_acc[r] * scale - lse_r[r]);
        if (causal && kg > qg) p = 0.f;
        if (DOC && kg < row_ds[r]) p = 0.f;
        st16_swz<64>(ds_lds, lg * 4 + r, sub * 16 + li,
                     f2bf(p * (dp_acc[r] - dl_r[r]) * scale));
      }
    }
    wave_lds_fence();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        dq_acc[dt] = mfma16(ld8_swz<64>(ds_lds, li, ks * 64 + lg * 16),
                            ld8_swz<64>(kt_lds, dt * 16 + li, ks * 64 + lg * 16),
                            dq_acc[dt]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    bf16* row = dQ + (((int64_t)(b * S + q0 + lg * 4 + r)) * H + h) * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) row[dt * 16 + li] = f2bf(dq_acc[dt][r]);
  }
}

// ---------------------------------------------- backward dK/dV v5 (32x32)
// Swapped the other way around from the fwd/dq kernels: St^T = Q·K^T puts
// each lane's scores at a FIXED key column (k = lane&31, the dimension
// this kernel accumulates over), so P^T/dS^T feed the dV/dK accumulation
// A-fragments after the same cvt_pk + permlane32_swap lane-pair exchange
// — no per-wave P/dS LDS bounce. K/V rows live in registers (per-wave
// constants), Q/dO rows are read per-lane from global (L1-resident across
// the d-slice loop), and only the genuinely-transposed operands (Qt/dOt
// tiles for the accumulation B-fragments) are staged, double-buffered.
// 8 waves x 32 k-rows = 256-row k tiles; fp32 split workspaces + reduce
// as in the 16x16 kernel.
template <int D, int FLAGS>
__global__ __launch_bounds__(512, 2) void flash_bwd_dkv_v5_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ Qt,
    const bf16* __restrict__ K, const bf16* __restrict__ V,
    const bf16* __restrict__ dO, const bf16* __restrict__ dOt,
    const float* __restrict__ lse, const float* __restrict__ delta,
    float* __restrict__ wsK, float* __restrict__ wsV, int B, int H, int Hkv,
    int S, float scale, int causal, int splits,
    int64_t sqb, int64_t sqs, int64_t sqh,
    int64_t skb, int64_t sks, int64_t skh,
    int64_t svb, int64_t svs, int64_t svh) {
  constexpr int DSL = D / 16;
  constexpr int DT32 = D / 32;
  const int n_kt = S / 256;
  const int per_split = (B * Hkv) * n_kt;
  const int split = blockIdx.x / per_split;
  const int rem = blockIdx.x - split * per_split;
  const int bh = rem / n_kt;
  const int kt = rem - bh * n_kt;
  const int b = bh / Hkv, hkv = bh - b * Hkv;
  const int group = H / Hkv;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lo = lane & 31, hi = lane >> 5;
  const int k0w = kt * 256 + wid * 32;  // this wave's first k row (global)

  const bf16* Kb = K + b * skb + hkv * skh;
  const bf16* Vb = V + b * svb + hkv * svh;

  __shared__ bf16 q_lds[2][64 * D];
  __shared__ bf16 do_lds[2][64 * D];
  __shared__ bf16 qt_lds[2][D * 64];
  __shared__ bf16 dot_lds[2][D * 64];

  // K^T / V^T B-fragment source rows (k0w+lo): loaded inline per MFMA —
  // holding all 8 slices of both in registers (64 VGPRs) pushed the
  // kernel to 256 regs + scratch spills; the rows stay L1-resident
  // across the q loop instead
  const bf16* krow = Kb + (int64_t)(k0w + lo) * sks;
  const bf16* vrow = Vb + (int64_t)(k0w + lo) * svs;
  f32x16 dk_acc[DT32], dv_acc[DT32];
#pragma unroll
  for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk_acc[dt][r] = 0.f; dv_acc[dt][r] = 0.f; }

  // flattened (g, q-tile) loop for double-buffered Qt/dOt prefetch
  const int q_start = (causal ? kt * 256 : 0) + split * 64;
  const int tiles_per_g = (S - q_start + 64 * splits - 1) / (64 * splits);
  const int n_iter = group * tiles_per_g;
  const auto stage_for = [&](int it, int buf) {
    const int g = it / tiles_per_g;
    const int q0g = q_start + (it - g * tiles_per_g) * 64 * splits;
    const int h = hkv * group + g;
    const bf16* Qb_ = Q + b * sqb + h * sqh;
    const bf16* dOb_ = dO + ((int64_t)b * S * H + h) * D;
    const bf16* Qtb = Qt + ((int64_t)(b * H + h) * D) * S;
    const bf16* dOtb = dOt + ((int64_t)(b * H + h) * D) * S;
    stage_tile<64, D, 512>(Qb_ + (int64_t)q0g * sqs, sqs, q_lds[buf], threadIdx.x);
    stage_tile<64, D, 512>(dOb_ + (int64_t)q0g * H * D, (int64_t)H * D, do_lds[buf], threadIdx.x);
    stage_tile<D, 64, 512>(Qtb + q0g, S, qt_lds[buf], threadIdx.x);
    stage_tile<D, 64, 512>(dOtb + q0g, S, dot_lds[buf], threadIdx.x);
  };
  stage_for(0, 0);
  for (int it = 0; it < n_iter; ++it) {
    const int cur = it & 1;
    __syncthreads();
    if (it + 1 < n_iter)
      stage_for(it + 1, cur ^ 1);
    const int g = it / tiles_per_g;
    const int q0g = q_start + (it - g * tiles_per_g) * 64 * splits;
    if (causal && q0g + 64 <= k0w) continue;  // fully masked for this wave
    const int h = hkv * group + g;
    const float* lse_b = lse + (int64_t)b * S * H + h;
    const float* dl_b = delta + (int64_t)b * S * H + h;

#pragma unroll
    for (int qs = 0; qs < 2; ++qs) {
      const int q32 = q0g + qs * 32;
      // St^T = Q·K^T, dPt^T = dO·V^T: C[32q][32k], k = lo (lane-local)
      f32x16 st, dpt;
#pragma unroll
      for (int r = 0; r < 16; ++r) { st[r] = 0.f; dpt[r] = 0.f; }
      if (FLAGS & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ds = 0; ds < DSL; ++ds) {
        const short8 qfr = ld8_swz<D>(q_lds[cur], qs * 32 + lo, ds * 32 + hi * 16);
        st = mfma32(qfr, ld8(krow + ds * 16 + hi * 8), st);
      }
#pragma unroll
      for (int ds = 0; ds < DSL; ++ds) {
        const short8 dofr = ld8_swz<D>(do_lds[cur], qs * 32 + lo, ds * 32 + hi * 16);
        dpt = mfma32(dofr, ld8(vrow + ds * 16 + hi * 8), dpt);
      }
      if (FLAGS & 1) __builtin_amdgcn_s_setprio(0);
      // P^T / dS^T in-register; lse/delta per q-row crow(r,hi) are
      // broadcast loads (same address across the 32 lo-lanes)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qg = q32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float lse_q = lse_b[(int64_t)qg * H];
        const float dl_q = dl_b[(int64_t)qg * H];
        float p = __expf(st[r] * scale - lse_q);
        if (causal && (k0w + lo) > qg) p = 0.f;
        st[r] = p;
        dpt[r] = p * (dpt[r] - dl_q) * scale;
      }
      // pack P^T / dS^T into accumulation A-fragments: A[32k][16q], the
      // q-slices split across the lane pair exactly like the fwd P
      short8 pa[2], da[2];
#pragma unroll
      for (int kst = 0; kst < 2; ++kst) {
        const int g0 = 4 * (2 * kst), g1 = 4 * (2 * kst + 1);
        unsigned x0 = cvt_pk_bf16(st[g0 + 0], st[g0 + 1]);
        unsigned x1 = cvt_pk_bf16(st[g0 + 2], st[g0 + 3]);
        unsigned y0 = cvt_pk_bf16(st[g1 + 0], st[g1 + 1]);
        unsigned y1 = cvt_pk_bf16(st[g1 + 2], st[g1 + 3]);
        permlane32_swap(x0, y0);
        permlane32_swap(x1, y1);
        short8 f;
        reinterpret_cast<unsigned*>(&f)[0] = x0;
        reinterpret_cast<unsigned*>(&f)[1] = x1;
        reinterpret_cast<unsigned*>(&f)[2] = y0;
        reinterpret_cast<unsigned*>(&f)[3] = y1;
        pa[kst] = f;
        x0 = cvt_pk_bf16(dpt[g0 + 0], dpt[g0 + 1]);
        x1 = cvt_pk_bf16(dpt[g0 + 2], dpt[g0 + 3]);
        y0 = cvt_pk_bf16(dpt[g1 + 0], dpt[g1 + 1]);
        y1 = cvt_pk_bf16(dpt[g1 + 2], dpt[g1 + 3]);
        permlane32_swap(x0, y0);
        permlane32_swap(x1, y1);
        reinterpret_cast<unsigned*>(&f)[0] = x0;
        reinterpret_cast<unsigned*>(&f)[1] = x1;
        reinterpret_cast<unsigned*>(&f)[2] = y0;
        reinterpret_cast<unsigned*>(&f)[3] = y1;
        da[kst] = f;
      }
      // dV += P^T·dO, dK += dS^T·Q (B-frags from swizzled dOt/Qt tiles)
      if (FLAGS & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
        for (int kst = 0; kst < 2; ++kst) {
          const int colb = qs * 64 + kst * 32 + hi * 16;
          dv_acc[dt] = mfma32(pa[kst],
                              ld8_swz<64>(dot_lds[cur], dt * 32 + lo, colb),
                              dv_acc[dt]);
          dk_acc[dt] = mfma32(da[kst],
                              ld8_swz<64>(qt_lds[cur], dt * 32 + lo, colb),
                              dk_acc[dt]);
        }
      if (FLAGS & 1) __builtin_amdgcn_s_setprio(0);
    }
  }
  // fp32 partials: ws[split][b][hkv][kg][d]; C[32k][32d] rows crow(r,hi)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kg = k0w + (r & 3) + 8 * (r >> 2) + 4 * hi;
    const int64_t base = ((((int64_t)split * B + b) * Hkv + hkv) * S + kg) * D;
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt) {
      wsK[base + dt * 32 + lo] = dk_acc[dt][r];
      wsV[base + dt * 32 + lo] = dv_acc[dt][r];
    }
  }
}

// -------------------------------------------------------- backward dK, dV
// Stages Q[64][D], dO[64][D] (operands of the score and dP products),
// Qt[D][64] and dOt[D][64] (operands of the dK and dV accumulation).
//
// Tile body (default): St = mfma16(kf, qb) leaves the key on the
// accumulator row, so each wave passes P and dS through its own LDS
// buffers (2-byte swizzled stores, a wave-local fence, 16-byte reads) to
// get them key-on-the-lane for dV += P^T·dO and dK += dS^T·Q. At NW=8,
// D=128, DBUF=2 that is 2x4x16 KiB stages + 8x2x2 KiB wave buffers =
// exactly the 160 KiB LDS limit. acc[dt][r] = [k0 + lg*4 + r][dt*16 + li].
//
// Tile body, -DPRIME_DKV_KEYLANE=1 (measured SLOWER, kept for A/B: 2.04 vs
// 1.88 ms whole backward at the bench shape, see profiles): key on the
// lane. S = mfma16(qb, kf) and dP = mfma16(dob, vf) leave
// S[q = sub*16 + lg*4 + r][k = k0 + li] in the accumulator — the same
// registers and LDS reads (the A and B maps mirror each other), roles
// swapped. For the 32-query half c of the tile a lane's eight values
// (subs 2c and 2c+1, four rows each), packed to bf16, are then already
// the B fragment of
//   dV^T[d][k] += dO^T[d][q] * P[q][k],   dK^T[d][k] += Q^T[d][q] * dS[q][k]
// with the K dimension in the permuted query order
//   kidx = lg*8 + j  ->  q = 32c + 16*(j>>2) + lg*4 + (j&3).
// The A fragment follows the same order: lane (lg, li) reads row
// d = dt*16 + li of dot_lds/qt_lds as two 8-byte runs at q = 32c + lg*4
// and q = 32c + 16 + lg*4 (ld4x2_swz). P and dS never touch LDS (128 KiB);
// acc[dt][r] = [k0 + li][dt*16 + lg*4 + r]. In this body four consecutive
// queries' lse/delta are one aligned 16-byte load each, issued one q-tile
// ahead (-DPRIME_DKV_ROWC_PREFETCH=0: at the point of use).
//
// lse/delta come from the [B,H,S] copies attn_delta_kernel writes (rowc =
// {lse_t, delta_t}): the 16 lanes of a group read 16 consecutive floats.
//
// DBUF=2: double-buffered q/do/qt/dot stages with prefetch-behind-barrier
// (one barrier per q-tile).
// direct=1: the block runs every q-tile of its k-tile and stores bf16
// dK/dV itself — no reduce kernel, no per-split partials. Causal blocks
// take k-tile kt and then n_kt-1-kt (their trip counts always add up to
// the same total), the middle tile of an odd n_kt once. The q-tiles are
// still taken in `splits` slices, summed in dkv_reduce_kernel's order, so
// the result has the bits of direct=0: the grid-split q loop with fp32
// partials in wsK/wsV.
// DOC: doc_end[B][S] bounds the q loop from above — queries at or past
// the end of the tile's LAST key's document see none of its keys, and
// monotonicity makes that one lookup exact for the whole tile.
__device__ __forceinline__ short8 ld4x2_swz(const bf16* lds_tile, int row,
                                            int colb) {
  typedef __attribute__((ext_vector_type(4))) short short4v;
  const char* base = reinterpret_cast<const char*>(lds_tile) + row * 128;
  const int sw = (row & 7) << 4;
  const short4v lo = *reinterpret_cast<const short4v*>(base + (colb ^ sw));
  const short4v hi = *reinterpret_cast<const short4v*>(base + ((colb + 32) ^ sw));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ short bf_bits(bf16 x) {
  return (short)__bfloat16_as_ushort(x);
}

#ifndef PRIME_DKV_KEYLANE
#define PRIME_DKV_KEYLANE 0  // 1: key-on-the-lane tile body (A/B build)
#endif
#ifndef PRIME_DKV_ROWC_PREFETCH
#define PRIME_DKV_ROWC_PREFETCH 1  // key-on-the-lane body only; 0: load at use
#endif
#if !PRIME_DKV_KEYLANE
#undef PRIME_DKV_ROWC_PREFETCH
#define PRIME_DKV_ROWC_PREFETCH 0
#endif

template <int D, int NW = 4, int DBUF = 1, bool DOC = false>  // NW waves x 16 k-rows
__global__ __launch_bounds__(512) void flash_bwd_dkv_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ Qt,
    const bf16* __restrict__ K, const bf16* __restrict__ V,
    const bf16* __restrict__ dO, const bf16* __restrict__ dOt,
    const float* __restrict__ rowc,
    float* __restrict__ wsK, float* __restrict__ wsV,
    bf16* __restrict__ dK, bf16* __restrict__ dV, int B, int H, int Hkv,
    int S, float scale, int causal, int splits, int direct,
    int64_t sqb, int64_t sqs, int64_t sqh,
    int64_t skb, int64_t sks, int64_t skh,
    int64_t svb, int64_t svs, int64_t svh,
    const int* __restrict__ doc_end) {
  constexpr int DS = D / 32;
  constexpr int DT = D / 16;
  const int n_kt = S / (NW * 16);
  // direct + causal: one block per pair (kt, n_kt-1-kt); otherwise one
  // block per (split, k-tile)
  const bool paired = direct && causal;
  const int per_bh = paired ? (n_kt + 1) / 2 : n_kt;
  const int per_split = (B * Hkv) * per_bh;
  const int blk_split = blockIdx.x / per_split;  // 0 when direct
  const int rem = blockIdx.x - blk_split * per_split;
  const int bh = rem / per_bh;
  const int kt0 = rem - bh * per_bh;
  const int n_pass = (paired && kt0 != n_kt - 1 - kt0) ? 2 : 1;
  const int b = bh / Hkv, hkv = bh - b * Hkv;
  const int group = H / Hkv;
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int lg = lane >> 4, li = lane & 15;

  const bf16* Kb = K + b * skb + hkv * skh;
  const bf16* Vb = V + b * svb + hkv * svh;
  const float* lse_t = rowc + (int64_t)b * H * S;
  const float* dl_t = lse_t + (int64_t)B * H * S;

  __shared__ bf16 q_lds[DBUF][64 * D];
  __shared__ bf16 do_lds[DBUF][64 * D];
  __shared__ bf16 qt_lds[DBUF][D * 64];
  __shared__ bf16 dot_lds[DBUF][D * 64];
#if !PRIME_DKV_KEYLANE
  __shared__ bf16 pt_lds_all[NW][16 * 64];
  __shared__ bf16 dst_lds_all[NW][16 * 64];
  bf16* pt_lds = pt_lds_all[wid];
  bf16* dst_lds = dst_lds_all[wid];
#endif

  // direct: the block walks the `splits` q-loop slices of its k-tile one
  // after the other, each from zeroed accumulators and in the order a
  // split-mode block takes them, and adds the slices up in the order
  // dkv_reduce_kernel does — so both modes give the same bits. The running
  // sum of slices 0..vs-1 waits in ws[0] (each thread re-reads only what
  // it wrote itself).
  const int n_vs = direct ? splits : 1;
  for (int pv = 0; pv < n_pass * n_vs; ++pv) {
  const int pass = pv / n_vs;
  const int vs = pv - pass * n_vs;
  const int split = direct ? vs : blk_split;
  const int kt = pass ? n_kt - 1 - kt0 : kt0;
  const int k0 = kt * (NW * 16) + wid * 16;
  // every wave must be done reading the stage images of the previous
  // slice or k-tile before they are primed again
  if (pv) __syncthreads();

  short8 kf[DS], vf[DS];
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) {
    kf[ds] = ld8(Kb + (int64_t)(k0 + li) * sks + ds * 32 + lg * 8);
    vf[ds] = ld8(Vb + (int64_t)(k0 + li) * svs + ds * 32 + lg * 8);
  }
  f32x4 dk_acc[DT], dv_acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    dk_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv_acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int q_start = (causal ? (kt * (NW * 16)) / 64 * 64 : 0) + split * 64;
  // DOC: q tiles run up to the end of the last key's document, rounded up
  // to a tile and clamped to S (block-uniform, so n_iter — which drives
  // the prefetch — is exact for every split and every head of the group);
  // my_q_end is the same for this wave's last key; key_end masks this
  // lane's key.
  int q_end = S, my_q_end = S, key_end = S;
  if (DOC) {
    const int* de_b = doc_end + (int64_t)b * S;
    q_end = (doc_clamp(de_b[kt * (NW * 16) + NW * 16 - 1], S) + 63) & ~63;
    my_q_end = doc_clamp(de_b[k0 + 15], S);
    key_end = de_b[k0 + li];
  }
#if !PRIME_DKV_KEYLANE
  int key_end4[4] = {S, S, S, S};
  if (DOC) {
#pragma unroll
    for (int r = 0; r < 4; ++r) key_end4[r] = doc_end[(int64_t)b * S + k0 + lg * 4 + r];
  }
#endif
  const int tiles_per_g =
      (q_end > q_start) ? (q_end - q_start + 64 * splits - 1) / (64 * splits) : 0;
  const int n_iter = group * tiles_per_g;
  const auto stage_it = [&](int it, int buf) {
    const int g_ = it / tiles_per_g;
    const int q0g_ = q_start + (it - g_ * tiles_per_g) * 64 * splits;
    const int h_ = hkv * group + g_;
    const bf16* Qb_ = Q + b * sqb + h_ * sqh;
    const bf16* dOb_ = dO + ((int64_t)b * S * H + h_) * D;
    const bf16* Qtb_ = Qt + ((int64_t)(b * H + h_) * D) * S;
    const bf16* dOtb_ = dOt + ((int64_t)(b * H + h_) * D) * S;
    stage_tile<64, D, NW * 64>(Qb_ + (int64_t)q0g_ * sqs, sqs, q_lds[buf], threadIdx.x);
    stage_tile<64, D, NW * 64>(dOb_ + (int64_t)q0g_ * H * D, (int64_t)H * D, do_lds[buf], threadIdx.x);
    stage_tile<D, 64, NW * 64>(Qtb_ + q0g_, S, qt_lds[buf], threadIdx.x);
    stage_tile<D, 64, NW * 64>(dOtb_ + q0g_, S, dot_lds[buf], threadIdx.x);
  };
  // row constants of q-tile `it`, sub-tile `sub`: queries q0g + sub*16 +
  // lg*4 .. +3 of head h (it < n_iter: always inside [0, S))
  const auto rowc_off = [&](int it, int sub) {
    const int g_ = it / tiles_per_g;
    const int q0g_ = q_start + (it - g_ * tiles_per_g) * 64 * splits;
    return (int64_t)(hkv * group + g_) * S + q0g_ + sub * 16 + lg * 4;
  };
  f32x4 lse_r[4], dl_r[4];
  if (PRIME_DKV_ROWC_PREFETCH && n_iter > 0) {
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const int64_t o = rowc_off(0, sub);
      lse_r[sub] = *reinterpret_cast<const f32x4*>(lse_t + o);
      dl_r[sub] = *reinterpret_cast<const f32x4*>(dl_t + o);
    }
  }
  if (DBUF == 2 && n_iter > 0) stage_it(0, 0);
  for (int it = 0; it < n_iter; ++it) {
    const int g = it / tiles_per_g;
    const int q0g = q_start + (it - g * tiles_per_g) * 64 * splits;
    const int cur = (DBUF == 2) ? (it & 1) : 0;
    // the tile whose row constants are fetched during this one (the last
    // iteration re-reads its own: in range, never used)
    const int itn = (it + 1 < n_iter) ? it + 1 : it;
    {
      __syncthreads();
      if (DBUF == 2) {
        // prefetch-behind-barrier: next tile's loads land under this
        // tile's compute; the next barrier drains them
        if (it + 1 < n_iter) stage_it(it + 1, cur ^ 1);
      } else {
        stage_it(it, 0);
        __syncthreads();
      }
      // per-wave causal clip: this wave's k-rows start at k0, so q-tiles
      // entirely below the diagonal are fully masked — skip their
      // compute (the wave still co-staged and hits the next barrier)
      const bool skip = (causal && q0g + 64 <= k0) || (DOC && q0g >= my_q_end);
      if (skip) {
        if (PRIME_DKV_ROWC_PREFETCH) {
#pragma unroll
          for (int sub = 0; sub < 4; ++sub) {
            const int64_t o = rowc_off(itn, sub);
            lse_r[sub] = *reinterpret_cast<const f32x4*>(lse_t + o);
            dl_r[sub] = *reinterpret_cast<const f32x4*>(dl_t + o);
          }
        }
        continue;
      }
#if !PRIME_DKV_KEYLANE
#pragma unroll
      for (int sub = 0; sub < 4; ++sub) {
        f32x4 st_acc{0.f, 0.f, 0.f, 0.f}, dpt_acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ds = 0; ds < DS; ++ds) {
          const short8 qb = ld8_swz<D>(q_lds[cur], sub * 16 + li, ds * 64 + lg * 16);
          const short8 dob = ld8_swz<D>(do_lds[cur], sub * 16 + li, ds * 64 + lg * 16);
          st_acc = mfma16(kf[ds], qb, st_acc);
          dpt_acc = mfma16(vf[ds], dob, dpt_acc);
        }
        const int qg = q0g + sub * 16 + li;
        const int64_t o = (int64_t)(hkv * group + g) * S + qg;
        const float lse_q = lse_t[o];
        const float dl_q = dl_t[o];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __expf(st_acc[r] * scale - lse_q);
          if (causal && k0 + lg * 4 + r > qg) p = 0.f;
          if (DOC && qg >= key_end4[r]) p = 0.f;
          st16_swz<64>(pt_lds, lg * 4 + r, sub * 16 + li, f2bf(p));
          st16_swz<64>(dst_lds, lg * 4 + r, sub * 16 + li,
                       f2bf(p * (dpt_acc[r] - dl_q) * scale));
        }
      }
      wave_lds_fence();
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const short8 pa = ld8_swz<64>(pt_lds, li, ks * 64 + lg * 16);
          const short8 da = ld8_swz<64>(dst_lds, li, ks * 64 + lg * 16);
          dv_acc[dt] = mfma16(pa, ld8_swz<64>(dot_lds[cur], dt * 16 + li, ks * 64 + lg * 16), dv_acc[dt]);
          dk_acc[dt] = mfma16(da, ld8_swz<64>(qt_lds[cur], dt * 16 + li, ks * 64 + lg * 16), dk_acc[dt]);
        }
#else
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        short8 pb, dsb;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int sub = c * 2 + s2;
          f32x4 s_acc{0.f, 0.f, 0.f, 0.f}, dp_acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ds = 0; ds < DS; ++ds) {
            const short8 qb = ld8_swz<D>(q_lds[cur], sub * 16 + li, ds * 64 + lg * 16);
            const short8 dob = ld8_swz<D>(do_lds[cur], sub * 16 + li, ds * 64 + lg * 16);
            s_acc = mfma16(qb, kf[ds], s_acc);
            dp_acc = mfma16(dob, vf[ds], dp_acc);
          }
          f32x4 lse_q, dl_q;
          if (PRIME_DKV_ROWC_PREFETCH) {
            lse_q = lse_r[sub];
            dl_q = dl_r[sub];
            const int64_t o = rowc_off(itn, sub);
            lse_r[sub] = *reinterpret_cast<const f32x4*>(lse_t + o);
            dl_r[sub] = *reinterpret_cast<const f32x4*>(dl_t + o);
          } else {
            const int64_t o = rowc_off(it, sub);
            lse_q = *reinterpret_cast<const f32x4*>(lse_t + o);
            dl_q = *reinterpret_cast<const f32x4*>(dl_t + o);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int qg = q0g + sub * 16 + lg * 4 + r;
            float p = __expf(s_acc[r] * scale - lse_q[r]);
            if (causal && k0 + li > qg) p = 0.f;
            if (DOC && qg >= key_end) p = 0.f;
            pb[s2 * 4 + r] = bf_bits(f2bf(p));
            dsb[s2 * 4 + r] = bf_bits(f2bf(p * (dp_acc[r] - dl_q[r]) * scale));
          }
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const short8 dota = ld4x2_swz(dot_lds[cur], dt * 16 + li, c * 64 + lg * 8);
          const short8 qta = ld4x2_swz(qt_lds[cur], dt * 16 + li, c * 64 + lg * 8);
          dv_acc[dt] = mfma16(dota, pb, dv_acc[dt]);
          dk_acc[dt] = mfma16(qta, dsb, dk_acc[dt]);
        }
      }
#endif
    }
  }
#if !PRIME_DKV_KEYLANE
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // acc[dt][r] = [k0 + lg*4 + r][dt*16 + li]
    const int kr = k0 + lg * 4 + r;
    const int64_t ob = (((int64_t)b * S + kr) * Hkv + hkv) * D + li;
    const int64_t wb = ((((int64_t)blk_split * B + b) * Hkv + hkv) * S + kr) * D + li;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      if (direct) {
        // sum = ((0 + slice0) + slice1) + ..., as dkv_reduce_kernel adds
        float sk = 0.f + dk_acc[dt][r], sv = 0.f + dv_acc[dt][r];
        if (vs > 0) {
          sk = wsK[wb + dt * 16] + dk_acc[dt][r];
          sv = wsV[wb + dt * 16] + dv_acc[dt][r];
        }
        if (vs + 1 < n_vs) {
          wsK[wb + dt * 16] = sk;
          wsV[wb + dt * 16] = sv;
        } else {
          dK[ob + dt * 16] = f2bf(sk);
          dV[ob + dt * 16] = f2bf(sv);
        }
      } else {
        wsK[wb + dt * 16] = dk_acc[dt][r];
        wsV[wb + dt * 16] = dv_acc[dt][r];
      }
    }
  }
#else
  const int kg = k0 + li;
  const int64_t wbase = ((((int64_t)blk_split * B + b) * Hkv + hkv) * S + kg) * D + lg * 4;
  if (direct) {
    // bf16 dK/dV [B,S,Hkv,D]: four consecutive d per lane, 8-byte stores
    const int64_t base = (((int64_t)b * S + kg) * Hkv + hkv) * D + lg * 4;
    const f32x4 zero{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      f32x4 sk = zero + dk_acc[dt], sv = zero + dv_acc[dt];
      if (vs > 0) {
        sk = *reinterpret_cast<f32x4*>(wsK + wbase + dt * 16) + dk_acc[dt];
        sv = *reinterpret_cast<f32x4*>(wsV + wbase + dt * 16) + dv_acc[dt];
      }
      if (vs + 1 < n_vs) {
        *reinterpret_cast<f32x4*>(wsK + wbase + dt * 16) = sk;
        *reinterpret_cast<f32x4*>(wsV + wbase + dt * 16) = sv;
      } else {
        bf16x4 ok, ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ok.v[r] = f2bf(sk[r]);
          ov.v[r] = f2bf(sv[r]);
        }
        *reinterpret_cast<bf16x4*>(dK + base + dt * 16) = ok;
        *reinterpret_cast<bf16x4*>(dV + base + dt * 16) = ov;
      }
    }
  } else {
    // fp32 partials: ws[split][b][hkv][kg][d]
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      *reinterpret_cast<f32x4*>(wsK + wbase + dt * 16) = dk_acc[dt];
      *reinterpret_cast<f32x4*>(wsV + wbase + dt * 16) = dv_acc[dt];
    }
  }
#endif
  }  // k-tile pass x q-loop slice
}

// reduce fp32 split-partials -> bf16 dK/dV in [B,S,Hkv,D]
__global__ void dkv_reduce_kernel(const float* __restrict__ wsK,
                                  const float* __restrict__ wsV,
                                  bf16* __restrict__ dK, bf16* __restrict__ dV,
                                  int B, int Hkv, int S, int D, int splits) {
  const int64_t n = (int64_t)B * Hkv * S * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float k = 0.f, v = 0.f;
    for (int sp = 0; sp < splits; ++sp) {
      k += wsK[(int64_t)sp * n + i];
      v += wsV[(int64_t)sp * n + i];
    }
    // i decodes as [b][hkv][s][d] -> output [b][s][hkv][d]
    const int d = (int)(i % D);
    int64_t r = i / D;
    const int sq = (int)(r % S);
    r /= S;
    const int hk = (int)(r % Hkv);
    const int bb = (int)(r / Hkv);
    const int64_t o = (((int64_t)(bb * S + sq)) * Hkv + hk) * D + d;
    dK[o] = f2bf(k);
    dV[o] = f2bf(v);
  }
}

// ------------------------------------------------------------------ host API
#define DISPATCH_D(KER, ...)                                            \
  do {                                                                  \
    if (D == 128)                                                       \
      hipLaunchKernelGGL(KER<128>, dim3(grid), dim3(256), 0, stream,    \
                         __VA_ARGS__);                                  \
    else                                                                \
      hipLaunchKernelGGL(KER<64>, dim3(grid), dim3(256), 0, stream,     \
                         __VA_ARGS__);                                  \
  } while (0)

PRIME_API int prime_flash_fwd(hipStream_t stream, const void* Q, const void* K,
                              const void* Vt, void* O, void* lse, int64_t B,
                              int64_t H, int64_t Hkv, int64_t S, int64_t D,
                              double scale, int64_t causal,
                              int64_t sqb, int64_t sqs, int64_t sqh,
                              int64_t skb, int64_t sks, int64_t skh,
                              const void* doc_start) {
  if (S % 64 != 0 || (D != 64 && D != 128)) return hipErrorInvalidValue;
  static const char* v5env = getenv("PRIME_ATTN_V5");
  static const char* flagenv = getenv("PRIME_ATTN_FLAGS");
  if (doc_start) {
    // document-masked instantiations (causal only): the default dispatch
    // with its default FLAGS; PRIME_ATTN_FLAGS is an A/B knob of the
    // unmasked kernels and is not honoured here
    if (!causal) return hipErrorInvalidValue;
    const bool v5 = (S % 256 == 0) && !(v5env && v5env[0] == '0');
#define LAUNCH_FWD_DOC(KER, QT, NT)                                          \
    hipLaunchKernelGGL(KER, dim3((int)(B * H * (S / QT))), dim3(NT), 0,      \
                       stream, (const bf16*)Q, (const bf16*)K,               \
                       (const bf16*)Vt, (bf16*)O, (float*)lse, (int)B,       \
                       (int)H, (int)Hkv, (int)S, (float)scale, 1, sqb, sqs,  \
                       sqh, skb, sks, skh, (const int*)doc_start)
    if (v5 && D == 128) LAUNCH_FWD_DOC((flash_fwd_v5_kernel<128, 2, true>), 256, 512);
    else if (v5) LAUNCH_FWD_DOC((flash_fwd_v5_kernel<64, 2, true>), 256, 512);
    else if (D == 128) LAUNCH_FWD_DOC((flash_fwd_kernel<128, 4, true>), 64, 256);
    else LAUNCH_FWD_DOC((flash_fwd_kernel<64, 4, true>), 64, 256);
    return (int)hipGetLastError();
  }
  // measured on MI355X (15-iter sweep): FLAGS=2 417 TF > 3 (406) > 0 (387)
  // > 1 (382) — defer-max pays, setprio slightly negative here. The
  // 3-buffer counted-vmcnt variant (FLAGS=6) measured 401-402 vs 417-418
  // in interleaved A/B: the prefetch-behind-barrier schedule already
  // covers the stage latency, and the third buffer only adds LDS +
  // addressing cost.
  const int flags = flagenv ? atoi(flagenv) : 2;
  const bool use_v5 =
      (D == 128 || D == 64) && (S % 256 == 0) && !(v5env && v5env[0] == '0');
  if (use_v5 && D == 64) {
    const int grid = (int)(B * H * (S / 256));
    switch (flags & 7) {
      case 0:
        hipLaunchKernelGGL((flash_fwd_v5_kernel<64, 0>), dim3(grid),
                           dim3(512), 0, stream, (const bf16*)Q,
                           (const bf16*)K, (const bf16*)Vt, (bf16*)O,
                           (float*)lse, (int)B, (int)H, (int)Hkv, (int)S,
                           (float)scale, (int)causal, sqb, sqs, sqh, skb,
                           sks, skh, (const int*)nullptr);
        break;
      default:
        hipLaunchKernelGGL((flash_fwd_v5_kernel<64, 2>), dim3(grid),
                           dim3(512), 0, stream, (const bf16*)Q,
                           (const bf16*)K, (const bf16*)Vt, (bf16*)O,
                           (float*)lse, (int)B, (int)H, (int)Hkv, (int)S,
                           (float)scale, (int)causal, sqb, sqs, sqh, skb,
                           sks, skh, (const int*)nullptr);
        break;
    }
    return (int)hipGetLastError();
  }
  if (use_v5) {
    const int grid = (int)(B * H * (S / 256));
#define LAUNCH_V5(F)                                                         \
    hipLaunchKernelGGL((flash_fwd_v5_kernel<128, F>), dim3(grid), dim3(512), \
                       0, stream, (const bf16*)Q, (const bf16*)K,            \
                       (const bf16*)Vt, (bf16*)O, (float*)lse, (int)B,       \
                       (int)H, (int)Hkv, (int)S, (float)scale, (int)causal,  \
                       sqb, sqs, sqh, skb, sks, skh, (const int*)nullptr)
    switch (flags & 7) {
      case 0: LAUNCH_V5(0); break;
      case 1: LAUNCH_V5(1); break;
      case 2: LAUNCH_V5(2); break;
      case 3: LAUNCH_V5(3); break;
      case 6: LAUNCH_V5(6); break;  // defer-max + deep prefetch
      case 7: LAUNCH_V5(7); break;
      default: LAUNCH_V5(2); break;
    }
    return (int)hipGetLastError();
  }
#define LAUNCH_FWD(DD, NW)                                                  \
  hipLaunchKernelGGL((flash_fwd_kernel<DD, NW>), dim3(grid),                \
                     dim3(NW * 64), 0, stream, (const bf16*)Q,              \
                     (const bf16*)K, (const bf16*)Vt, (bf16*)O, (float*)lse,\
                     (int)B, (int)H, (int)Hkv, (int)S, (float)scale,        \
                     (int)causal, sqb, sqs, sqh, skb, sks, skh,              \
                     (const int*)nullptr)
  // measured: 8-wave 128-row tiles were SLOWER (190 vs 205 TF/s —
  // redundant K/V fetches were already L2-absorbed; wider barriers and
  // +3% causal waste cost more than the halved staging saved)
  {
    const int grid = (int)(B * H * (S / 64));
    if (D == 128) LAUNCH_FWD(128, 4); else LAUNCH_FWD(64, 4);
  }
  return (int)hipGetLastError();
}

PRIME_API int prime_attn_delta(hipStream_t stream, const void* dO,
                               const void* O, void* delta, int64_t rows,
                               int64_t D) {
  int grid = prime_grid(rows * 64, 256);
  hipLaunchKernelGGL(attn_delta_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)dO, (const bf16*)O, (float*)delta, rows,
                     (int)D, (const float*)nullptr, (float*)nullptr, 1, 1);
  return (int)hipGetLastError();
}

// delta [B,S,H] as above, plus rowc_t [2][B][H][S] = {lse^T, delta^T}
PRIME_API int prime_attn_delta_t(hipStream_t stream, const void* dO,
                                 const void* O, const void* lse, void* delta,
                                 void* rowc_t, int64_t B, int64_t S, int64_t H,
                                 int64_t D) {
  if (!lse || !rowc_t) return hipErrorInvalidValue;
  const int64_t rows = B * S * H;
  int grid = prime_grid(rows * 64, 256);
  hipLaunchKernelGGL(attn_delta_kernel, dim3(grid), dim3(256), 0, stream,
                     (const bf16*)dO, (const bf16*)O, (float*)delta, rows,
                     (int)D, (const float*)lse, (float*)rowc_t, (int)S, (int)H);
  return (int)hipGetLastError();
}

PRIME_API int prime_flash_bwd_dq(hipStream_t stream, const void* Q,
                                 const void* K, const void* V, const void* Kt,
                                 const void* dO, const void* lse,
                                 const void* delta, void* dQ, int64_t B,
                                 int64_t H, int64_t Hkv, int64_t S, int64_t D,
                                 double scale, int64_t causal,
                                 int64_t sqb, int64_t sqs, int64_t sqh,
                                 int64_t skb, int64_t sks, int64_t skh,
                                 int64_t svb, int64_t svs, int64_t svh,
                                 const void* doc_start) {
  if (S % 64 != 0 || (D != 64 && D != 128)) return hipErrorInvalidValue;
  static const char* v5env = getenv("PRIME_ATTN_V5");
  static const char* flagenv = getenv("PRIME_ATTN_FLAGS");
  const int flags = flagenv ? atoi(flagenv) : 2;
  if (doc_start) {  // document-masked instantiations, default FLAGS
    if (!causal) return hipErrorInvalidValue;
    const bool v5 = (S % 256 == 0) && !(v5env && v5env[0] == '0');
#define LAUNCH_DQ_DOC(KER, QT, NT)                                           \
    hipLaunchKernelGGL(KER, dim3((int)(B * H * (S / QT))), dim3(NT), 0,      \
                       stream, (const bf16*)Q, (const bf16*)K,               \
                       (const bf16*)V, (const bf16*)Kt, (const bf16*)dO,     \
                       (const float*)lse, (const float*)delta, (bf16*)dQ,    \
                       (int)B, (int)H, (int)Hkv, (int)S, (float)scale, 1,    \
                       sqb, sqs, sqh, skb, sks, skh, svb, svs, svh,          \
                       (const int*)doc_start)
    if (v5 && D == 128) LAUNCH_DQ_DOC((flash_bwd_dq_v5_kernel<128, 0, true>), 256, 512);
    else if (v5) LAUNCH_DQ_DOC((flash_bwd_dq_v5_kernel<64, 0, true>), 256, 512);
    else if (D == 128) LAUNCH_DQ_DOC((flash_bwd_dq_kernel<128, true>), 64, 256);
    else LAUNCH_DQ_DOC((flash_bwd_dq_kernel<64, true>), 64, 256);
    return (int)hipGetLastError();
  }
  if ((D == 64) && (S % 256 == 0) && !(v5env && v5env[0] == '0')) {
    const int grid = (int)(B * H * (S / 256));
    hipLaunchKernelGGL((flash_bwd_dq_v5_kernel<64, 0>), dim3(grid),
                       dim3(512), 0, stream, (const bf16*)Q, (const bf16*)K,
                       (const bf16*)V, (const bf16*)Kt, (const bf16*)dO,
                       (const float*)lse, (const float*)delta, (bf16*)dQ,
                       (int)B, (int)H, (int)Hkv, (int)S, (float)scale,
                       (int)causal, sqb, sqs, sqh, skb, sks, skh,
                       svb, svs, svh, (const int*)nullptr);
    return (int)hipGetLastError();
  }
  if ((D == 128) && (S % 256 == 0) && !(v5env && v5env[0] == '0')) {
    const int grid = (int)(B * H * (S / 256));
#define LAUNCH_DQ5(F)                                                       \
    hipLaunchKernelGGL((flash_bwd_dq_v5_kernel<128, F>), dim3(grid),        \
                       dim3(512), 0, stream, (const bf16*)Q,                \
                       (const bf16*)K, (const bf16*)V, (const bf16*)Kt,     \
                       (const bf16*)dO, (const float*)lse,                  \
                       (const float*)delta, (bf16*)dQ, (int)B, (int)H,      \
                       (int)Hkv, (int)S, (float)scale, (int)causal,         \
                       sqb, sqs, sqh, skb, sks, skh, svb, svs, svh,         \
                       (const int*)nullptr)
    if (flags & 1) LAUNCH_DQ5(1); else LAUNCH_DQ5(0);
    return (int)hipGetLastError();
  }
  const int grid = (int)(B * H * (S / 64));
  DISPATCH_D(flash_bwd_dq_kernel, (const bf16*)Q, (const bf16*)K,
             (const bf16*)V, (const bf16*)Kt, (const bf16*)dO,
             (const float*)lse, (const float*)delta, (bf16*)dQ, (int)B, (int)H,
             (int)Hkv, (int)S, (float)scale, (int)causal, sqb, sqs, sqh, skb,
             sks, skh, svb, svs, svh, (const int*)nullptr);
  return (int)hipGetLastError();
}

static bool dkv_v5_selected(bool doc, int64_t D, int64_t S) {
  static const char* v5denv = getenv("PRIME_ATTN_DKV5");
  return !doc && (D == 128) && (S % 256 == 0) && (v5denv && v5denv[0] == '1');
}

static bool dkv_nw8(int64_t S) {
  static const char* nw8env = getenv("PRIME_ATTN_DKV8");
  return (S % 128 == 0) && !(nw8env && nw8env[0] == '0');
}

// dK/dV mode selection, the one place it is decided: 1 = direct output
// (one block per k-tile, or per causal pair of k-tiles; bf16 dK/dV stored
// by the kernel, no workspace), 0 = grid-split q loop with fp32 partials
// and dkv_reduce_kernel. A block's stage images take more than half the
// LDS, so one block runs per CU: direct mode is used when its grid has at
// least one block for every CU, and the split path — which exists to
// make more, shorter blocks — otherwise (e.g. B=1). The callers size
// their workspace by this answer. PRIME_ATTN_DKV_DIRECT=1 / =0 forces
// either mode (read on every call, so one process can A/B them).
PRIME_API int prime_flash_bwd_dkv_direct(int64_t B, int64_t Hkv, int64_t S,
                                         int64_t D, int64_t causal,
                                         int64_t has_doc) {
  if (dkv_v5_selected(has_doc != 0, D, S)) return 0;  // opt-in kernel: split only
  const char* env = getenv("PRIME_ATTN_DKV_DIRECT");
  if (env && env[0] == '1') return 1;
  if (env && env[0] == '0') return 0;
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0)
      n = 256;
    n_cu = n;
  }
  const int64_t n_kt = S / (dkv_nw8(S) ? 128 : 64);
  const int64_t blocks = B * Hkv * (causal ? (n_kt + 1) / 2 : n_kt);
  return blocks >= n_cu ? 1 : 0;
}

PRIME_API int prime_flash_bwd_dkv(hipStream_t stream, const void* Q,
                                  const void* Qt, const void* K, const void* V,
                                  const void* dO, const void* dOt,
                                  const void* lse, const void* delta,
                                  const void* rowc, void* dK,
                                  void* dV, void* wsK, void* wsV,
                                  int64_t splits, int64_t B, int64_t H,
                                  int64_t Hkv, int64_t S, int64_t D,
                                  double scale, int64_t causal,
                                  int64_t sqb, int64_t sqs, int64_t sqh,
                                  int64_t skb, int64_t sks, int64_t skh,
                                  int64_t svb, int64_t svs, int64_t svh,
                                  const void* doc_end) {
  if (S % 64 != 0 || (D != 64 && D != 128)) return hipErrorInvalidValue;
  if (doc_end && !causal) return hipErrorInvalidValue;
  // 8-wave blocks: one q/do/qt/dot stage feeds 128 k-rows (half the
  // staging traffic of the 4-wave version); fall back to 4 waves when the
  // sequence doesn't tile by 128
  // 32x32 swapped dkv measured SLOWER than the 16x16 split-q kernel
  // (160 vs 228 TF: the loop-invariant K/V row fragments don't fit the
  // register budget, and demoting them to inline L2 loads puts ~16 global
  // loads in every q-step's MFMA dependency chain). Opt-in for further
  // work via PRIME_ATTN_DKV5=1; see profiles/10b_1gpu_profile.md.
  static const char* fenv = getenv("PRIME_ATTN_FLAGS");
  const int flags = fenv ? atoi(fenv) : 2;
  const bool direct =
      prime_flash_bwd_dkv_direct(B, Hkv, S, D, causal, doc_end != nullptr) != 0;
  if (splits < 1) return hipErrorInvalidValue;
  // direct mode parks its running sum in one slice of workspace when the
  // q loop is walked in more than one slice
  if ((!direct || splits > 1) && (!wsK || !wsV)) return hipErrorInvalidValue;
  // the opt-in 32x32 kernel has no document mask: masked calls use the
  // 16x16 kernel whatever the env var says
  if (dkv_v5_selected(doc_end != nullptr, D, S)) {
    const int sp = (int)(splits > 4 ? 4 : splits);
    const int grid = (int)(B * Hkv * (S / 256) * sp);
#define LAUNCH_DKV5(F)                                                       \
    hipLaunchKernelGGL((flash_bwd_dkv_v5_kernel<128, F>), dim3(grid),        \
                       dim3(512), 0, stream, (const bf16*)Q,                 \
                       (const bf16*)Qt, (const bf16*)K, (const bf16*)V,      \
                       (const bf16*)dO, (const bf16*)dOt,                    \
                       (const float*)lse, (const float*)delta, (float*)wsK,  \
                       (float*)wsV, (int)B, (int)H, (int)Hkv, (int)S,        \
                       (float)scale, (int)causal, sp, sqb, sqs, sqh,         \
                       skb, sks, skh, svb, svs, svh)
    if (flags & 1) LAUNCH_DKV5(1); else LAUNCH_DKV5(0);
    int err5 = hipGetLastError();
    if (err5) return err5;
    int rgrid5 = prime_grid(B * Hkv * S * D, 256);
    hipLaunchKernelGGL(dkv_reduce_kernel, dim3(rgrid5), dim3(256), 0, stream,
                       (const float*)wsK, (const float*)wsV, (bf16*)dK,
                       (bf16*)dV, (int)B, (int)Hkv, (int)S, (int)D, sp);
    return (int)hipGetLastError();
  }
  if (!rowc) return hipErrorInvalidValue;
  const bool nw8 = dkv_nw8(S);
  // blocks per (b, kv head): k-tiles, or causal pairs of them when direct
  const int64_t n_kt = S / (nw8 ? 128 : 64);
  const int64_t per_bh = (direct && causal) ? (n_kt + 1) / 2 : n_kt;
#define LAUNCH_DKV(DD, NWV, DB) LAUNCH_DKV_(DD, NWV, DB, false, nullptr)
#define LAUNCH_DKV_DOC(DD, NWV, DB) LAUNCH_DKV_(DD, NWV, DB, true, doc_end)
#define LAUNCH_DKV_(DD, NWV, DB, DOCV, DOCP)                                 \
    hipLaunchKernelGGL((flash_bwd_dkv_kernel<DD, NWV, DB, DOCV>),            \
                       dim3((int)(B * Hkv * per_bh * (direct ? 1 : splits))), \
                       dim3(NWV * 64), 0, stream, (const bf16*)Q,            \
                       (const bf16*)Qt, (const bf16*)K, (const bf16*)V,      \
                       (const bf16*)dO, (const bf16*)dOt,                    \
                       (const float*)rowc, (float*)wsK, (float*)wsV,         \
                       (bf16*)dK, (bf16*)dV, (int)B, (int)H, (int)Hkv,       \
                       (int)S, (float)scale, (int)causal, (int)splits,       \
                       (int)direct, sqb, sqs, sqh, skb, sks, skh, svb, svs,  \
                       svh, (const int*)DOCP)
  static const char* dbenv = getenv("PRIME_ATTN_DKV_DBUF");
  const bool dbuf = !(dbenv && dbenv[0] == '0');
  if (doc_end) {
    if (nw8 && dbuf) {
      if (D == 128) LAUNCH_DKV_DOC(128, 8, 2); else LAUNCH_DKV_DOC(64, 8, 2);
    } else if (nw8) {
      if (D == 128) LAUNCH_DKV_DOC(128, 8, 1); else LAUNCH_DKV_DOC(64, 8, 1);
    } else {
      if (D == 128) LAUNCH_DKV_DOC(128, 4, 1); else LAUNCH_DKV_DOC(64, 4, 1);
    }
  } else if (nw8 && dbuf) {
    if (D == 128) LAUNCH_DKV(128, 8, 2); else LAUNCH_DKV(64, 8, 2);
  } else if (nw8) {
    if (D == 128) LAUNCH_DKV(128, 8, 1); else LAUNCH_DKV(64, 8, 1);
  } else {
    if (D == 128) LAUNCH_DKV(128, 4, 1); else LAUNCH_DKV(64, 4, 1);
  }
  int err = hipGetLastError();
  if (err || direct) return err;
  int rgrid = prime_grid(B * Hkv * S * D, 256);
  hipLaunchKernelGGL(dkv_reduce_kernel, dim3(rgrid), dim3(256), 0, stream,
                     (const float*)wsK, (const float*)wsV, (bf16*)dK,
                     (bf16*)dV, (int)B, (int)Hkv, (int)S, (int)D, (int)splits);
  return (int)hipGetLastError();
}
