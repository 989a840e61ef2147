// Flash attention (causal/non-causal, GQA) for gfx950 — MFMA
// v_mfma_f32_16x16x32_bf16 tiles, online softmax, FA2-style split backward
// (dQ q-outer; dK/dV kv-outer, direct bf16 output or a grid-split q loop
// with fp32 partial workspaces). Forward and dQ also have 8-wave 32x32
// swapped-operand kernels ("v5"), taken when S % 256 == 0. Variants that
// measured slower are recorded in docs/KERNELS.md, not kept here.
//
// Design (profiled v1 at ~70 TF: redundant per-wave global reads and
// unswizzled LDS dominated; measured after fixes: fwd ~240 TF / bwd ~168
// TF at the 10B shape):
//  - K/V(+transposed) tiles are staged COOPERATIVELY once per block with
//    __builtin_amdgcn_global_load_lds width-16 (no VGPR round trip), with
//    the T2 XOR-16B swizzle applied via the pre-swizzled SOURCE address
//    (global_load_lds writes linearly: guide §5.5 T2 + rule 21).
//  - all operand-fragment LDS reads are ld8 (16 B) at the swizzled address,
//    conflict-free under the gfx950 rule (64 banks, 16-lane groups: see
//    swz16 below).
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
#include <type_traits>

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

// ---- swizzled-tile helpers --------------------------------------------
// A [ROWS][COLS] bf16 tile lives linearly in LDS; byte (row, colb) is
// stored at row*COLS*2 + (colb ^ swz16<COLS>(row)). Stage from a strided
// global matrix; read 8-element fragments at the same swizzle.
//
// gfx950 LDS: 64 banks x 4 B, i.e. sixteen 16-byte slots per 256-byte
// line. A ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15,
// 20-27}, {4-11, 16-19, 28-31}, the same two + 32), one LDS cycle per
// group when its 16 lanes hit 16 distinct slots; N lanes on one slot cost
// N cycles — 2-way is NOT free for these reads. The XOR is therefore the
// index of the row's 256-byte line (mod the row's chunk count): row & 15
// for 256-byte rows, (row >> 1) & 7 for 128-byte rows, where two rows
// share a line and the row's parity already picks the half. Every operand
// read of the kernels below is then conflict-free, and the 4-byte P/dS
// stores are at most 2-way (free for ds_write_b32):
// tests/test_attn_swizzle_cpu.py walks each pattern.
template <int COLS>
__device__ __forceinline__ int swz16(int row) {
  static_assert(COLS == 64 || COLS == 128, "128- or 256-byte rows");
  return (COLS == 128 ? (row & 15) : ((row >> 1) & 7)) << 4;
}

// One 16-byte-per-lane LDS-DMA load that the compiler does not track. The
// builtin form is a pending LDS write in hipcc's wait bookkeeping, so the
// first ds_read after it gets an s_waitcnt vmcnt(0) even when it reads
// another buffer, and a prefetch issued behind the barrier lands before
// the tile's compute starts instead of under it. From inline assembly the
// load is invisible to that bookkeeping: nothing waits for it but the
// stage_wait_all() the double-buffered loops place in front of their
// tile-boundary barrier. M0 (the wave-uniform LDS destination) is
// compiler-reserved, so it is saved, set and restored in one statement.
__device__ __forceinline__ void glds16_untracked(const bf16* src, lds_char* dst) {
  const unsigned m0v = (unsigned)__builtin_amdgcn_readfirstlane(
      (int)(__UINTPTR_TYPE__)dst);
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(m0v)
      : "memory");
}

// s_waitcnt vmcnt(0): every load this wave issued, LDS-DMA included, has
// landed. As a builtin (not asm) the compiler's own bookkeeping sees it.
// gfx9 encoding: vmcnt = imm[15:14]:imm[3:0], expcnt and lgkmcnt left open.
__device__ __forceinline__ void stage_wait_all() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

// UNTRACKED: for the double-buffered loops. Their contract, per buffer:
// written only after the barrier that ends its last read; read only after
// every issuing wave's stage_wait_all() and the barrier that follows it.
template <int ROWS, int COLS, int NT = 256, bool UNTRACKED = false>
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
    const int colb = ((u % UPR) * 16) ^ swz16<COLS>(row);  // pre-swizzle src
    const bf16* src = gbase + (int64_t)row * row_stride + colb / 2;
    // linear dest: wave-uniform base + lane*16 (global_load_lds contract)
    const int wid = tid >> 6;
    lds_char* dst = (lds_char*)lds_tile + i * (NT * 16) + wid * 1024;
    if (UNTRACKED)
      glds16_untracked(src, dst);
    else
      __builtin_amdgcn_global_load_lds((g_void*)src, (lds_void*)dst, 16, 0, 0);
  }
}

template <int COLS>
__device__ __forceinline__ short8 ld8_swz(const bf16* lds_tile, int row,
                                          int colb) {
  return *reinterpret_cast<const short8*>(
      reinterpret_cast<const char*>(lds_tile) + row * (COLS * 2) +
      (colb ^ swz16<COLS>(row)));
}

template <int COLS>
__device__ __forceinline__ void st16_swz(bf16* lds_tile, int row, int col,
                                         bf16 v) {
  *reinterpret_cast<bf16*>(reinterpret_cast<char*>(lds_tile) + row * (COLS * 2) +
                           ((col * 2) ^ swz16<COLS>(row))) = v;
}

// two adjacent columns (col even) of one row as one 4-byte store
template <int COLS>
__device__ __forceinline__ void st32_swz(bf16* lds_tile, int row, int col,
                                         unsigned v) {
  *reinterpret_cast<unsigned*>(reinterpret_cast<char*>(lds_tile) + row * (COLS * 2) +
                               ((col * 2) ^ swz16<COLS>(row))) = v;
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
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      f32x4 acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < DS; ++ds)
        acc = mfma16(qf[ds], ld8_swz<D>(k_lds, sub * 16 + li, ds * 64 + lg * 16), acc);
      s[sub] = acc;
    }
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
      // no defer-max here (measured 230 vs 240 TF on MI355X): the per-tile
      // rescale is only 32 muls/lane, cheaper than the added branches
      const float mnew = fmaxf(m[r], tmax);
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
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        o_acc[dt] = mfma16(ld8_swz<64>(p_lds, li, ks * 64 + lg * 16),
                           ld8_swz<64>(vt_lds, dt * 16 + li, ks * 64 + lg * 16),
                           o_acc[dt]);
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
// skipping (T13), cheap P exchange and per-wave causal trip clipping.
// Measured at the 10B shape: defer-max 417 TF vs 387 without; setprio
// around the MFMA clusters (T5) lost 1-3 %; a third stage buffer with a
// counted vmcnt at the tile boundary 401 vs 417 — taken while the
// compiler's own vmcnt(0) still drained every prefetch in front of the
// tile's first read (see glds16_untracked), so it settles nothing now.
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

// the value of lane l^1 (DPP quad_perm [1,0,3,2]; every lane active)
__device__ __forceinline__ unsigned lane_xor1(unsigned x) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, 0xB1, 0xF, 0xF, false);
}

template <int D, bool DOC = false>
__global__ __launch_bounds__(512, 2) void flash_fwd_v5_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ Vt, bf16* __restrict__ O, float* __restrict__ lse,
    int B, int H, int Hkv, int S, float scale, int causal,
    int64_t sqb, int64_t sqs, int64_t sqh,
    int64_t skb, int64_t sks, int64_t skh,
    const int* __restrict__ doc) {
  constexpr int DSL = D / 16;   // 16-wide d slices for the K dim
  constexpr int DT32 = D / 32;  // 32-wide output d tiles
  // untracked stage loads, except where they cost a wave per SIMD (the
  // masked D = 64 instantiation went from 128 to 145 VGPRs with them)
  constexpr bool UT = !(DOC && D == 64);
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

  __shared__ bf16 k_lds[2][64 * D];
  __shared__ bf16 vt_lds[2][D * 64];
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
  stage_tile<64, D, 512, UT>(Kb + (int64_t)kv_begin * sks, sks, k_lds[0], threadIdx.x);
  stage_tile<D, 64, 512, UT>(Vtb + kv_begin, S, vt_lds[0], threadIdx.x);
  int idx = 0;
  for (int kv = kv_begin, kt = 0; kv < kv_end; kv += 64, ++kt) {
    idx = kt % 2;
    // tile boundary, reached on every path (the skips below included): this
    // wave's share of tile kt has landed; behind the barrier everyone's
    // has, and tile kt-1 is consumed
    stage_wait_all();
    __syncthreads();
    if (kv + 64 < kv_end) {
      // prefetch-behind-barrier: untracked loads, so no wait stands
      // between here and the next tile boundary — they get the whole
      // tile's compute to land
      stage_tile<64, D, 512, UT>(Kb + (int64_t)(kv + 64) * sks, sks,
                                 k_lds[(kt + 1) % 2], threadIdx.x);
      stage_tile<D, 64, 512, UT>(Vtb + kv + 64, S, vt_lds[(kt + 1) % 2],
                                 threadIdx.x);
    }
    if (kv >= my_kv_end) continue;  // fully-masked tile for this wave
    if (DOC && kv < my_kv_begin) continue;  // before this wave's documents

    // ---- St = (K q^T): two 32x32 C tiles over the 64-key block
    // The K fragments run RING reads ahead of the MFMAs that use them, in
    // registers of their own, so that no MFMA waits on a read issued
    // right in front of it (same products, same order).
    f32x16 st[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) st[t][r] = 0.f;
    {
      constexpr int NF = 2 * DSL, RING = 4;
      short8 kf[RING];
#pragma unroll
      for (int i = 0; i < RING; ++i)
        kf[i] = ld8_swz<D>(k_lds[idx], (i / DSL) * 32 + lo, (i % DSL) * 32 + hi * 16);
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        st[i / DSL] = mfma32(kf[i % RING], qf[i % DSL], st[i / DSL]);
        if (i + RING < NF)
          kf[i % RING] = ld8_swz<D>(k_lds[idx], ((i + RING) / DSL) * 32 + lo,
                                    ((i + RING) % DSL) * 32 + hi * 16);
      }
      // pin that order: hipcc's scheduler otherwise sinks every read back
      // in front of its MFMA (0x100 = DS read, 0x008 = MFMA)
      __builtin_amdgcn_sched_group_barrier(0x100, RING, 0);
#pragma unroll
      for (int i = 0; i < NF - RING; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, RING, 0);
    }
    // ---- online softmax: st[t][r] is k = kv + t*32 + crow(r,hi) for
    // q row q0w+lo; lane pair (l, l^32) splits the row's 64 scores
    float tmax = NEG_INF;
    if (DOC && kv < my_ds_last) {  // wave-uniform: a boundary tile
      // a row still wholly masked keeps m_run = NEG_INF through the
      // per-wave rescale below (alpha = exp(0) = 1 on o = l = 0) and
      // p = 0 through m_sub below, so nothing leaks
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kg = kv + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (kg < my_ds) st[t][r] = NEG_INF;
        }
    }
    if (causal && kv + 63 > q0w) {  // wave-uniform: the diagonal tile
      // the only computed tile that can hold a key past a row of this
      // wave: later tiles are skipped above, earlier ones end at or
      // before q0w
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kg = kv + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (kg > q0w + lo) st[t][r] = NEG_INF;
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, st[t][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    // defer-max (guide T13): skip the O-wide rescale while the running
    // max still bounds P by e^THR (fp32 accumulation tolerates it)
    const float thr = 8.f;
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
    // A masked score needs no select of its own: once a row has seen one
    // visible key m_run is finite, and exp(NEG_INF - m_run) is 0 by
    // itself. Without a document mask that holds from the first computed
    // tile on (it holds key 0, or every key when not causal). With one, a
    // row can reach a tile before its document starts with m_run still
    // NEG_INF; all its scores there are NEG_INF too, so subtracting 0 in
    // place of m_run gives the same 0. (An unmasked score at or below
    // NEG_INF would need |q.k| >= 1e30.)
    float m_sub = m_run;
    if (DOC && m_run <= NEG_INF) m_sub = 0.f;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pv = __expf(st[t][r] - m_sub);
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
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        o_acc[dt] = mfma32(pa[ks],
                           ld8_swz<64>(vt_lds[idx], dt * 32 + lo, ks * 32 + hi * 16),
                           o_acc[dt]);
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

// ----------------------------- delta, row constants and dO^T in one pass
// One block per (b, 64-token tile, h), h fastest so that neighbouring
// blocks read neighbouring 2*D-byte rows. dO and O are read once, in
// 16-byte loads; a row is spread over D/8 adjacent lanes. dO goes through a
// padded LDS tile and leaves as dOt [B,H,D,S] in 16-byte stores (as
// transpose_bshd_kernel does it); lse^T and delta^T leave as 64 consecutive
// floats each; delta [B,S,H] is still written for the dQ kernels.
//
// delta has the bits of attn_delta_kernel. There lane L of a wave holds
// p_L = dO[2L]*O[2L] + dO[2L+1]*O[2L+1] (zero for 2L >= D) and
// wave_reduce_sum pairs L with L+32, L+16, ..., L+1. Here lane m of a row
// holds p_{4m..4m+3}, so the same tree is: m with m+8 (at D = 64: with the
// zeros of the absent upper half), m+4, m+2, m+1 component by component,
// then components {0,2} and {1,3}, then those two.
template <int D>
__global__ __launch_bounds__(256) void attn_delta_dot_kernel(
    const bf16* __restrict__ dO, const bf16* __restrict__ O,
    const float* __restrict__ lse, float* __restrict__ delta,
    float* __restrict__ rowc_t, bf16* __restrict__ dOt, int S, int H,
    int64_t rows) {
  constexpr int LPR = D / 8;      // lanes per row
  constexpr int RPP = 256 / LPR;  // rows per pass
  constexpr int NP = 64 / RPP;    // passes over the 64-row tile
  constexpr int TPD = D + 8;      // padded LDS row, keeps 16-byte alignment
  __shared__ __attribute__((aligned(16))) bf16 tile[64][TPD];
  __shared__ float sdelta[64];
  int idx = blockIdx.x;
  const int h = idx % H; idx /= H;
  const int n_st = S / 64;
  const int st = idx % n_st;
  const int b = idx / n_st;
  const int t = threadIdx.x;
  const int m = t % LPR, rr = t / LPR;
  const int64_t tok0 = (int64_t)b * S + st * 64;   // first token of the tile
  const int64_t tcol = ((int64_t)b * H + h) * S + st * 64;  // same, [B,H,S]

  short8 vdo[NP], vo[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int64_t off = ((tok0 + p * RPP + rr) * H + h) * D + m * 8;
    vdo[p] = *reinterpret_cast<const short8*>(dO + off);
    vo[p] = *reinterpret_cast<const short8*>(O + off);
  }
  float lv = 0.f;
  if (t >= 64 && t < 128) lv = lse[(tok0 + (t - 64)) * H + h];

#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int row = p * RPP + rr;
    *reinterpret_cast<short8*>(&tile[row][m * 8]) = vdo[p];
    const bf16* a = reinterpret_cast<const bf16*>(&vdo[p]);
    const bf16* c = reinterpret_cast<const bf16*>(&vo[p]);
    float q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float acc = 0.f;
      acc += bf2f(a[2 * i]) * bf2f(c[2 * i]);
      acc += bf2f(a[2 * i + 1]) * bf2f(c[2 * i + 1]);
      q[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (D == 64) q[i] = q[i] + 0.f;
      else q[i] += __shfl_down(q[i], 8, 64);
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1)
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] += __shfl_down(q[i], off, 64);
    if (m == 0) sdelta[row] = (q[0] + q[2]) + (q[1] + q[3]);
  }
  __syncthreads();
  if (t < 64) {
    const float d = sdelta[t];
    delta[(tok0 + t) * H + h] = d;
    rowc_t[rows + tcol + t] = d;
  } else if (t < 128) {
    rowc_t[tcol + (t - 64)] = lv;
  }
  // dOt rows d = 0..D-1, 64 tokens each: D*8 16-byte units
  bf16* dbase = dOt + ((int64_t)b * H + h) * D * S + st * 64;
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int u = i * 256 + t;
    const int d = u >> 3, s8 = (u & 7) * 8;
    short8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      reinterpret_cast<short*>(&v)[j] =
          reinterpret_cast<const short*>(&tile[s8 + j][d])[0];
    *reinterpret_cast<short8*>(dbase + (int64_t)d * S + s8) = v;
  }
}

// ------------------------------------------------ backward dQ v5 (32x32)
// Same 8-wave swapped-operand structure as the v5 forward: St = K·Q^T and
// dPt = V·dO^T give lane-local q-rows (q = lane&31), so lse/delta are one
// scalar per lane and dS never touches LDS — it is packed straight into
// the dQ-accumulation A-fragments with cvt_pk + permlane32_swap.
template <int D, bool DOC = false>
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
  // score-loop fragments in registers, and untracked stage loads: what
  // each instantiation's register class allows (a deeper ring spills at
  // D = 128; the masked ones lose a wave per SIMD at D = 64 or spill at
  // D = 128 with untracked loads or a pinned ring)
  constexpr int DQ_RING = (D == 128 || DOC) ? 2 : 3;
  constexpr bool UT = !DOC;
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
  stage_tile<64, D, 512, UT>(Kb + (int64_t)kv_begin * sks, sks, k_lds[0], threadIdx.x);
  stage_tile<64, D, 512, UT>(Vb + (int64_t)kv_begin * svs, svs, v_lds[0], threadIdx.x);
  stage_tile<D, 64, 512, UT>(Ktb + kv_begin, S, kt_lds[0], threadIdx.x);
  int idx = 0;
  for (int kv = kv_begin; kv < kv_end; kv += 64, idx ^= 1) {
    // tile boundary as in the v5 forward: own stage landed, then barrier,
    // on every path; the untracked prefetch then flies under the compute
    stage_wait_all();
    __syncthreads();
    if (kv + 64 < kv_end) {
      stage_tile<64, D, 512, UT>(Kb + (int64_t)(kv + 64) * sks, sks,
                                 k_lds[idx ^ 1], threadIdx.x);
      stage_tile<64, D, 512, UT>(Vb + (int64_t)(kv + 64) * svs, svs,
                                 v_lds[idx ^ 1], threadIdx.x);
      stage_tile<D, 64, 512, UT>(Ktb + kv + 64, S, kt_lds[idx ^ 1], threadIdx.x);
    }
    if (kv >= my_kv_end) continue;
    if (DOC && kv < my_kv_begin) continue;

    // ---- St = K·Q^T (pre-scaled), dPt = V·dO^T: C[k][q], q = lo
    // The K and V fragments, taken alternately, run RING - 1 reads ahead
    // of the MFMAs that use them, as in the v5 forward (same products,
    // same order). RING is what the register file allows: see the table
    // in docs/KERNELS.md.
    f32x16 st[2], dpt[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) { st[t][r] = 0.f; dpt[t][r] = 0.f; }
    {
      constexpr int NF = 4 * DSL, RING = DQ_RING;
      // fragment j: K (j even) or V (j odd), row block (j/2)/DSL, slice (j/2)%DSL
      const auto frag = [&](int j) {
        const bf16* tile = (j & 1) ? v_lds[idx] : k_lds[idx];
        return ld8_swz<D>(tile, ((j / 2) / DSL) * 32 + lo, ((j / 2) % DSL) * 32 + hi * 16);
      };
      short8 f[RING];
#pragma unroll
      for (int j = 0; j < RING; ++j) f[j] = frag(j);
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int t = (j / 2) / DSL, ds = (j / 2) % DSL;
        if (j & 1) dpt[t] = mfma32(f[j % RING], dof[ds], dpt[t]);
        else st[t] = mfma32(f[j % RING], qf[ds], st[t]);
        if (j + RING < NF) f[j % RING] = frag(j + RING);
      }
      if (!DOC) {
        __builtin_amdgcn_sched_group_barrier(0x100, RING, 0);
#pragma unroll
        for (int j = 0; j < NF - RING; ++j) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, RING, 0);
      }
    }
    // ---- causal mask, on the wave's diagonal tile only (wave-uniform; no
    // other computed tile holds a key past one of its rows). A masked
    // score becomes NEG_INF, and exp(NEG_INF - lse) is the same +0 the
    // select on p gave: lse is finite, every row sees its own key. The
    // document-mask instantiation keeps both selects inline on every tile:
    // with this branch it needs 256 VGPRs plus scratch at D = 128 and
    // loses a wave per SIMD at D = 64.
    if (!DOC && causal && kv + 63 > q0w) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kg = kv + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (kg > q0w + lo) st[t][r] = NEG_INF;
        }
    }
    // ---- dS = P * (dP - delta) * scale, all in-register (q = lo)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kg = kv + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        float p = __expf(st[t][r] - lse_q);
        if (DOC && causal && kg > q0w + lo) p = 0.f;
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
#pragma unroll
    for (int dt = 0; dt < DT32; ++dt)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        dq_acc[dt] = mfma32(da[ks],
                            ld8_swz<64>(kt_lds[idx], dt * 32 + lo, ks * 32 + hi * 16),
                            dq_acc[dt]);
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

// -------------------------------------------------------- backward dK, dV
// Stages Q[64][D], dO[64][D] (operands of the score and dP products),
// Qt[D][64] and dOt[D][64] (operands of the dK and dV accumulation).
//
// Tile body: St = mfma16(kf, qb) leaves the key on the accumulator row, so
// each wave passes P and dS through its own LDS buffers (4-byte swizzled
// stores of column pairs, a wave-local fence, 16-byte reads) to get them
// key-on-the-lane for dV += P^T·dO and dK += dS^T·Q. At NW=8, D=128,
// DBUF=2 that is 2x4x16 KiB stages + 8x2x2 KiB wave buffers = exactly the
// 160 KiB LDS limit. acc[dt][r] = [k0 + lg*4 + r][dt*16 + li]. Keeping P and dS in
// registers instead (key on the lane from the start) and a 32x32 variant
// both measured slower: docs/KERNELS.md.
//
// lse/delta come from the [B,H,S] copies attn_delta_kernel writes (rowc =
// {lse_t, delta_t}): the 16 lanes of a group read 16 consecutive floats.
//
// Two shapes are instantiated: NW=8, DBUF=2 for S % 128 == 0 — one stage
// feeds 128 k-rows, double-buffered with prefetch-behind-barrier (one
// barrier per q-tile, untracked stage loads and one vmcnt(0) in front of
// it) — and NW=4, DBUF=1 for the other S % 64 == 0.
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
template <int D, int NW, int DBUF, bool DOC>  // NW waves x 16 k-rows
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
  static_assert((NW == 8 && DBUF == 2) || (NW == 4 && DBUF == 1),
                "only the two measured dK/dV shapes are built");
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
  __shared__ bf16 pt_lds_all[NW][16 * 64];
  __shared__ bf16 dst_lds_all[NW][16 * 64];
  bf16* pt_lds = pt_lds_all[wid];
  bf16* dst_lds = dst_lds_all[wid];

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
  // my_q_end is the same for this wave's last key; key_end4 masks this
  // lane's four keys (accumulator rows k0 + lg*4 + r).
  int q_end = S, my_q_end = S, key_end4[4] = {S, S, S, S};
  if (DOC) {
    const int* de_b = doc_end + (int64_t)b * S;
    q_end = (doc_clamp(de_b[kt * (NW * 16) + NW * 16 - 1], S) + 63) & ~63;
    my_q_end = doc_clamp(de_b[k0 + 15], S);
#pragma unroll
    for (int r = 0; r < 4; ++r) key_end4[r] = doc_end[(int64_t)b * S + k0 + lg * 4 + r];
  }
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
    // DBUF == 2: untracked loads, waited for at the tile boundary only
    constexpr bool UT = DBUF == 2;
    stage_tile<64, D, NW * 64, UT>(Qb_ + (int64_t)q0g_ * sqs, sqs, q_lds[buf], threadIdx.x);
    stage_tile<64, D, NW * 64, UT>(dOb_ + (int64_t)q0g_ * H * D, (int64_t)H * D, do_lds[buf], threadIdx.x);
    stage_tile<D, 64, NW * 64, UT>(Qtb_ + q0g_, S, qt_lds[buf], threadIdx.x);
    stage_tile<D, 64, NW * 64, UT>(dOtb_ + q0g_, S, dot_lds[buf], threadIdx.x);
  };
  // DBUF == 2: the lse/delta of q-tile it+1 (this lane's query of each 16-
  // row sub) are loaded one tile ahead, issued in front of that tile's
  // stage and waited for with it at the tile boundary, so no wait for
  // them stands behind the LDS-DMA (vmcnt retires in order: waiting for a
  // load issued after the stage would wait for the whole stage).
  float lse_nx[4], dl_nx[4], lse_c[4], dl_c[4];
  const auto load_rowc = [&](int it) {
    const int g_ = it / tiles_per_g;
    const int q0g_ = q_start + (it - g_ * tiles_per_g) * 64 * splits;
    const int64_t o_ = (int64_t)(hkv * group + g_) * S + q0g_ + li;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      lse_nx[sub] = lse_t[o_ + sub * 16];
      dl_nx[sub] = dl_t[o_ + sub * 16];
    }
  };
  if (DBUF == 2 && n_iter > 0) {
    load_rowc(0);
    stage_it(0, 0);
  }
  for (int it = 0; it < n_iter; ++it) {
    const int g = it / tiles_per_g;
    const int q0g = q_start + (it - g * tiles_per_g) * 64 * splits;
    const int cur = (DBUF == 2) ? (it & 1) : 0;
    {
      // DBUF == 2, tile boundary on every path (the skip below included):
      // this wave's share of tile `it` has landed, then the barrier
      if (DBUF == 2) stage_wait_all();
      __syncthreads();
      if (DBUF == 2) {
        // prefetch-behind-barrier: the next tile's untracked loads land
        // under this tile's compute; nothing waits for them before the
        // next tile boundary
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
          lse_c[sub] = lse_nx[sub];
          dl_c[sub] = dl_nx[sub];
        }
        if (it + 1 < n_iter) {
          load_rowc(it + 1);
          stage_it(it + 1, cur ^ 1);
        }
      } else {
        stage_it(it, 0);
        __syncthreads();
      }
      // per-wave causal clip: this wave's k-rows start at k0, so q-tiles
      // entirely below the diagonal are fully masked — skip their
      // compute (the wave still co-staged and hits the next barrier)
      const bool skip = (causal && q0g + 64 <= k0) || (DOC && q0g >= my_q_end);
      if (skip) continue;
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
        const float lse_q = (DBUF == 2) ? lse_c[sub] : lse_t[o];
        const float dl_q = (DBUF == 2) ? dl_c[sub] : dl_t[o];
        float pv[4], dsv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __expf(st_acc[r] * scale - lse_q);
          if (causal && k0 + lg * 4 + r > qg) p = 0.f;
          if (DOC && qg >= key_end4[r]) p = 0.f;
          pv[r] = p;
          dsv[r] = p * (dpt_acc[r] - dl_q) * scale;
        }
        // Lanes li and li^1 hold adjacent query columns of the same four
        // key rows. The even lane hands over rows 2-3 and takes rows 0-1
        // of the pair's two columns, the odd lane the reverse, so each
        // lane stores two 4-byte column pairs per buffer where it stored
        // four bf16: the same bytes at the same swizzled addresses (the
        // XOR moves 16-byte units, a column pair stays together).
        const unsigned p01 = cvt_pk_bf16(pv[0], pv[1]), p23 = cvt_pk_bf16(pv[2], pv[3]);
        const unsigned d01 = cvt_pk_bf16(dsv[0], dsv[1]), d23 = cvt_pk_bf16(dsv[2], dsv[3]);
        const int odd = li & 1;
        const unsigned pgot = lane_xor1(odd ? p01 : p23);
        const unsigned dgot = lane_xor1(odd ? d01 : d23);
        const unsigned pown = odd ? p23 : p01, down = odd ? d23 : d01;
        // v_perm_b32 byte selectors, 0-3 from own and 4-7 from got: the
        // lower column comes first, and that is the even lane's
        const unsigned sel0 = odd ? 0x01000504u : 0x05040100u;  // first row of the two
        const unsigned sel1 = odd ? 0x03020706u : 0x07060302u;  // second row
        const int prow = lg * 4 + 2 * odd, pcol = sub * 16 + (li & ~1);
        st32_swz<64>(pt_lds, prow, pcol, __builtin_amdgcn_perm(pgot, pown, sel0));
        st32_swz<64>(pt_lds, prow + 1, pcol, __builtin_amdgcn_perm(pgot, pown, sel1));
        st32_swz<64>(dst_lds, prow, pcol, __builtin_amdgcn_perm(dgot, down, sel0));
        st32_swz<64>(dst_lds, prow + 1, pcol, __builtin_amdgcn_perm(dgot, down, sel1));
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
    }
  }
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
// One launch per entry point: the entry point writes its argument list
// once, in the kernel's parameter order, and attn_launch converts each
// argument to the kernel's own parameter type (void* -> bf16*/float*/int*,
// int64_t -> int, double -> float). A pointer passed where the kernel takes
// a number, or the reverse, does not compile.
template <typename To, typename From>
static To kernel_arg(From v) {
  static_assert(std::is_pointer<To>::value == std::is_pointer<From>::value,
                "pointer / scalar mismatch in a kernel argument list");
  return (To)v;
}

template <typename... P, typename... A>
static int attn_launch(void (*kernel)(P...), int64_t grid, int block,
                       hipStream_t stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3((int)grid), dim3(block), 0, stream,
                     kernel_arg<P>(args)...);
  return (int)hipGetLastError();
}

// expands LAUNCH(D, DOC) for the call's head dim and mask; needs `D` and a
// bool `doc` in scope
#define BY_D_DOC(LAUNCH)                                          \
  (D == 128 ? (doc ? LAUNCH(128, true) : LAUNCH(128, false))      \
            : (doc ? LAUNCH(64, true) : LAUNCH(64, false)))

// forward and dQ: the 8-wave 32x32 kernels take 256-row q tiles, so they
// need S % 256 == 0; every other S % 64 == 0 (and PRIME_ATTN_V5=0, for
// A/B) runs the 4-wave 16x16 kernels. Masked and unmasked calls alike.
static bool attn_use_v5(int64_t S) {
  static const char* v5env = getenv("PRIME_ATTN_V5");
  return (S % 256 == 0) && !(v5env && v5env[0] == '0');
}

PRIME_API int prime_flash_fwd(hipStream_t stream, const void* Q, const void* K,
                              const void* Vt, void* O, void* lse, int64_t B,
                              int64_t H, int64_t Hkv, int64_t S, int64_t D,
                              double scale, int64_t causal,
                              int64_t sqb, int64_t sqs, int64_t sqh,
                              int64_t skb, int64_t sks, int64_t skh,
                              const void* doc_start) {
  if (S % 64 != 0 || (D != 64 && D != 128)) return hipErrorInvalidValue;
  const bool doc = doc_start != nullptr;
  if (doc && !causal) return hipErrorInvalidValue;
  // 16x16 kernel: 8-wave 128-row tiles measured SLOWER than 4-wave (190 vs
  // 205 TF/s — redundant K/V fetches were already L2-absorbed; wider
  // barriers and +3% causal waste cost more than the halved staging saved)
  const bool v5 = attn_use_v5(S);
#define FWD(DD, DOCV)                                                        \
  attn_launch(v5 ? flash_fwd_v5_kernel<DD, DOCV>                             \
                 : flash_fwd_kernel<DD, 4, DOCV>,                            \
              B * H * (S / (v5 ? 256 : 64)), v5 ? 512 : 256, stream, Q, K,   \
              Vt, O, lse, B, H, Hkv, S, scale, causal, sqb, sqs, sqh, skb,   \
              sks, skh, doc_start)
  return BY_D_DOC(FWD);
#undef FWD
}

// delta [B,S,H] = rowsum(dO*O), plus rowc_t [2][B][H][S] = {lse^T, delta^T}
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

// The same delta and rowc_t, plus dOt [B,H,D,S] = dO^T, in one pass over
// contiguous dO and O [B,S,H,D] (replaces prime_attn_delta_t followed by a
// transpose of dO).
PRIME_API int prime_attn_delta_dot(hipStream_t stream, const void* dO,
                                   const void* O, const void* lse, void* delta,
                                   void* rowc_t, void* dOt, int64_t B,
                                   int64_t S, int64_t H, int64_t D) {
  if (!dO || !O || !lse || !delta || !rowc_t || !dOt) return hipErrorInvalidValue;
  if (S % 64 != 0 || (D != 64 && D != 128)) return hipErrorInvalidValue;
  const int64_t rows = B * S * H;
  const int64_t grid = B * H * (S / 64);
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  if (grid == 0) return (int)hipSuccess;
  if (D == 64)
    hipLaunchKernelGGL(attn_delta_dot_kernel<64>, dim3((int)grid), dim3(256), 0,
                       stream, (const bf16*)dO, (const bf16*)O,
                       (const float*)lse, (float*)delta, (float*)rowc_t,
                       (bf16*)dOt, (int)S, (int)H, rows);
  else
    hipLaunchKernelGGL(attn_delta_dot_kernel<128>, dim3((int)grid), dim3(256),
                       0, stream, (const bf16*)dO, (const bf16*)O,
                       (const float*)lse, (float*)delta, (float*)rowc_t,
                       (bf16*)dOt, (int)S, (int)H, rows);
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
  const bool doc = doc_start != nullptr;
  if (doc && !causal) return hipErrorInvalidValue;
  const bool v5 = attn_use_v5(S);
#define DQ(DD, DOCV)                                                         \
  attn_launch(v5 ? flash_bwd_dq_v5_kernel<DD, DOCV>                          \
                 : flash_bwd_dq_kernel<DD, DOCV>,                            \
              B * H * (S / (v5 ? 256 : 64)), v5 ? 512 : 256, stream, Q, K,   \
              V, Kt, dO, lse, delta, dQ, B, H, Hkv, S, scale, causal, sqb,   \
              sqs, sqh, skb, sks, skh, svb, svs, svh, doc_start)
  return BY_D_DOC(DQ);
#undef DQ
}

// dK/dV k-tile rows: 8-wave blocks, where one q/do/qt/dot stage feeds 128
// k-rows (half the staging traffic of the 4-wave version), when the
// sequence tiles by 128; 4 waves x 16 rows otherwise
static int64_t dkv_tile_rows(int64_t S) { return (S % 128 == 0) ? 128 : 64; }

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
  const int64_t n_kt = S / dkv_tile_rows(S);
  const int64_t blocks = B * Hkv * (causal ? (n_kt + 1) / 2 : n_kt);
  return blocks >= n_cu ? 1 : 0;
}

PRIME_API int prime_flash_bwd_dkv(hipStream_t stream, const void* Q,
                                  const void* Qt, const void* K, const void* V,
                                  const void* dO, const void* dOt,
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
  const bool doc = doc_end != nullptr;
  if (doc && !causal) return hipErrorInvalidValue;
  const bool direct =
      prime_flash_bwd_dkv_direct(B, Hkv, S, D, causal, doc) != 0;
  if (splits < 1) return hipErrorInvalidValue;
  // direct mode parks its running sum in one slice of workspace when the
  // q loop is walked in more than one slice
  if ((!direct || splits > 1) && (!wsK || !wsV)) return hipErrorInvalidValue;
  if (!rowc) return hipErrorInvalidValue;
  const bool nw8 = dkv_tile_rows(S) == 128;
  // blocks per (b, kv head): k-tiles, or causal pairs of them when direct
  const int64_t n_kt = S / dkv_tile_rows(S);
  const int64_t per_bh = (direct && causal) ? (n_kt + 1) / 2 : n_kt;
#define DKV(DD, DOCV)                                                        \
  attn_launch(nw8 ? flash_bwd_dkv_kernel<DD, 8, 2, DOCV>                     \
                  : flash_bwd_dkv_kernel<DD, 4, 1, DOCV>,                    \
              B * Hkv * per_bh * (direct ? 1 : splits), nw8 ? 512 : 256,     \
              stream, Q, Qt, K, V, dO, dOt, rowc, wsK, wsV, dK, dV, B, H,    \
              Hkv, S, scale, causal, splits, direct, sqb, sqs, sqh, skb,     \
              sks, skh, svb, svs, svh, doc_end)
  int err = BY_D_DOC(DKV);
#undef DKV
  if (err || direct) return err;
  int rgrid = prime_grid(B * Hkv * S * D, 256);
  hipLaunchKernelGGL(dkv_reduce_kernel, dim3(rgrid), dim3(256), 0, stream,
                     (const float*)wsK, (const float*)wsV, (bf16*)dK,
                     (bf16*)dV, (int)B, (int)Hkv, (int)S, (int)D, (int)splits);
  return (int)hipGetLastError();
}
