// siren_x3_common.h — what more than one of the split-bf16 / fp16 FiLM-SIREN kernel families uses (siren_bwd_x3.hip: the fused
// backward; siren_fwd_x3.hip: the points / rays forward and the fused ray-march; siren_sigma_x3.inc, compiled with it: sigma and its gradient):
// the LDS carves and the swizzled image layout, the operand split, the register-chain dense layers with their fragment
// loaders, the weight staging, the sines, and the host helpers of the launchers.  Everything sits in an anonymous namespace:
// each of the three sources is compiled on its own and gets its own copy.
#pragma once
#include "common.h"
#include "../../include/cips3d_hip.h"
#include "raygen.h"
#include <type_traits>
#include <climits>

// wave priority of the forward chain's MFMA phases (probe builds: -DCIPS_X3_PRIO)
#ifdef CIPS_X3_PRIO
#define X3_PRIO(p) __builtin_amdgcn_s_setprio(p)
#else
#define X3_PRIO(p)
#endif

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned char uchar;

constexpr int H = 128, HC = 64, CF = 32;

// ---- LDS carve (bytes) ----
constexpr int O_W1H = 0, O_W1L = 32768;                 // [128 out][128 in] bf16, 256 B rows
constexpr int O_WCH = 65536, O_WCL = 81920;             // [64 out][128 in]
constexpr int O_WFH = 98304, O_WFL = 102400;            // [32 out][64 in], 128 B rows
constexpr int O_L0 = 106496;                            // float4[128]
constexpr int O_G1 = O_L0 + 2048, O_C1 = O_G1 + 512, O_WS = O_C1 + 512;
constexpr int O_GC = O_WS + 512, O_CC = O_GC + 256;
constexpr int O_AUX = O_CC + 256;                        // [128 points][8 bf16] hi plane, then lo plane (2 KiB each)
constexpr int O_STG = O_AUX + 4096;                      // 48 KiB staging
constexpr int STG_BYTES = 49152;
constexpr int SMEM_BYTES = O_STG + STG_BYTES;            // 163840 = the whole LDS of a CU
static_assert(O_AUX == 110592 && SMEM_BYTES == 163840, "LDS carve");
// The sigma-only forward (siren_sigma_x3_kernel) reads the W1 images, the layer-0 packs and G1 / C1 / WS: its own carve puts
// the vectors right behind W1, with the spacing of the carve above (the chain addresses them relative to the layer-0 packs).
constexpr int SG_L0 = O_WCH;                              // float4[128] where the full carve has the Wc image
constexpr int SG_SMEM_BYTES = SG_L0 + (O_GC - O_L0);      // 69120: two workgroups fit a CU's 160 KiB
static_assert(SG_L0 == 65536 && SG_SMEM_BYTES == 69120, "sigma LDS carve");

// A wave's activations in "register-chain" layout (lane = point; tile q, register r <-> feature
// 32q + (r&3) + 8(r>>2) + 4hf), packed to split bf16: dword j of tile q holds registers 2j, 2j+1, so dwords
// 2g, 2g+1 are one 8-byte LDS unit (4 consecutive features) and dwords 4t..4t+3 are the MFMA B operand of
// k-step (q,t).  Plain dword arrays on purpose: arrays of uint2 pairs defeat SROA and end up in scratch.
template <int Q> struct Act { unsigned hi[Q][8], lo[Q][8]; };

__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& lo) {
  f32x2 v = {a, b};
  bf16x2 h = __builtin_convertvector(v, bf16x2);
  hi = __builtin_bit_cast(unsigned, h);
  f32x2 hf = {__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
  f32x2 r = v - hf;
  bf16x2 l = __builtin_convertvector(r, bf16x2);
  lo = __builtin_bit_cast(unsigned, l);
}
// The same split on fp16 planes (x = hi + lo, 11 + 11 mantissa bits: 2^-22 relative where bf16 planes give 2^-17), for
// operands of known range only — the forward chain's activations are sines and its weights are staged with a per-matrix
// power-of-two scale (stage_weights_x3<PRE, true>) — fp16 has 5 exponent bits.  Same instruction count as split2.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split2h(float a, float b, unsigned& hi, unsigned& lo) {
  f32x2 v = {a, b};
  f16x2 h = __builtin_convertvector(v, f16x2);
  hi = __builtin_bit_cast(unsigned, h);
  // residual x - hi in ONE instruction per element: v_fma_mix_f32 reads the fp16 half in place (op_sel picks the half,
  // op_sel_hi marks source 0 as fp16) — hipcc's own code is v_cvt_f32_f16 x2 + v_pk_add_f32 (5 instead of 4 per pair, and
  // a packed-f32 op between MFMAs costs more than its slot, MI355X_MICROARCH.md); it has no builtin and folds
  // fma(-1, fpext(h), x) back into the subtraction.  Plain VALU -> VALU dependencies: no wait states to pad.
  float r0, r1;
  asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hi), "v"(a));
  asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hi), "v"(b));
  f32x2 r = {r0, r1};
  f16x2 l = __builtin_convertvector(r, f16x2);
  lo = __builtin_bit_cast(unsigned, l);
}
template <bool F16>
__device__ __forceinline__ void split2t(float a, float b, unsigned& hi, unsigned& lo) {
  if constexpr (F16) split2h(a, b, hi, lo); else split2(a, b, hi, lo);
}
// Pin packed values where they are computed: hipcc otherwise sinks the whole producing computation into the
// `if (wave == turn)` staging blocks, serialising it across the workgroup's waves.
template <int Q>
__device__ __forceinline__ void pin(Act<Q>& o) {
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) { asm volatile("" : "+v"(o.hi[q][j])); asm volatile("" : "+v"(o.lo[q][j])); }
}
__device__ __forceinline__ bf16x8 mk8(unsigned a, unsigned b, unsigned c, unsigned d) {
  u32x4 v = {a, b, c, d};
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ f32x16 x3(f32x16 acc, bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  return acc;
}
// same pass order on fp16 planes (v_mfma_f32_32x32x16_f16: the bf16 instruction's rate and fragment layout)
__device__ __forceinline__ f32x16 x3h(f32x16 acc, u32x4 ah, u32x4 al, u32x4 bh, u32x4 bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, al), __builtin_bit_cast(f16x8, bh), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, bl), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ah), __builtin_bit_cast(f16x8, bh), acc, 0, 0, 0);
  return acc;
}

// LDS image layout (weights and staging alike): [column/32][row][32 columns] — 64-byte rows of 8 units
// (unit = 4 bf16 = 8 B), column blocks R*64 bytes apart, the unit index XORed with 3 bits of the row:
//   weights  (SH = 2): unit ^ ((row >> 2) & 7)     staging (SH = 1): unit ^ ((row >> 1) & 7)
// Probed on hardware (scripts/probe/lds_layout_probe.hip, SQ_LDS_BANK_CONFLICT = 0 for all three patterns):
//  * ds_read_b64_tr_b16 — a 32-lane group covers 4 rows x 64 B = one 256-B bank row whatever the in-row order;
//  * forward fragments, ds_read_b64 — 32 consecutive rows at one unit: (row & 3) picks the 64-B quarter,
//    (row >> 2) & 7 the unit inside it;
//  * staging stores, ds_write_b64 (16-lane groups, 128-B bank row) — (row & 1) picks the half, (row >> 1) & 7
//    the unit.
// and every fragment address is  lane base + compile-time immediate  (LaneAddr below).
template <int SH> __device__ __forceinline__ int img_addr(int row, int unit, int R) {
  return (unit >> 3) * R * 64 + row * 64 + (((unit & 7) ^ ((row >> SH) & 7)) << 3);
}

// All LDS traffic goes through 32-bit LDS byte addresses (lane base + compile-time constant), so that the
// constant lands in the instruction's 16-bit offset field; arithmetic on generic pointers does not fold.
#define LDS_PTR(T, a) ((__attribute__((address_space(3))) T*)(uintptr_t)(a))
__device__ __forceinline__ uint2 lds_tr(unsigned a) {
  short4v v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(short4v, a));
  return __builtin_bit_cast(uint2, v);
}
// plain 8-byte LDS read that the load/store optimizer must not fuse into ds_read2st64_b64 (half the
// bandwidth and 2-way conflicts on this layout)
__device__ __forceinline__ uint2 lds_b64(unsigned a) {
  const unsigned long long v = *LDS_PTR(const volatile unsigned long long, a);
  return make_uint2((unsigned)v, (unsigned)(v >> 32));
}
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void lds_st64(unsigned a, unsigned x, unsigned y) { u32x2 v = {x, y}; *LDS_PTR(u32x2, a) = v; }
__device__ __forceinline__ float4 lds_ld4(unsigned a) { const f32x4 v = *LDS_PTR(const f32x4, a); return make_float4(v[0], v[1], v[2], v[3]); }


template <int NM>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NM]) {
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
}

struct Frag { unsigned h[4], l[4]; };   // one A (or B) fragment: 8 bf16 per plane
__device__ __forceinline__ void put(unsigned (&d)[4], int i, uint2 v) { d[i] = v.x; d[i + 1] = v.y; }

// Dense layers run as a flat list of (k-step, m-tile) items, three MFMAs each, with the A fragment of item
// i+2 requested from LDS before the MFMAs of item i issue (ring of 3 fragments = 24 registers);
// sched_barrier(0) pins that order — left alone, hipcc hoists hundreds of LDS reads and spills.
template <int NM, int KS, bool F16 = false, typename LoadF>
__device__ __forceinline__ void run_layer(LoadF load, const Act<(KS + 1) / 2>& in, f32x16 (&acc)[NM]) {
  constexpr int NI = NM * KS, D = 2;
  Frag ring[D + 1];
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < NI) load(i / NM, i % NM, ring[i]);
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    if (it + D < NI) load((it + D) / NM, (it + D) % NM, ring[(it + D) % (D + 1)]);
    const int s = it / NM, m = it % NM, q = s >> 1, t = s & 1;
    const Frag& f = ring[it % (D + 1)];
    if constexpr (F16) {
      const u32x4 bh = {in.hi[q][4 * t], in.hi[q][4 * t + 1], in.hi[q][4 * t + 2], in.hi[q][4 * t + 3]};
      const u32x4 bl = {in.lo[q][4 * t], in.lo[q][4 * t + 1], in.lo[q][4 * t + 2], in.lo[q][4 * t + 3]};
      const u32x4 ah = {f.h[0], f.h[1], f.h[2], f.h[3]}, al = {f.l[0], f.l[1], f.l[2], f.l[3]};
      __builtin_amdgcn_sched_barrier(0);
      acc[m] = x3h(acc[m], ah, al, bh, bl);
      __builtin_amdgcn_sched_barrier(0);
    } else {
    const bf16x8 bh = mk8(in.hi[q][4 * t], in.hi[q][4 * t + 1], in.hi[q][4 * t + 2], in.hi[q][4 * t + 3]);
    const bf16x8 bl = mk8(in.lo[q][4 * t], in.lo[q][4 * t + 1], in.lo[q][4 * t + 2], in.lo[q][4 * t + 3]);
    __builtin_amdgcn_sched_barrier(0);
    acc[m] = x3(acc[m], mk8(f.h[0], f.h[1], f.h[2], f.h[3]), mk8(f.l[0], f.l[1], f.l[2], f.l[3]), bh, bl);
    __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// m-major dense layer with woven side work (round 4).  scripts/probe/issue_overlap_probe.hip: with ONE wave per SIMD,
// "MFMA, 4-6 VALU, MFMA, ..." costs max(matrix pipe, VALU issue) — 16 x (MFMA, 4 v_fma) = 528 cycles against 532 for the
// MFMAs alone and 340 for the VALU alone — while "16 MFMA, then 64 v_fma" costs the sum (824): a wave's own VALU does hide
// under its own MFMAs, but only when it sits BETWEEN them in program order (an MFMA waits at issue for the pipe, and
// everything behind it waits too).  So: output tile m runs all its k-steps back to back, and after EVERY MFMA one slot
// of `side(slot)` is emitted (slot = 3 * item + pass; the callers put tile m-1's epilogue — FiLM, sine / cosine, hi / lo
// split — into the slots of tile m).  sched_barrier(0) pins the order.
template <int NM, int KS, typename LoadF, typename SideF>
__device__ __forceinline__ void run_layer_mm(LoadF load, const Act<(KS + 1) / 2>& in, f32x16 (&acc)[NM], SideF side) {
  constexpr int NI = NM * KS, D = 2;
  Frag ring[D + 1];
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < NI) load(i % KS, i / KS, ring[i]);
#pragma unroll
  for (int it = 0; it < NI; ++it) {
    if (it + D < NI) load((it + D) % KS, (it + D) / KS, ring[(it + D) % (D + 1)]);
    const int m = it / KS, s = it % KS, q = s >> 1, t = s & 1;
    const bf16x8 bh = mk8(in.hi[q][4 * t], in.hi[q][4 * t + 1], in.hi[q][4 * t + 2], in.hi[q][4 * t + 3]);
    const bf16x8 bl = mk8(in.lo[q][4 * t], in.lo[q][4 * t + 1], in.lo[q][4 * t + 2], in.lo[q][4 * t + 3]);
    const Frag& f = ring[it % (D + 1)];
    const bf16x8 ah = mk8(f.h[0], f.h[1], f.h[2], f.h[3]), al = mk8(f.l[0], f.l[1], f.l[2], f.l[3]);
    __builtin_amdgcn_sched_barrier(0);
    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[m], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    side(3 * it);
    __builtin_amdgcn_sched_barrier(0);
    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[m], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    side(3 * it + 1);
    __builtin_amdgcn_sched_barrier(0);
    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[m], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    side(3 * it + 2);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The DS offset field is 16 bits and the carve is 160 KiB: a region base (lane base + image offset) is made
// opaque with this so that hipcc keeps it in one register and folds only the in-region constant.
__device__ __forceinline__ unsigned opaque(unsigned v) { asm volatile("" : "+v"(v)); return v; }

// Per-lane LDS address bases (bytes, including the kernel's LDS base), recomputed every round from the
// laundered lane id.
struct LaneAddr {
  unsigned fb[2][2];   // forward fragments: [k-step parity t][second half]
  unsigned tb[2][2];   // transposed fragments, register-chain k order: [k-step parity][second half]
  unsigned sb[2];      // staging fragments, natural k order: [second half]; includes O_STG
  unsigned ab;         // aux fragments; includes O_AUX
  unsigned v16, v64;   // per-feature vectors, relative to O_L0: + 16*hf (float4 of 4 features), + 64*hf (4 float4 L0 packs)
};
__device__ __forceinline__ LaneAddr lane_addr(int lane, unsigned sbase) {
  const int l31 = lane & 31, hf = lane >> 5, s16 = lane & 15, mhalf = (lane >> 4) & 1;
  const int ul = 4 * mhalf + (s16 & 3);
  LaneAddr A;
  const int e = hf ^ ((l31 >> 2) & 7);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int sec = 0; sec < 2; ++sec) {
      A.fb[t][sec] = sbase + l31 * 64 + ((e ^ (4 * t) ^ (2 * sec)) << 3);
      A.tb[t][sec] = sbase + (4 * hf + (s16 >> 2)) * 64 + (((ul ^ hf) ^ (4 * t) ^ (2 * sec)) << 3);
    }
  const int gs = 4 * hf + (s16 >> 3);
  A.sb[0] = opaque(sbase + O_STG + (8 * hf + (s16 >> 2)) * 64 + ((ul ^ gs) << 3));
  A.sb[1] = opaque(sbase + O_STG + (8 * hf + (s16 >> 2)) * 64 + ((ul ^ gs ^ 2) << 3));
  A.ab = opaque(sbase + O_AUX + (8 * hf + (s16 >> 2)) * 16 + (s16 & 1) * 8);
  A.v16 = opaque(sbase + O_L0 + 16 * hf);
  A.v64 = opaque(sbase + O_L0 + 64 * hf);
  return A;
}

// One fragment (k-step, output tile) of a weight image in either orientation: b0 / b1 the lane bases of its two halves (image
// offset folded in: ImgBase), c the in-image constant of the (k-step, tile), PLANE the distance of the lo plane.  Forward:
// k-step 2q+t = units 8q+4t+hf and +2 of row 32m + lane (c = q * R * 64 + m * 2048, bases of parity t).  Transposed: k-step ks =
// rows 16ks.. of column block m (c = m * R * 64 + ks * 1024, bases of parity ks & 1).
template <int PLANE>
__device__ __forceinline__ void frag_fwd(unsigned b0, unsigned b1, int c, Frag& f) {
  put(f.h, 0, lds_b64(b0 + c));
  put(f.h, 2, lds_b64(b1 + c));
  put(f.l, 0, lds_b64(b0 + c + PLANE));
  put(f.l, 2, lds_b64(b1 + c + PLANE));
}
template <int PLANE>
__device__ __forceinline__ void frag_tr(unsigned b0, unsigned b1, int c, Frag& f) {
  put(f.h, 0, lds_tr(b0 + c));
  put(f.h, 2, lds_tr(b1 + c + 512));
  put(f.l, 0, lds_tr(b0 + c + PLANE));
  put(f.l, 2, lds_tr(b1 + c + 512 + PLANE));
}
// the four lane bases of LaneAddr::fb or ::tb moved to the image at LDS offset IMG, each held in one register (opaque)
struct ImgBase {
  unsigned b[2][2];
  __device__ __forceinline__ ImgBase(const unsigned (&lb)[2][2], int IMG)
      : b{{opaque(lb[0][0] + IMG), opaque(lb[0][1] + IMG)}, {opaque(lb[1][0] + IMG), opaque(lb[1][1] + IMG)}} {}
};

// Forward-orientation dense layer: acc[m] += W[32m + i][k] * in[k][pt]; W image (R rows = out features) at
// LDS offset IMG, lo plane PLANE bytes after the hi plane.
template <int NM, int Q, int R, int IMG, int PLANE, bool F16 = false>
__device__ __forceinline__ void layer_fwd(const LaneAddr& A, const Act<Q>& in, f32x16 (&acc)[NM]) {
  const ImgBase B(A.fb, IMG);
  auto load = [&](int s, int m, Frag& f) { frag_fwd<PLANE>(B.b[s & 1][0], B.b[s & 1][1], (s >> 1) * R * 64 + m * 2048, f); };
  run_layer<NM, 2 * Q, F16>(load, in, acc);
}

template <int NM, int Q, int R, int IMG, int PLANE, typename SideF>
__device__ __forceinline__ void layer_fwd_mm(const LaneAddr& A, const Act<Q>& in, f32x16 (&acc)[NM], SideF side) {
  const ImgBase B(A.fb, IMG);
  auto load = [&](int s, int m, Frag& f) { frag_fwd<PLANE>(B.b[s & 1][0], B.b[s & 1][1], (s >> 1) * R * 64 + m * 2048, f); };
  run_layer_mm<NM, 2 * Q>(load, in, acc, side);
}

// Transposed dense layer: acc[m] += W[k][32m + i] * in[k][pt]  (dh = W^T d), same image, transpose reads.
// KS = k-steps (16 rows each).  The B operand's k order is the register chain's: k-step ks, element e of half
// hf <-> row 16ks + 4hf + (e&3) + 8(e>>2).
template <int NM, int KS, int R, int IMG, int PLANE, bool F16 = false>
__device__ __forceinline__ void layer_tr(const LaneAddr& A, const Act<(KS + 1) / 2>& in, f32x16 (&acc)[NM]) {
  const ImgBase B(A.tb, IMG);
  auto load = [&](int ks, int m, Frag& f) { frag_tr<PLANE>(B.b[ks & 1][0], B.b[ks & 1][1], m * R * 64 + ks * 1024, f); };
  run_layer<NM, KS, F16>(load, in, acc);      // F16: fp16 planes (the 16-bit transpose read does not care which), x3h
}

template <int NM, int KS, int R, int IMG, int PLANE, typename SideF>
__device__ __forceinline__ void layer_tr_mm(const LaneAddr& A, const Act<(KS + 1) / 2>& in, f32x16 (&acc)[NM], SideF side) {
  const ImgBase B(A.tb, IMG);
  auto load = [&](int ks, int m, Frag& f) { frag_tr<PLANE>(B.b[ks & 1][0], B.b[ks & 1][1], m * R * 64 + ks * 1024, f); };
  run_layer_mm<NM, KS>(load, in, acc, side);
}

// Sines of the chains.  The argument is in revolutions with HW (images staged by stage_weights_x3<true, .>: v_fract + v_sin, no
// multiply), in radians without.  The three are kept expression for expression in step: sincos_rev's sine is sin_rev's — the
// sigma of the gradient kernel is the sigma kernel's bit for bit only while they agree (tests/test_gpu_density_gradient.py asserts
// torch.equal) — and the backward's software path (HW false) takes sine and cosine of one reduction from sincos_rev.
template <bool HW> __device__ __forceinline__ float sin_rev(float x) {
  if (HW) return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(x));
  float s_, c_; sincos_reduced(reduce_2pi(x), &s_, &c_); return s_;
}
template <bool HW> __device__ __forceinline__ float cos_rev(float x) {
  if (HW) return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(x));
  float s_, c_; sincos_reduced(reduce_2pi(x), &s_, &c_); return c_;
}
template <bool HW> __device__ __forceinline__ void sincos_rev(float x, float* s, float* c) {
  if (HW) { const float r = __builtin_amdgcn_fractf(x); *s = __builtin_amdgcn_sinf(r); *c = __builtin_amdgcn_cosf(r); }
  else sincos_reduced(reduce_2pi(x), s, c);
}

// PRE: everything that only ever feeds a sine argument is stored divided by 2 pi — W1, Wc, the layer-0 packs and the FiLM
// offsets c1 / cc — so that gain * (W h) + c comes out in REVOLUTIONS and the sine is v_fract + v_sin with no multiply
// (the FiLM gains g1 / gc and ws stay as they are: the backward multiplies by them).  A backward that runs on these images
// carries the factor through its linear chain and removes it where it writes its partial sums (siren_bwd_x4_kernel).
//
// F16 (the forward kernels, round 5): the three weight images are fp16 hi / lo planes of  W * 2^k,  k per matrix such that
// max |W| * 2^k lies in [2^13, 2^14) — every element down to 2^-17 of the largest keeps both planes normal, nothing
// overflows (fp16 max 65504), and the products hi*hi, hi*lo, lo*hi are exact in the fp32 accumulator.  The scale leaves
// through the consumers: G1 and GC hold gain * 2^-k (a power of two: exact), the colour head's 2^-k sits at O_AUX + 128
// for the kernel's output fma.  Why: sigma = ws . sin(g1 (W1 h1) + c1) is the argument of two DISCONTINUOUS consumers —
// relu(sigma + noise) in fancy_integration (pigan_utils.py:246-252) and the cdf search of sample_pdf (:164-209) — so its
// rounding decides how many samples take another branch than the fp32 reference's.  bf16 planes carry W1 h1 to ~5e-6 of
// its rms, fp16 planes to ~2e-7, the level of an fp32 fmaf chain, at the same three MFMAs per k-step.
__device__ __forceinline__ float pow2_scale_for(float m, int& k) {
  const unsigned u = __float_as_uint(m);
  const int e = (int)((u >> 23) & 0xffu) - 127;
  k = 13 - e;
  if (!(m > 0.f) || e == 128) k = 0;           // all-zero, NaN or inf weights: no scaling (the result is theirs anyway)
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  return __uint_as_float((unsigned)(k + 127) << 23);
}
// SIG (siren_sigma_x3_kernel): only what the chain needs up to sigma, on the sigma carve — W1, the layer-0 packs, G1, C1, WS,
// by the same arithmetic; w.wc, w.bc, w.wf, w.gc, w.pc are not read.
template <bool PRE = false, bool F16 = false, bool SIG = false>
__device__ __forceinline__ void stage_weights_x3(uchar* sm, const cips_siren_weights& w, int b) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const float pre = PRE ? CIPS_INV_2PI : 1.f;
  float s1 = 1.f, sc = 1.f, sf = 1.f, i1 = 1.f, ic = 1.f, isf = 1.f;
  if constexpr (F16) {
    // per-matrix max |W|: lane-local, wave (DPP) and workgroup (LDS words at the start of the not yet written W1 image)
    float m1 = 0.f, mc = 0.f, mf = 0.f;
    for (int i = tid; i < H * 32; i += nt) {
      const float4 v = *reinterpret_cast<const float4*>(w.w1 + 4 * i);
      m1 = fmaxf(fmaxf(m1, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    if constexpr (!SIG) {
    for (int i = tid; i < HC * 32; i += nt) {
      const float4 v = *reinterpret_cast<const float4*>(w.wc + 4 * i);
      mc = fmaxf(fmaxf(mc, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    for (int i = tid; i < CF * 16; i += nt) {
      const float4 v = *reinterpret_cast<const float4*>(w.wf + 4 * i);
      mf = fmaxf(fmaxf(mf, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    }
    // NaN weights: fmaxf drops them here; they reach the planes (and every output) through the split below
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      m1 = fmaxf(m1, __shfl_xor(m1, o)); mc = fmaxf(mc, __shfl_xor(mc, o)); mf = fmaxf(mf, __shfl_xor(mf, o));
    }
    float* red = reinterpret_cast<float*>(sm + O_W1H);
    const int wv = tid >> 6, nw = nt >> 6;
    if ((tid & 63) == 0) { red[3 * wv] = m1; red[3 * wv + 1] = mc; red[3 * wv + 2] = mf; }
    __syncthreads();
    m1 = 0.f; mc = 0.f; mf = 0.f;
    for (int i = 0; i < nw; ++i) { m1 = fmaxf(m1, red[3 * i]); mc = fmaxf(mc, red[3 * i + 1]); mf = fmaxf(mf, red[3 * i + 2]); }
    __syncthreads();
    int k1, kc, kf;
    s1 = pow2_scale_for(m1 * pre, k1); sc = pow2_scale_for(mc * pre, kc); sf = pow2_scale_for(mf, kf);
    i1 = __uint_as_float((unsigned)(127 - k1) << 23); ic = __uint_as_float((unsigned)(127 - kc) << 23);
    isf = __uint_as_float((unsigned)(127 - kf) << 23);
  }
  for (int i = tid; i < H * 32; i += nt) {                  // W1: 128 rows x 32 units
    const int row = i >> 5, u = i & 31;
    float4 v = *reinterpret_cast<const float4*>(w.w1 + row * H + 4 * u);
    if (PRE) { v.x *= pre; v.y *= pre; v.z *= pre; v.w *= pre; }
    if (F16) { v.x *= s1; v.y *= s1; v.z *= s1; v.w *= s1; }
    uint2 ph, pl;
    split2t<F16>(v.x, v.y, ph.x, pl.x); split2t<F16>(v.z, v.w, ph.y, pl.y);
    const int o = img_addr<2>(row, u, H);
    *reinterpret_cast<uint2*>(sm + O_W1H + o) = ph;
    *reinterpret_cast<uint2*>(sm + O_W1L + o) = pl;
  }
  if constexpr (!SIG) {
  for (int i = tid; i < HC * 32; i += nt) {                 // Wc: 64 rows x 32 units
    const int row = i >> 5, u = i & 31;
    float4 v = *reinterpret_cast<const float4*>(w.wc + row * H + 4 * u);
    if (PRE) { v.x *= pre; v.y *= pre; v.z *= pre; v.w *= pre; }
    if (F16) { v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }
    uint2 ph, pl;
    split2t<F16>(v.x, v.y, ph.x, pl.x); split2t<F16>(v.z, v.w, ph.y, pl.y);
    const int o = img_addr<2>(row, u, HC);
    *reinterpret_cast<uint2*>(sm + O_WCH + o) = ph;
    *reinterpret_cast<uint2*>(sm + O_WCL + o) = pl;
  }
  for (int i = tid; i < CF * 16; i += nt) {                 // Wf: 32 rows x 16 units
    const int row = i >> 4, u = i & 15;
    float4 v = *reinterpret_cast<const float4*>(w.wf + row * HC + 4 * u);
    if (F16) { v.x *= sf; v.y *= sf; v.z *= sf; v.w *= sf; }
    uint2 ph, pl;
    split2t<F16>(v.x, v.y, ph.x, pl.x); split2t<F16>(v.z, v.w, ph.y, pl.y);
    const int o = img_addr<2>(row, u, CF);
    *reinterpret_cast<uint2*>(sm + O_WFH + o) = ph;
    *reinterpret_cast<uint2*>(sm + O_WFL + o) = pl;
  }
  }
  constexpr int VB = SIG ? SG_L0 - O_L0 : 0;                // the per-feature vectors keep their spacing on the sigma carve
  float* L0 = reinterpret_cast<float*>(sm + VB + O_L0);
  float* G1 = reinterpret_cast<float*>(sm + VB + O_G1); float* C1 = reinterpret_cast<float*>(sm + VB + O_C1);
  float* WS = reinterpret_cast<float*>(sm + VB + O_WS);
  for (int f = tid; f < H; f += nt) {
    const float g0 = w.g0[b * H + f], gs = g0 * w.box_scale;
    float4 pk;
    pk.x = gs * w.w0[f * 3 + 0]; pk.y = gs * w.w0[f * 3 + 1]; pk.z = gs * w.w0[f * 3 + 2];
    pk.w = fmaf(g0, w.b0[f], w.p0[b * H + f]);
    if (PRE) { pk.x *= pre; pk.y *= pre; pk.z *= pre; pk.w *= pre; }
    reinterpret_cast<float4*>(L0)[f] = pk;
    const float g1 = w.g1[b * H + f];
    G1[f] = F16 ? g1 * i1 : g1; C1[f] = fmaf(g1, w.b1[f], w.p1[b * H + f]) * pre; WS[f] = w.ws[f];
  }
  if constexpr (!SIG) {
  float* GC = reinterpret_cast<float*>(sm + O_GC); float* CC = reinterpret_cast<float*>(sm + O_CC);
  for (int f = tid; f < HC; f += nt) {
    const float gc = w.gc[b * HC + f];
    GC[f] = F16 ? gc * ic : gc; CC[f] = fmaf(gc, w.bc[f], w.pc[b * HC + f]) * pre;
  }
  if (F16 && tid == 0) *reinterpret_cast<float*>(sm + O_AUX + 128) = isf;
  }
}

// ---- host side of the launchers ----

// The chunk rule of every points-major launch: 4096-point chunks when that still fills the chip (>= 3 workgroups per CU on 256
// CUs), else 2048 / 1024 / 512.  cips_siren_bwd_x3_chunks (from which the caller sizes its partial-sum buffers) reports it.
inline int x3_chunk(int B, int P) {
  int chunk = 4096;
  while (chunk > 512 && (long long)B * ((P + chunk - 1) / chunk) < 768) chunk >>= 1;
  return chunk;
}

// Run-time flags -> template arguments: x3_pick(f, a, b, ...) calls the generic lambda f with one std::bool_constant per flag.
template <class F> inline void x3_pick(F&& f) { f(); }
template <class F, class... Bs> inline void x3_pick(F&& f, bool b, Bs... rest) {
  if (b) x3_pick([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else x3_pick([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// Launch of kernel instance KERNEL with `smem` bytes of dynamic LDS; the first launch on a device raises the instance's limit.
template <auto KERNEL, class Args>
inline void x3_launch(dim3 grid, int threads, int smem, cips_stream_t stream, const Args& a) {
  static bool attr_set = false;
  CIPS_PER_DEVICE(attr_set, false);
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(threads), smem, (hipStream_t)stream, a);
}

}  // namespace
