// siren_bwd_x3.hip — fused FiLM-SIREN backward for gfx950 on the bf16 matrix cores (3-pass operand split,
// fp32 accumulate): forward recompute + data gradients + ALL weight-gradient contractions in one kernel.
//
// Backward of exp/cips3d/models/generator.py:260-317 (NeRFNetwork.forward_with_frequencies_phase_shifts)
// and exp/comm/models/film_layer.py:78-107 (autograd of FiLMLayer) — see siren.hip for the forward and the
// exact-fp32 backward ("data" pass + separate GEMMs) that this kernel replaces on the default path.
//
// Why a second kernel: the fp32 data pass has to stage h1, h2, hc, da2, dac for the weight-gradient GEMMs
// through HBM — 2 KiB per sample point, 6.4 GB per step at the headline workload — and runs its five dense
// layers on v_mfma_f32_32x32x2_f32 (157 TF peak).  Here
//   * every dense product is x = hi + lo split-bf16 on v_mfma_f32_32x32x16_bf16 (al*bh + ah*bl + ah*bh,
//     ~5e-6 relative; gradients only — the forward pass stays exact fp32),
//   * the five data layers keep siren.hip's register chain: weights are the A operand (M = features out),
//     the wave's 32 points the N dimension, so the accumulator of one layer (lane = point, 16 registers =
//     16 of a tile's 32 feature rows) is, once FiLM'd and packed to bf16 pairs, the B operand of the next
//     layer: k-step (q,t) takes registers 8t..8t+7 of tile q, i.e. features 32q+16t+4hf+{0..3, 8..11}, and
//     the A fragment is read from LDS with the same permuted k,
//   * the weight gradients  dW1 = da2^T h1, dWc = dac^T h2, dWf = dfeat^T hc  contract over POINTS, so both
//     operands are needed "feature per lane, 8 points per register group".  The packed registers are
//     written to an LDS staging image [point][feature] and read back with ds_read_b64_tr_b16 — the same
//     k-major fragment read as gemm_bf16x3.hip's K-major kernel — by all four waves, each of which owns a
//     fixed set of output tiles (112 accumulator registers) for the whole chunk.  Nothing but the final
//     per-workgroup partial dW (112 KiB) goes to HBM.
//
//   * the per-feature sums over points (FiLM phase/bias gradients, layer-0 weight gradient, sigma-head
//     weight gradient) ride on the same staged operands as one extra 32x32 accumulator tile per wave against
//     an 8-column "aux" operand [1, x, y, z, 1, dsigma, 1, 1] per point, each contraction masked to its own
//     columns — no cross-lane shuffles anywhere in the loop.
//
// LDS (all 160 KiB): W1, Wc, Wf as bf16 hi/lo images (104 KiB), the per-image FiLM vectors (4 KiB), the aux
// image (4 KiB), a 48 KiB staging buffer.  One image serves both orientations: forward fragments are two ds_read_b64 per
// plane, transposed fragments (dh = W^T d) two ds_read_b64_tr_b16.  Every image (weights and staging) is
// XOR-swizzled at 8-byte granularity by a bijection of the row index chosen so that (a) 32 lanes touching
// 32 consecutive rows at one column and (b) the transpose read's 4 rows x 64 B both cover all 64 banks.
//
// This file: the backward kernel, the EVEN plan of its live lists, the segment reduction and the finaliser, with their entry
// points.  The layout, the dense layers and the weight staging are siren_x3_common.h's, shared with the forward and march
// kernels (siren_fwd_x3.hip) and the sigma kernels (siren_sigma_x3.inc).
#include "siren_x3_common.h"

namespace {

// write a wave's packed activations (lane = point `row` of an R-row staging image, units of 4 features);
// HI / LO: offsets of the two planes inside the staging buffer
template <int Q, int R, int HI, int LO>
__device__ __forceinline__ void stage(unsigned sbase, int row, int hf, const Act<Q>& v) {
  const unsigned rb = opaque(sbase + O_STG + row * 64);
  const int g = (row >> 1) & 7;
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) {
    const unsigned o = rb + (((2 * gg + hf) ^ g) << 3);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      lds_st64(o + HI + q * R * 64, v.hi[q][2 * gg], v.hi[q][2 * gg + 1]);
      lds_st64(o + LO + q * R * 64, v.lo[q][2 * gg], v.lo[q][2 * gg + 1]);
    }
  }
}

// k-major fragment of an R-row staging image (planes at offsets HI / LO of the staging buffer; sb0 / sb1 include O_STG): lane i = feature col0 + (lane&31),
// k = points 16ks + 8hf + {0..7}
template <int R, int HI, int LO>
__device__ __forceinline__ void stg_frag(unsigned sb0, unsigned sb1, int col0, int ks, Frag& f) {
  const int c = (col0 >> 5) * R * 64 + ks * 1024;
  put(f.h, 0, lds_tr(sb0 + HI + c)); put(f.h, 2, lds_tr(sb1 + HI + c + 256));
  put(f.l, 0, lds_tr(sb0 + LO + c)); put(f.l, 2, lds_tr(sb1 + LO + c + 256));
}
__device__ __forceinline__ f32x16 x3f(f32x16 acc, const Frag& a, const Frag& b) {
  return x3(acc, mk8(a.h[0], a.h[1], a.h[2], a.h[3]), mk8(a.l[0], a.l[1], a.l[2], a.l[3]),
            mk8(b.h[0], b.h[1], b.h[2], b.h[3]), mk8(b.l[0], b.l[1], b.l[2], b.l[3]));
}

// B fragment of the aux image [point][8 columns] (16 B rows per plane, no swizzle): lane j supplies column
// j & 7 of points 16ks + 8hf + {0..7}; masked to the columns one contraction owns.
__device__ __forceinline__ void aux_frag(unsigned ab, int ks, unsigned mask, Frag& f) {
  const int c = ks * 256;
  put(f.h, 0, lds_tr(ab + c)); put(f.h, 2, lds_tr(ab + c + 64));
  put(f.l, 0, lds_tr(ab + c + 2048)); put(f.l, 2, lds_tr(ab + c + 2048 + 64));
#pragma unroll
  for (int i = 0; i < 4; ++i) { f.h[i] &= mask; f.l[i] &= mask; }
}
// A x B with an exact-in-bf16 B (lo plane zero, e.g. a column of ones): two passes suffice
__device__ __forceinline__ f32x16 x2f(f32x16 acc, const Frag& a, const Frag& b) {
  const bf16x8 bh = mk8(b.h[0], b.h[1], b.h[2], b.h[3]);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mk8(a.l[0], a.l[1], a.l[2], a.l[3]), bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(mk8(a.h[0], a.h[1], a.h[2], a.h[3]), bh, acc, 0, 0, 0);
  return acc;
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

struct BwdX3Args {
  cips_siren_weights w;
  const float* points;
  const float* dfeat;
  const float* dsigma;
  float* sred;    // [B*chunks][SRED]
  float* gpart;   // [B*chunks][GPART]
  int B, P, chunk, chunks;
  unsigned long long* prof;
  int dbg;        // timing attribution, probe builds only (-DCIPS_TUNING, env CIPS_X3_DBG): bit0/1/2 skip the dWf / dWc / dW1 phases
  RayGen rg;      // points == NULL: the points are generated from the ray parameters (point index = ray * S + s)
  const int* idx;    // LIVE / EVEN instances of siren_bwd_x4_kernel only: [B][P] ascending indices of the points to process, and
  const int* count;  // [B] how many of them are defined (LIVE; EVEN reads its ranges from seg)
  const int* seg;    // EVEN instances only: [B*chunks][4] image (-1: idle), first slot, end slot, rounds per flat workgroup id
};
// how a workgroup of siren_bwd_x4_kernel finds its points (MODE, below)
enum { X3_DENSE = 0, X3_LIVE = 1, X3_EVEN = 2 };
constexpr int GP_G1 = 0, GP_GC = H * H, GP_GF0 = GP_GC + HC * H, GP_GF1 = GP_GF0 + CF * HC, GPART = GP_GF1 + CF * HC;
constexpr int SRED = 4 * 32 * 8 + 8;   // per wave a 32x8 tile of column sums, then 4 per-wave sums of dsigma (+ pad)

// phase timestamps for tuning (probe builds, -DCIPS_TUNING, with CIPS_X3_PROF set): workgroup (0,0), lane 0 of each wave,
// first 8 rounds, s_memtime at each phase boundary.  The production build keeps the sched_barrier: it is part of the
// hand-pinned instruction order the kernel was tuned with.
#ifdef CIPS_TUNING
#define X3_TS(i)                                                                                   \
  __builtin_amdgcn_sched_barrier(0);                                                               \
  if (a.prof && blockIdx.x == 0 && blockIdx.y == 0 && lane0 == 0 && rnd < 8)                       \
    a.prof[(rnd * 4 + wave) * 16 + (i)] = __builtin_amdgcn_s_memtime();                            \
  __builtin_amdgcn_sched_barrier(0);
#else
#define X3_TS(i) __builtin_amdgcn_sched_barrier(0);
#endif

// ------------------------------------------------------------------------------------------------------------------
// The EVEN partition of the live lists: G = B * chunks workgroups (the grid of the dense and LIVE launches) are dealt to the
// images in proportion to their ROUNDS of 128 list slots, so that no workgroup walks more than T rounds, T as small as the
// budget allows:
//   r_b = ceil(count_b / 128), Rt = sum r_b;  T = the smallest integer >= max(1, ceil(Rt / G)) with
//   sum_b max(1, ceil(r_b / T)) <= G  (the sum does not grow with T and is B <= G at T = max r_b: a bisection finds it);
//   image b gets n_b = max(1, ceil(r_b / T)) workgroups, flat ids first_b = sum_{b' < b} n_b' .. first_b + n_b; its rounds are
//   dealt as evenly as integers allow (q = r_b / n_b, e = r_b % n_b: the first e workgroups take q + 1 rounds, the rest q);
//   slots = rounds * 128, the end clipped to count_b.  An image without live points keeps one workgroup with an empty range
//   (it writes the all-zero partials its FiLM gradients are finalised from); ids from sum n_b up to G are idle (image -1).
// Equal counts give every image G / B = chunks workgroups of equal length: the LIVE partition, and the dense one when every
// point is listed and the dense chunk is a multiple of 128 that divides P.
// Written once for a TEAM of cooperating threads: one on the host (X3Solo: cips_siren_bwd_x3_live_plan_host), a wave on the
// device (X3Wave: siren_bwd_plan_kernel), member k of a group of size() holding image b0 + k.  Every member runs every statement;
// sum / max / scan return the team's value to all of them.  The search for T is what the team is for: one division per image
// and step, ~10 steps at the headline shape.  Nothing the team stores is read back, and each member writes the segments of its
// own image one after the other (n_b of them: 1 .. 37 at the headline shape; a single image that takes the whole grid is
// written by one member).  Measured at B = 32, G = 768 in the step's eager trace (profiles/even_siren_bwd_kernel_stats_after.txt):
// 85 us per launch.  A first form that looked every flat id up in the img table just written (five dependent global loads per
// id) took 185 us; where the remaining 85 us go is not attributed (serving the images one by one with the whole team instead
// of per member measured the same), so a single-thread plan was not tried against it.
// seg [G][4] = image, first slot, end slot, rounds;  img [B][2] = first id, n_b.  count_b is clamped to [0, P]: whatever the
// count array holds, no range leaves the list.
struct X3Solo {
  __host__ __device__ int rank() const { return 0; }
  __host__ __device__ int size() const { return 1; }
  __host__ __device__ long long sum(long long v) const { return v; }
  __host__ __device__ int max(int v) const { return v; }
  __host__ __device__ int scan(int v) const { return v; }          // inclusive prefix sum over the ranks
};
template <class Team>
__host__ __device__ inline void x3_even_plan(const int* count, int B, int P, int G, int* seg, int* img, const Team& tm) {
  const int me = tm.rank(), nt = tm.size();
  auto clamped = [&](int b) { const int c = count[b]; return c < 0 ? 0 : (c > P ? P : c); };
  auto rounds = [](int c) { return (int)(((long long)c + 127) >> 7); };
  auto wgs = [](int r, int T) { const int n = (r + T - 1) / T; return n < 1 ? 1 : n; };     // r + T - 1 < 2^25 + 2^24
  const int c_own = me < B ? clamped(me) : 0;       // the first group's counts stay in registers through the search
  auto cnt = [&](int b) { return b == me ? c_own : clamped(b); };
  long long rt = 0;
  int rmax = 0;
  for (int b = me; b < B; b += nt) { const int r = rounds(cnt(b)); rt += r; rmax = r > rmax ? r : rmax; }
  rt = tm.sum(rt); rmax = tm.max(rmax);
  int lo = (int)((rt + G - 1) / G);                 // <= rmax, because Rt <= B * rmax <= G * rmax
  if (lo < 1) lo = 1;
  int hi = rmax > lo ? rmax : lo;
  while (lo < hi) {                                 // invariant: the budget holds at hi
    const int mid = lo + (hi - lo) / 2;
    long long n = 0;
    for (int b = me; b < B; b += nt) n += wgs(rounds(cnt(b)), mid);
    if (tm.sum(n) <= G) hi = mid; else lo = mid + 1;
  }
  const int T = lo;
  int first = 0;                                    // ids handed out so far
  for (int b0 = 0; b0 < B; b0 += nt) {
    const int b = b0 + me;
    const int c = b < B ? cnt(b) : 0, r = rounds(c), n = b < B ? wgs(r, T) : 0;
    const int f = first + tm.scan(n) - n;           // exclusive scan of n_b inside the group
    if (b < B) {
      img[2 * b] = f; img[2 * b + 1] = n;
      const int q = r / n, e = r % n;
      int r0 = 0;
      for (int j = 0; j < n; ++j) {
        const int nr = q + (j < e ? 1 : 0);
        const long long end = ((long long)r0 + nr) * 128;
        int* sg = seg + 4 * (long long)(f + j);
        sg[0] = b; sg[1] = r0 * 128; sg[2] = end < c ? (int)end : c; sg[3] = nr;
        r0 += nr;
      }
    }
    first += (int)tm.sum(n);
  }
  for (int w = first + me; w < G; w += nt) { int* sg = seg + 4 * (long long)w; sg[0] = -1; sg[1] = 0; sg[2] = 0; sg[3] = 0; }
}

// one wave: every team operation is a shuffle, there is no barrier and no LDS
struct X3Wave {
  __device__ int rank() const { return threadIdx.x; }
  __device__ int size() const { return 64; }
  __device__ long long sum(long long v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  }
  __device__ int max(int v) const {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
  }
  __device__ int scan(int v) const {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o); if ((int)threadIdx.x >= o) v += u; }
    return v;
  }
};
__global__ __launch_bounds__(64) void siren_bwd_plan_kernel(const int* count, int B, int P, int G, int* seg, int* img) {
  x3_even_plan(count, B, P, G, seg, img, X3Wave{});
}

// out[b][j] = sum of part[w][j] over image b's rows w = first_b .. first_b + n_b - 1 (img), in ascending w, for both partial
// arrays in one launch: a row of gpart (GPART floats) followed by a row of sred (SRED floats), one float4 column per thread.
// Rows that belong to no image (idle ids) are never read.
constexpr int RS_G4 = GPART / 4, RS_S4 = SRED / 4;
static_assert(GPART % 4 == 0 && SRED % 4 == 0, "rows of float4");
__global__ __launch_bounds__(256) void siren_bwd_reduce_segments_kernel(const float4* sred, const float4* gpart, const int* img,
                                                                        float4* sred_out, float4* gpart_out) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= RS_G4 + RS_S4) return;
  const int first = img[2 * b], n = img[2 * b + 1];
  const bool g = j < RS_G4;
  const int col = g ? j : j - RS_G4, w4 = g ? RS_G4 : RS_S4;
  const float4* src = (g ? gpart : sred) + (long long)first * w4 + col;
  float4 acc = src[0];
  int i = 1;
  for (; i + 4 <= n; i += 4) {                      // four rows in flight; added in row order
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[(long long)(i + u) * w4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
  }
  for (; i < n; ++i) { const float4 v = src[(long long)i * w4]; acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
  (g ? gpart_out : sred_out)[(long long)b * w4 + col] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
// siren_bwd_x4_kernel — the fused FiLM-SIREN backward in its round-4 schedule (the math, LDS images, staging windows,
// accumulator ownership and partial-sum layout are the ones the head of this file describes; the reference is
// exp/cips3d/models/generator.py:260-317 and exp/comm/models/film_layer.py:78-107).  What the schedule adds:
//  * the five dense layers of the data chain run m-major with the PREVIOUS output tile's epilogue (FiLM, sine / cosine,
//    hi / lo split) woven between the MFMAs of the current tile, five or six VALU instructions per MFMA
//    (run_layer_mm; scripts/probe/issue_overlap_probe.hip is the measurement behind it);
//  * with hardware trigonometry (HW) the sine arguments are in revolutions (stage_weights_x3<true>): v_fract + v_sin,
//    no multiply, no rint / subtract.  The backward chain carries the factor: d h2, d a2 and d p2 are 1/(2 pi) of their
//    values, d h1 and d a1 1/(2 pi)^2; the weight-gradient and column-sum accumulators they feed are multiplied back when the
//    workgroup writes its partials (the partials keep their documented meaning).
// Values computed in a slot are pinned there: sched_barrier(0) only binds the machine scheduler, and hipcc's IR-level sinking
// otherwise moves the whole (side-effect-free) epilogue below the layer's MFMAs, next to its first use.
__device__ __forceinline__ void pinf(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pinf(float& a, float& b) { asm volatile("" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void pinf(float& a, float& b, float& c, float& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
__device__ __forceinline__ void pinu(unsigned& a, unsigned& b) { asm volatile("" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void pinu(unsigned& a, unsigned& b, unsigned& c, unsigned& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }

// MODE X3_LIVE: the workgroup walks a list of point indices instead of a contiguous range (cips_siren_bwd_x3_live in
// cips3d_hip.h).  Image b's list is a.idx[b * P + 0 .. a.count[b]); workgroup (c, b) takes the slots
// [c * len, min((c + 1) * len, count[b])), len = ceil(count[b] / chunks) rounded up to whole 128-point rounds.  cstart / cend /
// pbase then count list SLOTS, and the three places that form a point index look it up; everything else in a round is the dense
// kernel's.  The trip count comes from device memory, so a replayed graph follows the data.  With every point listed in order
// the partition is the dense one whenever the dense chunk is a multiple of 128 that divides P, and the partials are
// bit-identical.
// MODE X3_EVEN: the same list walk, but image, first slot and end slot of the workgroup come from row (flat workgroup id) of the
// table a.seg that cips_siren_bwd_x3_live_plan wrote (x3_even_plan above: every workgroup of the launch gets about the same
// number of rounds, whatever its image's live share), and the partials go to row = flat id.  An idle id (image -1) leaves
// before anything is staged; the table row is the same for every thread, so the workgroup leaves together.
template <bool HW, int MODE>
__global__ __launch_bounds__(256, 1) void siren_bwd_x4_kernel(BwdX3Args a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  constexpr bool LIVE = MODE != X3_DENSE;
  int b_ = blockIdx.y, prow_ = 0, cs_ = 0, ce_ = 0;
  if constexpr (MODE == X3_EVEN) {
    prow_ = blockIdx.y * gridDim.x + blockIdx.x;
    const int* const sg = a.seg + 4 * (long long)prow_;
    b_ = __builtin_amdgcn_readfirstlane(sg[0]);
    if (b_ < 0) return;
    cs_ = __builtin_amdgcn_readfirstlane(sg[1]);
    ce_ = __builtin_amdgcn_readfirstlane(sg[2]);
  }
  const int b = b_;
  stage_weights_x3<HW>(smem, a.w, b);
  __syncthreads();
  constexpr float TWO_PI = 6.283185307179586f;

  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int cstart = blockIdx.x * a.chunk;
  int cend = min(cstart + a.chunk, a.P);
  if constexpr (MODE == X3_EVEN) {
    cstart = cs_; cend = ce_;
  } else if (LIVE) {
    const int cnt = a.count[b];
    const int len = ((cnt + a.chunks - 1) / a.chunks + 127) & ~127;
    cstart = blockIdx.x * len;
    cend = min(cstart + len, cnt);          // >= 1 unless the image has no live point at all
  }
  const int* const lidx = LIVE ? a.idx + (long long)b * a.P : nullptr;
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);

  // weight-gradient accumulators, owned per wave for the whole chunk; aS: column sums (see SRED)
  f32x16 aG1[4], aGc[2], aGf[1], aS[1];
  zero_acc(aG1); zero_acc(aGc); zero_acc(aGf); zero_acc(aS);
  float r_dsg = 0.f;

  // inputs of the first round
  float px, py, pz, dsg;
  {
    const int slot = cstart + wave * 32 + (lane0 & 31);
    const bool valid = slot < cend;
    int p = valid ? slot : cend - 1;
    if (LIVE) p = cend > 0 ? lidx[p] : 0;   // an image without live points: no list entry is defined, any point will do
    const long long gp = (long long)b * a.P + p;
    if (a.points) { px = a.points[gp * 3 + 0]; py = a.points[gp * 3 + 1]; pz = a.points[gp * 3 + 2]; }
    else gen_point(a.rg, b, p, px, py, pz);
    dsg = valid ? a.dsigma[gp] : 0.f;
  }

  // The first NPRE of layer 0's 16 feature groups of the NEXT round's points are produced inside the dW1 phase of the current
  // round, by the three waves that would otherwise wait at the barrier while the fourth stages its operands (a third each; the
  // first round's come from this prologue); the rest is computed at the start of the round.  NPRE trades idle-slot use against
  // the registers that carry the packed sines across the phase and the round boundary.  Measured (forward + backward at C2,
  // one box each, profiles/r4_siren_bwd_ab_microbench.log): NPRE 16 -> 161 spilled VGPRs, 3.15 ms; 8 -> 94, 3.03 ms; 4 -> 61,
  // 3.02 ms; 0 -> 39, 2.90 ms (2.97 with the dW1 loop rolled): the spill traffic lands in the layer-1 recompute and costs more
  // than the idle slots give, so the shipped value is 0 — the mechanism stays for a chain with a smaller register footprint.
  constexpr int NPRE = 0;
  Act<4> h1n;
  auto l0_groups = [&](auto G0c, auto G1c, float x, float y, float z) __attribute__((always_inline)) {
    constexpr int G0 = decltype(G0c)::value, G1 = decltype(G1c)::value;
    if (G0 >= G1) return;
    int ln = lane0;
    asm volatile("" : "+v"(ln));
    const unsigned sbase_ = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
    const unsigned v64 = opaque(sbase_ + O_L0 + 64 * (ln >> 5));
    float4 pn[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) pn[e] = lds_ld4(v64 + 128 * G0 + 16 * e);
#pragma unroll
    for (int grp = G0; grp < G1; ++grp) {          // grp = 4q + g: features 32q + 8g + 4hf + {0..3}
      float4 pk[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = pn[e];
      if (grp + 1 < G1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) pn[e] = lds_ld4(v64 + 128 * (grp + 1) + 16 * e);
      }
      __builtin_amdgcn_sched_barrier(0);
      float s4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) s4[e] = sin_rev<HW>(fmaf(pk[e].x, x, fmaf(pk[e].y, y, fmaf(pk[e].z, z, pk[e].w))));
      const int q = grp >> 2, g = grp & 3;
      split2(s4[0], s4[1], h1n.hi[q][2 * g], h1n.lo[q][2 * g]);
      split2(s4[2], s4[3], h1n.hi[q][2 * g + 1], h1n.lo[q][2 * g + 1]);
      pinu(h1n.hi[q][2 * g], h1n.lo[q][2 * g], h1n.hi[q][2 * g + 1], h1n.lo[q][2 * g + 1]);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  using IC0 = std::integral_constant<int, 0>; using ICA = std::integral_constant<int, (NPRE + 2) / 3>;
  using ICB = std::integral_constant<int, (2 * NPRE + 2) / 3>; using ICN = std::integral_constant<int, NPRE>;
  using IC16 = std::integral_constant<int, 16>;
  l0_groups(IC0{}, ICN{}, px, py, pz);

  int rnd = -1;
  for (int pbase = cstart; pbase < cend; pbase += 128) {
    ++rnd;
    X3_TS(0)
    // every LDS address below is loop-invariant; laundering the lane id keeps hipcc from hoisting a few hundred
    // of them out of the loop into live registers
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int l31 = lane & 31, hf = lane >> 5;
    const LaneAddr LA = lane_addr(lane, sbase);
    const int prow = wave * 32 + l31;
    const unsigned c7 = l31 & 7;
    const unsigned m_d1 = c7 < 4 ? ~0u : 0u, m_d2 = c7 == 4 ? ~0u : 0u, m_h2 = c7 == 5 ? ~0u : 0u;
    const unsigned m_dc = c7 == 6 ? ~0u : 0u, m_df = c7 == 7 ? ~0u : 0u;

    // ---- upstream gradient of the 32 colour features: requested now, consumed after two layers ----
    float4 df4[4];
    {
      const int slot = pbase + prow;
      const bool valid = slot < cend;
      int p = valid ? slot : cend - 1;
      if (LIVE) p = lidx[p];
      const float* dp = a.dfeat + ((long long)b * a.P + p) * CF + 4 * hf;
#pragma unroll
      for (int g = 0; g < 4; ++g) df4[g] = valid ? ld4(dp + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- aux row of this point: [1, x, y, z, 1, dsigma, 1, 1] ----
    if (hf == 0) {
      uint4 ah, al;
      split2(1.f, px, ah.x, al.x); split2(py, pz, ah.y, al.y); split2(1.f, dsg, ah.z, al.z); split2(1.f, 1.f, ah.w, al.w);
      const u32x4 vh = {ah.x, ah.y, ah.z, ah.w}, vl = {al.x, al.y, al.z, al.w};
      *LDS_PTR(u32x4, sbase + O_AUX + prow * 16) = vh;
      *LDS_PTR(u32x4, sbase + O_AUX + 2048 + prow * 16) = vl;
      r_dsg += dsg;
    }

    // ws * dsigma enters d h2, which this kernel carries as d h2 / (2 pi) when the images are pre-scaled
    const float dsg_s = HW ? dsg * CIPS_INV_2PI : dsg;

    // ---- layer 0 (VALU); only the packed sines are kept, and only until layer 1 has consumed them ----
    f32x16 acc[4];
    zero_acc(acc);
    float cs2[4][16];
    Act<4> h2p;
    // state of the woven epilogues (one group of 4 features at a time)
    float rv[4], sn[4];
    float4 gq, cq;
    // FiLM + sine / cosine + split of features (q, g) of layer 1's output, in six slots of ~30 issue cycles
    auto film2_slot = [&](int q, int g, int j) __attribute__((always_inline)) {
      const float gg[4] = {gq.x, gq.y, gq.z, gq.w}, cc[4] = {cq.x, cq.y, cq.z, cq.w};
      if (HW) {
        if (j == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) rv[e] = fmaf(gg[e], acc[q][4 * g + e], cc[e]);
          rv[0] = __builtin_amdgcn_fractf(rv[0]); rv[1] = __builtin_amdgcn_fractf(rv[1]);
          pinf(rv[0], rv[1], rv[2], rv[3]);
        } else if (j == 1) {
          rv[2] = __builtin_amdgcn_fractf(rv[2]); rv[3] = __builtin_amdgcn_fractf(rv[3]);
          sn[0] = __builtin_amdgcn_sinf(rv[0]); sn[1] = __builtin_amdgcn_sinf(rv[1]);
          pinf(rv[2], rv[3], sn[0], sn[1]);
        } else if (j == 2) {
          cs2[q][4 * g + 0] = __builtin_amdgcn_cosf(rv[0]); cs2[q][4 * g + 1] = __builtin_amdgcn_cosf(rv[1]);
          sn[2] = __builtin_amdgcn_sinf(rv[2]);
          pinf(cs2[q][4 * g + 0], cs2[q][4 * g + 1]); pinf(sn[2]);
        } else if (j == 3) {
          sn[3] = __builtin_amdgcn_sinf(rv[3]);
          cs2[q][4 * g + 2] = __builtin_amdgcn_cosf(rv[2]); cs2[q][4 * g + 3] = __builtin_amdgcn_cosf(rv[3]);
          pinf(cs2[q][4 * g + 2], cs2[q][4 * g + 3]); pinf(sn[3]);
        }
      } else if (j == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sincos_rev<false>(fmaf(gg[e], acc[q][4 * g + e], cc[e]), &sn[e], &cs2[q][4 * g + e]);
        pinf(sn[0], sn[1], sn[2], sn[3]);
      }
      if (j == 4) { split2(sn[0], sn[1], h2p.hi[q][2 * g], h2p.lo[q][2 * g]); pinu(h2p.hi[q][2 * g], h2p.lo[q][2 * g]); }
      if (j == 5) {
        split2(sn[2], sn[3], h2p.hi[q][2 * g + 1], h2p.lo[q][2 * g + 1]);
        pinu(h2p.hi[q][2 * g + 1], h2p.lo[q][2 * g + 1]);
        if (4 * q + g + 1 < 16) {               // next group's gains / offsets
          gq = lds_ld4(LA.v16 + (O_G1 - O_L0) + 32 * (4 * q + g + 1)); cq = lds_ld4(LA.v16 + (O_C1 - O_L0) + 32 * (4 * q + g + 1));
        }
      }
    };
    {
      l0_groups(ICN{}, IC16{}, px, py, pz);      // the groups the previous round's idle slots did not cover
      gq = lds_ld4(LA.v16 + (O_G1 - O_L0)); cq = lds_ld4(LA.v16 + (O_C1 - O_L0));
      // ---- recompute layer 1, m-major: the slots of tile m carry the epilogue of tile m - 1 ----
      layer_fwd_mm<4, 4, H, O_W1H, O_W1L - O_W1H>(LA, h1n, acc, [&](int slot) __attribute__((always_inline)) {
        const int m = slot / 24, j = slot % 24;
        if (m >= 1) film2_slot(m - 1, j / 6, j % 6);
      });
    }
    X3_TS(1)
    // tile 3 of layer 1: its first group here, the other three under the colour layer's first six k-steps (which read h2 tiles
    // 0..2; k-steps 6 and 7 read tile 3 and come after slot 17)
#pragma unroll
    for (int j = 0; j < 6; ++j) { film2_slot(3, 0, j); __builtin_amdgcn_sched_barrier(0); }

    X3_TS(2)
    // ---- recompute colour sine layer, m-major ----
    f32x16 accc[2];
    zero_acc(accc);
    float csc[2][16];
    Act<2> hcp;
    float4 gcq, ccq;
    auto filmc_slot = [&](int q, int g, int j) __attribute__((always_inline)) {
      const float gg[4] = {gcq.x, gcq.y, gcq.z, gcq.w}, cc[4] = {ccq.x, ccq.y, ccq.z, ccq.w};
      if (HW) {
        if (j == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) rv[e] = fmaf(gg[e], accc[q][4 * g + e], cc[e]);
          rv[0] = __builtin_amdgcn_fractf(rv[0]); rv[1] = __builtin_amdgcn_fractf(rv[1]);
          pinf(rv[0], rv[1], rv[2], rv[3]);
        } else if (j == 1) {
          rv[2] = __builtin_amdgcn_fractf(rv[2]); rv[3] = __builtin_amdgcn_fractf(rv[3]);
          sn[0] = __builtin_amdgcn_sinf(rv[0]); sn[1] = __builtin_amdgcn_sinf(rv[1]);
          pinf(rv[2], rv[3], sn[0], sn[1]);
        } else if (j == 2) {
          csc[q][4 * g + 0] = __builtin_amdgcn_cosf(rv[0]); csc[q][4 * g + 1] = __builtin_amdgcn_cosf(rv[1]);
          sn[2] = __builtin_amdgcn_sinf(rv[2]);
          pinf(csc[q][4 * g + 0], csc[q][4 * g + 1]); pinf(sn[2]);
        } else if (j == 3) {
          sn[3] = __builtin_amdgcn_sinf(rv[3]);
          csc[q][4 * g + 2] = __builtin_amdgcn_cosf(rv[2]); csc[q][4 * g + 3] = __builtin_amdgcn_cosf(rv[3]);
          pinf(csc[q][4 * g + 2], csc[q][4 * g + 3]); pinf(sn[3]);
        }
      } else if (j == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sincos_rev<false>(fmaf(gg[e], accc[q][4 * g + e], cc[e]), &sn[e], &csc[q][4 * g + e]);
        pinf(sn[0], sn[1], sn[2], sn[3]);
      }
      if (j == 4) { split2(sn[0], sn[1], hcp.hi[q][2 * g], hcp.lo[q][2 * g]); pinu(hcp.hi[q][2 * g], hcp.lo[q][2 * g]); }
      if (j == 5) {
        split2(sn[2], sn[3], hcp.hi[q][2 * g + 1], hcp.lo[q][2 * g + 1]);
        pinu(hcp.hi[q][2 * g + 1], hcp.lo[q][2 * g + 1]);
        if (4 * q + g + 1 < 8) {
          gcq = lds_ld4(LA.v16 + (O_GC - O_L0) + 32 * (4 * q + g + 1)); ccq = lds_ld4(LA.v16 + (O_CC - O_L0) + 32 * (4 * q + g + 1));
        }
      }
    };
    gcq = lds_ld4(LA.v16 + (O_GC - O_L0)); ccq = lds_ld4(LA.v16 + (O_CC - O_L0));
    layer_fwd_mm<2, 4, HC, O_WCH, O_WCL - O_WCH>(LA, h2p, accc, [&](int slot) __attribute__((always_inline)) {
      if (slot < 18) film2_slot(3, 1 + slot / 6, slot % 6);
      else if (slot >= 24) filmc_slot(0, (slot - 24) / 6, (slot - 24) % 6);
    });
#pragma unroll
    for (int j = 0; j < 24; ++j) { filmc_slot(1, j / 6, j % 6); __builtin_amdgcn_sched_barrier(0); }

    X3_TS(3)
    Act<1> dfp;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      split2(df4[g].x, df4[g].y, dfp.hi[0][2 * g], dfp.lo[0][2 * g]);
      split2(df4[g].z, df4[g].w, dfp.hi[0][2 * g + 1], dfp.lo[0][2 * g + 1]);
    }

    // ---- dWf += dfeat^T hc over the workgroup's 128 points: wave -> (hc column tile w&1, point half w>>1);
    //      waves 0 and 2 also take sum_p dfeat (aux column 7) ----
    if (!CIPS_TUNE(a.dbg & 1)) {
      constexpr int DFH = 0, DFL = 8192, HCH = 16384, HCL = 32768;
      stage<1, 128, DFH, DFL>(sbase, prow, hf, dfp);
      stage<2, 128, HCH, HCL>(sbase, prow, hf, hcp);
      __syncthreads();
      const int jt = wave & 1, kh = wave >> 1;
      const unsigned mdf = jt == 0 ? m_df : 0u;          // waves 1 and 3 add zeros: no wave-dependent branches here
      Frag fa[2], fb[2], fx[2];
      // this wave's k-steps (4kh + k) and hc column block are folded into the lane bases
      const unsigned d0 = opaque(LA.sb[0] + kh * 4096), d1 = opaque(LA.sb[1] + kh * 4096);      // dfeat: k-steps 4kh..
      const unsigned h0 = opaque(d0 + jt * 8192), h1_ = opaque(d1 + jt * 8192);                  // hc: same k-steps, column block jt
      const unsigned ax = opaque(LA.ab + kh * 1024);
      stg_frag<128, DFH, DFL>(d0, d1, 0, 0, fa[0]);
      stg_frag<128, HCH, HCL>(h0, h1_, 0, 0, fb[0]);
      aux_frag(ax, 0, mdf, fx[0]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k + 1 < 4) {
          stg_frag<128, DFH, DFL>(d0, d1, 0, k + 1, fa[(k + 1) & 1]);
          stg_frag<128, HCH, HCL>(h0, h1_, 0, k + 1, fb[(k + 1) & 1]);
          aux_frag(ax, k + 1, mdf, fx[(k + 1) & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
        aGf[0] = x3f(aGf[0], fa[k & 1], fb[k & 1]);
        aS[0] = x2f(aS[0], fa[k & 1], fx[k & 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }

    X3_TS(4)
    // ---- d hc = Wf^T dfeat  (K = 32, M = 64);  dac = d hc * cos;  dpc = gc * dac ----
    zero_acc(accc);
    layer_tr<2, 2, CF, O_WFH, O_WFL - O_WFH>(LA, dfp, accc);
    Act<2> dacp, dpcp;
    {
      float4 gn = lds_ld4(LA.v16 + (O_GC - O_L0));
#pragma unroll
      for (int grp = 0; grp < 8; ++grp) {
        const float4 g4 = gn;
        if (grp + 1 < 8) gn = lds_ld4(LA.v16 + (O_GC - O_L0) + 32 * (grp + 1));
        __builtin_amdgcn_sched_barrier(0);
        const int q = grp >> 2, g = grp & 3;
        const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
        float v[4], w_[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = accc[q][4 * g + e] * csc[q][4 * g + e]; w_[e] = gg[e] * v[e]; }
        split2(v[0], v[1], dacp.hi[q][2 * g], dacp.lo[q][2 * g]);
        split2(v[2], v[3], dacp.hi[q][2 * g + 1], dacp.lo[q][2 * g + 1]);
        split2(w_[0], w_[1], dpcp.hi[q][2 * g], dpcp.lo[q][2 * g]);
        split2(w_[2], w_[3], dpcp.hi[q][2 * g + 1], dpcp.lo[q][2 * g + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    pin(dacp); pin(h2p);
    X3_TS(5)
    // ---- dWc += dac^T h2: two sub-phases of 64 points; wave -> (dac row tile w&1, h2 column tiles 2(w>>1)+{0,1});
    //      plus sum_p dsigma*h2 (h2 row tile w, aux column 5) and, on waves 0 and 1, sum_p dac (aux column 6).
    //      Fragment reads run half a k-step ahead of their MFMAs. ----
    if (!CIPS_TUNE(a.dbg & 2)) {
      constexpr int DAH = 0, DAL = 8192, H2H = 16384, H2L = 32768;
      const int it = wave & 1, jt0 = 2 * (wave >> 1);
      const unsigned mdc = wave < 2 ? m_dc : 0u;         // waves 2 and 3 add zeros: no wave-dependent branches here
      // wave-dependent column blocks folded into the lane bases (block stride of a 64-row image: 4096 B)
      const unsigned i0 = opaque(LA.sb[0] + it * 4096), i1 = opaque(LA.sb[1] + it * 4096);
      const unsigned j0 = opaque(LA.sb[0] + jt0 * 4096), j1 = opaque(LA.sb[1] + jt0 * 4096);
      const unsigned w0 = opaque(LA.sb[0] + wave * 4096), w1 = opaque(LA.sb[1] + wave * 4096);
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        if ((wave >> 1) == sp) {
          stage<2, 64, DAH, DAL>(sbase, (wave & 1) * 32 + l31, hf, dacp);
          stage<4, 64, H2H, H2L>(sbase, (wave & 1) * 32 + l31, hf, h2p);
        }
        __syncthreads();
        Frag fa, fb0, fb1, fh, fx, fy;
        stg_frag<64, DAH, DAL>(i0, i1, 0, 0, fa);
        stg_frag<64, H2H, H2L>(j0, j1, 0, 0, fb0);
        stg_frag<64, H2H, H2L>(j0, j1, 32, 0, fb1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          stg_frag<64, H2H, H2L>(w0, w1, 0, k, fh);
          aux_frag(LA.ab, 4 * sp + k, m_h2, fx);
          aux_frag(LA.ab, 4 * sp + k, mdc, fy);
          __builtin_amdgcn_sched_barrier(0);
          aGc[0] = x3f(aGc[0], fa, fb0);
          aGc[1] = x3f(aGc[1], fa, fb1);
          aS[0] = x2f(aS[0], fa, fy);
          __builtin_amdgcn_sched_barrier(0);
          if (k + 1 < 4) {
            stg_frag<64, DAH, DAL>(i0, i1, 0, k + 1, fa);
            stg_frag<64, H2H, H2L>(j0, j1, 0, k + 1, fb0);
            stg_frag<64, H2H, H2L>(j0, j1, 32, k + 1, fb1);
          }
          __builtin_amdgcn_sched_barrier(0);
          aS[0] = x3f(aS[0], fh, fx);
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
      }
    }

    X3_TS(6)
    // ---- d h2 = Wc^T dpc + ws * dsigma  (K = 64, M = 128), m-major;  da2 = d h2 * cos;  dp2 = g1 * da2.  A tile has only
    //      12 MFMA slots here (4 k-steps) against ~36 VALU instructions per group: three slots per group, VALU-bound ----
    zero_acc(acc);
    Act<4> da2p;
    Act<4> h1p;
    Act<4> da1p;                         // consumed tile by tile inside the d h1 layer (da1_sums): never 64 live registers
    float npx, npy, npz, ndsg;
    {
      Act<4> dp2p;
      float v4[4], w4_[4];
      float4 gq2, wq2;
      auto dh2_slot = [&](int q, int g, int j) __attribute__((always_inline)) {
        if (j == 0) {
          const float gg[4] = {gq2.x, gq2.y, gq2.z, gq2.w}, ww[4] = {wq2.x, wq2.y, wq2.z, wq2.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v4[e] = fmaf(ww[e], dsg_s, acc[q][4 * g + e]) * cs2[q][4 * g + e];
            w4_[e] = gg[e] * v4[e];
          }
          pinf(v4[0], v4[1], v4[2], v4[3]); pinf(w4_[0], w4_[1], w4_[2], w4_[3]);
          if (4 * q + g + 1 < 16) {
            gq2 = lds_ld4(LA.v16 + (O_G1 - O_L0) + 32 * (4 * q + g + 1)); wq2 = lds_ld4(LA.v16 + (O_WS - O_L0) + 32 * (4 * q + g + 1));
          }
        } else if (j == 1) {
          split2(v4[0], v4[1], da2p.hi[q][2 * g], da2p.lo[q][2 * g]);
          split2(v4[2], v4[3], da2p.hi[q][2 * g + 1], da2p.lo[q][2 * g + 1]);
          pinu(da2p.hi[q][2 * g], da2p.lo[q][2 * g], da2p.hi[q][2 * g + 1], da2p.lo[q][2 * g + 1]);
        } else {
          split2(w4_[0], w4_[1], dp2p.hi[q][2 * g], dp2p.lo[q][2 * g]);
          split2(w4_[2], w4_[3], dp2p.hi[q][2 * g + 1], dp2p.lo[q][2 * g + 1]);
          pinu(dp2p.hi[q][2 * g], dp2p.lo[q][2 * g], dp2p.hi[q][2 * g + 1], dp2p.lo[q][2 * g + 1]);
        }
      };
      gq2 = lds_ld4(LA.v16 + (O_G1 - O_L0)); wq2 = lds_ld4(LA.v16 + (O_WS - O_L0));
      layer_tr_mm<4, 4, HC, O_WCH, O_WCL - O_WCH>(LA, dpcp, acc, [&](int slot) __attribute__((always_inline)) {
        const int m = slot / 12, j = slot % 12;
        if (m >= 1) dh2_slot(m - 1, j / 3, j % 3);
      });
#pragma unroll
      for (int j = 0; j < 12; ++j) { dh2_slot(3, j / 3, j % 3); __builtin_amdgcn_sched_barrier(0); }

      // ---- inputs of the next round: requested here, a whole layer before their first use (layer 0 of the next round inside
      //      the dW1 phase below) ----
      {
        const int slot = pbase + 128 + prow;
        const bool valid = slot < cend;
        int p = valid ? slot : cend - 1;
        if (LIVE) p = lidx[p];
        const long long gp = (long long)b * a.P + p;
        if (a.points) { npx = a.points[gp * 3 + 0]; npy = a.points[gp * 3 + 1]; npz = a.points[gp * 3 + 2]; }
        else gen_point(a.rg, b, p, npx, npy, npz);
        ndsg = valid ? a.dsigma[gp] : 0.f;
      }
      // ---- d h1 = W1^T dp2  (K = 128, M = 128), m-major;  da1 = d h1 * cos(layer-0 argument), the layer-0 sines recomputed
      //      alongside for dW1: ~52 VALU instructions per group of 4 features in six slots ----
      f32x16 acc1[4];
      zero_acc(acc1);
      float4 pq[4];
      float ar[4], s1[4], c1[4], d1[4];
      auto dh1_slot = [&](int q, int g, int j) __attribute__((always_inline)) {
        if (j == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ar[e] = fmaf(pq[e].x, px, fmaf(pq[e].y, py, fmaf(pq[e].z, pz, pq[e].w)));
          pinf(ar[0], ar[1], ar[2], ar[3]);
          if (4 * q + g + 1 < 16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) pq[e] = lds_ld4(LA.v64 + 128 * (4 * q + g + 1) + 16 * e);
          }
        } else if (j == 1) {
          if (HW) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ar[e] = __builtin_amdgcn_fractf(ar[e]);
            s1[0] = __builtin_amdgcn_sinf(ar[0]); s1[1] = __builtin_amdgcn_sinf(ar[1]);
            pinf(ar[0], ar[1], ar[2], ar[3]); pinf(s1[0], s1[1]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) sincos_rev<false>(ar[e], &s1[e], &c1[e]);
            pinf(s1[0], s1[1], s1[2], s1[3]); pinf(c1[0], c1[1], c1[2], c1[3]);
          }
        } else if (j == 2) {
          if (HW) {
            s1[2] = __builtin_amdgcn_sinf(ar[2]); s1[3] = __builtin_amdgcn_sinf(ar[3]);
            c1[0] = __builtin_amdgcn_cosf(ar[0]); c1[1] = __builtin_amdgcn_cosf(ar[1]);
            pinf(s1[2], s1[3], c1[0], c1[1]);
          }
        } else if (j == 3) {
          if (HW) { c1[2] = __builtin_amdgcn_cosf(ar[2]); c1[3] = __builtin_amdgcn_cosf(ar[3]); }
#pragma unroll
          for (int e = 0; e < 4; ++e) d1[e] = acc1[q][4 * g + e] * c1[e];
          pinf(d1[0], d1[1], d1[2], d1[3]);
        } else if (j == 4) {
          split2(s1[0], s1[1], h1p.hi[q][2 * g], h1p.lo[q][2 * g]);
          split2(s1[2], s1[3], h1p.hi[q][2 * g + 1], h1p.lo[q][2 * g + 1]);
          pinu(h1p.hi[q][2 * g], h1p.lo[q][2 * g], h1p.hi[q][2 * g + 1], h1p.lo[q][2 * g + 1]);
        } else {
          split2(d1[0], d1[1], da1p.hi[q][2 * g], da1p.lo[q][2 * g]);
          split2(d1[2], d1[3], da1p.hi[q][2 * g + 1], da1p.lo[q][2 * g + 1]);
          pinu(da1p.hi[q][2 * g], da1p.lo[q][2 * g], da1p.hi[q][2 * g + 1], da1p.lo[q][2 * g + 1]);
        }
      };
#pragma unroll
      for (int e = 0; e < 4; ++e) pq[e] = lds_ld4(LA.v64 + 16 * e);
      // sum_p da1 * [1, x, y, z] of feature tile q over this wave's OWN 32 points (round 4; was part of the dW1 phase: a third of
      // its staging and 6 of its 34 MFMAs per sub-phase).  da1 tile q goes through a wave-private 4 KiB slot behind the (now
      // 32 KiB) dW1 window and comes back feature-per-lane; the aux operand is masked to columns 0..3 AND to lane group q.  The
      // column-sum tile aS has 32 columns of which the masks (functions of lane & 7) used only 8 — lane groups 1..3 were copies
      // of group 0 — so tile q's sums land in columns 8 q + {0..3} of the SAME accumulator: no new registers; the waves' partial
      // sums are added when the workgroup writes its partials.  Same-wave LDS traffic: the DS queue is in order, no barrier.
      const unsigned prv = opaque(sbase + O_STG + 32768 + wave * 4096);
      auto da1_put = [&](int q) __attribute__((always_inline)) {          // tile q -> the wave's private slot
        const unsigned rb = opaque(prv + l31 * 64);
        const int gsw = (l31 >> 1) & 7;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          const unsigned o = rb + (((2 * gg + hf) ^ gsw) << 3);
          lds_st64(o, da1p.hi[q][2 * gg], da1p.hi[q][2 * gg + 1]);
          lds_st64(o + 2048, da1p.lo[q][2 * gg], da1p.lo[q][2 * gg + 1]);
        }
      };
      auto da1_sum = [&](int q) __attribute__((always_inline)) {          // read it back feature-per-lane, contract with aux
        const unsigned mq = ((l31 >> 3) == q && c7 < 4) ? ~0u : 0u;
        const unsigned p0 = opaque(LA.sb[0] + 32768 + wave * 4096), p1 = opaque(LA.sb[1] + 32768 + wave * 4096);
        const unsigned axw = opaque(LA.ab + wave * 512);
        Frag fd0, fd1, fy0, fy1;
        stg_frag<32, 0, 2048>(p0, p1, 0, 0, fd0);
        stg_frag<32, 0, 2048>(p0, p1, 0, 1, fd1);
        aux_frag(axw, 0, mq, fy0);
        aux_frag(axw, 1, mq, fy1);
        __builtin_amdgcn_sched_barrier(0);
        aS[0] = x3f(aS[0], fd0, fy0);
        aS[0] = x3f(aS[0], fd1, fy1);
        __builtin_amdgcn_sched_barrier(0);
      };
      // tile q's epilogue runs under tile q + 1's MFMAs; its slot is written at the first slot of tile q + 2 and read back eight
      // slots later (the LDS round trip has long completed: the read costs its own latency only)
      layer_tr_mm<4, 8, H, O_W1H, O_W1L - O_W1H>(LA, dp2p, acc1, [&](int slot) __attribute__((always_inline)) {
        const int m = slot / 24, j = slot % 24;
        if (m >= 2 && j == 0) da1_put(m - 2);
        if (m >= 2 && j == 8) da1_sum(m - 2);
        if (m >= 1) dh1_slot(m - 1, j / 6, j % 6);
      });
      X3_TS(7)
      da1_put(2);
#pragma unroll
      for (int j = 0; j < 12; ++j) { dh1_slot(3, j / 6, j % 6); __builtin_amdgcn_sched_barrier(0); }
      da1_sum(2);
#pragma unroll
      for (int j = 12; j < 24; ++j) { dh1_slot(3, j / 6, j % 6); __builtin_amdgcn_sched_barrier(0); }
      da1_put(3);
      da1_sum(3);
    }

    pin(da2p); pin(h1p);
    X3_TS(8)
    // ---- dW1 += da2^T h1: four sub-phases of 32 points; wave -> da2 row tile w, all four h1 column tiles;
    //      plus sum_p da2 (aux column 4) and sum_p da1 * [1, x, y, z] (aux columns 0..3) for row tile w ----
    if (!CIPS_TUNE(a.dbg & 4)) {
      constexpr int DAH = 0, DAL = 8192, H1H = 16384, H1L = 24576;      // 32 KiB; the last 16 KiB hold the waves' private slots
      const unsigned w0 = opaque(LA.sb[0] + wave * 2048), w1 = opaque(LA.sb[1] + wave * 2048);   // row tile w
#pragma unroll
      for (int sp = 0; sp < 4; ++sp) {
        if (sp == 1) { X3_TS(10) }
        if (wave == sp) {
          stage<4, 32, DAH, DAL>(sbase, l31, hf, da2p);
          stage<4, 32, H1H, H1L>(sbase, l31, hf, h1p);
        } else if (NPRE > 0) {
          // this wave's k-th idle sub-phase (k = sp for sp < wave, sp - 1 after its own turn): a third of the NPRE groups
          const int k = sp - (sp > wave ? 1 : 0);
          if (k == 0) l0_groups(IC0{}, ICA{}, npx, npy, npz);
          else if (k == 1) l0_groups(ICA{}, ICB{}, npx, npy, npz);
          else l0_groups(ICB{}, ICN{}, npx, npy, npz);
        }
        if (sp == 1) { X3_TS(11) }
        __syncthreads();
        if (sp == 1) { X3_TS(12) }
        const unsigned ax = opaque(LA.ab + sp * 512);      // aux k-steps 2sp + k
        Frag fa, fb0, fb1, fb2, fb3, fx;
        stg_frag<32, DAH, DAL>(w0, w1, 0, 0, fa);
        stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 0, 0, fb0);
        stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 32, 0, fb1);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 64, k, fb2);
          stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 96, k, fb3);
          aux_frag(ax, k, m_d2, fx);
          __builtin_amdgcn_sched_barrier(0);
          aG1[0] = x3f(aG1[0], fa, fb0);
          aG1[1] = x3f(aG1[1], fa, fb1);
          __builtin_amdgcn_sched_barrier(0);
          aG1[2] = x3f(aG1[2], fa, fb2);
          aG1[3] = x3f(aG1[3], fa, fb3);
          aS[0] = x2f(aS[0], fa, fx);
          __builtin_amdgcn_sched_barrier(0);
          if (k + 1 < 2) {
            stg_frag<32, DAH, DAL>(w0, w1, 0, k + 1, fa);
            stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 0, k + 1, fb0);
            stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 32, k + 1, fb1);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (sp == 1) { X3_TS(13) }
        __syncthreads();
        if (sp == 1) { X3_TS(14) }
      }
    }
    px = npx; py = npy; pz = npz; dsg = ndsg;
    X3_TS(9)
  }

  const int lane = lane0, l31 = lane & 31, hf = lane >> 5;
  // ---- per-wave column sums and sum of dsigma.  Columns 4..7 of lane group 0 are this wave's row-tile sums as before; columns
  //      8 q + {0..3} hold sum_p da1 * [1, x, y, z] of feature tile q over this wave's own points: the four waves' tiles meet in
  //      the idle staging window and wave t adds tile t's four partials in wave order ----
  {
    float* part = reinterpret_cast<float*>(smem + O_STG);      // [wave][32 rows][32 columns] floats = 16 KiB
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(wave * 32 + mfma_row(r, hf)) * 32 + l31] = aS[0][r];
    __syncthreads();
    float* sr = a.sred + (long long)(MODE == X3_EVEN ? prow_ : b * a.chunks + blockIdx.x) * SRED;
    if (l31 < 8) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_row(r, hf);
        // columns 0..3 are carried as 1/(2 pi)^2, column 4 (sum_p da2) as 1/(2 pi); 5..7 unscaled
        float v = aS[0][r] * ((HW && l31 == 4) ? TWO_PI : 1.f);
        if (l31 < 4) {
          v = part[(0 * 32 + row) * 32 + 8 * wave + l31];
          v += part[(1 * 32 + row) * 32 + 8 * wave + l31];
          v += part[(2 * 32 + row) * 32 + 8 * wave + l31];
          v += part[(3 * 32 + row) * 32 + 8 * wave + l31];
          if (HW) v *= TWO_PI * TWO_PI;
        }
        sr[wave * 256 + row * 8 + l31] = v;
      }
    }
    float t = r_dsg;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
    if (lane == 0) sr[1024 + wave] = t;
    if (lane == 1) sr[1028 + wave] = 0.f;
  }
  // ---- write the workgroup's partial weight gradients ----
  {
    float* gp_ = a.gpart + (long long)(MODE == X3_EVEN ? prow_ : b * a.chunks + blockIdx.x) * GPART;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) gp_[GP_G1 + (32 * wave + mfma_row(r, hf)) * H + 32 * j + l31] = aG1[j][r] * (HW ? TWO_PI : 1.f);
    const int it = wave & 1, jt0 = 2 * (wave >> 1);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) gp_[GP_GC + (32 * it + mfma_row(r, hf)) * H + 32 * (jt0 + j) + l31] = aGc[j][r];
    float* gf = gp_ + ((wave >> 1) ? GP_GF1 : GP_GF0);
#pragma unroll
    for (int r = 0; r < 16; ++r) gf[mfma_row(r, hf) * HC + 32 * (wave & 1) + l31] = aGf[0][r];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Finalisation of the fused backward: the per-workgroup partials (sred, gpart) -> the 16 gradient tensors autograd
// expects (FiLM gains / phases per image, weights and biases summed over the batch), in one launch instead of ~40 tiny
// torch reductions / broadcasts.  Chain rule of film_layer.py:88-107 (arg = gain * (W x + b) + phase):
//   d phase = sum_p d arg;  d gain = sum_j G[f][j] W[f][j] + b[f] d phase  (G = d arg^T h_in);  dW = sum_b gain_b G_b;
//   db = sum_b gain_b d phase_b.  Layer 0's input is box_scale * point.  Fixed summation order: chunks, then images.
// One workgroup of 128 threads per output row: [0,128) rows of dW1 (+ layer 0 and the sigma head of feature f),
// [128,192) rows of dWc, [192,224) rows of dWf (+ its bias), 224: the sigma bias.
// SEGS (cips_siren_bwd_x3_finalize_segments): the partials are the EVEN launch's, image b's rows are first_b .. first_b + n_b - 1
// of the img table, and every value the code below reads from "row b" is the sum of that column over those rows, formed here
// in ascending row order — the value siren_bwd_reduce_segments_kernel would have stored, so the 16 gradients are the
// two-launch sequence's bit for bit, without the per-image sums' round trip through HBM.
struct FinArgs {
  cips_siren_weights w;
  const float* sred; const float* gpart;
  const int* img;
  cips_siren_grads o;
  int B, chunks;
};

template <bool SEGS>
__global__ __launch_bounds__(128) void siren_bwd_finalize_kernel(FinArgs a) {
  __shared__ float cols[8];
  __shared__ float red[128];
  const int task = blockIdx.x, j = threadIdx.x;
  const int B = a.B, C = SEGS ? 1 : a.chunks;
  // SEGS: s0 / s1 = the sums of p0[w * W0] / p1[w * W1] over image b's rows w, ascending (p1 may be NULL).  The rows are loaded
  // FIN_ROWS at a time before any is added: the walk costs a load latency per batch, not per row, and a thread that needs two
  // columns (the SRED columns ride with threads 0..7) pays for one walk.
  constexpr int FIN_ROWS = 16;
  auto seg_sum = [&](int b, const float* p0, int W0, const float* p1, int W1, float& s0, float& s1) {
    const int first = a.img[2 * b], n = a.img[2 * b + 1];
    p0 += (long long)first * W0;
    if (p1) p1 += (long long)first * W1;
    float a0 = 0.f, a1 = 0.f;
    for (int i = 0; i < n; i += FIN_ROWS) {
      float v0[FIN_ROWS], v1[FIN_ROWS];
#pragma unroll
      for (int u = 0; u < FIN_ROWS; ++u) {
        const int r = i + u < n ? i + u : n - 1;
        v0[u] = p0[(long long)r * W0];
        v1[u] = p1 ? p1[(long long)r * W1] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < FIN_ROWS; ++u)
        if (i + u < n) { a0 = i + u ? a0 + v0[u] : v0[u]; a1 = i + u ? a1 + v1[u] : v1[u]; }
    }
    s0 = a0; s1 = a1;
  };
  // element `off` of row (b, c) of a partial array with rows of W floats (SEGS: c = 0, the image's row sum)
  auto at = [&](const float* arr, int W, int b, int c, int off) {
    if constexpr (!SEGS) return arr[((long long)b * C + c) * W + off];
    else {
      float s0, s1;
      seg_sum(b, arr + off, W, nullptr, 0, s0, s1);
      return s0;
    }
  };
  auto colofs = [](int f, int col) { return (f >> 5) * 256 + (f & 31) * 8 + col; };
  auto colsum = [&](int b, int f, int col) {       // sum over chunks of column `col` of feature row f (SRED layout)
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += at(a.sred, SRED, b, c, colofs(f, col));
    return s;
  };
  auto block_sum = [&](float v) {
    red[j] = v;
    __syncthreads();
    for (int s_ = 64; s_ > 0; s_ >>= 1) {
      if (j < s_) red[j] += red[j + s_];
      __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
  };
  if (task < 192) {
    const bool l1 = task < 128;
    const int f = l1 ? task : task - 128;
    const int goff = l1 ? GP_G1 : GP_GC;
    const float* Wrow = (l1 ? a.w.w1 : a.w.wc) + f * H;
    const float* gain = l1 ? a.w.g1 : a.w.gc;
    const int gdim = l1 ? H : HC;
    const float bias = l1 ? a.w.b1[f] : a.w.bc[f];
    const float wj = Wrow[j];
    float acc_w = 0.f, acc_b = 0.f, acc_ws = 0.f, acc_b0 = 0.f, acc_w0[3] = {0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) {
      float v = 0.f, cs = 0.f;
      if constexpr (SEGS) {
        float sv, sc;
        seg_sum(b, a.gpart + goff + f * H + j, GPART, j < 8 ? a.sred + colofs(f, j) : nullptr, SRED, sv, sc);
        v += sv; cs += sc;
      } else {
        for (int c = 0; c < C; ++c) v += at(a.gpart, GPART, b, c, goff + f * H + j);
        if (j < 8) cs = colsum(b, f, j);
      }
      const float gn = gain[b * gdim + f];
      acc_w = fmaf(gn, v, acc_w);
      if (j < 8) cols[j] = cs;
      const float dot = block_sum(v * wj);           // (its barriers also publish cols)
      if (j == 0) {
        const float dph = l1 ? cols[4] : cols[6];
        (l1 ? a.o.dp1 : a.o.dpc)[b * gdim + f] = dph;
        (l1 ? a.o.dg1 : a.o.dgc)[b * gdim + f] = fmaf(bias, dph, dot);
        acc_b = fmaf(gn, dph, acc_b);
        if (l1) {
          // layer 0 and the sigma head ride along with feature f
          const float dp0 = cols[0], g0 = a.w.g0[b * H + f];
          float s0[3], dg0 = a.w.b0[f] * dp0;
#pragma unroll
          for (int c = 0; c < 3; ++c) { s0[c] = cols[1 + c] * a.w.box_scale; dg0 = fmaf(s0[c], a.w.w0[f * 3 + c], dg0); acc_w0[c] = fmaf(g0, s0[c], acc_w0[c]); }
          a.o.dp0[b * H + f] = dp0;
          a.o.dg0[b * H + f] = dg0;
          acc_b0 = fmaf(g0, dp0, acc_b0);
          acc_ws += cols[5];
        }
      }
      __syncthreads();
    }
    (l1 ? a.o.dw1 : a.o.dwc)[f * H + j] = acc_w;
    if (j == 0) {
      (l1 ? a.o.db1 : a.o.dbc)[f] = acc_b;
      if (l1) {
        a.o.db0[f] = acc_b0; a.o.dws[f] = acc_ws;
        a.o.dw0[f * 3 + 0] = acc_w0[0]; a.o.dw0[f * 3 + 1] = acc_w0[1]; a.o.dw0[f * 3 + 2] = acc_w0[2];
      }
    }
  } else if (task < 224) {
    const int ch = task - 192;
    if (j < HC) {
      float v = 0.f;
      for (int b = 0; b < B; ++b) {
        float vb = 0.f;
        if constexpr (SEGS) {
          float s0, s1;
          seg_sum(b, a.gpart + GP_GF0 + ch * HC + j, GPART, a.gpart + GP_GF1 + ch * HC + j, GPART, s0, s1);
          vb += s0 + s1;
        } else {
          for (int c = 0; c < C; ++c) vb += at(a.gpart, GPART, b, c, GP_GF0 + ch * HC + j) + at(a.gpart, GPART, b, c, GP_GF1 + ch * HC + j);
        }
        v += vb;
      }
      a.o.dwf[ch * HC + j] = v;
    }
    // the bias: one image's term per thread of the second wave (beside the first wave's walk above), added in image order
    float s = 0.f;
    for (int b0 = 0; b0 < B; b0 += 64) {
      const int b = b0 + j - 64;
      if (j >= 64 && b < B) red[j - 64] = colsum(b, ch, 7) + colsum(b, 64 + ch, 7);     // waves 0 and 2 hold the two halves
      __syncthreads();
      if (j == 0)
        for (int t = 0; t < 64 && b0 + t < B; ++t) s += red[t];
      __syncthreads();
    }
    if (j == 0) a.o.dbf[ch] = s;
  } else {
    // the sigma bias: one row's term per thread, added in row order (images, then chunks)
    float s = 0.f;
    for (int i0 = 0; i0 < B * C; i0 += 128) {
      const int it = i0 + j;
      if (it < B * C) {
        const int b = it / C, c = it % C;
        red[j] = (at(a.sred, SRED, b, c, 1024) + at(a.sred, SRED, b, c, 1025)) + (at(a.sred, SRED, b, c, 1026) + at(a.sred, SRED, b, c, 1027));
      }
      __syncthreads();
      if (j == 0)
        for (int t = 0; t < 128 && i0 + t < B * C; ++t) s += red[t];
      __syncthreads();
    }
    if (j == 0) a.o.dbs[0] = s;
  }
}

}  // namespace

extern "C" int cips_siren_bwd_x3_chunks(int B, int P) {
  const int chunk = x3_chunk(B, P);
  return (P + chunk - 1) / chunk;
}
extern "C" int cips_siren_bwd_x3_gpart(void) { return GPART; }
#ifdef CIPS_TUNING
static unsigned long long* g_prof = nullptr;
extern "C" int cips_siren_bwd_x3_prof(unsigned long long* host_out) {   // tuning aid: copies the 8x4x16 timestamps
  if (!g_prof) return (int)hipErrorNotReady;
  return (int)hipMemcpy(host_out, g_prof, 8 * 4 * 16 * 8, hipMemcpyDeviceToHost);
}
#endif
extern "C" int cips_siren_bwd_x3_sred(void) { return SRED; }


static int siren_bwd_x3_launch(const cips_siren_weights* w, const float* points, const cips_ray_params* rays,
                               const float* dfeat, const float* dsigma, float* sred, float* gpart, int B, int P,
                               cips_stream_t stream, const int* idx = nullptr, const int* count = nullptr,
                               const int* seg = nullptr);

extern "C" int cips_siren_bwd_x3(const cips_siren_weights* w, const float* points, const float* dfeat,
                                 const float* dsigma, float* sred, float* gpart, int B, int P,
                                 cips_stream_t stream) {
  if (!points) return (int)hipErrorInvalidValue;
  return siren_bwd_x3_launch(w, points, nullptr, dfeat, dsigma, sred, gpart, B, P, stream);
}

extern "C" int cips_siren_bwd_x3_rays(const cips_siren_weights* w, const cips_ray_params* rays, const float* dfeat,
                                      const float* dsigma, float* sred, float* gpart, int B, cips_stream_t stream) {
  if (!rays) return (int)hipErrorInvalidValue;
  return siren_bwd_x3_launch(w, nullptr, rays, dfeat, dsigma, sred, gpart, B, rays->W * rays->H * rays->S, stream);
}

extern "C" int cips_siren_bwd_x3_live(const cips_siren_weights* w, const float* points, const float* dfeat,
                                      const float* dsigma, const int* idx, const int* count, float* sred, float* gpart,
                                      int B, int P, cips_stream_t stream) {
  if (!points || !idx || !count) return (int)hipErrorInvalidValue;
  return siren_bwd_x3_launch(w, points, nullptr, dfeat, dsigma, sred, gpart, B, P, stream, idx, count);
}

extern "C" int cips_siren_bwd_x3_rays_live(const cips_siren_weights* w, const cips_ray_params* rays, const float* dfeat,
                                           const float* dsigma, const int* idx, const int* count, float* sred,
                                           float* gpart, int B, cips_stream_t stream) {
  if (!rays || !idx || !count) return (int)hipErrorInvalidValue;
  return siren_bwd_x3_launch(w, nullptr, rays, dfeat, dsigma, sred, gpart, B, rays->W * rays->H * rays->S, stream, idx, count);
}

extern "C" int cips_siren_bwd_x3_live_even(const cips_siren_weights* w, const float* points, const float* dfeat,
                                           const float* dsigma, const int* idx, const int* count, const int* seg,
                                           float* sred, float* gpart, int B, int P, cips_stream_t stream) {
  if (!points || !idx || !count || !seg) return (int)hipErrorInvalidValue;
  return siren_bwd_x3_launch(w, points, nullptr, dfeat, dsigma, sred, gpart, B, P, stream, idx, count, seg);
}

extern "C" int cips_siren_bwd_x3_rays_live_even(const cips_siren_weights* w, const cips_ray_params* rays, const float* dfeat,
                                                const float* dsigma, const int* idx, const int* count, const int* seg,
                                                float* sred, float* gpart, int B, cips_stream_t stream) {
  if (!rays || !idx || !count || !seg) return (int)hipErrorInvalidValue;
  return siren_bwd_x3_launch(w, nullptr, rays, dfeat, dsigma, sred, gpart, B, rays->W * rays->H * rays->S, stream, idx, count, seg);
}

extern "C" int cips_siren_bwd_x3_live_plan_host(const int* count, int B, int P, int* seg, int* img) {
  if (!count || !seg || !img || B <= 0 || P <= 0) return (int)hipErrorInvalidValue;
  x3_even_plan(count, B, P, B * cips_siren_bwd_x3_chunks(B, P), seg, img, X3Solo{});
  return 0;
}

extern "C" int cips_siren_bwd_x3_live_plan(const int* count, int B, int P, int* seg, int* img, cips_stream_t stream) {
  if (!count || !seg || !img || B <= 0 || P <= 0) return (int)hipErrorInvalidValue;
  const int G = B * cips_siren_bwd_x3_chunks(B, P);
  hipLaunchKernelGGL(siren_bwd_plan_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, count, B, P, G, seg, img);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_siren_bwd_x3_reduce_segments(const float* sred, const float* gpart, const int* img, int B, float* sred_out,
                                                 float* gpart_out, cips_stream_t stream) {
  if (!sred || !gpart || !img || !sred_out || !gpart_out || B <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(siren_bwd_reduce_segments_kernel, dim3((RS_G4 + RS_S4 + 255) / 256, B), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4*>(sred), reinterpret_cast<const float4*>(gpart), img,
                     reinterpret_cast<float4*>(sred_out), reinterpret_cast<float4*>(gpart_out));
  return CIPS_CHECK_LAUNCH();
}

static int siren_bwd_x3_launch(const cips_siren_weights* w, const float* points, const cips_ray_params* rays,
                               const float* dfeat, const float* dsigma, float* sred, float* gpart, int B, int P,
                               cips_stream_t stream, const int* idx, const int* count, const int* seg) {
  if (!w || !dfeat || !dsigma || !sred || !gpart || B <= 0 || P <= 0) return (int)hipErrorInvalidValue;
  BwdX3Args a;
  a.idx = idx; a.count = count; a.seg = seg;
  a.w = *w; a.points = points; a.dfeat = dfeat; a.dsigma = dsigma; a.sred = sred; a.gpart = gpart;
  a.B = B; a.P = P;
  a.rg = RayGen{};
  if (!points) { const int rc = fill_raygen(a.rg, rays); if (rc) return rc; }
  a.dbg = 0; a.prof = nullptr;
#ifdef CIPS_TUNING
  a.dbg = cips_tune_env("CIPS_X3_DBG", 0);
  static unsigned long long* prof = nullptr;
  static int want_prof = -1;
  if (want_prof < 0) {
    want_prof = cips_tune_env("CIPS_X3_PROF", 0) ? 1 : 0;
    if (want_prof && hipMalloc(&prof, 8 * 4 * 16 * 8) != hipSuccess) prof = nullptr;
  }
  a.prof = prof; g_prof = prof;
#endif
  a.chunk = x3_chunk(B, P);
  a.chunks = (P + a.chunk - 1) / a.chunk;
  dim3 grid(a.chunks, B);
  auto go = [&](auto HW_, auto MODE_) {
    x3_launch<siren_bwd_x4_kernel<decltype(HW_)::value, decltype(MODE_)::value>>(grid, 256, SMEM_BYTES, stream, a);
  };
  x3_pick([&](auto HW_) {
    if (seg) go(HW_, std::integral_constant<int, X3_EVEN>{});
    else if (idx) go(HW_, std::integral_constant<int, X3_LIVE>{});
    else go(HW_, std::integral_constant<int, X3_DENSE>{});
  }, (w->trig_mode & 1) != 0);
  return CIPS_CHECK_LAUNCH();
}

static int siren_bwd_finalize_launch(const cips_siren_weights* w, const float* sred, const float* gpart, const int* img, int B,
                                     int chunks, const cips_siren_grads* out, cips_stream_t stream) {
  if (!w || !sred || !gpart || !out || B <= 0 || chunks <= 0) return (int)hipErrorInvalidValue;
  const float* const* po = reinterpret_cast<const float* const*>(out);
  for (int i = 0; i < 16; ++i) if (!po[i]) return (int)hipErrorInvalidValue;
  FinArgs a;
  a.w = *w; a.sred = sred; a.gpart = gpart; a.img = img; a.o = *out; a.B = B; a.chunks = chunks;
  if (img) hipLaunchKernelGGL(siren_bwd_finalize_kernel<true>, dim3(225), dim3(128), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(siren_bwd_finalize_kernel<false>, dim3(225), dim3(128), 0, (hipStream_t)stream, a);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_siren_bwd_x3_finalize(const cips_siren_weights* w, const float* sred, const float* gpart, int B,
                                          int chunks, const cips_siren_grads* out, cips_stream_t stream) {
  return siren_bwd_finalize_launch(w, sred, gpart, nullptr, B, chunks, out, stream);
}

extern "C" int cips_siren_bwd_x3_finalize_segments(const cips_siren_weights* w, const float* sred, const float* gpart,
                                                   const int* img, int B, const cips_siren_grads* out, cips_stream_t stream) {
  if (!img) return (int)hipErrorInvalidValue;
  return siren_bwd_finalize_launch(w, sred, gpart, img, B, 1, out, stream);
}
