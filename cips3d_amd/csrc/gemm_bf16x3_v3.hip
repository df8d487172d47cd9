// gemm_bf16x3_v3.hip — third form of the split-bf16 "NT" GEMM for the CIPS head's large shapes
// (M = pixels per image, N = K = 512; numerics, operand planes and epilogue contract: gemm_bf16x3.hip; the tile
// geometry, the LDS image and the LDS-DMA staging are those of gemm_bf16x3_wide.hip).  What changes is the schedule:
//
//   * the wave's 12 operand fragments of a k-step live in TWO register sets: the ds_read_b128 of k-step j+1 are issued
//     between the MFMAs of k-step j, so no k-step opens with the matrix pipe waiting for twelve LDS reads (the two
//     waves of a SIMD run in lockstep behind the barriers, so the partner could not cover that wait either: 148 us of
//     fragment reads + MFMAs against 106 us of MFMAs in the round-2 kernel);
//   * one barrier per k-tile, placed four MFMAs into the tile's second k-step: by then every wave has issued (and
//     waited for) its last fragment read of the stage, so the barrier both publishes k-tile t+1 (DMA'd a whole k-tile
//     period earlier) and frees the current stage for k-tile t+2, whose eight DMA pieces follow one per two MFMAs;
//   * the epilogue's transposing scratch is private to the wave and does NOT alias a stage (2 x 64 KiB stages +
//     8 x 4 KiB = all 160 KiB of the CU): the first TWO k-tiles of the workgroup's next output tile stream into both
//     stages under the epilogue, and the epilogue needs no workgroup barrier;
//   * the epilogue itself is about half the instructions: all tiles are interior (the entry point refuses other shapes),
//     uniform base pointers + one 32-bit lane offset per tensor, LeakyReLU + gate bit in 4 instructions per element
//     (v_cmp / v_cndmask / v_addc carry trick), gate application as bfe_i32 + bfi, steps of 8 rows x 64 columns ping-pong
//     through the scratch so the LDS round trip of one step hides behind the arithmetic of the other; eight adjacent
//     lanes move a whole 128-byte line of a plane row (stores and the residual / addend loads: a mixed read + write
//     stream of 64-byte pieces runs at 4.85 TB/s, of whole lines at 5.59, profiles/r6_head_gemm_epilogue_experiments.txt),
//     and the gate bit plane is written as one dword per four lanes.
// Accumulation order and epilogue arithmetic are those of the wide kernel: results are bit-identical to it.
//
// Restrictions (else hipErrorNotSupported and the caller falls back to gemm_bf16x3_wide): M, N multiples of 256,
// K a multiple of 64, no transposed planes, gate planes as bit planes, 16-byte aligned rows of every tensor.  B planes [K][ldb]
// (b_kmajor, the BKM instantiations below): the backward's epilogues only, 3-pass only — and no fallback, the entry point
// refuses what this kernel does not take.
#include "gemm_x3_common.h"
#include "../../include/cips3d_hip.h"
#include <utility>

namespace {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));

constexpr int BM = 256, BN = 256, BK = 32, ROWB = 64;
constexpr int KROW = 512;                       // BKM: bytes per k-row of the B image (256 bf16)
constexpr int OFF_AHI = 0, OFF_ALO = BM * ROWB, OFF_BHI = 2 * BM * ROWB, OFF_BLO = OFF_BHI + BN * ROWB;
constexpr int STAGE = OFF_BLO + BN * ROWB;      // 65536
constexpr int SCR_OFF = 2 * STAGE;              // the epilogue scratch starts behind the two stages
constexpr int SCR_WAVE = 4096;                  // per wave: two fp32 [8][64] halves (ping-pong)
constexpr int SMEM_BYTES = SCR_OFF + 8 * SCR_WAVE;
static_assert(SMEM_BYTES == 163840, "the kernel owns the whole LDS of the CU");
static_assert(OFF_ALO == X3_PLANE_BYTES && OFF_BHI == 2 * X3_PLANE_BYTES && OFF_BLO == 3 * X3_PLANE_BYTES && ROWB == 64, "stage layout of gemm_x3_common.h");

struct VArgs {
  cips_gemm_x3_desc d;
  int tiles_m, tiles_n, total;
};

#define LDS_B128(a) (*((__attribute__((address_space(3))) const bf16x8*)(uintptr_t)(a)))
#define LDS_F4(a) (*((__attribute__((address_space(3))) const f32x4*)(uintptr_t)(a)))
#define LDS_W32(a) (*((__attribute__((address_space(3))) float*)(uintptr_t)(a)))
#define LDS_TR(a) __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)(uintptr_t)(a))
#define SB() __builtin_amdgcn_sched_barrier(0)

// FAST: the epilogue shapes of the training step, decided at compile time — planes out, no fp32 C; forward flavours
// (no gate input) apply the LeakyReLU and write the gate bit plane, backward flavours (gate input) do neither; only
// C_unmasked (the skip gradient of the add flavour) stays a run-time switch.  !FAST: every switch of the descriptor.
// RGBF: ToRGB forward folded in (descriptor fields torgb_w / torgb_part): per row and 128-column block the three partial
// dot products of the final values with the ToRGB weights, accumulated over the wave's four column sub-blocks as four
// chains per row (handed between lanes by DPP), combined with two DPP adds and stored as one float4 per row.
// ADDP: the addend (HAS_ADD) arrives as the split planes of a gated tensor plus the bit plane of that gate (descriptor fields
// addp_*): value = (hi + lo) * (bit ? 1 : addp_gain), same bytes in as the fp32 addend, and no C_unmasked copy is needed by
// the next layer.
// X1: the single-pass form (cips_gemm_bf16: sum_k a_hi b_hi, lo operand planes never addressed) — stage contents, fragment
// numbering and the k-tile schedule x1_ktile are described in gemm_x3_common.h; tile walk, DMA pieces and epilogue are
// the ones below.  K is a multiple of 128 (an even number of 64-deep k-tiles, at least two).
// BKM: the B planes are row-major [K][ldb] (descriptor field b_kmajor: the head's dX GEMMs on the forward's wbt planes).  The
// B half of a stage is then the K-major image of gemm_bf16x3_km_wide.hip — 32 k-rows of 512 bytes per plane, 32-byte column
// pairs XOR-swizzled by 2 (k & 3) in the DMA source address, pieces of 2 k-rows x 512 bytes at the same LDS places as the NT
// pieces — and a B fragment is two ds_read_b64_tr_b16 (k-rows kb and kb + 4) into the registers of the one ds_read_b128:
// same values in the same lanes, same MFMA order, bit-identical results; the A half, the barrier, the DMA slots and the
// epilogue are untouched.  The four 32-column tiles of the wave's B block meet the swizzle in address bits 6-7, so each has
// a lane base of its own (bq[4], in place of the NT form's two); k-step 1 is an immediate (+ 16 k-rows) and the stage flips
// by one add per base and k-tile.  3-pass only.
template <bool HAS_ADD, bool HAS_MASK, bool HAS_RES, bool FAST, bool RGBF = false, bool ADDP = false, bool X1 = false, bool BKM = false>
__global__ __launch_bounds__(512) void gemm_bf16x3_v3_kernel(VArgs g) {
  static_assert(!(BKM && X1), "the single-pass form reads B contraction-contiguous only");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const cips_gemm_x3_desc& d = g.d;
  const int tid = threadIdx.x;
  const int lane0 = tid & 63;
  const int uw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = uw >> 1, wn = uw & 1;                     // 4 x 2 waves, 64 x 128 outputs each
  constexpr int KT = X1 ? X1_BK : BK;                      // contraction depth of an LDS stage
  const int nk = d.K / KT;                                 // even, >= 2
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)smem);

  auto decode = [&](int t, int& tm, int& tn, int& bz) {
    const int bid = xcd_tile(t, g.total);
    tn = bid % g.tiles_n;
    tm = (bid / g.tiles_n) % g.tiles_m;
    bz = bid / (g.tiles_n * g.tiles_m);
  };
  // LDS-DMA source of one output tile: four uniform plane pointers + one 32-bit byte offset per lane, operand and
  // row-group half (lane L = row L>>2 of the wave's 16-row group, 16-byte slot (L&3) ^ ((row>>2)&3): the swizzle
  // lives in the source address, the LDS image is lane-linear)
  struct Src { const u16 *Ahi, *Alo, *Bhi, *Blo; unsigned offA[2], offB[2]; };
  auto make_src = [&](int tm, int tn, int bz, int lane, Src& sr) {
    sr.Ahi = (const u16*)d.A_hi + (long long)bz * d.strideA + (long long)tm * BM * d.lda;
    if constexpr (X1) {                   // planes 1 and 3 of the stage: the hi planes' second 32 contraction indices
      sr.Bhi = (const u16*)d.B_hi + (long long)bz * d.strideB + (long long)tn * BN * d.ldb;
      sr.Alo = sr.Ahi + 32;
      sr.Blo = sr.Bhi + 32;
    } else {
      sr.Alo = (const u16*)d.A_lo + (long long)bz * d.strideA + (long long)tm * BM * d.lda;
      const long long bt = BKM ? (long long)tn * BN : (long long)tn * BN * d.ldb;       // the tile's columns / rows of B
      sr.Bhi = (const u16*)d.B_hi + (long long)bz * d.strideB + bt;
      sr.Blo = (const u16*)d.B_lo + (long long)bz * d.strideB + bt;
    }
    const int drow = lane >> 2, dslot = lane & 3;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = (uw + 8 * p) * 16 + drow;
      const int kcsw = dslot ^ ((row >> 2) & 3);
      sr.offA[p] = (unsigned)(row * d.lda + kcsw * 8) * 2u;
      if constexpr (BKM) {
        // piece idx = uw + 8 p: k-rows 2 idx + (lane >> 5), 16-byte chunk lane & 31 of the row; the LDS place c16 holds the
        // columns of chunk 2 pr + (c16 & 1), pr = (c16 >> 1) ^ 2 (k & 3), k & 3 = 2 (uw & 1) + (lane >> 5) for both p
        const int lh = lane >> 5, c16 = lane & 31;
        const int pr = (c16 >> 1) ^ (2 * (2 * (uw & 1) + lh));
        sr.offB[p] = (unsigned)(lh * d.ldb + (pr * 2 + (c16 & 1)) * 8) * 2u;
      } else {
        sr.offB[p] = (unsigned)(row * d.ldb + kcsw * 8) * 2u;
      }
    }
  };
  // piece pc = 0..7 of the k-tile starting at contraction index k0, into the stage at LDS byte offset `st`
  auto dma_piece = [&](const Src& sr, int pc, int k0, unsigned st) {
    const int pp = pc >> 2, which = pc & 3;
    const unsigned la = sbase + st + (unsigned)((uw + 8 * pp) * 16 * ROWB);
    if (which == 0) lds_dma16(sr.Ahi + k0, sr.offA[pp], la + OFF_AHI);
    else if (which == 1) lds_dma16(sr.Alo + k0, sr.offA[pp], la + OFF_ALO);
    else if constexpr (BKM) {
      const long long krow = (long long)(k0 + 2 * (uw + 8 * pp)) * d.ldb;      // the piece's first k-row (uniform)
      if (which == 2) lds_dma16(sr.Bhi + krow, sr.offB[pp], la + OFF_BHI);
      else lds_dma16(sr.Blo + krow, sr.offB[pp], la + OFF_BLO);
    }
    else if (which == 2) lds_dma16(sr.Bhi + k0, sr.offB[pp], la + OFF_BHI);
    else lds_dma16(sr.Blo + k0, sr.offB[pp], la + OFF_BLO);
  };

  // ---- kernel prologue: the first tile's k-tiles 0 and 1
  bool have = (int)blockIdx.x < g.total;
  if (have) {
    int tm, tn, bz;
    decode(blockIdx.x, tm, tn, bz);
    Src s0;
    make_src(tm, tn, bz, lane0, s0);
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) dma_piece(s0, pc, 0, 0);
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) dma_piece(s0, pc, KT, STAGE);
  }
  int younger = 0;        // lower bound of the VMEM operations issued after the 16 DMA pieces of the coming tile

  for (int tseq = blockIdx.x; tseq < g.total; tseq += gridDim.x) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));        // keeps the per-lane epilogue addresses out of the persistent loop's preheader
    const int l31 = lane & 31, hf = lane >> 5;
    int tm, tn, bz;
    decode(tseq, tm, tn, bz);
    const int m0 = tm * BM, n0 = tn * BN;
    Src src;
    make_src(tm, tn, bz, lane, src);
    const int tnext = tseq + (int)gridDim.x;
    const bool have_next = tnext < g.total;

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment read addresses: row R = tile row + lane&31, 16-byte chunk (2 ks + hf) ^ ((R>>2)&3); one lane base per
    // operand and k-step, everything else is an immediate
    const int csw = (l31 >> 2) & 3;
    const unsigned fa0 = sbase + (wm * 64 + l31) * ROWB + ((hf ^ csw) << 4), fa1 = sbase + (wm * 64 + l31) * ROWB + (((2 + hf) ^ csw) << 4);
    const unsigned fb0 = sbase + (wn * 128 + l31) * ROWB + ((hf ^ csw) << 4), fb1 = sbase + (wn * 128 + l31) * ROWB + (((2 + hf) ^ csw) << 4);

    // BKM, transpose reads of the B image: lane = column 16 (lane>>4 & 1) + 4 (lane & 3) .. + 4 of the 32-column tile, k-row
    // kb = 8 hf + (lane>>2 & 3) (+ 4 for the second read, + 16 for k-step 1: kb & 3 is the same for all four), 32-byte pair
    // (col >> 4) ^ 2 (kb & 3).  bq[j]: tile j of the stage whose k-step 0 is read next (stage 0 here; ktile flips it)
    unsigned bq[4] = {0, 0, 0, 0};
    if constexpr (BKM) {
      const int s16 = lane & 15, mhalf = (lane >> 4) & 1;
      const int kb = 8 * hf + (s16 >> 2);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = wn * 128 + j * 32 + 16 * mhalf + 4 * (s16 & 3);
        bq[j] = sbase + kb * KROW + (((col >> 4) ^ (2 * (kb & 3))) << 5) + (col & 15) * 2;
      }
    }
    auto frag_tr = [&](unsigned a) -> bf16x8 {
      const short4v x = LDS_TR(a), y = LDS_TR(a + 4 * KROW);
      const short8v v = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
      return __builtin_bit_cast(bf16x8, v);
    };
    // fragment q of the 3-pass k-step: A (and the NT B) from the lane base of its operand, the BKM B from bq + KOFF
    auto rdq = [&](auto Q_, unsigned abase, unsigned bbase, auto KOFF_) -> bf16x8 {
      constexpr int q = decltype(Q_)::value;
      if constexpr (x3_frag_is_a(q)) return LDS_B128(abase + x3_frag_off_nt(q));
      else if constexpr (BKM) return frag_tr(bq[x3_frag_tile(q)] + x3_frag_plane(q) + decltype(KOFF_)::value);
      else return LDS_B128(bbase + x3_frag_off_nt(q));
    };
    constexpr std::integral_constant<int, 0> KS0{};
    constexpr std::integral_constant<int, 16 * KROW> KS1{};

    bf16x8 F0[12], F1[12];        // the 3-pass schedule's two fragment sets
    bf16x8 G[2][6];               // the single-pass schedule's

    // ---- epilogue plumbing declared here: the first inputs are requested inside the last k-tile
    const long long cbase = (long long)bz * d.strideC + (long long)m0 * d.ldc + n0;      // fp32 tensors (ld = ldc)
    const long long pbase = (long long)bz * d.strideP + (long long)m0 * d.ldp + n0;      // planes / gate planes (ld = ldp)
    auto st16 = [&](void* ubase, unsigned off, u32x4 v) { *(u32x4*)((char*)ubase + off) = v; };
    auto st16f = [&](void* ubase, unsigned off, float a, float b, float c, float e) {
      u32x4 v = {__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(e)};
      st16(ubase, off, v);
    };
    // an epilogue step is 8 rows x 64 columns of the wave's 64 x 128 block: lane = (row h_rr, 8-column chunk c8), so the
    // eight lanes of a row move one whole 128-byte line of each bf16 plane per instruction (stores, residual and addend loads)
    // and the row's 8 bytes of a gate bit plane; q2 = the lane's place in its quad (the bit plane moves as one dword per quad).
    // Lane group j = lane >> 3 takes row 0,1,5,4,2,3,7,6 of the step: a ds_read_b128 serves lanes in groups of 16 that hold
    // halves of the lane groups (0,1,2,3) or (4,5,6,7), and this order puts the pairs that meet on the same 16-byte chunks,
    // (0,3), (1,2), (4,7), (5,6), on opposite sides of row 4, which is all the scratch image's swizzle looks at (below)
    // They are derived inside the last k-tile (its second k-step, where one fragment set is dead), in front of the first
    // input requests: held across the main loop they put the <1,1,0,!FAST> instantiation 8 bytes into scratch.
    int c8, q2, h_rr;
    unsigned eC, eP;                                                                       // lane element offsets in the tile
    auto epi_lanes = [&]() {
      int l = lane;
      asm volatile("" : "+v"(l));
      c8 = l & 7; q2 = l & 3;
      h_rr = ((l >> 2) & 4) | ((l >> 4) & 2) | (((l >> 3) ^ (l >> 4)) & 1);
      eC = (unsigned)((wm * 64 + h_rr) * d.ldc + wn * 128 + c8 * 8);
      eP = (unsigned)((wm * 64 + h_rr) * d.ldp + wn * 128 + c8 * 8);
    };
    // step hs = (row set hs >> 1: rows 8 (hs >> 1) .. + 8, column half hs & 1): the column half runs innermost, so the two
    // 128-byte lines of a row's 256 output bytes are stored back to back (column-innermost against column-outermost order,
    // measured on the C2 shape with 64-byte pieces: plain 232 -> 210 us, res 280 -> 266, gate 236 -> 220, add 363 -> 351),
    // and a row's ToRGB sums (RGBF) are complete after two consecutive steps: one set of three accumulators is live
    auto CP = [](int hs) -> int { return hs & 1; };
    auto RS = [](int hs) -> int { return hs >> 1; };
    auto uoffC = [&](int hs) -> long long { return (long long)(RS(hs) * 8) * d.ldc + CP(hs) * 64; };
    auto uoffP = [&](int hs) -> long long { return (long long)(RS(hs) * 8) * d.ldp + CP(hs) * 64; };
    struct Pre { float4 add[(HAS_ADD && !ADDP) ? 2 : 1]; float gg[HAS_ADD ? 3 : 1]; unsigned mask, amask; uint4 rh, rl; };      // rh / rl: residual planes (HAS_RES) or the planes addend (ADDP)
    const bool has_rgb = HAS_ADD && d.rgb_g != nullptr;
    auto prefetch = [&](int hs, Pre& p) {
      if constexpr (HAS_ADD) {
        if constexpr (ADDP) {
          const char* qh = (const char*)((const u16*)d.addp_hi + pbase + uoffP(hs));
          const char* ql = (const char*)((const u16*)d.addp_lo + pbase + uoffP(hs));
          p.rh = *reinterpret_cast<const uint4*>(qh + eP * 2u);
          p.rl = *reinterpret_cast<const uint4*>(ql + eP * 2u);
          const unsigned char* q = (const unsigned char*)d.addp_gate + ((pbase + uoffP(hs)) >> 3);
          p.amask = q[eP >> 3];
        } else {
          const char* q = (const char*)(d.add + cbase + uoffC(hs));
          p.add[0] = *reinterpret_cast<const float4*>(q + eC * 4u);
          p.add[1] = *reinterpret_cast<const float4*>(q + eC * 4u + 16);
        }
        if (has_rgb) {
          const int row = m0 + wm * 64 + RS(hs) * 8 + h_rr;
          const float* gp = d.rgb_g + ((long long)bz * d.M + row) * 3;
          p.gg[0] = gp[0]; p.gg[1] = gp[1]; p.gg[2] = gp[2];
        }
      }
      if constexpr (HAS_MASK) {
        const unsigned char* q = (const unsigned char*)d.mask + ((pbase + uoffP(hs)) >> 3);
        p.mask = q[eP >> 3];
      }
      if constexpr (HAS_RES) {
        const char* qh = (const char*)((const u16*)d.res_hi + pbase + uoffP(hs));
        const char* ql = (const char*)((const u16*)d.res_lo + pbase + uoffP(hs));
        p.rh = *reinterpret_cast<const uint4*>(qh + eP * 2u);
        p.rl = *reinterpret_cast<const uint4*>(ql + eP * 2u);
      }
    };
    constexpr bool HAS_IN = HAS_ADD || HAS_MASK || HAS_RES;
    constexpr int NPF = (HAS_ADD || RGBF) ? 3 : 4;        // ring of epilogue-input slots; slot hs % NPF is refilled NPF-1 steps ahead
    Pre pre[NPF];

    // ---- one k-tile.  MODE 0: steady state (fragments of the next k-tile + DMA of k-tile kt+2); 1: next-to-last
    // (fragments only); 2: last (epilogue inputs + the next output tile's two first k-tiles)
    auto ktile = [&](auto MODE_, int kt) {
      constexpr int MODE = decltype(MODE_)::value;
      const unsigned cur = (unsigned)(kt & 1) * STAGE, nxt = STAGE - cur;
      unsigned a1 = fa1 + cur, b1 = fb1 + cur, a0n = fa0 + nxt, b0n = fb0 + nxt;
      if constexpr (BKM) asm volatile("" : "+v"(a1), "+v"(a0n));
      else asm volatile("" : "+v"(a1), "+v"(b1), "+v"(a0n), "+v"(b0n));
      // k-step a: MFMAs on set 0, the twelve reads of k-step b into set 1 (one per two MFMAs)
      static_for(std::make_integer_sequence<int, 24>{}, [&](auto M_) {
        constexpr int m = decltype(M_)::value;
        acc[(m >> 2) & 1][m & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F0[x3_mfma_a(m)], F0[x3_mfma_b(m)], acc[(m >> 2) & 1][m & 3], 0, 0, 0);
        if constexpr ((m & 1) == 0) {
          constexpr int q = m >> 1;
          F1[q] = rdq(std::integral_constant<int, q>{}, a1, b1, KS1);
        }
        if constexpr (BKM && m == 23) {       // the last B read of stage `cur` is issued: the bases move to stage `nxt`
#pragma unroll
          for (int j = 0; j < 4; ++j) bq[j] += nxt - cur;
        }
        SB();
      });
      // k-step b
      Src nsrc;
      if constexpr (MODE == 2) {
        epi_lanes();
        if (have_next) {
          int tm2, tn2, bz2;
          decode(tnext, tm2, tn2, bz2);
          make_src(tm2, tn2, bz2, lane, nsrc);
        }
      }
      static_for(std::make_integer_sequence<int, 24>{}, [&](auto M_) {
        constexpr int m = decltype(M_)::value;
        acc[(m >> 2) & 1][m & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F1[x3_mfma_a(m)], F1[x3_mfma_b(m)], acc[(m >> 2) & 1][m & 3], 0, 0, 0);
        if constexpr (m == 3) {
          // every fragment read of stage `cur` has returned (lgkmcnt), this wave's pieces of k-tile kt+1 have landed
          // (vmcnt; they were issued a k-tile period ago): behind the barrier stage `nxt` is readable, `cur` writable
          asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        if constexpr (MODE == 0) {
          if constexpr (m >= 4 && m <= 18 && (m & 1) == 0) dma_piece(src, (m - 4) >> 1, (kt + 2) * BK, cur);
        }
        if constexpr (MODE <= 1) {
          if constexpr (m >= 5 && m <= 15 && (m & 1) == 1) {
            constexpr int q = m - 5;
            F0[q] = rdq(std::integral_constant<int, q>{}, a0n, b0n, KS0);
            F0[q + 1] = rdq(std::integral_constant<int, q + 1>{}, a0n, b0n, KS0);
          }
        }
        if constexpr (MODE == 2) {
          if constexpr (HAS_IN && m >= 4 && m < 4 + NPF - 1) prefetch(m - 4, pre[m - 4]);
          if constexpr (m >= 7 && m <= 22) {
            if (have_next) dma_piece(nsrc, (m - 7) & 7, ((m - 7) >> 3) * BK, (unsigned)((m - 7) >> 3) * STAGE);
          }
        }
        SB();
      });
    };

    // ---- single pass: the same three k-tile forms on x1_ktile.  MODE 0 refills this stage behind the barrier; MODE 2 requests
    // the next output tile's k-tile 0 into the other stage (free since the previous k-tile's barrier) under its first two
    // k-steps, the first epilogue inputs under the third, and k-tile 1 into this stage behind the barrier
    auto ktile1 = [&](auto MODE_, int kt) {
      constexpr int MODE = decltype(MODE_)::value;
      const unsigned cur = (unsigned)(kt & 1) * STAGE, nxt = STAGE - cur;
      unsigned ac0 = fa0 + cur, ac1 = fa1 + cur, bc0 = fb0 + cur, bc1 = fb1 + cur, an = fa0 + nxt, bn = fb0 + nxt;
      asm volatile("" : "+v"(ac0), "+v"(ac1), "+v"(bc0), "+v"(bc1), "+v"(an), "+v"(bn));
      Src nsrc;
      if constexpr (MODE == 2) {
        epi_lanes();
        if (have_next) {
          int tm2, tn2, bz2;
          decode(tnext, tm2, tn2, bz2);
          make_src(tm2, tn2, bz2, lane, nsrc);
        }
      }
      auto rd = [&](auto Q_, auto S_, auto NEXT_) -> bf16x8 {
        constexpr int q = decltype(Q_)::value, s = decltype(S_)::value;
        constexpr int off = x1_frag_plane(q, s) + x1_frag_tile(q) * 32 * ROWB;
        if constexpr (decltype(NEXT_)::value) return LDS_B128((x1_frag_is_a(q) ? an : bn) + off);
        else return LDS_B128((x1_frag_is_a(q) ? ((s & 1) ? ac1 : ac0) : ((s & 1) ? bc1 : bc0)) + off);
      };
      auto slot = [&](auto S_, auto M_) {
        constexpr int s = decltype(S_)::value, m = decltype(M_)::value;
        if constexpr (MODE == 0 && s == 3 && m >= 2) {
#pragma unroll
          for (int i = 0; i < x1_pieces(m); ++i) dma_piece(src, x1_piece0(m) + i, (kt + 2) * KT, cur);
        }
        if constexpr (MODE == 2) {
          if constexpr (s < 2 && (m & 1) == 0) {
            if (have_next) dma_piece(nsrc, 4 * s + (m >> 1), 0, 0);
          }
          if constexpr (HAS_IN && s == 2 && m < NPF - 1) prefetch(m, pre[m]);
          if constexpr (s == 3 && m >= 2) {
            if (have_next) {
#pragma unroll
              for (int i = 0; i < x1_pieces(m); ++i) dma_piece(nsrc, x1_piece0(m) + i, KT, STAGE);
            }
          }
        }
      };
      x1_ktile<MODE>(acc, G, rd, slot);
    };

    // ---- tile start: k-tile 0 has landed everywhere; its first fragments (the only exposed reads of the tile)
    if (younger >= 24) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");      // 8 pieces of k-tile 1 + >= 24 younger ops stay in flight
    else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    if constexpr (X1) {
      static_for(std::make_integer_sequence<int, 6>{}, [&](auto Q_) {
        constexpr int q = decltype(Q_)::value;
        G[0][q] = LDS_B128((x1_frag_is_a(q) ? fa0 : fb0) + x1_frag_plane(q, 0) + x1_frag_tile(q) * 32 * ROWB);
      });
      SB();
      for (int kt = 0; kt < nk - 2; ++kt) ktile1(std::integral_constant<int, 0>{}, kt);
      ktile1(std::integral_constant<int, 1>{}, nk - 2);
      ktile1(std::integral_constant<int, 2>{}, nk - 1);
    } else {
      static_for(std::make_integer_sequence<int, 12>{}, [&](auto Q_) { F0[decltype(Q_)::value] = rdq(Q_, fa0, fb0, KS0); });
      SB();
      for (int kt = 0; kt < nk - 2; ++kt) ktile(std::integral_constant<int, 0>{}, kt);
      ktile(std::integral_constant<int, 1>{}, nk - 2);
      ktile(std::integral_constant<int, 2>{}, nk - 1);
    }

    // ---- epilogue (order of operations: +add, +rgb term, C_unmasked, gate, act, mask_out, +res, outputs)
    u16* Phi = (u16*)d.P_hi; u16* Plo = (u16*)d.P_lo;
    const bool do_act = FAST ? !HAS_MASK : (d.act != 0);
    const bool do_bits = FAST ? !HAS_MASK : (d.mask_out != nullptr);
    const bool do_c = FAST ? false : (d.C != nullptr);
    const bool do_p = FAST ? true : (Phi != nullptr);
    const bool do_cu = (FAST && !HAS_ADD) ? false : (d.C_unmasked != nullptr);
    younger = (has_rgb || !(do_p || do_c)) ? 0 : 24;
    const unsigned sw = sbase + SCR_OFF + uw * SCR_WAVE;
    // scratch image of a step: fp32 [8][64] (rows of 256 bytes = all 64 banks), the 16-byte chunk index of row R XORed
    // with R>>2.  Writes (MFMA layout: a ds_write_b32 puts 32 consecutive columns of rows r and r + 4, one row per
    // 32-lane group, the XOR permutes chunks inside the group's 128 bytes) and reads (ds_read_b128: a 16-lane group holds
    // the 8-column chunks 0-3 of two rows and 4-7 of two rows, every lane the same half of its 32 bytes; each pair lies
    // on opposite sides of row 4, so the XOR sends it to opposite halves) are both conflict-free
    const unsigned wb = sw + (4 * hf) * 256 + (l31 ^ (4 * hf)) * 4;
    const unsigned rsw = h_rr >> 2;
    const unsigned rb0 = sw + h_rr * 256 + (((2 * c8) ^ rsw) << 4), rb1 = sw + h_rr * 256 + (((2 * c8 + 1) ^ rsw) << 4);
    auto put = [&](auto HS_) {                // accumulators of step hs -> scratch half hs & 1
      constexpr int hs = decltype(HS_)::value, cp = hs & 1, rsx = hs >> 1, si = rsx >> 2, g = rsx & 3;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r)           // accumulator register 4 g + r: tile row 8 g + 4 hf + r, column lane & 31
          LDS_W32(wb + (hs & 1) * 2048 + r * 256 + c * 128) = acc[si][2 * cp + c][4 * g + r];
    };
    float rw[3][8];                           // rgb_w columns of the current column block
    float tacc[3] = {0.f, 0.f, 0.f};          // RGBF: the current row set's ToRGB sums
    put(std::integral_constant<int, 0>{});
    static_for(std::make_integer_sequence<int, 16>{}, [&](auto HS_) {
      constexpr int hs = decltype(HS_)::value;
      if constexpr (hs + 1 < 16) put(std::integral_constant<int, hs + 1>{});
      float y[8];
      {
        const f32x4 a = LDS_F4(rb0 + (hs & 1) * 2048), b = LDS_F4(rb1 + (hs & 1) * 2048);
        y[0] = a[0]; y[1] = a[1]; y[2] = a[2]; y[3] = a[3]; y[4] = b[0]; y[5] = b[1]; y[6] = b[2]; y[7] = b[3];
      }
      Pre& cur = pre[hs % NPF];
      const long long uc = uoffC(hs), up = uoffP(hs);
      if constexpr (HAS_ADD) {
        if constexpr (ADDP) {
          const unsigned wh[4] = {cur.rh.x, cur.rh.y, cur.rh.z, cur.rh.w}, wl[4] = {cur.rl.x, cur.rl.y, cur.rl.z, cur.rl.w};
          const unsigned am = cur.amask;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float v0 = __uint_as_float(wh[e] << 16) + __uint_as_float(wl[e] << 16);
            const float v1 = __uint_as_float(wh[e] & 0xffff0000u) + __uint_as_float(wl[e] & 0xffff0000u);
            const int s0 = ((int)(am << (31 - 2 * e))) >> 31, s1 = ((int)(am << (30 - 2 * e))) >> 31;
            const float t0 = v0 * d.addp_gain, t1 = v1 * d.addp_gain;
            y[2 * e] += __int_as_float((s0 & __float_as_int(v0)) | (~s0 & __float_as_int(t0)));
            y[2 * e + 1] += __int_as_float((s1 & __float_as_int(v1)) | (~s1 & __float_as_int(t1)));
          }
        } else {
          y[0] += cur.add[0].x; y[1] += cur.add[0].y; y[2] += cur.add[0].z; y[3] += cur.add[0].w;
          y[4] += cur.add[1].x; y[5] += cur.add[1].y; y[6] += cur.add[1].z; y[7] += cur.add[1].w;
        }
        if (has_rgb) {                                       // rank-3 term: + g[row][0..2] . rgb_w[0..2][col..col+8]
          {
            const int col = n0 + wn * 128 + (hs & 1) * 64 + c8 * 8;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float4 w0 = *reinterpret_cast<const float4*>(d.rgb_w + (long long)c * d.N + col);
              const float4 w1 = *reinterpret_cast<const float4*>(d.rgb_w + (long long)c * d.N + col + 4);
              rw[c][0] = w0.x; rw[c][1] = w0.y; rw[c][2] = w0.z; rw[c][3] = w0.w; rw[c][4] = w1.x; rw[c][5] = w1.y; rw[c][6] = w1.z; rw[c][7] = w1.w;
            }
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) y[e] = fmaf(cur.gg[0], rw[0][e], fmaf(cur.gg[1], rw[1][e], fmaf(cur.gg[2], rw[2][e], y[e])));
        }
      }
      if (do_cu) {
        float* q = d.C_unmasked + cbase + uc;
        st16f(q, eC * 4u, y[0], y[1], y[2], y[3]);
        st16f(q, eC * 4u + 16, y[4], y[5], y[6], y[7]);
      }
      if constexpr (HAS_MASK) {                              // y *= gate ? 1 : slope, as a bit select
        const unsigned w = cur.mask;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int sel = ((int)(w << (31 - e))) >> 31;
          const float t = y[e] * d.slope;
          y[e] = __int_as_float((sel & __float_as_int(y[e])) | (~sel & __float_as_int(t)));
        }
      }
      unsigned bits = 0;
      if (do_act) {
        if (do_bits) {
          // LeakyReLU and the gate bit from one compare: vcc = y > 0; y = vcc ? y : slope*y; bits = 2*bits + vcc
#pragma unroll
          for (int e = 7; e >= 0; --e) {
            const float t = y[e] * d.slope;
            float o;
            asm volatile("v_cmp_lt_f32 vcc, 0, %2\n\tv_cndmask_b32 %1, %3, %2, vcc\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
                         : "+v"(bits), "=&v"(o) : "v"(y[e]), "v"(t) : "vcc");
            y[e] = o;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) y[e] = lrelu(y[e], d.slope);
        }
      } else if (do_bits) {
#pragma unroll
        for (int e = 0; e < 8; ++e) bits |= (y[e] > 0.f ? 1u : 0u) << e;
      }
      if (do_bits) {
        // a lane's 8 columns are one byte of the bit plane; the quad's four bytes as one dword, stored by its first lane
        // (the two dwords of a row's 64 columns are adjacent in lanes and in memory)
        unsigned v = bits << (8 * q2);
        v |= (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);     // quad_perm [1,0,3,2]
        v |= (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);     // quad_perm [2,3,0,1]
        if (q2 == 0) {
          unsigned char* q = (unsigned char*)d.mask_out + ((pbase + up) >> 3);
          *reinterpret_cast<unsigned*>(q + (eP >> 3)) = v;
        }
      }
      if constexpr (HAS_RES) {
        const unsigned wh[4] = {cur.rh.x, cur.rh.y, cur.rh.z, cur.rh.w}, wl[4] = {cur.rl.x, cur.rl.y, cur.rl.z, cur.rl.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          y[2 * e] += __uint_as_float(wh[e] << 16) + __uint_as_float(wl[e] << 16);
          y[2 * e + 1] += __uint_as_float(wh[e] & 0xffff0000u) + __uint_as_float(wl[e] & 0xffff0000u);
        }
      }
      if constexpr (RGBF) {
        // The sums keep the order of the 16 x 32 steps this epilogue used to take: per row, four chains (q = 0..3) of 32
        // FMAs over the columns 32 jj + 8 q + e (jj = 0..3, then e = 0..7), combined as (t0 + t1) + (t2 + t3).  Here chain q
        // alternates between the lanes c8 = q (column blocks jj = 0, 2) and c8 = q + 4 (jj = 1, 3): every lane runs the
        // step's eight FMAs twice, first on the carry of lanes 0-3, then on what lanes 0-3 hand to lanes 4-7 (row_shr:4);
        // after the first column half lanes 4-7 hand the chain back (row_shl:4), after the second they hold t0..t3 as a quad.
        constexpr int cp = hs & 1, rs = hs >> 1;             // column half (innermost), row set
        const int col = n0 + wn * 128 + cp * 64 + c8 * 8;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float4 w0 = *reinterpret_cast<const float4*>(d.torgb_w + (long long)c * d.N + col);
          const float4 w1 = *reinterpret_cast<const float4*>(d.torgb_w + (long long)c * d.N + col + 4);
          float t = (cp == 0) ? 0.f : tacc[c];
          t = fmaf(y[0], w0.x, t); t = fmaf(y[1], w0.y, t); t = fmaf(y[2], w0.z, t); t = fmaf(y[3], w0.w, t);
          t = fmaf(y[4], w1.x, t); t = fmaf(y[5], w1.y, t); t = fmaf(y[6], w1.z, t); t = fmaf(y[7], w1.w, t);
          t = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0x114, 0xF, 0xF, true));      // row_shr:4
          t = fmaf(y[0], w0.x, t); t = fmaf(y[1], w0.y, t); t = fmaf(y[2], w0.z, t); t = fmaf(y[3], w0.w, t);
          t = fmaf(y[4], w1.x, t); t = fmaf(y[5], w1.y, t); t = fmaf(y[6], w1.z, t); t = fmaf(y[7], w1.w, t);
          if constexpr (cp == 0) t = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0x104, 0xF, 0xF, true));      // row_shl:4
          tacc[c] = t;
        }
        if constexpr (cp == 1) {
          float v[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float t = tacc[c];
            t += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0xB1, 0xF, 0xF, true));
            t += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(t), 0x4E, 0xF, 0xF, true));
            v[c] = t;
          }
          if (c8 == 4) {
            const long long row = (long long)bz * d.M + m0 + wm * 64 + rs * 8 + h_rr;
            float* q = d.torgb_part + ((long long)(tn * 2 + wn) * d.batch * d.M + row) * 4;
            *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], 0.f);
          }
        }
      }
      if (do_c) {
        float* q = d.C + cbase + uc;
        st16f(q, eC * 4u, y[0], y[1], y[2], y[3]);
        st16f(q, eC * 4u + 16, y[4], y[5], y[6], y[7]);
      }
      if (do_p) {
        unsigned hw[4], lw[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x2 t = {y[2 * e], y[2 * e + 1]};
          hw[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(t, bf16x2));
          const f32x2 l = {y[2 * e] - __uint_as_float(hw[e] << 16), y[2 * e + 1] - __uint_as_float(hw[e] & 0xffff0000u)};
          lw[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(l, bf16x2));
        }
        const u32x4 vh = {hw[0], hw[1], hw[2], hw[3]}, vl = {lw[0], lw[1], lw[2], lw[3]};
        st16(Phi + pbase + up, eP * 2u, vh);
        st16(Plo + pbase + up, eP * 2u, vl);
      }
      if constexpr (HAS_IN && hs + NPF - 1 < 16) prefetch(hs + NPF - 1, pre[(hs + NPF - 1) % NPF]);
    });
  }  // persistent tile loop
}

}  // namespace

template <bool X1, bool A, bool Mk, bool R, bool FAST, bool RGBF = false, bool ADDP = false, bool BKM = false>
static void launch_v3f(const VArgs& g, int grid, hipStream_t stream) {
  static bool attr = false;
  CIPS_PER_DEVICE(attr, false);
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)gemm_bf16x3_v3_kernel<A, Mk, R, FAST, RGBF, ADDP, X1, BKM>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
    attr = true;
  }
  hipLaunchKernelGGL((gemm_bf16x3_v3_kernel<A, Mk, R, FAST, RGBF, ADDP, X1, BKM>), dim3(grid), dim3(512), SMEM_BYTES, stream, g);
}
template <bool X1, bool A, bool Mk, bool R>
static void launch_v3(const VArgs& g, int grid, hipStream_t stream) {
  const cips_gemm_x3_desc& d = g.d;
  if constexpr (!X1 && !R) {
    if (d.b_kmajor) {      // the three forms v3_accepts admits: the backward's dX flavours
      if constexpr (A) launch_v3f<X1, true, true, false, true, false, true, true>(g, grid, stream);             // planes addend (+ rgb term) + gate
      else if constexpr (Mk) launch_v3f<X1, false, true, false, true, false, false, true>(g, grid, stream);    // gate bits in, planes out
      else launch_v3f<X1, false, false, false, false, false, false, true>(g, grid, stream);                    // plain: fp32 C and / or planes
      return;
    }
  }
  // the training step's epilogues take the compile-time form
  const bool fwd = !Mk && d.act == 1 && d.mask_out != nullptr, bwd = Mk && d.act == 0 && d.mask_out == nullptr;
  const bool fast = d.P_hi != nullptr && d.C == nullptr && (fwd || bwd) && (A || d.C_unmasked == nullptr);
  if constexpr (!A && !Mk) {
    if (d.torgb_w) { launch_v3f<X1, A, Mk, R, true, true>(g, grid, stream); return; }     // the entry point checked `fast`
  }
  if constexpr (A && Mk && !R) {
    if (d.addp_hi) { launch_v3f<X1, A, Mk, R, true, false, true>(g, grid, stream); return; }   // likewise
  }
  if (fast) launch_v3f<X1, A, Mk, R, true>(g, grid, stream);
  else launch_v3f<X1, A, Mk, R, false>(g, grid, stream);
}

// 0: this kernel takes the descriptor (x1: in its single-pass form); else the error code cips_gemm_bf16x3_v3 / cips_gemm_bf16_v3
// returns for it
static int v3_accepts(const cips_gemm_x3_desc* d, bool x1 = false) {
  if (!d || d->M <= 0 || d->N <= 0 || d->K <= 0 || d->batch <= 0) return (int)hipErrorInvalidValue;
  if ((d->M % BM) || (d->N % BN) || (d->K % (2 * (x1 ? X1_BK : BK)))) return (int)hipErrorNotSupported;
  if ((d->lda & 7) || (d->ldb & 7) || (d->strideA & 7) || (d->strideB & 7)) return (int)hipErrorInvalidValue;
  if (d->T_hi || (d->ldc & 3) || (d->strideC & 3) || (d->ldp & 31) || (d->strideP & 31)) return (int)hipErrorNotSupported;
  const bool a = d->add != nullptr || d->addp_hi != nullptr, m = d->mask != nullptr, r = d->res_hi != nullptr;
  if ((a && !m) || (r && (a || m))) return (int)hipErrorNotSupported;
  if (d->addp_hi) {      // planes addend: the backward flavours' compile-time epilogue only
    if (d->add || !d->addp_lo || !d->addp_gate || !(d->act == 0 && !d->mask_out && d->P_hi && !d->C)) return (int)hipErrorNotSupported;
    if (((uintptr_t)d->addp_hi & 15) || ((uintptr_t)d->addp_lo & 15)) return (int)hipErrorNotSupported;
  }
  if ((m && !(d->gate_bits & 1)) || (d->mask_out && !(d->gate_bits & 2))) return (int)hipErrorNotSupported;   // bit planes only
  if (d->rgb_g && !a) return (int)hipErrorNotSupported;
  if (d->mask_out && ((uintptr_t)d->mask_out & 3)) return (int)hipErrorNotSupported;                         // dword stores of the bit plane
  // 32-bit lane offsets
  if ((long long)BM * d->lda * 2 >= 0x7fffffffLL || (long long)BN * d->ldb * 2 >= 0x7fffffffLL ||
      (long long)BM * d->ldc * 4 >= 0x7fffffffLL || (long long)BM * d->ldp * 2 >= 0x7fffffffLL) return (int)hipErrorNotSupported;
  if (d->torgb_w) {      // fused ToRGB: the forward flavours' compile-time epilogue only
    if (!d->torgb_part || a || m || !(d->act == 1 && d->mask_out && d->P_hi && !d->C && !d->C_unmasked)) return (int)hipErrorNotSupported;
    if ((d->N & 127) || ((uintptr_t)d->torgb_part & 15) || ((uintptr_t)d->torgb_w & 15)) return (int)hipErrorNotSupported;
  }
  if (d->b_kmajor) {     // B planes [K][ldb]: 3-pass, the instantiations of launch_v3 — no activation, no gate output, no residual, and
    if (d->b_kmajor != 1 || x1 || d->ldb < d->N || r || d->torgb_w || d->act || d->mask_out) return (int)hipErrorNotSupported;
    if (m) {             // with a gate input the compile-time epilogue: planes out, no fp32 C; the addend as planes or none
      if (d->add || !d->P_hi || d->C || (!a && d->C_unmasked)) return (int)hipErrorNotSupported;
    }
  }
  return 0;
}
extern "C" CIPS_INTERNAL int cips_gemm_bf16x3_v3_accepts(const cips_gemm_x3_desc* d) { return v3_accepts(d); }
extern "C" CIPS_INTERNAL int cips_gemm_bf16_v3_accepts(const cips_gemm_x3_desc* d) { return v3_accepts(d, true); }

// Internal entry (called by cips_gemm_bf16x3 ahead of the wide kernel): same descriptor.  hipErrorNotSupported for
// every shape / epilogue it has no code for.
template <bool X1>
static int run_v3(const cips_gemm_x3_desc* d, cips_stream_t stream) {
  { const int rc = v3_accepts(d, X1); if (rc) return rc; }
  const bool a = d->add != nullptr || d->addp_hi != nullptr, m = d->mask != nullptr, r = d->res_hi != nullptr;
  VArgs g = {};
  g.d = *d;
  g.tiles_m = d->M / BM;
  g.tiles_n = d->N / BN;
  const long long total = (long long)g.tiles_m * g.tiles_n * d->batch;
  if (total > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  g.total = (int)total;
  const int ncu = cips_persistent_cus();
  const int grid = g.total < ncu ? g.total : ncu;
  hipStream_t st = (hipStream_t)stream;
  if (a) launch_v3<X1, true, true, false>(g, grid, st);
  else if (m) launch_v3<X1, false, true, false>(g, grid, st);
  else if (r) launch_v3<X1, false, false, true>(g, grid, st);
  else launch_v3<X1, false, false, false>(g, grid, st);
  return CIPS_CHECK_LAUNCH();
}
extern "C" CIPS_INTERNAL int cips_gemm_bf16x3_v3(const cips_gemm_x3_desc* d, cips_stream_t stream) { return run_v3<false>(d, stream); }
// the single-pass form, called by cips_gemm_bf16 (gemm_bf16x3.hip) ahead of its 256x128 kernel
extern "C" CIPS_INTERNAL int cips_gemm_bf16_v3(const cips_gemm_x3_desc* d, cips_stream_t stream) { return run_v3<true>(d, stream); }
