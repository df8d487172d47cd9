// gemm_x3_common.h — building blocks shared by the GEMM kernels (gemm_f32.hip and the split-bf16 family
// gemm_bf16x3*.hip; the bf16 conversions also by modfc.hip and disc_ops.hip).
#pragma once
#include "common.h"
#include <utility>

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// fp32 -> bf16, round to nearest even; bf16 -> fp32; the split x = hi + lo of the operand planes (gemm_bf16x3.hip)
__device__ __forceinline__ u16 f2bf(float v) {
  unsigned u = __float_as_uint(v);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}
__device__ __forceinline__ float bf2f(u16 h) { return __uint_as_float(((unsigned)h) << 16); }
__device__ __forceinline__ void split2(float v, u16& hi, u16& lo) {
  hi = f2bf(v);
  lo = f2bf(v - bf2f(hi));
}

// compile-time loop: f(std::integral_constant<int, I>) for every I of the sequence, so that the body can index register
// arrays with constants (a dynamic index puts them in scratch)
template <typename F, int... I>
__device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }

// XCD-contiguous tile order: workgroup / tile sequence number t runs on XCD t % 8; the tiles [0, total) are cut into eight
// contiguous ranges and XCD x walks range x, so the tiles that share an operand panel meet in one L2.  Bijective on [0, total).
__device__ __forceinline__ int xcd_tile(int t, int total) {
  const int nx = 8;
  const int q = total / nx, r = total % nx;
  const int xcd = t % nx, idx = t / nx;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

// LDS-DMA of 16 bytes per lane (global_load_lds_dwordx4) in the SGPR-base form: uniform base pointer p in SGPRs, one 32-bit
// byte offset per lane, the wave's LDS destination in M0.  Written as asm because the builtin takes a flat 64-bit pointer,
// and hipcc then builds 64-bit per-lane addresses with two v_lshl_add_u64 per piece (gemm_bf16x3_wide.hip: main loop
// 207 -> 197 us, 20 fewer VGPRs).  M0 is used by nothing else in these kernels.
__device__ __forceinline__ void lds_dma16(const u16* p, unsigned off, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(off), "s"(p), "s"(lds_addr) : "memory");
}

// The pass-major k-step of the 256x256 kernels (gemm_bf16x3_v3.hip, conv2d_x3_v3_kernel, gemm_bf16x3_km_v3_kernel): 24 MFMAs,
// MFMA m = pass m >> 3 (0: a_lo b_hi, 1: a_hi b_lo, 2: a_hi b_hi) into output tile ((m >> 2) & 1, m & 3), on 12 fragments
// numbered in the order the MFMA stream first needs them:
//   0: a_lo[0]   1..4: b_hi[0..3]   5: a_lo[1]   6: a_hi[0]   7..10: b_lo[0..3]   11: a_hi[1]
// An LDS stage of these kernels is four 16 KiB planes A_hi, A_lo, B_hi, B_lo; fragment q lies in plane x3_frag_plane(q)
// (byte offset), 32-row (NT) or 32-column (K-major) tile x3_frag_tile(q) of the wave's block.
constexpr int X3_PLANE_BYTES = 16384;
__device__ __forceinline__ constexpr bool x3_frag_is_a(int q) { return q == 0 || q == 5 || q == 6 || q == 11; }
__device__ __forceinline__ constexpr int x3_frag_tile(int q) { return q == 0 || q == 6 ? 0 : q == 5 || q == 11 ? 1 : q <= 4 ? q - 1 : q - 7; }
__device__ __forceinline__ constexpr int x3_frag_plane(int q) {
  return (q == 0 || q == 5 ? 1 : q == 6 || q == 11 ? 0 : q <= 4 ? 2 : 3) * X3_PLANE_BYTES;
}
// NT image (rows of 64 bytes): the fragment's offset from the lane's read base
__device__ __forceinline__ constexpr int x3_frag_off_nt(int q) { return x3_frag_plane(q) + x3_frag_tile(q) * 32 * 64; }
__device__ __forceinline__ constexpr int x3_mfma_a(int m) { return (m >> 3) == 0 ? (((m >> 2) & 1) ? 5 : 0) : (((m >> 2) & 1) ? 11 : 6); }
__device__ __forceinline__ constexpr int x3_mfma_b(int m) { return (m >> 3) == 1 ? 7 + (m & 3) : 1 + (m & 3); }

// ---- single-pass ("bf16") forms of the 256x256 kernels: sum_k a_hi b_hi only, the lo planes are never addressed.
// The LDS stage keeps its four 16 KiB planes, DMA pieces, swizzle and fragment reads; what changes is what the planes hold —
// A_hi[k0, k0+32), A_hi[k0+32, k0+64), B_hi[k0, k0+32), B_hi[k0+32, k0+64) — so a stage is a 64-deep k-tile of four
// 16-deep k-steps: k-step s reads planes (s >> 1) and (2 + (s >> 1)), k-chunk pair s & 1.  A k-step is 8 MFMAs (output
// tile (m >> 2, m & 3)) on 6 fragments, numbered in the order the MFMA stream first needs them:
//   0: a[0]   1..4: b[0..3]   5: a[1]
constexpr int X1_BK = 64;
__device__ __forceinline__ constexpr bool x1_frag_is_a(int q) { return q == 0 || q == 5; }
__device__ __forceinline__ constexpr int x1_frag_tile(int q) { return q == 0 ? 0 : q == 5 ? 1 : q - 1; }
__device__ __forceinline__ constexpr int x1_frag_plane(int q, int s) { return ((x1_frag_is_a(q) ? 0 : 2) + (s >> 1)) * X3_PLANE_BYTES; }
__device__ __forceinline__ constexpr int x1_mfma_a(int m) { return (m >> 2) ? 5 : 0; }
__device__ __forceinline__ constexpr int x1_mfma_b(int m) { return 1 + (m & 3); }
// first DMA piece and number of pieces behind MFMA m = 2..7 of a k-tile's last k-step (eight pieces in six slots)
__device__ __forceinline__ constexpr int x1_piece0(int m) { return m == 2 ? 0 : m == 3 ? 2 : m == 4 ? 3 : m == 5 ? 4 : m == 6 ? 6 : 7; }
__device__ __forceinline__ constexpr int x1_pieces(int m) { return (m == 2 || m == 5) ? 2 : 1; }

// One 64-deep k-tile of the single-pass schedule: 32 MFMAs on two fragment sets G[0] / G[1] (k-step s multiplies set s & 1
// while the six fragments of k-step s + 1 are read into the other, one per MFMA).  The k-tile's one barrier stands behind the
// second MFMA of the last k-step: every wave has then received all its fragments of this stage, so the barrier publishes the
// other stage (its DMA pieces were issued a k-tile period ago and are waited for here) and frees this one; the first k-step
// of the next k-tile is read behind it, two fragments per MFMA.  MODE 0: steady state; 1: next-to-last k-tile (same, the
// kernel's `slot` issues no DMA); 2: last (no next k-tile to read or wait for).
//   rd(q, s, next): fragment q of k-step s from this stage (next = false) or the other one (true)
//   slot(s, m): the kernel's own work behind MFMA m of k-step s (DMA pieces, epilogue prefetch)
template <int MODE, typename Rd, typename Slot>
__device__ __forceinline__ void x1_ktile(f32x16 (&acc)[2][4], bf16x8 (&G)[2][6], Rd&& rd, Slot&& slot) {
  static_for(std::make_integer_sequence<int, 32>{}, [&](auto T_) {
    constexpr int t = decltype(T_)::value, s = t >> 3, m = t & 7;
    acc[m >> 2][m & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(G[s & 1][x1_mfma_a(m)], G[s & 1][x1_mfma_b(m)], acc[m >> 2][m & 3], 0, 0, 0);
    if constexpr (s < 3) {
      if constexpr (m < 6) G[(s + 1) & 1][m] = rd(std::integral_constant<int, m>{}, std::integral_constant<int, s + 1>{}, std::false_type{});
    } else {
      if constexpr (m == 1) {
        if constexpr (MODE == 2) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
      if constexpr (MODE <= 1 && m >= 2 && m <= 4) {
        constexpr int q = 2 * (m - 2);
        G[0][q] = rd(std::integral_constant<int, q>{}, std::integral_constant<int, 0>{}, std::true_type{});
        G[0][q + 1] = rd(std::integral_constant<int, q + 1>{}, std::integral_constant<int, 0>{}, std::true_type{});
      }
    }
    slot(std::integral_constant<int, s>{}, std::integral_constant<int, m>{});
    __builtin_amdgcn_sched_barrier(0);
  });
}

// Persistent grids: one workgroup per CU, the CU count rounded down to a multiple of 8 so that a workgroup striding by the
// grid size stays on its XCD.  256 if the device properties cannot be read.
static inline int cips_persistent_cus() {
  static int ncu = 0;
  CIPS_PER_DEVICE(ncu, 0);
  if (!ncu) {
    int dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
    if (ncu <= 0) ncu = 256;
    ncu = (ncu / 8) * 8;
  }
  return ncu;
}
