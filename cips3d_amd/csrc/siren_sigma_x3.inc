// siren_sigma_x3.inc — the density kernels on the split-bf16 / fp16 register chain of siren_x3_common.h: the sigma-only forward
// (cips_siren_sigma_x3, _grid) and sigma with its gradient w.r.t. the point (cips_siren_sigma_grad_x3, _grid), with their entry
// points.  The two share the sigma LDS carve, the points sources, the first half of their wave-step (siren_sigma_w1.inc) and one
// launcher.  Included by siren_fwd_x3.hip, which says why this is no source of its own.
#include "siren_x3_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// Sigma-only forward (density volumes: cips_siren_sigma_x3, cips_siren_sigma_x3_grid): siren_fwd_x3_kernel's layout — lane =
// point, a wave owns 32 points, the two lane halves split the features — running siren_sigma_chain.inc, the forward chain
// up to sigma: 16 896 MAC per point instead of 27 136, 256 sines instead of 320, no operand split of h2, and one dword per
// point to HBM instead of 132 B.  LDS: the sigma carve (67.5 KiB: W1 hi / lo, layer-0 packs, G1, C1, WS).
// GRID: the point of index p = (i * ny + j) * nz + k is (gx[i], gy[j], gz[k]) — three host-built coordinate arrays READ by
// the kernel, which does index arithmetic only: the lattice is whatever the host built, bit for bit.
// Occupancy: two 512-thread workgroups fit a CU's LDS at 67.5 KiB each, and co-reside when the kernel stays at or below 128
// VGPRs — which the chain does because it builds h1 one 32-feature tile at a time (siren_sigma_w1.inc).
// __launch_bounds__' second argument is the minimum waves per SIMD asked of the register allocator: 4 = two workgroups of
// 512 per CU.  profiles/density_grid.txt has this form timed against one workgroup per CU (bound 2, which also lets the
// allocator use up to 256 VGPRs, and the launch's LDS request padded to 96 KiB): two per CU is 6.5 % faster.
struct SigmaX3Args {
  cips_siren_weights w;
  const float* points;               // (B, P, 3); unused with GRID
  const float *gx, *gy, *gz;         // GRID: the lattice's coordinates (nx), (ny), (nz)
  float* sigma;                      // (B, P)
  int ny, nz;
  int B, P, chunk;
};

template <bool HW, bool F16, bool GRID>
__global__ __launch_bounds__(512, 4) void siren_sigma_x3_kernel(SigmaX3Args a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  const int b = blockIdx.y;
  stage_weights_x3<HW, F16, true>(smem, a.w, b);
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
  const float bs = a.w.bs[0];
  const int cstart = blockIdx.x * a.chunk;
  const int cend = min(cstart + a.chunk, a.P);
  for (int pbase = cstart + wave * 32; pbase < cend; pbase += 8 * 32) {
#include "siren_sigma_chain.inc"
    if (valid && hf == 0) a.sigma[gp] = sig;
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Sigma and its gradient w.r.t. the point (cips_siren_sigma_grad_x3, cips_siren_sigma_grad_x3_grid): the sigma kernel's layout,
// LDS carve, staging, points sources and chunking, running siren_sigma_grad_chain.inc — the sigma chain, then
//   dp1 = g1 * ws * cos(a1),  dh1 = W1^T dp1  (the W1 image read transposed: no second image),
//   grad = box_scale * W0^T (g0 * cos(a0) * dh1) = sum_f pack[f].xyz * cos(a0[f]) * dh1[f]
// — 16 896 + 16 384 MAC and 256 + 256 trigonometric evaluations per point.  sigma is the sigma kernel's bit for bit.
// Two scale factors leave in fp32 at the output:
//  * HW: the staging stores W1 and the layer-0 packs divided by 2 pi (the sines take revolutions), so both transposed factors
//    carry 1 / (2 pi): the gradient is multiplied by (2 pi)^2;
//  * F16: G1 holds g1 * 2^-k next to the W1 * 2^k image, so g1 * ws * cos can sit far below fp16's normal range.  Every wave
//    takes  m = max_f |G1[f] * ws[f]|  of its image from LDS and multiplies dp1 by pow2_scale_for(m) — the staging rule: the
//    largest |dp1| a point can have lies in [2^13, 2^14) — and the output by its inverse.  A power of two: exact to undo.
// Registers: the packed dp1 (64) is live next to the 64 accumulators of dh1 plus the fragment ring, more than the 128 registers
// two co-resident 512-thread workgroups would leave a wave, so the kernel asks for one workgroup per CU (bound 2: up to 256).
struct SigmaGradX3Args {
  cips_siren_weights w;
  const float* points;               // (B, P, 3); unused with GRID
  const float *gx, *gy, *gz;         // GRID: the lattice's coordinates (nx), (ny), (nz)
  float* sigma;                      // (B, P) or NULL
  float* grad;                       // (B, P, 3)
  int ny, nz;
  int B, P, chunk;
};

template <bool HW, bool F16, bool GRID>
__global__ __launch_bounds__(512, 2) void siren_sigma_grad_x3_kernel(SigmaGradX3Args a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  const int b = blockIdx.y;
  stage_weights_x3<HW, F16, true>(smem, a.w, b);
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
  const float bs = a.w.bs[0];
  float dscale = 1.f, oscale = HW ? 39.47841760435743f : 1.f;      // (2 pi)^2
  if constexpr (F16) {
    const float* G1 = reinterpret_cast<const float*>(smem + SG_L0 + (O_G1 - O_L0));
    const float* WS = reinterpret_cast<const float*>(smem + SG_L0 + (O_WS - O_L0));
    float m = fmaxf(fabsf(G1[lane0] * WS[lane0]), fabsf(G1[lane0 + 64] * WS[lane0 + 64]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    int k;
    dscale = pow2_scale_for(m, k);
    oscale *= __uint_as_float((unsigned)(127 - k) << 23);
  }
  const int cstart = blockIdx.x * a.chunk;
  const int cend = min(cstart + a.chunk, a.P);
  for (int pbase = cstart + wave * 32; pbase < cend; pbase += 8 * 32) {
#include "siren_sigma_grad_chain.inc"
    if (valid && hf == 0) {
      if (a.sigma) a.sigma[gp] = sig;
      float* go = a.grad + gp * 3;
      go[0] = gx * oscale; go[1] = gy * oscale; go[2] = gz * oscale;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace

// One launcher for both kernels (GRAD: sigma and its gradient): the chunk rule of the forward (x3_chunk; a ragged tail is clamped
// to the last valid point in-kernel).  grid == NULL: points (B, P, 3).
template <bool GRAD>
static int siren_sigma_x3_launch(const cips_siren_weights* w, const float* points, const cips_grid_params* grid, float* sigma,
                                 float* grad, int B, int P, cips_stream_t stream) {
  std::conditional_t<GRAD, SigmaGradX3Args, SigmaX3Args> a;
  a.w = *w; a.points = points; a.sigma = sigma; a.B = B; a.P = P;
  if constexpr (GRAD) a.grad = grad;
  a.gx = a.gy = a.gz = nullptr; a.ny = a.nz = 1;
  if (grid) { a.gx = grid->gx; a.gy = grid->gy; a.gz = grid->gz; a.ny = grid->ny; a.nz = grid->nz; }
  a.chunk = x3_chunk(B, P);
  dim3 g((P + a.chunk - 1) / a.chunk, B);
  x3_pick([&](auto HW_, auto F16_, auto GRID_) {
    constexpr bool HW = decltype(HW_)::value, F16 = decltype(F16_)::value, GRID = decltype(GRID_)::value;
    if constexpr (GRAD) x3_launch<siren_sigma_grad_x3_kernel<HW, F16, GRID>>(g, 512, SG_SMEM_BYTES, stream, a);
    else x3_launch<siren_sigma_x3_kernel<HW, F16, GRID>>(g, 512, SG_SMEM_BYTES, stream, a);
  }, (w->trig_mode & 1) != 0, (w->trig_mode & 2) == 0, grid != nullptr);
  return CIPS_CHECK_LAUNCH();
}

// the lattice of a _grid entry point: P = nx * ny * nz, or an error when an array is missing or the product does not fit an int
static int sigma_grid_points(const cips_grid_params* grid, int* P) {
  if (!grid->gx || !grid->gy || !grid->gz || grid->nx <= 0 || grid->ny <= 0 || grid->nz <= 0) return (int)hipErrorInvalidValue;
  const long long nxy = (long long)grid->nx * grid->ny;               // < 2^62; times nz only once it is known to fit an int
  if (nxy > INT_MAX || nxy * grid->nz > INT_MAX) return (int)hipErrorInvalidValue;
  *P = (int)(nxy * grid->nz);
  return 0;
}

extern "C" int cips_siren_sigma_x3(const cips_siren_weights* w, const float* points, float* sigma, int B, int P,
                                   cips_stream_t stream) {
  if (!w || !points || !sigma || B <= 0 || P <= 0) return (int)hipErrorInvalidValue;
  return siren_sigma_x3_launch<false>(w, points, nullptr, sigma, nullptr, B, P, stream);
}

extern "C" int cips_siren_sigma_x3_grid(const cips_siren_weights* w, const cips_grid_params* grid, float* sigma, int B,
                                        cips_stream_t stream) {
  if (!w || !grid || !sigma || B <= 0) return (int)hipErrorInvalidValue;
  int P;
  if (const int rc = sigma_grid_points(grid, &P)) return rc;
  return siren_sigma_x3_launch<false>(w, nullptr, grid, sigma, nullptr, B, P, stream);
}

extern "C" int cips_siren_sigma_grad_x3(const cips_siren_weights* w, const float* points, float* sigma, float* grad, int B, int P,
                                        cips_stream_t stream) {
  if (!w || !points || !grad || B <= 0 || P <= 0) return (int)hipErrorInvalidValue;
  return siren_sigma_x3_launch<true>(w, points, nullptr, sigma, grad, B, P, stream);
}

extern "C" int cips_siren_sigma_grad_x3_grid(const cips_siren_weights* w, const cips_grid_params* grid, float* sigma, float* grad,
                                             int B, cips_stream_t stream) {
  if (!w || !grid || !grad || B <= 0) return (int)hipErrorInvalidValue;
  int P;
  if (const int rc = sigma_grid_points(grid, &P)) return rc;
  return siren_sigma_x3_launch<true>(w, nullptr, grid, sigma, grad, B, P, stream);
}
