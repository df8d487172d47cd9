// siren_surface_x3.hip — ray casting of the density iso-surface sigma = level on the split-bf16 / fp16 register chain of
// siren_x3_common.h: cips_siren_surface_x3, first-hit depth, hit mask, surface point and the density there, per camera ray.
// A source of its own (like siren_bwd_points_x3.hip): it runs only when a caller asks for a surface image, and as a separate module
// it leaves the listings of the forward, sigma and backward kernels as they are (profiles/surface_cast.txt has the resource table of
// the sigma kernels before and after).  The evaluation of sigma is the sigma kernel's, text for text: siren_sigma_w1.inc and
// siren_sigma_dot.inc behind a prologue that takes the point from registers.
#include "siren_x3_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// The search, per ray (the rule in full: include/cips3d_hip.h, DESIGN.md section 3 "Surface ray casting"):
//   coarse   sigma at the unjittered depths zg[0], zg[1], ...: inside at zg[0] -> hit 2; else the first s with
//            sigma[s-1] < level <= sigma[s] -> hit 1 and the bracket [zg[s-1], zg[s]]; none -> hit 0, depth zg[S-1]
//   refine   `refine` bisection steps on the bracket of a hit-1 ray, then one secant step -> depth
//   final    one more evaluation at the point of that depth -> points, sigma
// The sigma kernel's layout, LDS carve and staging (lane = ray, a wave owns 32 rays, the two lane halves split the features; both
// halves hold the same sigma — the cross-half add is commutative — and take the same decisions).  Every evaluation is one
// wave-step of the sigma chain, so lanes are never switched off one by one (MFMAs and __shfl_xor need the whole wave): a ray that
// has found its crossing, or has none, goes on evaluating a harmless point (the wave's coarse depth; its own final depth during
// the refinement) and ignores the result.  All control flow is wave-uniform: the coarse walk ends for a wave when no lane is
// still searching (ballot), the refinement is skipped by a wave without a hit-1 ray, and there is no barrier behind the one
// that follows the staging, so the waves of a workgroup leave at different steps.
// ONE chain site: coarse, refine and final steps are the iterations of one loop with a wave-uniform mode, so the chain's text is
// instantiated once per kernel; next to it lives the ray's hit state, the rest waits in LDS.
// TRACE: every (t, sigma) the ray's wave evaluated, slot s of the coarse walk and S + k of the refinement; what the wave never
// evaluated stays at the NaN the kernel fills in first.  An instantiation of its own: the production launch keeps its registers.
struct SurfaceX3Args {
  cips_siren_weights w;
  RayGen rg;                         // jitter and zvals NULL: the walk is on the grid zg itself
  float level;
  int refine;
  float* depth;                      // (B, n)
  unsigned char* hit;                // (B, n): 0 no crossing, 1 crossing, 2 the ray starts inside
  float* sigma;                      // (B, n) or NULL: the density at the point of `depth`
  float* points;                     // (B, n, 3) or NULL
  float* trace;                      // (B, n, S + refine, 2) or NULL (TRACE instantiations only)
  int B, chunk;                      // chunk: rays per workgroup
};

// world direction of ray `ray`: gen_point_materialised's zvals form (the direction normalised in camera space, then rotated),
// every rounding written out
__device__ __forceinline__ void surface_ray_dir(const RayGen& g, const float* M, int ray, float& rx, float& ry, float& rz) {
#pragma clang fp contract(off)
  const int row = ray / g.W, col = ray - row * g.W;
  const float x = g.xg[col], y = g.yg[row];
  const float nrm = sqrtf((x * x + y * y) + g.zc * g.zc);
  const float dx = x / nrm, dy = y / nrm, dz = g.zc / nrm;
  rx = __builtin_fmaf(dz, M[2], __builtin_fmaf(dy, M[1], dx * M[0]));
  ry = __builtin_fmaf(dz, M[6], __builtin_fmaf(dx, M[4], dy * M[5]));
  rz = __builtin_fmaf(dz, M[10], __builtin_fmaf(dx, M[8], dy * M[9]));
}
// THE point at depth t (origin + world direction * t), the one expression of the kernel: coarse, bisection and final points
__device__ __forceinline__ void surface_point(float rx, float ry, float rz, float ox, float oy, float oz, float t, float& px,
                                              float& py, float& pz) {
#pragma clang fp contract(off)
  px = __builtin_fmaf(rx, t, ox); py = __builtin_fmaf(ry, t, oy); pz = __builtin_fmaf(rz, t, oz);
}
__device__ __forceinline__ float surface_mid(float lo, float hi) {
#pragma clang fp contract(off)
  return 0.5f * (lo + hi);
}
// the secant step on the final bracket: a subtraction, a division, a subtraction, a product and a sum, each rounded on its own
__device__ __forceinline__ float surface_secant(float level, float lo, float hi, float slo, float shi) {
#pragma clang fp contract(off)
  const float f = (level - slo) / (shi - slo);
  const float w = hi - lo;
  const float fw = f * w;
  return lo + fw;
}

// The ray's state between evaluations — world direction, bracket [lo, hi], the densities at its ends, the depth t under way — is parked in LDS behind
// the sigma carve: eight words per ray, 8 KiB per workgroup (lanes l and l + 32 hold the same ray and write the same words).  Next
// to the chain's 64 accumulators a wave has no registers left for them (in registers: 8 to 19 spilled VGPRs and 36 to 84 B of
// scratch per lane under the bound of 128); volatile accesses, or hipcc forwards the stored values through registers again.
// Slot LO doubles as the depth of a ray that is not refined (hit 0 / 2): the point it goes on evaluating.
enum { ST_RX, ST_RY, ST_RZ, ST_LO, ST_HI, ST_SLO, ST_SHI, ST_T, ST_WORDS };
constexpr int SF_SMEM_BYTES = SG_SMEM_BYTES + ST_WORDS * 1024;      // 77312: two workgroups still fit a CU's 160 KiB
static_assert(2 * SF_SMEM_BYTES <= SMEM_BYTES, "surface LDS carve");
__device__ __forceinline__ float st_ld(unsigned base, int i) { return *LDS_PTR(const volatile float, base + 1024 * i); }
__device__ __forceinline__ void st_st(unsigned base, int i, float v) { *LDS_PTR(volatile float, base + 1024 * i) = v; }

// Occupancy: with the hardware sines (trig_mode bit 0, the default) the kernel stays at 126 / 128 VGPRs with no scratch and runs
// two workgroups per CU like the sigma kernel (bound 4).  The polynomial sines (trig_mode 0) are 1 (TRACE: 5) VGPRs short under that
// bound — hipcc spills 8 / 24 B per lane — so those instantiations ask for bound 2: 132 / 136 VGPRs, no scratch, one workgroup
// per CU.  profiles/surface_cast.txt has the figures of all eight.

template <bool HW, bool F16, bool TRACE>
__global__ __launch_bounds__(512, HW ? 4 : 2) void siren_surface_x3_kernel(SurfaceX3Args a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  const int b = blockIdx.y;
  stage_weights_x3<HW, F16, true>(smem, a.w, b);
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
  const float bs = a.w.bs[0];
  const float* M = a.rg.c2w + (long long)b * 16;             // per image: scalar loads
  const float ox = M[3], oy = M[7], oz = M[11];
  const int n = a.rg.n, S = a.rg.S, refine = a.refine, NT = S + refine;
  const float level = a.level;
  const int cstart = blockIdx.x * a.chunk;
  const int cend = min(cstart + a.chunk, n);
  for (int rbase = cstart + wave * 32; rbase < cend; rbase += 8 * 32) {
    float tn = a.rg.zg[0];                         // the depth of the next evaluation
    {
      const int r = rbase + (lane0 & 31);
      const int rc = r < cend ? r : cend - 1;      // ragged tail: the last valid ray again, nothing stored
      const unsigned stb = sbase + SG_SMEM_BYTES + 4 * (wave * 32 + (lane0 & 31));
      float rx, ry, rz;
      surface_ray_dir(a.rg, M, rc, rx, ry, rz);
      st_st(stb, ST_RX, rx); st_st(stb, ST_RY, ry); st_st(stb, ST_RZ, rz);
      if constexpr (TRACE) {
        if (r < cend && lane0 < 32) {
          float* tr = a.trace + ((long long)b * n + rc) * NT * 2;
          for (int i = 0; i < 2 * NT; ++i) tr[i] = __builtin_nanf("");
        }
      }
    }
    int hit = -1;                                  // -1: still searching
    int mode = 0, s = 0, k = 0;                    // wave-uniform: 0 coarse step s, 1 bisection step k, 2 the final evaluation
    for (;;) {
      int lane = lane0;                            // the sigma kernel's prologue, per evaluation
      asm volatile("" : "+v"(lane));
      const int l31 = lane & 31, hf = lane >> 5;
      LaneAddr LA = lane_addr(lane, sbase);
      LA.v16 = opaque(sbase + SG_L0 + 16 * hf);
      LA.v64 = opaque(sbase + SG_L0 + 64 * hf);
      float px, py, pz;
      {
        const unsigned stb = sbase + SG_SMEM_BYTES + 4 * (wave * 32 + l31);
        surface_point(st_ld(stb, ST_RX), st_ld(stb, ST_RY), st_ld(stb, ST_RZ), ox, oy, oz, tn, px, py, pz);
        st_st(stb, ST_T, tn);
      }
#include "siren_sigma_w1.inc"
#include "siren_sigma_dot.inc"
      int lane_e = lane0;                          // the epilogue's indices, made again behind the chain
      asm volatile("" : "+v"(lane_e));
      const int r = rbase + (lane_e & 31);
      const bool store = r < cend && lane_e < 32;
      const long long gr = (long long)b * n + (r < cend ? r : cend - 1);
      const unsigned stb = sbase + SG_SMEM_BYTES + 4 * (wave * 32 + (lane_e & 31));
      const float t = st_ld(stb, ST_T);            // the depth of this evaluation
      if (mode == 2) {                             // t is the ray's depth
        if (store) {
          a.depth[gr] = t;
          a.hit[gr] = (unsigned char)hit;
          if (a.sigma) a.sigma[gr] = sig;
          if (a.points) { float* po = a.points + gr * 3; po[0] = px; po[1] = py; po[2] = pz; }
        }
        break;
      }
      if constexpr (TRACE) {
        if (store) {
          float* tr = a.trace + (gr * NT + (mode == 0 ? s : S + k)) * 2;
          tr[0] = t; tr[1] = sig;
        }
      }
      if (mode == 0) {
        if (hit < 0) {
          // slot SLO holds sigma of step s - 1 (nothing at s == 0)
          const bool cross = s > 0 && st_ld(stb, ST_SLO) < level && level <= sig;
          if (cross) { hit = 1; st_st(stb, ST_HI, t); st_st(stb, ST_SHI, sig); }
          else {
            st_st(stb, ST_LO, t); st_st(stb, ST_SLO, sig);
            if (s == 0 && sig >= level) hit = 2;   // the ray starts inside: its depth zg[0] is in LO
          }
        }
        ++s;
        if (s == S || __builtin_amdgcn_ballot_w64(hit < 0) == 0) {
          if (hit < 0) hit = 0;                    // only with s == S: LO holds zg[S - 1], the depth of a ray without crossing
          mode = (refine > 0 && __builtin_amdgcn_ballot_w64(hit == 1) != 0) ? 1 : 2;
        }
      } else {
        if (hit == 1) {
          if (sig >= level) { st_st(stb, ST_HI, t); st_st(stb, ST_SHI, sig); }
          else { st_st(stb, ST_LO, t); st_st(stb, ST_SLO, sig); }
        }
        if (++k == refine) mode = 2;
      }
      if (mode == 0) tn = a.rg.zg[s];
      else {
        const float lo = st_ld(stb, ST_LO), hi = st_ld(stb, ST_HI);
        if (mode == 1) tn = hit == 1 ? surface_mid(lo, hi) : lo;
        else tn = hit == 1 ? surface_secant(level, lo, hi, st_ld(stb, ST_SLO), st_ld(stb, ST_SHI)) : lo;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Rays per workgroup, by the rule of x3_chunk: a workgroup pass is 256 rays of S + refine + 1 evaluations each, so one pass already
// amortises the staging; more passes per workgroup (up to 4) only when the launch still has 3 workgroups per CU on 256 CUs.
inline int surface_chunk(int B, int n) {
  int chunk = 1024;
  while (chunk > 256 && (long long)B * ((n + chunk - 1) / chunk) < 768) chunk >>= 1;
  return chunk;
}

}  // namespace

extern "C" int cips_siren_surface_x3(const cips_siren_weights* w, const cips_ray_params* rays, float level, int refine, float* depth,
                                     unsigned char* hit, float* sigma, float* points, float* trace, int B, cips_stream_t stream) {
  if (!w || !rays || !depth || !hit || B <= 0 || B > 65535 || refine < 0 || refine > 32) return (int)hipErrorInvalidValue;
  if (rays->jitter || rays->zvals || rays->W <= 0 || rays->H <= 0) return (int)hipErrorInvalidValue;
  if ((long long)rays->W * rays->H > INT_MAX) return (int)hipErrorInvalidValue;
  SurfaceX3Args a;
  if (const int rc = fill_raygen(a.rg, rays)) return rc;
  a.w = *w; a.level = level; a.refine = refine; a.depth = depth; a.hit = hit; a.sigma = sigma; a.points = points; a.trace = trace;
  a.B = B; a.chunk = surface_chunk(B, a.rg.n);
  dim3 g((a.rg.n + a.chunk - 1) / a.chunk, B);
  x3_pick([&](auto HW_, auto F16_, auto TRACE_) {
    x3_launch<siren_surface_x3_kernel<decltype(HW_)::value, decltype(F16_)::value, decltype(TRACE_)::value>>(g, 512, SF_SMEM_BYTES,
                                                                                                              stream, a);
  }, (w->trig_mode & 1) != 0, (w->trig_mode & 2) == 0, trace != nullptr);
  return CIPS_CHECK_LAUNCH();
}
