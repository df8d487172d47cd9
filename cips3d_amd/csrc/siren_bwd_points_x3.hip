// siren_bwd_points_x3.hip — gradients w.r.t. WHERE the samples are, on the split-bf16 register chain of siren_x3_common.h:
//   cips_siren_bwd_points_x3 / _rays   the vector-Jacobian product of the FiLM-SIREN w.r.t. the point: (dfeat, dsigma) -> dpoint
//   cips_rays_bwd_cam                  per-point gradients -> the camera matrix (a streaming reduction)
// A source of its own: it runs only when a caller asks for a point or camera gradient, and as a separate module it leaves the
// listings of the forward, sigma and fused backward kernels as they are (profiles/points_gradient.txt has the resource table of
// every x3 kernel before and after).  The kernel stages all three weight images itself, so img_addr is instantiated with the
// three row counts as in the forward module.
#include "siren_x3_common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// VJP of the SIREN w.r.t. the point.  The sigma-gradient kernel's layout (lane = point, a wave owns 32 points, the two lane
// halves split the features, accumulators feed the next layer as B operand) on the forward's LDS carve (W1, Wc, Wf images, the
// layer-0 packs and the FiLM vectors: O_STG bytes).  ONE 256-thread workgroup per CU like the fused backward — one wave per SIMD,
// 512 registers per lane: under __launch_bounds__(512, 2) hipcc is 21 (hardware sines) to 82 (polynomial) registers short and
// spills; here it uses 254-256 VGPRs + 64-114 AGPRs, no scratch, no spilled VGPR in any instantiation.
// RAYS: the point is regenerated from the ray parameters by gen_point_materialised (raygen.h), whose roundings are those of the
// kernels that materialise points: the result is the points form's at cips_rays_fwd's / cips_resample_fwd's points bit for bit.
//   recompute   a0 = pack . (x, 1), h1 = sin a0;  a1 = g1 (W1 h1) + c1, h2 = sin a1;  ac = gc (Wc h2) + cc
//   VJP         dhc = Wf^T dfeat;  dpc = gc cos(ac) dhc;  dh2 = Wc^T dpc + dsigma ws;  dp1 = g1 cos(a1) dh2;  dh1 = W1^T dp1;
//               dpoint = sum_f pack[f].xyz cos(a0[f]) dh1[f]          (pack.xyz = g0 box_scale W0: the 2 / 0.24 is in it)
// 25 088 MAC of recompute and 26 624 + 384 MAC of transposed layers per point, 448 trigonometric evaluations, no weight-gradient
// contraction.  Operands: three-pass split bf16 like the fused backward, whatever trig_mode's bit 1 says — the upstream gradient
// has no known range, and bf16 planes have fp32's exponent: no rescaling rule, nothing to overflow or go subnormal for any
// weight or gradient magnitude fp32 itself holds.
// HW (trig_mode bit 0): the staging stores W1, Wc and the layer-0 packs divided by 2 pi (sines take revolutions), so each of the
// three transposed factors carries 1 / (2 pi): dsigma ws joins the chain divided by 2 pi (behind Wc^T), and the output is
// multiplied by (2 pi)^3.
// g1 cos(a1) and gc cos(ac) overwrite the accumulators they come from: 64 + 32 registers carry the forward to the VJP.
struct BwdPointsX3Args {
  cips_siren_weights w;
  const float* points;               // (B, P, 3) or NULL: generated from rg (point index = ray * S + s)
  const float* dfeat;                // (B, P, 32)
  const float* dsigma;               // (B, P)
  float* dpoints;                    // (B, P, 3)
  RayGen rg;
  int B, P, chunk;
};

template <bool HW, bool RAYS>
__global__ __launch_bounds__(256, 1) void siren_bwd_points_x3_kernel(BwdPointsX3Args a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  const int b = blockIdx.y;
  stage_weights_x3<HW, false>(smem, a.w, b);
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
  const float oscale = HW ? 248.05021344239853f : 1.f;         // (2 pi)^3
  const int cstart = blockIdx.x * a.chunk;
  const int cend = min(cstart + a.chunk, a.P);
  for (int pbase = cstart + wave * 32; pbase < cend; pbase += 4 * 32) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int l31 = lane & 31, hf = lane >> 5;
    const LaneAddr LA = lane_addr(lane, sbase);
    const int p = pbase + l31;
    const bool valid = p < cend;
    const int pc = valid ? p : cend - 1;           // ragged tail: the last valid point again, nothing stored
    const long long gp = (long long)b * a.P + pc;
    float px, py, pz;
    if constexpr (RAYS) gen_point_materialised(a.rg, b, pc, px, py, pz);
    else { px = a.points[gp * 3 + 0]; py = a.points[gp * 3 + 1]; pz = a.points[gp * 3 + 2]; }
    const float dsg = a.dsigma[gp];
    const float dsw = HW ? dsg * CIPS_INV_2PI : dsg;

    // ---- recompute: layer 0 and the W1 product, one 32-feature tile of h1 at a time (siren_sigma_w1.inc's order) ----
    f32x16 acc[4];
    zero_acc(acc);
    {
      const ImgBase wb(LA.fb, O_W1H);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        Act<1> h1q;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 pk[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = lds_ld4(LA.v64 + 128 * (4 * q + g) + 16 * e);
          __builtin_amdgcn_sched_barrier(0);
          float sn[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) sn[e] = sin_rev<HW>(fmaf(pk[e].x, px, fmaf(pk[e].y, py, fmaf(pk[e].z, pz, pk[e].w))));
          split2(sn[0], sn[1], h1q.hi[0][2 * g], h1q.lo[0][2 * g]);
          split2(sn[2], sn[3], h1q.hi[0][2 * g + 1], h1q.lo[0][2 * g + 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
        auto load = [&](int t, int m, Frag& f) {            // layer_fwd's fragment of k-step 2q + t, output tile m
          frag_fwd<O_W1L - O_W1H>(wb.b[t][0], wb.b[t][1], q * H * 64 + m * 2048, f);
        };
        run_layer<4, 2>(load, h1q, acc);
      }
    }
    // layer-1 epilogue: h2 = sin a1 packed for Wc; g1 cos a1 replaces the pre-activation in acc
    f32x16 accc[2];
    {
      Act<4> h2p;
      float4 gn = lds_ld4(LA.v16 + (O_G1 - O_L0)), cn = lds_ld4(LA.v16 + (O_C1 - O_L0));
#pragma unroll
      for (int grp = 0; grp < 16; ++grp) {
        const float4 g4 = gn, c4 = cn;
        if (grp + 1 < 16) { gn = lds_ld4(LA.v16 + (O_G1 - O_L0) + 32 * (grp + 1)); cn = lds_ld4(LA.v16 + (O_C1 - O_L0) + 32 * (grp + 1)); }
        __builtin_amdgcn_sched_barrier(0);
        const int q = grp >> 2, g = grp & 3;
        const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, cc[4] = {c4.x, c4.y, c4.z, c4.w};
        float sn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float cs;
          sincos_rev<HW>(fmaf(gg[e], acc[q][4 * g + e], cc[e]), &sn[e], &cs);
          acc[q][4 * g + e] = gg[e] * cs;
        }
        split2(sn[0], sn[1], h2p.hi[q][2 * g], h2p.lo[q][2 * g]);
        split2(sn[2], sn[3], h2p.hi[q][2 * g + 1], h2p.lo[q][2 * g + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      zero_acc(accc);
      layer_fwd<2, 4, HC, O_WCH, O_WCL - O_WCH>(LA, h2p, accc);
    }
    // colour epilogue: gc cos ac replaces the pre-activation in accc (hc = sin ac feeds no output of the VJP)
    {
      float4 gn = lds_ld4(LA.v16 + (O_GC - O_L0)), cn = lds_ld4(LA.v16 + (O_CC - O_L0));
#pragma unroll
      for (int grp = 0; grp < 8; ++grp) {
        const float4 g4 = gn, c4 = cn;
        if (grp + 1 < 8) { gn = lds_ld4(LA.v16 + (O_GC - O_L0) + 32 * (grp + 1)); cn = lds_ld4(LA.v16 + (O_CC - O_L0) + 32 * (grp + 1)); }
        __builtin_amdgcn_sched_barrier(0);
        const int q = grp >> 2, g = grp & 3;
        const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, cc[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) accc[q][4 * g + e] = gg[e] * cos_rev<HW>(fmaf(gg[e], accc[q][4 * g + e], cc[e]));
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ---- VJP.  dfeat enters as B operand in the chain's k order: register r <-> channel (r&3) + 8(r>>2) + 4hf ----
    f32x16 dhc[2];
    {
      Act<1> dfp;
      const float* fi = a.dfeat + gp * CF + 4 * hf;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(fi + 8 * g);
        split2(v.x, v.y, dfp.hi[0][2 * g], dfp.lo[0][2 * g]);
        split2(v.z, v.w, dfp.hi[0][2 * g + 1], dfp.lo[0][2 * g + 1]);
      }
      zero_acc(dhc);
      layer_tr<2, 2, CF, O_WFH, O_WFL - O_WFH>(LA, dfp, dhc);       // dhc = Wf^T dfeat
    }
    f32x16 dh2[4];
    {
      Act<2> dpcp;                                                  // dpc = gc cos(ac) dhc
#pragma unroll
      for (int grp = 0; grp < 8; ++grp) {
        const int q = grp >> 2, g = grp & 3;
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = accc[q][4 * g + e] * dhc[q][4 * g + e];
        split2(d[0], d[1], dpcp.hi[q][2 * g], dpcp.lo[q][2 * g]);
        split2(d[2], d[3], dpcp.hi[q][2 * g + 1], dpcp.lo[q][2 * g + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      zero_acc(dh2);
      layer_tr<4, 4, HC, O_WCH, O_WCL - O_WCH>(LA, dpcp, dh2);      // Wc^T dpc
    }
    f32x16 dh1[4];
    {
      Act<4> dp1;                                                   // dp1 = g1 cos(a1) (Wc^T dpc + dsigma ws)
      float4 wn = lds_ld4(LA.v16 + (O_WS - O_L0));
#pragma unroll
      for (int grp = 0; grp < 16; ++grp) {
        const float4 w4 = wn;
        if (grp + 1 < 16) wn = lds_ld4(LA.v16 + (O_WS - O_L0) + 32 * (grp + 1));
        __builtin_amdgcn_sched_barrier(0);
        const int q = grp >> 2, g = grp & 3;
        const float ww[4] = {w4.x, w4.y, w4.z, w4.w};
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = acc[q][4 * g + e] * fmaf(dsw, ww[e], dh2[q][4 * g + e]);
        split2(d[0], d[1], dp1.hi[q][2 * g], dp1.lo[q][2 * g]);
        split2(d[2], d[3], dp1.hi[q][2 * g + 1], dp1.lo[q][2 * g + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      zero_acc(dh1);
      layer_tr<4, 8, H, O_W1H, O_W1L - O_W1H>(LA, dp1, dh1);        // dh1 = W1^T dp1
    }

    // layer 0 again: cos(a0) from the packs, and the three components as fmaf chains over the lane half's 64 features
    float gx = 0.f, gy = 0.f, gz = 0.f;
    {
      float4 pn[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) pn[e] = lds_ld4(LA.v64 + 16 * e);
#pragma unroll
      for (int grp = 0; grp < 16; ++grp) {
        float4 pk[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) pk[e] = pn[e];
        if (grp + 1 < 16) {
#pragma unroll
          for (int e = 0; e < 4; ++e) pn[e] = lds_ld4(LA.v64 + 128 * (grp + 1) + 16 * e);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int q = grp >> 2, g = grp & 3;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = cos_rev<HW>(fmaf(pk[e].x, px, fmaf(pk[e].y, py, fmaf(pk[e].z, pz, pk[e].w)))) * dh1[q][4 * g + e];
          gx = fmaf(pk[e].x, t, gx); gy = fmaf(pk[e].y, t, gy); gz = fmaf(pk[e].z, t, gz);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    gx += __shfl_xor(gx, 32); gy += __shfl_xor(gy, 32); gz += __shfl_xor(gz, 32);
    if (valid && hf == 0) {
      float* go = a.dpoints + gp * 3;
      go[0] = gx * oscale; go[1] = gy * oscale; go[2] = gz * oscale;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Per-point gradients -> camera matrix.  The world point is  p = R q + t  with q the camera-space sample (gen_point_cam), so
// dR = sum_p dpoint q^T and dt = sum_p dpoint: twelve sums over an image's points.  One workgroup of 1024 threads per image:
// thread t adds points t, t + 1024, ... in ascending order, the 64 lanes of a wave are folded by a butterfly, the 16 waves by
// thread 0 in ascending order — a fixed order throughout, no atomics, the same bits on every call.  12 B of gradient and at most
// 4 B of jitter or depth per point are read.
struct RaysBwdCamArgs {
  RayGen rg;
  const float* dpoints;              // (B, P, 3)
  float* dc2w;                       // (B, 4, 4)
};

__global__ __launch_bounds__(1024) void rays_bwd_cam_kernel(RaysBwdCamArgs a) {
  __shared__ float part[16][12];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int P = a.rg.n * a.rg.S;
  const float* dp = a.dpoints + (long long)b * P * 3;
  float s[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) s[i] = 0.f;
#pragma unroll 4
  for (int p = tid; p < P; p += 1024) {
    float q[3];
    gen_point_cam(a.rg, b, p, q[0], q[1], q[2]);
    const float d[3] = {dp[3 * (long long)p], dp[3 * (long long)p + 1], dp[3 * (long long)p + 2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) s[4 * i + j] = fmaf(d[i], q[j], s[4 * i + j]);
      s[4 * i + 3] += d[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) part[tid >> 6][i] = s[i];
  }
  __syncthreads();
  if (tid < 16) {
    float v = 0.f;
    if (tid < 12) {
      for (int w = 0; w < 16; ++w) v += part[w][tid];
    }
    a.dc2w[(long long)b * 16 + tid] = v;         // row 3 (tid 12..15): zeros
  }
}

// the ray form's point count, or an error when the parameters are refused or W * H * S does not fit an int
int rays_point_count(RayGen& g, const cips_ray_params* rays, int* P) {
  if (const int rc = fill_raygen(g, rays)) return rc;
  const long long n = (long long)rays->W * rays->H;
  if (n > INT_MAX || n * rays->S > INT_MAX) return (int)hipErrorInvalidValue;
  *P = (int)(n * rays->S);
  return 0;
}

int siren_bwd_points_x3_launch(const cips_siren_weights* w, const float* points, const RayGen& rg, const float* dfeat,
                               const float* dsigma, float* dpoints, int B, int P, cips_stream_t stream) {
  BwdPointsX3Args a;
  a.w = *w; a.points = points; a.dfeat = dfeat; a.dsigma = dsigma; a.dpoints = dpoints; a.rg = rg; a.B = B; a.P = P;
  a.chunk = x3_chunk(B, P);
  dim3 grid((P + a.chunk - 1) / a.chunk, B);
  x3_pick([&](auto HW_, auto RAYS_) {
    x3_launch<siren_bwd_points_x3_kernel<decltype(HW_)::value, decltype(RAYS_)::value>>(grid, 256, O_STG, stream, a);
  }, (w->trig_mode & 1) != 0, points == nullptr);
  return CIPS_CHECK_LAUNCH();
}

}  // namespace

extern "C" int cips_siren_bwd_points_x3(const cips_siren_weights* w, const float* points, const float* dfeat, const float* dsigma,
                                        float* dpoints, int B, int P, cips_stream_t stream) {
  if (!w || !points || !dfeat || !dsigma || !dpoints || B <= 0 || B > 65535 || P <= 0) return (int)hipErrorInvalidValue;
  return siren_bwd_points_x3_launch(w, points, RayGen{}, dfeat, dsigma, dpoints, B, P, stream);
}

extern "C" int cips_siren_bwd_points_x3_rays(const cips_siren_weights* w, const cips_ray_params* rays, const float* dfeat,
                                             const float* dsigma, float* dpoints, int B, cips_stream_t stream) {
  if (!w || !rays || !dfeat || !dsigma || !dpoints || B <= 0 || B > 65535) return (int)hipErrorInvalidValue;
  RayGen rg;
  int P;
  if (const int rc = rays_point_count(rg, rays, &P)) return rc;
  return siren_bwd_points_x3_launch(w, nullptr, rg, dfeat, dsigma, dpoints, B, P, stream);
}

extern "C" int cips_rays_bwd_cam(const cips_ray_params* rays, const float* dpoints, float* dcam2world, int B, cips_stream_t stream) {
  if (!rays || !dpoints || !dcam2world || B <= 0) return (int)hipErrorInvalidValue;
  RaysBwdCamArgs a;
  int P;
  if (const int rc = rays_point_count(a.rg, rays, &P)) return rc;
  a.dpoints = dpoints; a.dc2w = dcam2world;
  hipLaunchKernelGGL(rays_bwd_cam_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, a);
  return CIPS_CHECK_LAUNCH();
}
