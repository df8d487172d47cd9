// raygen.h — in-kernel ray set-up shared by the SIREN kernels (siren_bwd_x3.hip, siren_fwd_x3.hip) and the resampler (render.hip).
#pragma once
#include "common.h"
#include "../../include/cips3d_hip.h"

// In-kernel ray set-up (what rays_kernel of render.hip materialises; exp/comm/comm_utils.py:365-438, 584-679): the
// sample point of (image b, ray, sample s) from the three linspace grids, the camera matrix and the jitter draw — 4 B
// per point read instead of 12 B, and no (B, n, S, 3) tensor in HBM.  Same expressions, in the same order, as
// rays_kernel.
struct RayGen {
  const float *xg, *yg, *zg;   // torch.linspace grids (W), (H), (S)
  const float* c2w;            // (B, 4, 4)
  const float* jitter;         // (B, n, S) uniforms or NULL
  const float* zvals;          // (B, n, S) depths or NULL; if set: point = camera origin + world ray direction * zvals[p]
                               // (the resampled "fine" points, generator_nerf_inr.py:590-592), grids / jitter unused
  float zc;
  int W, n, S;
};
struct RayDir { float dx, dy, dz; };
__device__ __forceinline__ RayDir ray_dir(const RayGen& g, int ray) {
  const int row = ray / g.W, col = ray - row * g.W;
  const float x = g.xg[col], y = g.yg[row];
  const float nrm = sqrtf(x * x + y * y + g.zc * g.zc);
  RayDir d = {x / nrm, y / nrm, g.zc / nrm};
  return d;
}
// camera-space sample at depth grid value z0 with jitter draw u (raw uniform; ignored when has_jit is false) -> world
// point and the jittered depth
__device__ __forceinline__ void ray_point(const RayGen& g, const float* M, const RayDir& d, float z0, float u, bool has_jit,
                                          float& wx, float& wy, float& wz, float& zout) {
  float z = z0;
  float px = d.dx * z, py = d.dy * z, pz = d.dz * z;
  if (has_jit) {
    const float off = (u - 0.5f) * (g.zg[1] - g.zg[0]);
    z = z + off;
    px = px + off * d.dx; py = py + off * d.dy; pz = pz + off * d.dz;
  }
  wx = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3];
  wy = ((M[4] * px + M[5] * py) + M[6] * pz) + M[7];
  wz = ((M[8] * px + M[9] * py) + M[10] * pz) + M[11];
  zout = z;
}
// point-major index p = ray * S + s of image b -> world point (and its depth)
__device__ __forceinline__ void gen_point(const RayGen& g, int b, int p, float& wx, float& wy, float& wz, float& z) {
  const int ray = p / g.S, s = p - ray * g.S;
  const RayDir d = ray_dir(g, ray);
  const float* M = g.c2w + (long long)b * 16;
  if (g.zvals) {
    // origin + direction * depth, with the direction rotated like rays_kernel and the sum like resample_kernel
    z = g.zvals[(long long)b * g.n * g.S + p];
    const float dx = (M[0] * d.dx + M[1] * d.dy) + M[2] * d.dz;
    const float dy = (M[4] * d.dx + M[5] * d.dy) + M[6] * d.dz;
    const float dz = (M[8] * d.dx + M[9] * d.dy) + M[10] * d.dz;
    wx = M[3] + dx * z; wy = M[7] + dy * z; wz = M[11] + dz * z;
    return;
  }
  const float u = g.jitter ? g.jitter[(long long)b * g.n * g.S + p] : 0.f;
  ray_point(g, M, d, g.zg[s], u, g.jitter != nullptr, wx, wy, wz, z);
}
__device__ __forceinline__ void gen_point(const RayGen& g, int b, int p, float& wx, float& wy, float& wz) {
  float z;
  gen_point(g, b, p, wx, wy, wz, z);
}

// gen_point with every rounding written out, for a kernel whose result is compared BIT FOR BIT with one computed at the points
// cips_rays_fwd / cips_resample_fwd materialised (cips_siren_bwd_points_x3_rays).  "The same expressions in the same order" is not
// enough for that: hipcc contracts a * b + c into an fma where it sees fit, differently from kernel to kernel (in rays_kernel the
// x and y jitter offsets are fused and the z offset is not; each row of the matrix product rounds ONE of its products and fuses
// the other two).  This is the sequence rays_kernel (points, directions) and resample_kernel (origin + direction * depth) are
// built with — contraction is off in here and every fused operation is an explicit fmaf — so it does not move with its caller.
// tests/test_gpu_points_gradient.py holds the two together: a compiler that builds those kernels otherwise shows there.
__device__ __forceinline__ void gen_point_materialised(const RayGen& g, int b, int p, float& wx, float& wy, float& wz) {
#pragma clang fp contract(off)
  const int ray = p / g.S, s = p - ray * g.S;
  const int row = ray / g.W, col = ray - row * g.W;
  const float x = g.xg[col], y = g.yg[row];
  const float nrm = sqrtf((x * x + y * y) + g.zc * g.zc);
  const float dx = x / nrm, dy = y / nrm, dz = g.zc / nrm;
  const float* M = g.c2w + (long long)b * 16;
  if (g.zvals) {
    const float z = g.zvals[(long long)b * g.n * g.S + p];
    const float rx = __builtin_fmaf(dz, M[2], __builtin_fmaf(dy, M[1], dx * M[0]));
    const float ry = __builtin_fmaf(dz, M[6], __builtin_fmaf(dx, M[4], dy * M[5]));
    const float rz = __builtin_fmaf(dz, M[10], __builtin_fmaf(dx, M[8], dy * M[9]));
    wx = __builtin_fmaf(rx, z, M[3]); wy = __builtin_fmaf(ry, z, M[7]); wz = __builtin_fmaf(rz, z, M[11]);
    return;
  }
  const float z0 = g.zg[s];
  float px = dx * z0, py = dy * z0, pz = dz * z0;
  if (g.jitter) {
    const float off = (g.jitter[(long long)b * g.n * g.S + p] - 0.5f) * (g.zg[1] - g.zg[0]);
    px = __builtin_fmaf(dx, off, px); py = __builtin_fmaf(dy, off, py); pz = pz + dz * off;
  }
  wx = __builtin_fmaf(pz, M[2], __builtin_fmaf(py, M[1], px * M[0])) + M[3];
  wy = __builtin_fmaf(pz, M[6], __builtin_fmaf(px, M[4], py * M[5])) + M[7];
  wz = __builtin_fmaf(pz, M[10], __builtin_fmaf(px, M[8], py * M[9])) + M[11];
}

// point-major index p of image b -> the CAMERA-space sample q of gen_point's world point (world = R q + t with R, t of cam2world):
// the px, py, pz ray_point forms before it applies the matrix, or direction * depth for the zvals form (where gen_point rotates
// the direction first and scales after).  For the reduction of per-point gradients to the camera matrix (cips_rays_bwd_cam).
__device__ __forceinline__ void gen_point_cam(const RayGen& g, int b, int p, float& qx, float& qy, float& qz) {
  const int ray = p / g.S, s = p - ray * g.S;
  const RayDir d = ray_dir(g, ray);
  if (g.zvals) {
    const float z = g.zvals[(long long)b * g.n * g.S + p];
    qx = d.dx * z; qy = d.dy * z; qz = d.dz * z;
    return;
  }
  const float z0 = g.zg[s];
  qx = d.dx * z0; qy = d.dy * z0; qz = d.dz * z0;
  if (g.jitter) {
    const float off = (g.jitter[(long long)b * g.n * g.S + p] - 0.5f) * (g.zg[1] - g.zg[0]);
    qx = qx + off * d.dx; qy = qy + off * d.dy; qz = qz + off * d.dz;
  }
}

static inline int fill_raygen(RayGen& g, const cips_ray_params* r) {
  if (!r || !r->xg || !r->yg || !r->zg || !r->cam2world || r->W <= 0 || r->H <= 0 || r->S <= 1) return (int)hipErrorInvalidValue;
  g.xg = r->xg; g.yg = r->yg; g.zg = r->zg; g.c2w = r->cam2world; g.jitter = r->jitter; g.zvals = r->zvals; g.zc = r->zc;
  g.W = r->W; g.n = r->W * r->H; g.S = r->S;
  return 0;
}
