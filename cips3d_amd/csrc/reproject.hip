// reproject.hip — depth-based view reprojection for gfx950: what the pixels of a TARGET view see of a SOURCE view, and the
// gradient of that with respect to the source image and the target depth.
//
//   target pixel (i, j), depth t   ->  q  = d(i, j) * t          d = (x, y, zc_tgt) / |(x, y, zc_tgt)|   (raygen.h's camera)
//                                      q' = R q + tr             [R | tr] = tgt2src of the image
//                                      (u, v) = source pixel coordinates of q' (pinhole, image plane at zc_src)
//                                      out = bilinear sample of src at (u, v);  visible iff |q'| <= sample of src_depth + occ_tol
//
// The definition, decision by decision, is in include/cips3d_hip.h.  Replaces the ATen composition (a dozen elementwise
// launches around grid_sample, in fp32 on coordinates that have just been through the subtraction of two camera positions).
//
//   launch 1  reproject_fwd_kernel   one thread per 4 consecutive target columns, all channels: out and uv leave as 16-byte
//                                    stores and the mask as one dword where the row length is a multiple of 4 (scalar stores
//                                    otherwise: no shape is refused).  blockIdx.y is the image: its 12 transform values are
//                                    wave-uniform.
//   launch 2  reproject_bwd_kernel   one thread per target pixel: d tgt_depth is a gather (plain stores, reproducible);
//                                    d src is a scatter-add of the four bilinear weights per channel with no-return fp32
//                                    atomicAdd (one global_atomic_add_f32) into a buffer the entry point zeroes.  Neighbouring
//                                    lanes are neighbouring target pixels, which a smooth warp sends to neighbouring source
//                                    addresses.  The sums of d src depend on arrival order: it is the one output here whose
//                                    last bits can differ from call to call.
//
// The geometry of a pixel (a few dozen operations) runs in fp64 and (u, v) is rounded to fp32 once: the chain ends in the
// difference of numbers of size 1 scaled by |zc| * W / 2 (~10^3 at fov 12, 256 px), and the frame / occlusion decisions and
// the bilinear weights are taken from it.  The per-channel arithmetic is fp32.  Both kernels are bound by their memory
// traffic and their launches, not by that arithmetic.
#include <cmath>
#include "common.h"
#include "../../include/cips3d_hip.h"

namespace {

constexpr int COLS = 4;                  // target columns per thread of the forward kernel
constexpr double SLACK = 1.0 / 256.0;    // px by which (u, v) may leave the source frame and still count as inside

struct ReprojArgs {
  const float* src; const float* src_depth; const float* tgt_depth; const float* tgt2src;
  float* out; unsigned char* mask; float* uv;                 // forward outputs (uv may be NULL)
  const float* dout; const unsigned char* mask_in;            // backward inputs
  float* d_src; float* d_tgt_depth;                           // backward outputs (either may be NULL)
  double zc_tgt, zc_src, occ_tol;
  int B, C, Hs, Ws, Ht, Wt;
  int vec;                                                     // forward: Wt % 4 == 0 and every stored pointer is 16-byte aligned
};

// the image's transform, wave-uniform (b comes from blockIdx)
struct Pose { double m[12]; };
__device__ __forceinline__ Pose load_pose(const float* tgt2src, int b) {
  Pose p;
#pragma unroll
  for (int k = 0; k < 12; ++k) p.m[k] = (double)tgt2src[(size_t)b * 12 + k];
  return p;
}

// one target pixel: its point in source-camera space and its source pixel coordinates
struct Pix {
  double dx, dy, dz;        // the normalised ray
  double qx, qy, qz;        // q'
  double u, v;              // clamped to the source frame
  bool in;                  // in frame (step 5 of the definition)
  bool u_free, v_free;      // the clamp left u / v alone: it passes the derivative
};
__device__ __forceinline__ Pix project_pixel(const ReprojArgs& a, const Pose& P, int i, int j, float depth) {
  Pix p;
  const double x = -1.0 + 2.0 * (double)j / (double)(a.Wt - 1);
  const double y = 1.0 - 2.0 * (double)i / (double)(a.Ht - 1);
  const double nrm = sqrt(x * x + y * y + a.zc_tgt * a.zc_tgt);
  p.dx = x / nrm; p.dy = y / nrm; p.dz = a.zc_tgt / nrm;
  const double t = (double)depth;
  const double qx = p.dx * t, qy = p.dy * t, qz = p.dz * t;
  p.qx = P.m[0] * qx + P.m[1] * qy + P.m[2] * qz + P.m[3];
  p.qy = P.m[4] * qx + P.m[5] * qy + P.m[6] * qz + P.m[7];
  p.qz = P.m[8] * qx + P.m[9] * qy + P.m[10] * qz + P.m[11];
  const double xs = p.qx * a.zc_src / p.qz, ys = p.qy * a.zc_src / p.qz;
  const double u = (xs + 1.0) * 0.5 * (double)(a.Ws - 1), v = (1.0 - ys) * 0.5 * (double)(a.Hs - 1);
  const double umax = (double)(a.Ws - 1), vmax = (double)(a.Hs - 1);
  // every test is written so that a NaN fails it
  p.in = (depth > 0.f) && (depth <= 3.402823466e38f) && (p.qz * a.zc_src > 0.0) && (u >= -SLACK) && (u <= umax + SLACK) &&
         (v >= -SLACK) && (v <= vmax + SLACK);
  p.u_free = (u >= 0.0) && (u <= umax);
  p.v_free = (v >= 0.0) && (v <= vmax);
  // fmax / fmin return the other operand for a NaN: (u, v) is inside the frame whatever came in, and so is every index
  p.u = fmin(fmax(u, 0.0), umax);
  p.v = fmin(fmax(v, 0.0), vmax);
  return p;
}

// the bilinear cell of a clamped (u, v): offset of its top-left pixel in a source plane and the two weights
struct Cell { int u0, v0, off; float fu, fv; };
__device__ __forceinline__ Cell cell_of(const ReprojArgs& a, double u, double v) {
  int u0 = (int)floor(u), v0 = (int)floor(v);
  u0 = min(max(u0, 0), a.Ws - 2);
  v0 = min(max(v0, 0), a.Hs - 2);
  Cell c;
  c.u0 = u0; c.v0 = v0;
  c.off = v0 * a.Ws + u0;
  c.fu = (float)(u - (double)u0);
  c.fv = (float)(v - (double)v0);
  return c;
}

__device__ __forceinline__ float bilinear(const float* __restrict__ plane, const Cell& c, int Ws) {
  const float s00 = plane[c.off], s01 = plane[c.off + 1], s10 = plane[c.off + Ws], s11 = plane[c.off + Ws + 1];
  const float top = fmaf(c.fu, s01 - s00, s00), bot = fmaf(c.fu, s11 - s10, s10);
  return fmaf(c.fv, bot - top, top);
}

__global__ __launch_bounds__(256) void reproject_fwd_kernel(ReprojArgs a) {
  const int quads_per_row = (a.Wt + COLS - 1) / COLS;
  const long long quad = (long long)blockIdx.x * 256 + threadIdx.x;
  if (quad >= (long long)a.Ht * quads_per_row) return;
  const int b = blockIdx.y;
  const int i = (int)(quad / quads_per_row), j0 = (int)(quad - (long long)i * quads_per_row) * COLS;
  const Pose P = load_pose(a.tgt2src, b);
  const size_t tplane = (size_t)a.Ht * a.Wt, splane = (size_t)a.Hs * a.Ws;
  const size_t pix0 = (size_t)i * a.Wt + j0;                       // of this thread's first pixel, in a target plane
  const int ncol = min(COLS, a.Wt - j0);

  float depth[COLS];
  if (a.vec) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(a.tgt_depth + (size_t)b * tplane + pix0);
    depth[0] = t.x; depth[1] = t.y; depth[2] = t.z; depth[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < COLS; ++k) depth[k] = k < ncol ? a.tgt_depth[(size_t)b * tplane + pix0 + k] : 0.f;
  }

  Cell cell[COLS];
  unsigned char m[COLS];
  float uo[COLS], vo[COLS];
#pragma unroll
  for (int k = 0; k < COLS; ++k) {
    const Pix p = project_pixel(a, P, i, j0 + k, depth[k]);
    cell[k] = cell_of(a, p.u, p.v);
    m[k] = 0;
    if (p.in && k < ncol) {
      m[k] = 1;
      if (a.src_depth) {
        const double rho = sqrt(p.qx * p.qx + p.qy * p.qy + p.qz * p.qz);
        const float* dp = a.src_depth + (size_t)b * splane;
        const double s00 = dp[cell[k].off], s01 = dp[cell[k].off + 1], s10 = dp[cell[k].off + a.Ws],
                     s11 = dp[cell[k].off + a.Ws + 1];
        const double fu = p.u - (double)cell[k].u0, fv = p.v - (double)cell[k].v0;
        const double top = s00 + fu * (s01 - s00), bot = s10 + fu * (s11 - s10);
        const double ds = top + fv * (bot - top);
        m[k] = (rho <= ds + a.occ_tol) ? 1 : 2;                   // a NaN in ds compares false: occluded
      }
    }
    const float nan = __int_as_float(0x7fc00000);
    uo[k] = m[k] ? (float)p.u : nan;
    vo[k] = m[k] ? (float)p.v : nan;
  }

  if (a.vec) {
    *reinterpret_cast<unsigned int*>(a.mask + (size_t)b * tplane + pix0) =
        (unsigned)m[0] | ((unsigned)m[1] << 8) | ((unsigned)m[2] << 16) | ((unsigned)m[3] << 24);
    if (a.uv) {
      f32x4 w;
      w.x = uo[0]; w.y = uo[1]; w.z = uo[2]; w.w = uo[3];
      *reinterpret_cast<f32x4*>(a.uv + ((size_t)b * 2) * tplane + pix0) = w;
      w.x = vo[0]; w.y = vo[1]; w.z = vo[2]; w.w = vo[3];
      *reinterpret_cast<f32x4*>(a.uv + ((size_t)b * 2 + 1) * tplane + pix0) = w;
    }
  } else {
    for (int k = 0; k < ncol; ++k) {
      a.mask[(size_t)b * tplane + pix0 + k] = m[k];
      if (a.uv) {
        a.uv[((size_t)b * 2) * tplane + pix0 + k] = uo[k];
        a.uv[((size_t)b * 2 + 1) * tplane + pix0 + k] = vo[k];
      }
    }
  }

  for (int c = 0; c < a.C; ++c) {
    const float* sp = a.src + ((size_t)b * a.C + c) * splane;
    float* op = a.out + ((size_t)b * a.C + c) * tplane + pix0;
    float r[COLS];
#pragma unroll
    for (int k = 0; k < COLS; ++k) r[k] = m[k] == 1 ? bilinear(sp, cell[k], a.Ws) : 0.f;
    if (a.vec) {
      f32x4 w;
      w.x = r[0]; w.y = r[1]; w.z = r[2]; w.w = r[3];
      *reinterpret_cast<f32x4*>(op) = w;
    } else {
      for (int k = 0; k < ncol; ++k) op[k] = r[k];
    }
  }
}

__global__ __launch_bounds__(256) void reproject_bwd_kernel(ReprojArgs a) {
  const size_t tplane = (size_t)a.Ht * a.Wt, splane = (size_t)a.Hs * a.Ws;
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= tplane) return;
  const int b = blockIdx.y;
  // the forward's decision, read, not taken again
  if (a.mask_in[(size_t)b * tplane + pix] != 1) {
    if (a.d_tgt_depth) a.d_tgt_depth[(size_t)b * tplane + pix] = 0.f;
    return;
  }
  const int i = (int)(pix / a.Wt), j = (int)(pix - (size_t)i * a.Wt);
  const Pose P = load_pose(a.tgt2src, b);
  const Pix p = project_pixel(a, P, i, j, a.tgt_depth[(size_t)b * tplane + pix]);
  const Cell cl = cell_of(a, p.u, p.v);
  const float w00 = (1.f - cl.fu) * (1.f - cl.fv), w01 = cl.fu * (1.f - cl.fv), w10 = (1.f - cl.fu) * cl.fv, w11 = cl.fu * cl.fv;
  double gu = 0.0, gv = 0.0;                                     // sum_c dout_c * d out_c / d u, / d v
  for (int c = 0; c < a.C; ++c) {
    const float g = a.dout[((size_t)b * a.C + c) * tplane + pix];
    if (a.d_tgt_depth) {
      const float* sp = a.src + ((size_t)b * a.C + c) * splane + cl.off;
      const float s00 = sp[0], s01 = sp[1], s10 = sp[a.Ws], s11 = sp[a.Ws + 1];
      const float du = fmaf(cl.fv, (s11 - s10) - (s01 - s00), s01 - s00);
      const float dv = fmaf(cl.fu, (s11 - s01) - (s10 - s00), s10 - s00);
      gu += (double)g * (double)du;
      gv += (double)g * (double)dv;
    }
    if (a.d_src) {
      float* dp = a.d_src + ((size_t)b * a.C + c) * splane + cl.off;
      atomicAdd(dp, w00 * g);
      atomicAdd(dp + 1, w01 * g);
      atomicAdd(dp + a.Ws, w10 * g);
      atomicAdd(dp + a.Ws + 1, w11 * g);
    }
  }
  if (a.d_tgt_depth) {
    // e = R d;  d u / d depth = (Ws - 1) / 2 * zc_src * (e_x q'_z - q'_x e_z) / q'_z^2, zero where the clamp holds u
    const double ex = P.m[0] * p.dx + P.m[1] * p.dy + P.m[2] * p.dz;
    const double ey = P.m[4] * p.dx + P.m[5] * p.dy + P.m[6] * p.dz;
    const double ez = P.m[8] * p.dx + P.m[9] * p.dy + P.m[10] * p.dz;
    const double iz2 = a.zc_src / (p.qz * p.qz);
    const double dudt = p.u_free ? 0.5 * (double)(a.Ws - 1) * iz2 * (ex * p.qz - p.qx * ez) : 0.0;
    const double dvdt = p.v_free ? -0.5 * (double)(a.Hs - 1) * iz2 * (ey * p.qz - p.qy * ez) : 0.0;
    a.d_tgt_depth[(size_t)b * tplane + pix] = (float)(gu * dudt + gv * dvdt);
  }
}

bool shape_ok(int B, int C, int Hs, int Ws, int Ht, int Wt, float zc_tgt, float zc_src) {
  if (B < 1 || C < 1 || Hs < 2 || Ws < 2 || Ht < 2 || Wt < 2) return false;
  if (!std::isfinite(zc_tgt) || !std::isfinite(zc_src) || zc_tgt == 0.f || zc_src == 0.f) return false;
  // offsets inside one plane are ints; grid limits: x < 2^31, y < 65536
  return (long long)Hs * Ws <= 0x7fffffffLL && (long long)Ht * Wt <= 0x7fffffffLL && B <= 65535;
}

bool aligned(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" int cips_reproject_fwd(const float* src, const float* src_depth, const float* tgt_depth, const float* tgt2src,
                                  float zc_tgt, float zc_src, float occ_tol, float* out, unsigned char* mask, float* uv,
                                  int B, int C, int Hs, int Ws, int Ht, int Wt, cips_stream_t stream) {
  if (!src || !tgt_depth || !tgt2src || !out || !mask) return (int)hipErrorInvalidValue;
  if (!shape_ok(B, C, Hs, Ws, Ht, Wt, zc_tgt, zc_src)) return (int)hipErrorInvalidValue;
  if (src_depth && !(std::isfinite(occ_tol) && occ_tol >= 0.f)) return (int)hipErrorInvalidValue;
  ReprojArgs a = {};
  a.src = src; a.src_depth = src_depth; a.tgt_depth = tgt_depth; a.tgt2src = tgt2src; a.out = out; a.mask = mask; a.uv = uv;
  a.zc_tgt = zc_tgt; a.zc_src = zc_src; a.occ_tol = src_depth ? occ_tol : 0.0;
  a.B = B; a.C = C; a.Hs = Hs; a.Ws = Ws; a.Ht = Ht; a.Wt = Wt;
  a.vec = Wt % COLS == 0 && aligned(tgt_depth, 16) && aligned(out, 16) && aligned(mask, 4) && (!uv || aligned(uv, 16));
  const long long quads = (long long)Ht * ((Wt + COLS - 1) / COLS);
  hipLaunchKernelGGL(reproject_fwd_kernel, dim3((unsigned)((quads + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, a);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_reproject_bwd(const float* dout, const float* src, const float* tgt_depth, const float* tgt2src,
                                  const unsigned char* mask, float zc_tgt, float zc_src, float* d_src, float* d_tgt_depth,
                                  int B, int C, int Hs, int Ws, int Ht, int Wt, cips_stream_t stream) {
  if (!dout || !src || !tgt_depth || !tgt2src || !mask) return (int)hipErrorInvalidValue;
  if (!shape_ok(B, C, Hs, Ws, Ht, Wt, zc_tgt, zc_src)) return (int)hipErrorInvalidValue;
  if (!d_src && !d_tgt_depth) return 0;
  ReprojArgs a = {};
  a.src = src; a.tgt_depth = tgt_depth; a.tgt2src = tgt2src; a.dout = dout; a.mask_in = mask;
  a.d_src = d_src; a.d_tgt_depth = d_tgt_depth;
  a.zc_tgt = zc_tgt; a.zc_src = zc_src;
  a.B = B; a.C = C; a.Hs = Hs; a.Ws = Ws; a.Ht = Ht; a.Wt = Wt;
  hipStream_t st = (hipStream_t)stream;
  if (d_src) {
    const hipError_t e = hipMemsetAsync(d_src, 0, (size_t)B * C * Hs * Ws * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
  }
  const long long pixels = (long long)Ht * Wt;
  hipLaunchKernelGGL(reproject_bwd_kernel, dim3((unsigned)((pixels + 255) / 256), B), dim3(256), 0, st, a);
  return CIPS_CHECK_LAUNCH();
}
