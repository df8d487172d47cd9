// volume.hip — baked radiance volumes for gfx950: pack sigma and colour on a lattice into 16-byte nodes with a brick occupancy,
// and volume-render the result from any camera of raygen.h with the network out of the loop.  The rule, decision by decision,
// is in include/cips3d_hip.h (cips_volume_bake, cips_volume_render).
//
//   volume_pack_kernel    one thread per node: r, g, b, sigma leave as ONE 16-byte record (bits copied, nothing computed).
//   volume_occ_kernel     one wave per brick of 8 x 8 x 8 cells: the maximum of sigma over its 9 x 9 x 9 nodes (fewer at the
//                         upper faces), lanes stride the nodes, a butterfly of fmaxf.  A maximum has no rounding.
//   volume_render_kernel  one ray per lane, a wave is an 8 x 8 tile of pixels so that its 64 rays gather from neighbouring cells.
//                         Per ray: ray_dir once.  Per sample: ray_point, the inside test, (with skip) one 4-byte read of the
//                         brick's occupancy, eight 16-byte loads (four pairs of z-neighbours, 32 contiguous bytes each), seven
//                         vector lerps, the composite step.  No LDS, no cross-lane traffic: the kernel waits on gathers, not
//                         on arithmetic.
//
// The skip and the fetch run through the same code in the same kernel, and so do Bv = 1 and Bv = b: a fetched sample has the
// same bits whichever way it was reached.  Every float -> int conversion follows the inside test (0 <= u <= n - 1, false for a
// NaN), and every index is built from the clamped cell.
#include <cmath>
#include "common.h"
#include "raygen.h"
#include "../../include/cips3d_hip.h"

namespace {

constexpr int BRICK_SHIFT = 3;           // a brick is 8 cells per axis

struct PackArgs {
  const float* sigma; const float* rgb; f32x4* packed; float* occ;
  long long total;                       // Bv * nx * ny * nz
  int Bv, nx, ny, nz, bx, by, bz;
};

__global__ __launch_bounds__(256) void volume_pack_kernel(PackArgs a) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= a.total) return;
  f32x4 v;
  v.x = a.rgb[id * 3]; v.y = a.rgb[id * 3 + 1]; v.z = a.rgb[id * 3 + 2]; v.w = a.sigma[id];
  a.packed[id] = v;
}

__global__ __launch_bounds__(64) void volume_occ_kernel(PackArgs a) {
  const int bricks = a.bx * a.by * a.bz;                 // <= nx * ny * nz: fits
  const int vb = blockIdx.x / bricks, br = blockIdx.x - vb * bricks;
  const int I = br / (a.by * a.bz), rem = br - I * (a.by * a.bz), J = rem / a.bz, K = rem - J * a.bz;
  const int i0 = I << BRICK_SHIFT, j0 = J << BRICK_SHIFT, k0 = K << BRICK_SHIFT;
  const int ni = min(i0 + 8, a.nx - 1) - i0 + 1, nj = min(j0 + 8, a.ny - 1) - j0 + 1, nk = min(k0 + 8, a.nz - 1) - k0 + 1;
  const float* s = a.sigma + (size_t)vb * a.nx * a.ny * a.nz;
  float m = -INFINITY;
  for (int t = threadIdx.x; t < ni * nj * nk; t += 64) {
    const int di = t / (nj * nk), r2 = t - di * (nj * nk), dj = r2 / nk, dk = r2 - dj * nk;
    m = fmaxf(m, s[((size_t)(i0 + di) * a.ny + (j0 + dj)) * a.nz + (k0 + dk)]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if (threadIdx.x == 0) a.occ[blockIdx.x] = m;
}

struct VolArgs {
  const f32x4* vol; const float* occ;
  RayGen g;
  float lo[3], inv_h[3], umax[3];
  float *rgb, *depth, *opacity;
  int b, Bv, nx, ny, nz, by, bz, H, W, S, clamp_mode, flags;
  int tiles_x, tiles, blocks_per_image;
  long long nodes, bricks;
};

// F.relu / F.softplus (beta = 1, threshold = 20): clamp_density of render.hip
__device__ __forceinline__ float vol_clamp(float x, int mode) {
  if (mode == 1) return (x > 20.f) ? x : log1pf(expf(x));
  return fmaxf(x, 0.f);
}

__device__ __forceinline__ f32x4 vol_lerp(f32x4 p, f32x4 q, float t) { return p + t * (q - p); }

__global__ __launch_bounds__(256) void volume_render_kernel(VolArgs a) {
  const int img = blockIdx.x / a.blocks_per_image;
  const int tile = (blockIdx.x - img * a.blocks_per_image) * 4 + (threadIdx.x >> 6);
  if (tile >= a.tiles) return;
  const int lane = threadIdx.x & 63;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int r = ty * 8 + (lane >> 3), c = tx * 8 + (lane & 7);
  if (r >= a.H || c >= a.W) return;
  const int ray = r * a.W + c, S = a.S;
  const f32x4* vol = a.vol + (a.Bv == 1 ? 0 : (size_t)img * a.nodes);
  const bool skip = (a.flags & 4) && a.clamp_mode == 0;
  const bool last_back = a.flags & 1;
  const float* occ = skip ? a.occ + (a.Bv == 1 ? 0 : (size_t)img * a.bricks) : nullptr;
  const size_t sy = (size_t)a.nz, sx = (size_t)a.ny * a.nz;

  float cr = 0.f, cg = 0.f, cb = 0.f, depth = 0.f, wsum = 0.f, zlast = 0.f;
  f32x4 vlast = {0.f, 0.f, 0.f, 0.f};
  double T = 1.0;                         // the transmittance as composite_fwd_kernel keeps it: double, rounded per prefix
  // gen_point's two halves (raygen.h), the one that is constant along the ray taken out of the sample loop: the same expressions
  const RayDir dir = ray_dir(a.g, ray);
  const float* M = a.g.c2w + (size_t)img * 16;
  for (int s = 0; s < S; ++s) {
    float wx, wy, wz, z;
    ray_point(a.g, M, dir, a.g.zg[s], 0.f, false, wx, wy, wz, z);
    const float ux = (wx - a.lo[0]) * a.inv_h[0], uy = (wy - a.lo[1]) * a.inv_h[1], uz = (wz - a.lo[2]) * a.inv_h[2];
    const bool inside = ux >= 0.f && ux <= a.umax[0] && uy >= 0.f && uy <= a.umax[1] && uz >= 0.f && uz <= a.umax[2];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (inside) {
      const int i = min((int)ux, a.nx - 2), j = min((int)uy, a.ny - 2), k = min((int)uz, a.nz - 2);
      bool fetch = true;
      if (skip && !(last_back && s == S - 1))
        fetch = !(occ[((size_t)(i >> BRICK_SHIFT) * a.by + (j >> BRICK_SHIFT)) * a.bz + (k >> BRICK_SHIFT)] <= 0.f);
      if (fetch) {
        const float tx_ = ux - (float)i, ty_ = uy - (float)j, tz_ = uz - (float)k;
        const f32x4* p = vol + ((size_t)i * a.ny + j) * a.nz + k;
        const f32x4 c000 = p[0], c001 = p[1], c010 = p[sy], c011 = p[sy + 1];
        const f32x4 c100 = p[sx], c101 = p[sx + 1], c110 = p[sx + sy], c111 = p[sx + sy + 1];
        const f32x4 c00 = vol_lerp(c000, c001, tz_), c01 = vol_lerp(c010, c011, tz_);
        const f32x4 c10 = vol_lerp(c100, c101, tz_), c11 = vol_lerp(c110, c111, tz_);
        v = vol_lerp(vol_lerp(c00, c01, ty_), vol_lerp(c10, c11, ty_), tx_);
      }
    }
    const float delta = (s + 1 < S) ? (a.g.zg[s + 1] - z) : 1e10f;
    const float alpha = 1.f - expf(-delta * vol_clamp(v.w, a.clamp_mode));
    const float w = alpha * (float)T;
    T *= (double)(1.f - alpha + 1e-10f);
    cr = fmaf(w, v.x, cr); cg = fmaf(w, v.y, cg); cb = fmaf(w, v.z, cb);
    depth = fmaf(w, z, depth);
    wsum += w;
    vlast = v; zlast = z;
  }
  if (last_back) {                        // the last weight gains 1 - sum w
    const float extra = 1.f - wsum;
    cr = fmaf(extra, vlast.x, cr); cg = fmaf(extra, vlast.y, cg); cb = fmaf(extra, vlast.z, cb);
    depth = fmaf(extra, zlast, depth);
  }
  if (a.flags & 2) {                      // white_back
    const float extra = 1.f - wsum;
    cr += extra; cg += extra; cb += extra;
  }
  const size_t plane = (size_t)a.H * a.W, pix = (size_t)img * plane + ray;
  float* o = a.rgb + (size_t)img * 3 * plane + ray;
  o[0] = cr; o[plane] = cg; o[2 * plane] = cb;
  a.depth[pix] = depth;
  a.opacity[pix] = wsum;                  // neither adjustment above changed it
}

bool lattice_ok(int nx, int ny, int nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (long long)nx * ny * nz <= 0x7fffffffLL;
}

int bricks_of(int n) { return (n - 1 + 7) >> BRICK_SHIFT; }

}  // namespace

extern "C" int cips_volume_bake(const float* sigma, const float* rgb, void* packed, float* occ, int Bv, int nx, int ny, int nz,
                                cips_stream_t stream) {
  if (Bv < 0 || !lattice_ok(nx, ny, nz)) return (int)hipErrorInvalidValue;
  if (!sigma || !rgb || !packed || !occ) return (int)hipErrorInvalidValue;
  if ((uintptr_t)packed & 15) return (int)hipErrorInvalidValue;
  PackArgs a = {};
  a.sigma = sigma; a.rgb = rgb; a.packed = (f32x4*)packed; a.occ = occ;
  a.Bv = Bv; a.nx = nx; a.ny = ny; a.nz = nz; a.bx = bricks_of(nx); a.by = bricks_of(ny); a.bz = bricks_of(nz);
  a.total = (long long)Bv * nx * ny * nz;
  const long long pack_blocks = (a.total + 255) / 256, occ_blocks = (long long)Bv * a.bx * a.by * a.bz;
  if (pack_blocks > 0x7fffffffLL || occ_blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (Bv == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(volume_pack_kernel, dim3((unsigned)pack_blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(volume_occ_kernel, dim3((unsigned)occ_blocks), dim3(64), 0, st, a);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_volume_render(const void* packed, const float* occ, const float* lo, const float* hi, const float* xg,
                                  const float* yg, const float* zg, const float* cam2world, float zc, int clamp_mode, int flags,
                                  float* rgb, float* depth, float* opacity, int b, int Bv, int nx, int ny, int nz, int H, int W,
                                  int S, cips_stream_t stream) {
  if (b < 0 || Bv < 0 || !lattice_ok(nx, ny, nz) || H < 2 || W < 2 || S < 2) return (int)hipErrorInvalidValue;
  if (Bv != 1 && Bv != b) return (int)hipErrorInvalidValue;
  if ((long long)b * H * W > 0x7fffffffLL || (long long)H * W * S > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (clamp_mode != 0 && clamp_mode != 1) return (int)hipErrorInvalidValue;
  if (flags < 0 || flags > 7) return (int)hipErrorInvalidValue;
  if (!packed || !lo || !hi || !xg || !yg || !zg || !cam2world || !rgb || !depth || !opacity) return (int)hipErrorInvalidValue;
  if ((flags & 4) && !occ) return (int)hipErrorInvalidValue;
  if ((uintptr_t)packed & 15) return (int)hipErrorInvalidValue;
  if (std::isnan(zc) || std::isinf(zc) || !(zc < 0.f)) return (int)hipErrorInvalidValue;
  VolArgs a = {};
  const int n[3] = {nx, ny, nz};
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !(hi[k] > lo[k])) return (int)hipErrorInvalidValue;
    a.lo[k] = lo[k];
    a.umax[k] = (float)(n[k] - 1);
    a.inv_h[k] = a.umax[k] / (hi[k] - lo[k]);
    if (!std::isfinite(a.inv_h[k]) || !(a.inv_h[k] > 0.f)) return (int)hipErrorInvalidValue;
  }
  if (b == 0) return 0;
  a.vol = (const f32x4*)packed; a.occ = occ;
  a.g.xg = xg; a.g.yg = yg; a.g.zg = zg; a.g.c2w = cam2world; a.g.jitter = nullptr; a.g.zvals = nullptr; a.g.zc = zc;
  a.g.W = W; a.g.n = W * H; a.g.S = S;
  a.rgb = rgb; a.depth = depth; a.opacity = opacity;
  a.b = b; a.Bv = Bv; a.nx = nx; a.ny = ny; a.nz = nz; a.by = bricks_of(ny); a.bz = bricks_of(nz);
  a.H = H; a.W = W; a.S = S; a.clamp_mode = clamp_mode; a.flags = flags;
  a.nodes = (long long)nx * ny * nz; a.bricks = (long long)bricks_of(nx) * a.by * a.bz;
  a.tiles_x = (W + 7) >> 3;
  a.tiles = a.tiles_x * ((H + 7) >> 3);                  // <= H * W
  a.blocks_per_image = (a.tiles + 3) >> 2;
  const long long grid = (long long)b * a.blocks_per_image;          // <= b * H * W
  hipLaunchKernelGGL(volume_render_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  return CIPS_CHECK_LAUNCH();
}
