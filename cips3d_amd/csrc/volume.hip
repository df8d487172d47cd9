// volume.hip — baked radiance volumes for gfx950: pack sigma and colour on a lattice into 16-byte nodes with a brick occupancy,
// and volume-render the result from any camera of raygen.h with the network out of the loop.  The rule, decision by decision,
// is in include/cips3d_hip.h (cips_volume_bake, cips_volume_render, cips_volume_render_bwd).
//
//   volume_pack_kernel    one thread per node: r, g, b, sigma leave as ONE 16-byte record (bits copied, nothing computed).
//   volume_occ_kernel     one wave per brick of 8 x 8 x 8 cells: the maximum of sigma over its 9 x 9 x 9 nodes (fewer at the
//                         upper faces), lanes stride the nodes, a butterfly of fmaxf.  A maximum has no rounding.
//   volume_render_kernel  one ray per lane, a wave is an 8 x 8 tile of pixels so that its 64 rays gather from neighbouring cells.
//                         Per ray: ray_dir once.  Per sample: ray_point, the inside test, (with skip) one 4-byte read of the
//                         brick's occupancy, eight 16-byte loads (four pairs of z-neighbours, 32 contiguous bytes each), seven
//                         vector lerps, the composite step.  No LDS, no cross-lane traffic: the kernel waits on gathers, not
//                         on arithmetic.
//   volume_render_bwd_kernel  the gradient with respect to the nodes: the same lane marches the same ray, stores one 16-byte
//                         record per sample, walks the records backwards (composite_bwd_kernel<true>'s reverse scan) and adds
//                         into the eight nodes of every live sample with fp32 atomic adds.  volume_occ_kernel with stride 4
//                         rebuilds the occupancy of a packed volume whose nodes have moved (cips_volume_occupancy).
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
  int stride;                            // floats between two nodes' sigma (volume_occ_kernel)
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
  // sigma of node n at sigma[n * stride]: stride 1 for a plain sigma tensor, 4 (from channel 3 on) for a packed volume
  const float* s = a.sigma + (size_t)vb * a.nx * a.ny * a.nz * a.stride;
  float m = -INFINITY;
  for (int t = threadIdx.x; t < ni * nj * nk; t += 64) {
    const int di = t / (nj * nk), r2 = t - di * (nj * nk), dj = r2 / nk, dk = r2 - dj * nk;
    m = fmaxf(m, s[(((size_t)(i0 + di) * a.ny + (j0 + dj)) * a.nz + (k0 + dk)) * a.stride]);
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

// Where a sample lands: the inside test, the cell and the three weights, in this one place for the forward and the backward (the
// backward must find exactly the cell the forward did).  false outside the box, and for a NaN.
struct VolCell { int i, j, k; float tx, ty, tz; };

__device__ __forceinline__ bool vol_locate(const VolArgs& a, float wx, float wy, float wz, VolCell& c) {
  const float ux = (wx - a.lo[0]) * a.inv_h[0], uy = (wy - a.lo[1]) * a.inv_h[1], uz = (wz - a.lo[2]) * a.inv_h[2];
  const bool inside = ux >= 0.f && ux <= a.umax[0] && uy >= 0.f && uy <= a.umax[1] && uz >= 0.f && uz <= a.umax[2];
  if (inside) {
    c.i = min((int)ux, a.nx - 2); c.j = min((int)uy, a.ny - 2); c.k = min((int)uz, a.nz - 2);
    c.tx = ux - (float)c.i; c.ty = uy - (float)c.j; c.tz = uz - (float)c.k;
  }
  return inside;
}

// Is sample s at this world point fetched, and from which cell?  occ: the image's occupancy with the skip on, else NULL.
__device__ __forceinline__ bool vol_sample_cell(const VolArgs& a, const float* occ, bool last_back, int s, float wx, float wy,
                                                float wz, VolCell& c) {
  if (!vol_locate(a, wx, wy, wz, c)) return false;
  if (occ && !(last_back && s == a.S - 1))
    return !(occ[((size_t)(c.i >> BRICK_SHIFT) * a.by + (c.j >> BRICK_SHIFT)) * a.bz + (c.k >> BRICK_SHIFT)] <= 0.f);
  return true;
}

__device__ __forceinline__ f32x4 vol_fetch(const VolArgs& a, const f32x4* vol, const VolCell& c) {
  const size_t sy = (size_t)a.nz, sx = (size_t)a.ny * a.nz;
  const f32x4* p = vol + ((size_t)c.i * a.ny + c.j) * a.nz + c.k;
  const f32x4 c000 = p[0], c001 = p[1], c010 = p[sy], c011 = p[sy + 1];
  const f32x4 c100 = p[sx], c101 = p[sx + 1], c110 = p[sx + sy], c111 = p[sx + sy + 1];
  const f32x4 c00 = vol_lerp(c000, c001, c.tz), c01 = vol_lerp(c010, c011, c.tz);
  const f32x4 c10 = vol_lerp(c100, c101, c.tz), c11 = vol_lerp(c110, c111, c.tz);
  return vol_lerp(vol_lerp(c00, c01, c.ty), vol_lerp(c10, c11, c.ty), c.tx);
}

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

  float cr = 0.f, cg = 0.f, cb = 0.f, depth = 0.f, wsum = 0.f, zlast = 0.f;
  f32x4 vlast = {0.f, 0.f, 0.f, 0.f};
  double T = 1.0;                         // the transmittance as composite_fwd_kernel keeps it: double, rounded per prefix
  // gen_point's two halves (raygen.h), the one that is constant along the ray taken out of the sample loop: the same expressions
  const RayDir dir = ray_dir(a.g, ray);
  const float* M = a.g.c2w + (size_t)img * 16;
  for (int s = 0; s < S; ++s) {
    float wx, wy, wz, z;
    ray_point(a.g, M, dir, a.g.zg[s], 0.f, false, wx, wy, wz, z);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    VolCell cell;
    if (vol_sample_cell(a, occ, last_back, s, wx, wy, wz, cell)) v = vol_fetch(a, vol, cell);
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

// d clamp / d x: clamp_density_grad of render.hip
__device__ __forceinline__ float vol_clamp_grad(float x, int mode) {
  if (mode == 1) return (x > 20.f) ? 1.f : 1.f / (1.f + expf(-x));
  return x > 0.f ? 1.f : 0.f;
}

__device__ __forceinline__ float sel4(int c, float v0, float v1, float v2, float v3) {
  return c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : v3;
}

struct VolBwdArgs {
  VolArgs f;                              // the forward's arguments (its three outputs unused)
  const float *drgb, *ddepth, *dopacity;  // the last two may be NULL (zeros)
  float* dpacked;                         // zeroed by the entry point
  f32x4* rec;                             // S * threads records (alpha, fp32(T), s, x), sample-major
  size_t threads;                         // grid * 256
};

// The backward of volume_render_kernel with respect to the nodes: the same lane marches the same ray forward once, storing one
// 16-byte record per sample (sample-major by the thread's linear id: a wave stores 1 KiB contiguous), then walks the records
// backwards with composite_bwd_kernel<true>'s reverse scan (no division) and adds omega * (w G, dx) to the eight nodes of every
// live sample.  The reverse pass gathers nothing from the volume: it recomputes the cell and t through the forward's helpers.
// A thread reads back only its own stores, so there is no fence.
//   QUAD = false: every lane adds its own four dwords per corner — per wave-instruction 64 dwords in up to 64 nodes.
//   QUAD = true:  the four lanes of a quad transpose their 4 x 4 values among themselves first (three shuffles), so that in
//                 instruction r the quad covers the 16 contiguous bytes of the node of its lane r: the same number of atomic
//                 instructions, 16-byte segments.  Lanes off the image stay for the shuffles; they march and add nothing.
template <bool QUAD>
__global__ __launch_bounds__(256) void volume_render_bwd_kernel(VolBwdArgs q) {
  const VolArgs& a = q.f;
  const int img = blockIdx.x / a.blocks_per_image;
  const int tile = (blockIdx.x - img * a.blocks_per_image) * 4 + (threadIdx.x >> 6);
  if (tile >= a.tiles) return;            // the whole wave
  const int lane = threadIdx.x & 63;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int r = ty * 8 + (lane >> 3), c = tx * 8 + (lane & 7);
  const bool on = r < a.H && c < a.W;
  if (!QUAD && !on) return;
  const int ray = on ? r * a.W + c : 0, S = a.S;
  const bool skip = (a.flags & 4) && a.clamp_mode == 0;
  const bool last_back = a.flags & 1;
  const float* occ = skip ? a.occ + (a.Bv == 1 ? 0 : (size_t)img * a.bricks) : nullptr;
  f32x4* rec = q.rec + ((size_t)blockIdx.x * 256 + threadIdx.x);
  const RayDir dir = ray_dir(a.g, ray);
  const float* M = a.g.c2w + (size_t)img * 16;

  float Gr = 0.f, Gg = 0.f, Gb = 0.f, gd = 0.f, wsum = 0.f, s_off = 0.f;
  if (on) {
    const f32x4* vol = a.vol + (a.Bv == 1 ? 0 : (size_t)img * a.nodes);
    const size_t plane = (size_t)a.H * a.W, pix = (size_t)img * plane + ray;
    const float* gp = q.drgb + (size_t)img * 3 * plane + ray;
    Gr = gp[0]; Gg = gp[plane]; Gb = gp[2 * plane];
    gd = q.ddepth ? q.ddepth[pix] : 0.f;
    const float go = q.dopacity ? q.dopacity[pix] : 0.f;
    double T = 1.0;
    float slast = 0.f;
    for (int s = 0; s < S; ++s) {         // the forward's march, expression by expression
      float wx, wy, wz, z;
      ray_point(a.g, M, dir, a.g.zg[s], 0.f, false, wx, wy, wz, z);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      VolCell cell;
      if (vol_sample_cell(a, occ, last_back, s, wx, wy, wz, cell)) v = vol_fetch(a, vol, cell);
      const float delta = (s + 1 < S) ? (a.g.zg[s + 1] - z) : 1e10f;
      const float alpha = 1.f - expf(-delta * vol_clamp(v.w, a.clamp_mode));
      const float Tf = (float)T;
      wsum += alpha * Tf;
      T *= (double)(1.f - alpha + 1e-10f);
      slast = fmaf(gd, z, Gr * v.x + Gg * v.y + Gb * v.z);
      const f32x4 rc = {alpha, Tf, slast, v.w};
      rec[(size_t)s * q.threads] = rc;
    }
    s_off = (last_back ? slast : 0.f) + ((a.flags & 2) ? (Gr + Gg + Gb) : 0.f) - go;
  }

  float* dvol = q.dpacked + (a.Bv == 1 ? 0 : (size_t)img * a.nodes * 4);
  const int sy = a.nz, sx = a.ny * a.nz;  // nx * ny * nz fits in int
  float Q = 0.f;
  for (int k = S - 1; k >= 0; --k) {
    bool live = false;
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    VolCell cell = {0, 0, 0, 0.f, 0.f, 0.f};
    if (on) {
      float wx, wy, wz, z;
      ray_point(a.g, M, dir, a.g.zg[k], 0.f, false, wx, wy, wz, z);
      const bool fetched = vol_sample_cell(a, occ, last_back, k, wx, wy, wz, cell);
      const f32x4 rc = rec[(size_t)k * q.threads];
      const float alpha = rc.x, Tk = rc.y, s = rc.z - s_off, x = rc.w;
      float w = alpha * Tk;
      if (last_back && k == S - 1) w += 1.f - wsum;         // the colour of the last sample sees the topped-up weight
      const float dalpha = Tk * (s - Q);
      Q = fmaf(alpha, s, (1.f - alpha + 1e-10f) * Q);
      const float delta = (k + 1 < S) ? (a.g.zg[k + 1] - z) : 1e10f;
      const float dx = dalpha * (delta * expf(-delta * vol_clamp(x, a.clamp_mode))) * vol_clamp_grad(x, a.clamp_mode);
      // live: a sample the forward fetched whose colour weight or sigma gradient is not zero (a NaN is not zero)
      live = fetched && ((w != 0.f) || (dx != 0.f));
      g.x = w * Gr; g.y = w * Gg; g.z = w * Gb; g.w = dx;
    }
    if (QUAD) {
      if (__ballot(live) == 0) continue;                    // wave-uniform
    } else if (!live) {
      continue;
    }
    const int base = (cell.i * a.ny + cell.j) * a.nz + cell.k;
    if (!QUAD) {
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) {
        const int di = corner >> 2, dj = (corner >> 1) & 1, dk = corner & 1;
        const float om = ((di ? cell.tx : 1.f - cell.tx) * (dj ? cell.ty : 1.f - cell.ty)) * (dk ? cell.tz : 1.f - cell.tz);
        float* p = dvol + (size_t)(base + di * sx + dj * sy + dk) * 4;
        atomicAdd(p, om * g.x); atomicAdd(p + 1, om * g.y); atomicAdd(p + 2, om * g.z); atomicAdd(p + 3, om * g.w);
      }
    } else {
      const int qc = lane & 3, q0 = lane & ~3;
      const int mine = live ? base : -1;
      const int n0 = __shfl(mine, q0), n1 = __shfl(mine, q0 + 1), n2 = __shfl(mine, q0 + 2), n3 = __shfl(mine, q0 + 3);
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) {
        const int di = corner >> 2, dj = (corner >> 1) & 1, dk = corner & 1;
        const float om = ((di ? cell.tx : 1.f - cell.tx) * (dj ? cell.ty : 1.f - cell.ty)) * (dk ? cell.tz : 1.f - cell.tz);
        const float v0 = om * g.x, v1 = om * g.y, v2 = om * g.z, v3 = om * g.w;
        // a 4 x 4 transpose inside the quad.  A_j = v[(qc + j) & 3]; B_j = A_j of quad lane (qc - j) & 3 = that lane's v[qc];
        // the value of quad lane r for this lane's channel qc is B[(qc - r) & 3].
        const float A0 = sel4(qc, v0, v1, v2, v3), A1 = sel4(qc, v1, v2, v3, v0);
        const float A2 = sel4(qc, v2, v3, v0, v1), A3 = sel4(qc, v3, v0, v1, v2);
        const float B0 = A0, B1 = __shfl(A1, q0 + ((qc + 3) & 3)), B2 = __shfl(A2, q0 + ((qc + 2) & 3));
        const float B3 = __shfl(A3, q0 + ((qc + 1) & 3));
        const float t0 = sel4(qc, B0, B1, B2, B3), t1 = sel4(qc, B3, B0, B1, B2);
        const float t2 = sel4(qc, B2, B3, B0, B1), t3 = sel4(qc, B1, B2, B3, B0);
        const int off = di * sx + dj * sy + dk;
        if (n0 >= 0) atomicAdd(dvol + (size_t)(n0 + off) * 4 + qc, t0);
        if (n1 >= 0) atomicAdd(dvol + (size_t)(n1 + off) * 4 + qc, t1);
        if (n2 >= 0) atomicAdd(dvol + (size_t)(n2 + off) * 4 + qc, t2);
        if (n3 >= 0) atomicAdd(dvol + (size_t)(n3 + off) * 4 + qc, t3);
      }
    }
  }
}

// d v / d t_a (a = x, y, z) of vol_fetch's interpolant, from the same eight corners through the same addressing: the difference
// of the cell's two bilinear faces along axis a, which is exact for the trilinear rule.
struct VolSlope { f32x4 x, y, z; };

__device__ __forceinline__ VolSlope vol_fetch_slope(const VolArgs& a, const f32x4* vol, const VolCell& c) {
  const size_t sy = (size_t)a.nz, sx = (size_t)a.ny * a.nz;
  const f32x4* p = vol + ((size_t)c.i * a.ny + c.j) * a.nz + c.k;
  const f32x4 c000 = p[0], c001 = p[1], c010 = p[sy], c011 = p[sy + 1];
  const f32x4 c100 = p[sx], c101 = p[sx + 1], c110 = p[sx + sy], c111 = p[sx + sy + 1];
  const f32x4 c00 = vol_lerp(c000, c001, c.tz), c01 = vol_lerp(c010, c011, c.tz);
  const f32x4 c10 = vol_lerp(c100, c101, c.tz), c11 = vol_lerp(c110, c111, c.tz);
  VolSlope g;
  g.x = vol_lerp(c10, c11, c.ty) - vol_lerp(c00, c01, c.ty);
  g.y = vol_lerp(c01 - c00, c11 - c10, c.tx);
  g.z = vol_lerp(vol_lerp(c001 - c000, c011 - c010, c.ty), vol_lerp(c101 - c100, c111 - c110, c.ty), c.tx);
  return g;
}

struct VolCamArgs {
  VolArgs f;                              // the forward's arguments (its three outputs unused)
  const float *drgb, *ddepth, *dopacity;  // the last two may be NULL (zeros)
  float* dcam;                            // (b,4,4), fully written by volume_cam_finish_kernel
  f32x4* rec;                             // S * threads records (alpha, fp32(T), s, x), sample-major
  float* part;                            // b * tiles * 12 floats: one 3 x 4 block per tile, behind the records
  size_t threads;                         // grid * 256
};

// The backward of volume_render_kernel with respect to cam2world.  The march and the reverse scan are volume_render_bwd_kernel's,
// expression by expression; where that kernel scatters omega (w G, dx) into eight nodes, this one gathers the eight nodes again
// (live samples only) and forms dp = w (G . grad c) + dx grad sigma, then A = sum dp and B = sum z dp per ray.  With
// world = R (dir z) + t:  d R[a][c] = B_a dir_c,  d t_a = A_a.  The wave adds its 64 rays' twelve products by a butterfly of
// shuffles (a fixed order) and lane 0 stores them: no atomics, the same bits on every call.  Lanes off the image stay for the
// shuffles with zeros.
__global__ __launch_bounds__(256) void volume_render_bwd_cam_kernel(VolCamArgs q) {
  const VolArgs& a = q.f;
  const int img = blockIdx.x / a.blocks_per_image;
  const int tile = (blockIdx.x - img * a.blocks_per_image) * 4 + (threadIdx.x >> 6);
  if (tile >= a.tiles) return;            // the whole wave
  const int lane = threadIdx.x & 63;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int r = ty * 8 + (lane >> 3), c = tx * 8 + (lane & 7);
  const bool on = r < a.H && c < a.W;
  const int ray = on ? r * a.W + c : 0, S = a.S;
  const RayDir dir = ray_dir(a.g, ray);
  float Ax = 0.f, Ay = 0.f, Az = 0.f, Bx = 0.f, By = 0.f, Bz = 0.f;
  if (on) {
    const bool skip = (a.flags & 4) && a.clamp_mode == 0;
    const bool last_back = a.flags & 1;
    const float* occ = skip ? a.occ + (a.Bv == 1 ? 0 : (size_t)img * a.bricks) : nullptr;
    f32x4* rec = q.rec + ((size_t)blockIdx.x * 256 + threadIdx.x);
    const float* M = a.g.c2w + (size_t)img * 16;
    const f32x4* vol = a.vol + (a.Bv == 1 ? 0 : (size_t)img * a.nodes);
    const size_t plane = (size_t)a.H * a.W, pix = (size_t)img * plane + ray;
    const float* gp = q.drgb + (size_t)img * 3 * plane + ray;
    const float Gr = gp[0], Gg = gp[plane], Gb = gp[2 * plane];
    const float gd = q.ddepth ? q.ddepth[pix] : 0.f;
    const float go = q.dopacity ? q.dopacity[pix] : 0.f;
    double T = 1.0;
    float wsum = 0.f, slast = 0.f;
    for (int s = 0; s < S; ++s) {         // the forward's march, expression by expression
      float wx, wy, wz, z;
      ray_point(a.g, M, dir, a.g.zg[s], 0.f, false, wx, wy, wz, z);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      VolCell cell;
      if (vol_sample_cell(a, occ, last_back, s, wx, wy, wz, cell)) v = vol_fetch(a, vol, cell);
      const float delta = (s + 1 < S) ? (a.g.zg[s + 1] - z) : 1e10f;
      const float alpha = 1.f - expf(-delta * vol_clamp(v.w, a.clamp_mode));
      const float Tf = (float)T;
      wsum += alpha * Tf;
      T *= (double)(1.f - alpha + 1e-10f);
      slast = fmaf(gd, z, Gr * v.x + Gg * v.y + Gb * v.z);
      const f32x4 rc = {alpha, Tf, slast, v.w};
      rec[(size_t)s * q.threads] = rc;
    }
    const float s_off = (last_back ? slast : 0.f) + ((a.flags & 2) ? (Gr + Gg + Gb) : 0.f) - go;

    float Q = 0.f;
    for (int k = S - 1; k >= 0; --k) {
      float wx, wy, wz, z;
      ray_point(a.g, M, dir, a.g.zg[k], 0.f, false, wx, wy, wz, z);
      VolCell cell;
      const bool fetched = vol_sample_cell(a, occ, last_back, k, wx, wy, wz, cell);
      const f32x4 rc = rec[(size_t)k * q.threads];
      const float alpha = rc.x, Tk = rc.y, s = rc.z - s_off, x = rc.w;
      float w = alpha * Tk;
      if (last_back && k == S - 1) w += 1.f - wsum;           // the colour of the last sample sees the topped-up weight
      const float dalpha = Tk * (s - Q);
      Q = fmaf(alpha, s, (1.f - alpha + 1e-10f) * Q);
      const float delta = (k + 1 < S) ? (a.g.zg[k + 1] - z) : 1e10f;
      const float dx = dalpha * (delta * expf(-delta * vol_clamp(x, a.clamp_mode))) * vol_clamp_grad(x, a.clamp_mode);
      // live: volume_render_bwd_kernel's rule.  A skipped sample and a fetched one that is not live add nothing either way.
      if (!(fetched && ((w != 0.f) || (dx != 0.f)))) continue;
      const VolSlope g = vol_fetch_slope(a, vol, cell);
      const float px = a.inv_h[0] * fmaf(dx, g.x.w, w * (Gr * g.x.x + Gg * g.x.y + Gb * g.x.z));
      const float py = a.inv_h[1] * fmaf(dx, g.y.w, w * (Gr * g.y.x + Gg * g.y.y + Gb * g.y.z));
      const float pz = a.inv_h[2] * fmaf(dx, g.z.w, w * (Gr * g.z.x + Gg * g.z.y + Gb * g.z.z));
      Ax += px; Ay += py; Az += pz;
      Bx = fmaf(z, px, Bx); By = fmaf(z, py, By); Bz = fmaf(z, pz, Bz);
    }
  }
  // rows a = x, y, z of d cam2world: (B_a dir_x, B_a dir_y, B_a dir_z, A_a)
  float m[12] = {Bx * dir.dx, Bx * dir.dy, Bx * dir.dz, Ax, By * dir.dx, By * dir.dy, By * dir.dz, Ay,
                 Bz * dir.dx, Bz * dir.dy, Bz * dir.dz, Az};
#pragma unroll
  for (int j = 0; j < 12; ++j) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m[j] += __shfl_xor(m[j], off, 64);
  }
  if (lane == 0) {
    float* o = q.part + ((size_t)img * a.tiles + tile) * 12;
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = m[j];
  }
}

// One block of 12 waves per image: wave j adds entry j of the image's tiles, lane l the tiles l, l + 64, ... in order, then the
// same butterfly.  Writes the image's whole 4 x 4 matrix, row 3 as zeros.
__global__ __launch_bounds__(768) void volume_cam_finish_kernel(const float* part, float* dcam, int tiles) {
  const int img = blockIdx.x, j = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* p = part + (size_t)img * tiles * 12 + j;
  float acc = 0.f;
  for (int t = lane; t < tiles; t += 64) acc += p[(size_t)t * 12];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) dcam[(size_t)img * 16 + j] = acc;
  if (j == 0 && lane < 4) dcam[(size_t)img * 16 + 12 + lane] = 0.f;
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
  a.sigma = sigma; a.rgb = rgb; a.packed = (f32x4*)packed; a.occ = occ; a.stride = 1;
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

namespace {

// The checks and the launch geometry that cips_volume_render and cips_volume_render_bwd share (everything but their own
// pointers): hipErrorInvalidValue, or 0 with `a` filled.  Host arithmetic only.
int vol_render_args(VolArgs& a, const void* packed, const float* occ, const float* lo, const float* hi, const float* xg,
                    const float* yg, const float* zg, const float* cam2world, float zc, int clamp_mode, int flags, int b, int Bv,
                    int nx, int ny, int nz, int H, int W, int S) {
  if (b < 0 || Bv < 0 || !lattice_ok(nx, ny, nz) || H < 2 || W < 2 || S < 2) return (int)hipErrorInvalidValue;
  if (Bv != 1 && Bv != b) return (int)hipErrorInvalidValue;
  if ((long long)b * H * W > 0x7fffffffLL || (long long)H * W * S > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (clamp_mode != 0 && clamp_mode != 1) return (int)hipErrorInvalidValue;
  if (!packed || !lo || !hi || !xg || !yg || !zg || !cam2world) return (int)hipErrorInvalidValue;
  if ((flags & 4) && !occ) return (int)hipErrorInvalidValue;
  if ((uintptr_t)packed & 15) return (int)hipErrorInvalidValue;
  if (std::isnan(zc) || std::isinf(zc) || !(zc < 0.f)) return (int)hipErrorInvalidValue;
  const int n[3] = {nx, ny, nz};
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !(hi[k] > lo[k])) return (int)hipErrorInvalidValue;
    a.lo[k] = lo[k];
    a.umax[k] = (float)(n[k] - 1);
    a.inv_h[k] = a.umax[k] / (hi[k] - lo[k]);
    if (!std::isfinite(a.inv_h[k]) || !(a.inv_h[k] > 0.f)) return (int)hipErrorInvalidValue;
  }
  a.vol = (const f32x4*)packed; a.occ = occ;
  a.g.xg = xg; a.g.yg = yg; a.g.zg = zg; a.g.c2w = cam2world; a.g.jitter = nullptr; a.g.zvals = nullptr; a.g.zc = zc;
  a.g.W = W; a.g.n = W * H; a.g.S = S;
  a.b = b; a.Bv = Bv; a.nx = nx; a.ny = ny; a.nz = nz; a.by = bricks_of(ny); a.bz = bricks_of(nz);
  a.H = H; a.W = W; a.S = S; a.clamp_mode = clamp_mode; a.flags = flags & 7;
  a.nodes = (long long)nx * ny * nz; a.bricks = (long long)bricks_of(nx) * a.by * a.bz;
  a.tiles_x = (W + 7) >> 3;
  a.tiles = a.tiles_x * ((H + 7) >> 3);                  // <= H * W
  a.blocks_per_image = (a.tiles + 3) >> 2;               // grid = b * blocks_per_image <= b * H * W
  return 0;
}

}  // namespace

extern "C" int cips_volume_render(const void* packed, const float* occ, const float* lo, const float* hi, const float* xg,
                                  const float* yg, const float* zg, const float* cam2world, float zc, int clamp_mode, int flags,
                                  float* rgb, float* depth, float* opacity, int b, int Bv, int nx, int ny, int nz, int H, int W,
                                  int S, cips_stream_t stream) {
  if (flags < 0 || flags > 7 || !rgb || !depth || !opacity) return (int)hipErrorInvalidValue;
  VolArgs a = {};
  const int bad = vol_render_args(a, packed, occ, lo, hi, xg, yg, zg, cam2world, zc, clamp_mode, flags, b, Bv, nx, ny, nz, H, W, S);
  if (bad) return bad;
  if (b == 0) return 0;
  a.rgb = rgb; a.depth = depth; a.opacity = opacity;
  const long long grid = (long long)b * a.blocks_per_image;
  hipLaunchKernelGGL(volume_render_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
  return CIPS_CHECK_LAUNCH();
}

extern "C" long long cips_volume_render_bwd_scratch(int b, int H, int W, int S) {
  if (b < 0 || H < 2 || W < 2 || S < 2) return -1;
  if ((long long)b * H * W > 0x7fffffffLL || (long long)H * W * S > 0x7fffffffLL) return -1;
  const long long tiles = (long long)((W + 7) >> 3) * ((H + 7) >> 3);
  return (long long)S * (b * ((tiles + 3) >> 2) * 256) * 16;
}

extern "C" int cips_volume_render_bwd(const void* packed, const float* occ, const float* lo, const float* hi, const float* xg,
                                      const float* yg, const float* zg, const float* cam2world, float zc, int clamp_mode,
                                      int flags, const float* drgb, const float* ddepth, const float* dopacity, void* dpacked,
                                      void* scratch, int b, int Bv, int nx, int ny, int nz, int H, int W, int S,
                                      cips_stream_t stream) {
  if (flags < 0 || flags > 15 || !drgb || !dpacked || !scratch) return (int)hipErrorInvalidValue;
  if (((uintptr_t)dpacked & 15) || ((uintptr_t)scratch & 15)) return (int)hipErrorInvalidValue;
  VolBwdArgs q = {};
  const int bad = vol_render_args(q.f, packed, occ, lo, hi, xg, yg, zg, cam2world, zc, clamp_mode, flags, b, Bv, nx, ny, nz, H, W,
                                  S);
  if (bad) return bad;
  if (Bv == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(dpacked, 0, (size_t)Bv * q.f.nodes * 16, st);
  if (e != hipSuccess) return (int)e;
  if (b == 0) return 0;
  q.drgb = drgb; q.ddepth = ddepth; q.dopacity = dopacity; q.dpacked = (float*)dpacked; q.rec = (f32x4*)scratch;
  const long long grid = (long long)b * q.f.blocks_per_image;
  q.threads = (size_t)grid * 256;
  if (flags & 8)
    hipLaunchKernelGGL(volume_render_bwd_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, q);
  else
    hipLaunchKernelGGL(volume_render_bwd_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, q);
  return CIPS_CHECK_LAUNCH();
}

extern "C" long long cips_volume_render_bwd_cam_scratch(int b, int H, int W, int S) {
  if (b < 0 || H < 2 || W < 2 || S < 2) return -1;
  if ((long long)b * H * W > 0x7fffffffLL || (long long)H * W * S > 0x7fffffffLL) return -1;
  const long long tiles = (long long)((W + 7) >> 3) * ((H + 7) >> 3);           // <= H * W
  const long long threads = b * ((tiles + 3) >> 2) * 256;                        // <= 256 b H W < 2^39
  const long long part = b * tiles * 48;                                         // < 2^37
  if (threads > (0x7fffffffffffffffLL - part) / 16 / S) return -1;               // S * threads * 16 + part would overflow
  return (long long)S * threads * 16 + part;
}

extern "C" int cips_volume_render_bwd_cam(const void* packed, const float* occ, const float* lo, const float* hi, const float* xg,
                                          const float* yg, const float* zg, const float* cam2world, float zc, int clamp_mode,
                                          int flags, const float* drgb, const float* ddepth, const float* dopacity,
                                          float* dcam2world, void* scratch, int b, int Bv, int nx, int ny, int nz, int H, int W,
                                          int S, cips_stream_t stream) {
  if (flags < 0 || flags > 7 || !drgb || !dcam2world || !scratch) return (int)hipErrorInvalidValue;
  if ((uintptr_t)scratch & 15) return (int)hipErrorInvalidValue;
  VolCamArgs q = {};
  const int bad = vol_render_args(q.f, packed, occ, lo, hi, xg, yg, zg, cam2world, zc, clamp_mode, flags, b, Bv, nx, ny, nz, H, W,
                                  S);
  if (bad) return bad;
  if (cips_volume_render_bwd_cam_scratch(b, H, W, S) < 0) return (int)hipErrorInvalidValue;
  if (b == 0) return 0;
  const long long grid = (long long)b * q.f.blocks_per_image;
  q.threads = (size_t)grid * 256;
  q.drgb = drgb; q.ddepth = ddepth; q.dopacity = dopacity; q.dcam = dcam2world;
  q.rec = (f32x4*)scratch; q.part = (float*)(q.rec + (size_t)S * q.threads);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(volume_render_bwd_cam_kernel, dim3((unsigned)grid), dim3(256), 0, st, q);
  hipLaunchKernelGGL(volume_cam_finish_kernel, dim3((unsigned)b), dim3(768), 0, st, (const float*)q.part, dcam2world, q.f.tiles);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_volume_occupancy(const void* packed, float* occ, int Bv, int nx, int ny, int nz, cips_stream_t stream) {
  if (Bv < 0 || !lattice_ok(nx, ny, nz)) return (int)hipErrorInvalidValue;
  if (!packed || !occ) return (int)hipErrorInvalidValue;
  if ((uintptr_t)packed & 15) return (int)hipErrorInvalidValue;
  PackArgs a = {};
  a.sigma = (const float*)packed + 3; a.occ = occ; a.stride = 4;
  a.Bv = Bv; a.nx = nx; a.ny = ny; a.nz = nz; a.bx = bricks_of(nx); a.by = bricks_of(ny); a.bz = bricks_of(nz);
  const long long occ_blocks = (long long)Bv * a.bx * a.by * a.bz;
  if (occ_blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (Bv == 0) return 0;
  hipLaunchKernelGGL(volume_occ_kernel, dim3((unsigned)occ_blocks), dim3(64), 0, (hipStream_t)stream, a);
  return CIPS_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// Baked FEATURE volumes: the 32 colour features of the SIREN on the lattice instead of a colour, composited per ray into the
// (b, H W, 32) rows the INR head takes.  The rule is cips_volume_render's with 32 channels in place of 3 (include/cips3d_hip.h,
// cips_feature_volume_render); everything a sample's place and weight depend on runs through the helpers above.
//
//   feature_pack_kernel    one thread per node and channel group: 16 bytes of a (node, 32) row leave as one record of the
//                          group's plane (bits copied).  Reads are contiguous; a wave's writes are 8 runs of 128 bytes.
//   feature_render_kernel  volume_render_kernel's lane and tile mapping.  Per sample: the eight 4-byte sigma nodes, seven lerps,
//                          the composite step; only a sample whose weight is not zero gathers its eight groups (8 x vol_fetch:
//                          64 16-byte loads) and adds them into 32 accumulators.  No LDS, no scratch, no atomics.
namespace {

struct FeatPackArgs {
  const f32x4* rows; f32x4* planes;
  long long total;                       // Bv * sx * ny * nz * 8 records
  long long slab, nodes;                 // sx * ny * nz and nx * ny * nz
  long long first;                       // x0 * ny * nz: the slab's first node
};

__global__ __launch_bounds__(256) void feature_pack_kernel(FeatPackArgs a) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= a.total) return;
  const long long node = id >> 3, v = node / a.slab, n = node - v * a.slab;
  const int g = (int)(id & 7);
  a.planes[(v * 8 + g) * a.nodes + a.first + n] = a.rows[id];
}

struct FeatArgs {
  VolArgs f;                             // vol = planes; its rgb pointer is unused
  const float* sigma;
  f32x4* fea;
};

__device__ __forceinline__ float lerp1(float p, float q, float t) { return p + t * (q - p); }

// vol_fetch for the one channel of a plain (nx, ny, nz) tensor: the same corners in the same order
__device__ __forceinline__ float sigma_fetch(const VolArgs& a, const float* sig, const VolCell& c) {
  const size_t sy = (size_t)a.nz, sx = (size_t)a.ny * a.nz;
  const float* p = sig + ((size_t)c.i * a.ny + c.j) * a.nz + c.k;
  const float c000 = p[0], c001 = p[1], c010 = p[sy], c011 = p[sy + 1];
  const float c100 = p[sx], c101 = p[sx + 1], c110 = p[sx + sy], c111 = p[sx + sy + 1];
  const float c00 = lerp1(c000, c001, c.tz), c01 = lerp1(c010, c011, c.tz);
  const float c10 = lerp1(c100, c101, c.tz), c11 = lerp1(c110, c111, c.tz);
  return lerp1(lerp1(c00, c01, c.ty), lerp1(c10, c11, c.ty), c.tx);
}

__device__ __forceinline__ f32x4 fma4(float w, f32x4 v, f32x4 c) {
  f32x4 r;
  r.x = fmaf(w, v.x, c.x); r.y = fmaf(w, v.y, c.y); r.z = fmaf(w, v.z, c.z); r.w = fmaf(w, v.w, c.w);
  return r;
}

__global__ __launch_bounds__(256) void feature_render_kernel(FeatArgs q) {
  const VolArgs& a = q.f;
  const int img = blockIdx.x / a.blocks_per_image;
  const int tile = (blockIdx.x - img * a.blocks_per_image) * 4 + (threadIdx.x >> 6);
  if (tile >= a.tiles) return;
  const int lane = threadIdx.x & 63;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int r = ty * 8 + (lane >> 3), c = tx * 8 + (lane & 7);
  if (r >= a.H || c >= a.W) return;
  const int ray = r * a.W + c, S = a.S;
  const f32x4* planes = a.vol + (a.Bv == 1 ? 0 : (size_t)img * 8 * a.nodes);
  const float* sig = q.sigma + (a.Bv == 1 ? 0 : (size_t)img * a.nodes);
  const bool skip = (a.flags & 4) && a.clamp_mode == 0;
  const bool last_back = a.flags & 1;
  const float* occ = skip ? a.occ + (a.Bv == 1 ? 0 : (size_t)img * a.bricks) : nullptr;

  f32x4 acc[8];
#pragma unroll
  for (int g = 0; g < 8; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  float depth = 0.f, wsum = 0.f, zlast = 0.f, wlast = 0.f;
  bool last_in = false;                   // under last_back: the last sample lies inside, its features take the top-up
  VolCell clast = {0, 0, 0, 0.f, 0.f, 0.f};
  double T = 1.0;
  const RayDir dir = ray_dir(a.g, ray);
  const float* M = a.g.c2w + (size_t)img * 16;
  for (int s = 0; s < S; ++s) {           // volume_render_kernel's march, expression by expression
    float wx, wy, wz, z;
    ray_point(a.g, M, dir, a.g.zg[s], 0.f, false, wx, wy, wz, z);
    float x = 0.f;
    VolCell cell;
    const bool fetched = vol_sample_cell(a, occ, last_back, s, wx, wy, wz, cell);
    if (fetched) x = sigma_fetch(a, sig, cell);
    const float delta = (s + 1 < S) ? (a.g.zg[s + 1] - z) : 1e10f;
    const float alpha = 1.f - expf(-delta * vol_clamp(x, a.clamp_mode));
    const float Tf = (float)T;
    const float w = alpha * Tf;
    T *= (double)(1.f - alpha + 1e-10f);
    depth = fmaf(w, z, depth);
    // opacity takes alpha T through one fused multiply-add, which is what volume_render_kernel's `wsum += w` compiles to (the
    // product is contracted into the sum): written out here so that the two kernels agree bit for bit whatever the compiler does
    // with this one; tests/test_gpu_feature_volume.py holds them to each other
    wsum = fmaf(alpha, Tf, wsum);
    zlast = z;
    if (last_back && s == S - 1) {        // resolved behind the loop, where 1 - sum w is known
      last_in = fetched; wlast = w; clast = cell;
    } else if (fetched && w != 0.f) {     // fmaf(0, f, c) == c for finite f: a zero weight needs no features
#pragma unroll
      for (int g = 0; g < 8; ++g) acc[g] = fma4(w, vol_fetch(a, planes + (size_t)g * a.nodes, cell), acc[g]);
    }
  }
  const float extra = 1.f - wsum;
  if (last_back) {                        // the last weight gains 1 - sum w: two fmafs per channel, as volume_render_kernel
    if (last_in && (wlast != 0.f || extra != 0.f)) {
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const f32x4 v = vol_fetch(a, planes + (size_t)g * a.nodes, clast);
        acc[g] = fma4(extra, v, fma4(wlast, v, acc[g]));
      }
    }
    depth = fmaf(extra, zlast, depth);
  }
  if (a.flags & 2) {                      // white_back, every channel
#pragma unroll
    for (int g = 0; g < 8; ++g) acc[g] += extra;
  }
  const size_t pix = (size_t)img * a.H * a.W + ray;
  f32x4* o = q.fea + pix * 8;             // the lane's 128 contiguous bytes
#pragma unroll
  for (int g = 0; g < 8; ++g) o[g] = acc[g];
  a.depth[pix] = depth;
  a.opacity[pix] = wsum;
}

}  // namespace

extern "C" int cips_feature_volume_bake_slab(const float* sigma, const float* feat_rows, void* planes, float* occ, int Bv, int nx,
                                             int ny, int nz, int x0, int sx, cips_stream_t stream) {
  if (Bv < 0 || !lattice_ok(nx, ny, nz)) return (int)hipErrorInvalidValue;
  if (x0 < 0 || sx < 1 || x0 > nx - sx) return (int)hipErrorInvalidValue;
  if (!sigma || !feat_rows || !planes || !occ) return (int)hipErrorInvalidValue;
  if (((uintptr_t)planes & 15) || ((uintptr_t)feat_rows & 15)) return (int)hipErrorInvalidValue;
  FeatPackArgs p = {};
  p.rows = (const f32x4*)feat_rows; p.planes = (f32x4*)planes;
  p.slab = (long long)sx * ny * nz; p.nodes = (long long)nx * ny * nz; p.first = (long long)x0 * ny * nz;
  if (Bv > 0 && p.slab > 0x7fffffffLL * 32 / Bv) return (int)hipErrorInvalidValue;            // the pack grid, beyond int32
  p.total = (long long)Bv * p.slab * 8;
  PackArgs a = {};
  a.sigma = sigma; a.occ = occ; a.stride = 1;
  a.Bv = Bv; a.nx = nx; a.ny = ny; a.nz = nz; a.bx = bricks_of(nx); a.by = bricks_of(ny); a.bz = bricks_of(nz);
  const long long pack_blocks = (p.total + 255) / 256, occ_blocks = (long long)Bv * a.bx * a.by * a.bz;
  if (pack_blocks > 0x7fffffffLL || occ_blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (Bv == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(feature_pack_kernel, dim3((unsigned)pack_blocks), dim3(256), 0, st, p);
  if (x0 + sx == nx) hipLaunchKernelGGL(volume_occ_kernel, dim3((unsigned)occ_blocks), dim3(64), 0, st, a);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_feature_volume_bake(const float* sigma, const float* feat_rows, void* planes, float* occ, int Bv, int nx,
                                        int ny, int nz, cips_stream_t stream) {
  return cips_feature_volume_bake_slab(sigma, feat_rows, planes, occ, Bv, nx, ny, nz, 0, nx, stream);
}

extern "C" int cips_feature_volume_render(const float* sigma, const void* planes, const float* occ, const float* lo, const float* hi,
                                          const float* xg, const float* yg, const float* zg, const float* cam2world, float zc,
                                          int clamp_mode, int flags, float* fea, float* depth, float* opacity, int b, int Bv, int nx,
                                          int ny, int nz, int H, int W, int S, cips_stream_t stream) {
  if (flags < 0 || flags > 7 || !sigma || !fea || !depth || !opacity) return (int)hipErrorInvalidValue;
  if ((uintptr_t)fea & 15) return (int)hipErrorInvalidValue;
  FeatArgs q = {};
  const int bad = vol_render_args(q.f, planes, occ, lo, hi, xg, yg, zg, cam2world, zc, clamp_mode, flags, b, Bv, nx, ny, nz, H, W, S);
  if (bad) return bad;
  if (b == 0) return 0;
  q.sigma = sigma; q.fea = (f32x4*)fea; q.f.depth = depth; q.f.opacity = opacity;
  const long long grid = (long long)b * q.f.blocks_per_image;
  hipLaunchKernelGGL(feature_render_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, q);
  return CIPS_CHECK_LAUNCH();
}
