// raster.hip — a forward-only rasteriser for indexed triangle meshes in the camera of raygen.h, for gfx950: which triangle does
// the ray of pixel (r, c) hit first, and at what distance along the unit ray direction.  The rule, decision by decision, is in
// include/cips3d_hip.h (cips_raster_fwd).  No network in it: a mesh of GeneratorNerfINR.extract_mesh is view-independent, a view
// of it is one pass over T triangles and H * W pixels.
//
//   launch 1  raster_vertex_kernel   one thread per (camera b, vertex i): q = R v + t, the screen position (u, v), q.z and the
//                                    validity flag leave as ONE 16-byte record.  A vertex shared by several triangles has one set
//                                    of bits, whoever reads it.
//   launch 2  raster_face_kernel     one lane per (camera, triangle): set-up, the bounding box clamped to the frame, a walk over
//                                    the box (at most BIG_BOX pixels) with a 64-bit atomicMin of  depth bits << 32 | face  into
//                                    the key buffer.  A mesh at N = 256 is 10^5..10^6 triangles of one to a few pixels: most
//                                    lanes test one to four centres.  A triangle whose box holds more than BIG_BOX pixels is
//                                    appended to the large-triangle list (one 32-bit atomicAdd) and not walked here.
//   launch 3  raster_big_kernel      blockIdx.x strides the list, blockIdx.y * 256 + thread strides the box of an entry: a
//                                    triangle that covers the frame is shared by gridDim.y workgroups.  The list's order varies
//                                    from call to call; the keys do not care.
//   launch 4  raster_resolve_kernel  one thread per pixel: the key's face, its barycentrics recomputed with the set-up of launch
//                                    2 (the same device function: the same bits), face / bary / depth / mask.
//             raster_interp_kernel   one thread per pixel, a loop over the channels of a per-vertex attribute.
//
// Both paths that test coverage call the same two functions (tri_setup, fragment) compiled with contraction off: an edge value
// is the same bits in the lane path, the workgroup path and the resolve, and for the two triangles that share the edge (it is
// evaluated from the lower vertex index to the higher, and negated — exactly — for the triangle that runs the other way).
// Every float -> int conversion follows a clamp in float and every loop bound is built from clamped values.
#include <cmath>
#include "common.h"
#include "../../include/cips3d_hip.h"

namespace {

constexpr int BIG_BOX = 256;             // pixels in a clamped bounding box above which a triangle goes to the list (16 x 16)
constexpr int BIG_GRID_X = 1024;         // launch 3: workgroups that stride the list ...
constexpr int BIG_GRID_Y = 16;           // ... times workgroups that share one entry's box
constexpr unsigned long long NO_KEY = ~0ull;

struct RasterArgs {
  const float* vertices; const int* faces; const float* world2cam; const float* xg; const float* yg;
  f32x4* screen; unsigned long long* keys; int* big_list; int* big_count;
  int* face_out; float* bary; float* depth; unsigned char* mask;
  float zc, near_, far_;
  int cull, B, V, T, H, W;
  long long big_cap;
};

__global__ __launch_bounds__(256) void raster_vertex_kernel(RasterArgs a) {
#pragma clang fp contract(off)
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)a.B * a.V) return;
  const int b = (int)(id / a.V), i = (int)(id - (long long)b * a.V);
  const float* M = a.world2cam + (size_t)b * 12;
  const float x = a.vertices[(size_t)i * 3], y = a.vertices[(size_t)i * 3 + 1], z = a.vertices[(size_t)i * 3 + 2];
  // four roundings per component: one product, two fused steps, the translation
  const float qx = __builtin_fmaf(M[2], z, __builtin_fmaf(M[1], y, M[0] * x)) + M[3];
  const float qy = __builtin_fmaf(M[6], z, __builtin_fmaf(M[5], y, M[4] * x)) + M[7];
  const float qz = __builtin_fmaf(M[10], z, __builtin_fmaf(M[9], y, M[8] * x)) + M[11];
  const bool finite = fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY;      // false for a NaN
  const bool valid = finite && (-qz >= a.near_);
  f32x4 s;
  s.x = ((qx * a.zc) / qz + 1.f) * ((float)(a.W - 1) * 0.5f);
  s.y = (1.f - (qy * a.zc) / qz) * ((float)(a.H - 1) * 0.5f);
  s.z = qz;
  s.w = valid ? 1.f : 0.f;
  a.screen[id] = s;
}

// edge {lo, hi} at the point (px, py), lower vertex index first: ONE fp32 expression, seven roundings
__device__ __forceinline__ float edge_value(float ulo, float vlo, float uhi, float vhi, float px, float py) {
#pragma clang fp contract(off)
  return (uhi - ulo) * (py - vlo) - (vhi - vlo) * (px - ulo);
}

// a triangle that survived the drop rules: edge i is the one opposite vertex i, stored from its lower vertex index to the
// higher with the sign sg[i] that turns it back into the triangle's own direction
struct Tri {
  float ul[3], vl[3], uh[3], vh[3], sg[3], z[3];
  float s;                     // the orientation sign: the sign every edge value of a covered pixel has (or zero)
  int x0, x1, y0, y1;          // the bounding box clamped to the frame, inclusive
};

__device__ __forceinline__ float tri_edge(const Tri& t, int i, float px, float py) {
  return t.sg[i] * edge_value(t.ul[i], t.vl[i], t.uh[i], t.vh[i], px, py);
}

// false: the triangle is dropped whole (an index outside [0, V), an invalid vertex, a zero or non-finite screen area, culled,
// or a box that misses the frame)
__device__ __forceinline__ bool tri_setup(const RasterArgs& a, int b, int f, Tri& t) {
  int idx[3];
  float su[3], sv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    idx[i] = a.faces[(size_t)f * 3 + i];
    if ((unsigned)idx[i] >= (unsigned)a.V) return false;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const f32x4 s = a.screen[(size_t)b * a.V + idx[i]];
    if (s.w == 0.f) return false;
    su[i] = s.x; sv[i] = s.y; t.z[i] = s.z;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    const bool fwd = idx[j] < idx[k];                        // the triangle runs j -> k
    t.ul[i] = fwd ? su[j] : su[k]; t.vl[i] = fwd ? sv[j] : sv[k];
    t.uh[i] = fwd ? su[k] : su[j]; t.vh[i] = fwd ? sv[k] : sv[j];
    t.sg[i] = fwd ? 1.f : -1.f;
  }
  // twice the screen area, signed: edge 0 at vertex 0.  v runs downwards, so a triangle whose geometric normal points towards
  // the camera (counter-clockwise in camera x, y) has a NEGATIVE area here.
  const float area = tri_edge(t, 0, su[0], sv[0]);
  if (!(fabsf(area) > 0.f) || !(fabsf(area) < INFINITY)) return false;                 // zero, NaN, infinite
  if (a.cull && area > 0.f) return false;
  t.s = area < 0.f ? -1.f : 1.f;
  // the area is finite, so every u, v is: the clamps below see no NaN, and would map one into the frame if they did
  const float umin = fminf(su[0], fminf(su[1], su[2])), umax = fmaxf(su[0], fmaxf(su[1], su[2]));
  const float vmin = fminf(sv[0], fminf(sv[1], sv[2])), vmax = fmaxf(sv[0], fmaxf(sv[1], sv[2]));
  const float fx0 = fmaxf(ceilf(umin), 0.f), fx1 = fminf(floorf(umax), (float)(a.W - 1));
  const float fy0 = fmaxf(ceilf(vmin), 0.f), fy1 = fminf(floorf(vmax), (float)(a.H - 1));
  if (!(fx0 <= fx1) || !(fy0 <= fy1)) return false;
  // in [0, W-1] and [0, H-1] as floats; the integer clamp covers a W - 1 that fp32 rounds up
  t.x0 = min((int)fx0, a.W - 1); t.x1 = min((int)fx1, a.W - 1);
  t.y0 = min((int)fy0, a.H - 1); t.y1 = min((int)fy1, a.H - 1);
  return true;
}

// pixel (r, c) against a triangle: covered iff every edge value has the orientation sign or is zero.  Then 1/z is interpolated
// in screen space: with E_i the edge values (the area cancels), w_i = E_i / z_i, z = sum E / sum w, lambda_i = w_i / sum w and
// depth = (z / zc) |(xg[c], yg[r], zc)|, the distance along the unit ray.
__device__ __forceinline__ bool fragment(const RasterArgs& a, const Tri& t, int r, int c, float& depth, float lam[3]) {
#pragma clang fp contract(off)
  const float px = (float)c, py = (float)r;
  const float e0 = tri_edge(t, 0, px, py), e1 = tri_edge(t, 1, px, py), e2 = tri_edge(t, 2, px, py);
  if (!(t.s * e0 >= 0.f) || !(t.s * e1 >= 0.f) || !(t.s * e2 >= 0.f)) return false;        // a NaN covers nothing
  const float w0 = e0 / t.z[0], w1 = e1 / t.z[1], w2 = e2 / t.z[2];
  const float den = (w0 + w1) + w2, num = (e0 + e1) + e2;
  const float z = num / den;
  const float x = a.xg[c], y = a.yg[r];
  depth = (z / a.zc) * sqrtf((x * x + y * y) + a.zc * a.zc);
  if (!(depth > 0.f) || !(depth < INFINITY)) return false;                                  // positive: its bits are monotonic
  lam[0] = w0 / den; lam[1] = w1 / den; lam[2] = w2 / den;
  return true;
}

__device__ __forceinline__ void emit(const RasterArgs& a, const Tri& t, int b, int f, int r, int c) {
  float depth, lam[3];
  if (!fragment(a, t, r, c, depth, lam)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned)f;
  unsigned long long* slot = a.keys + ((size_t)b * a.H + r) * a.W + c;
  if (key < *slot) atomicMin(slot, key);             // the plain load skips occluded fragments; a stale value only costs an atomic
}

__global__ __launch_bounds__(256) void raster_face_kernel(RasterArgs a) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= (long long)a.B * a.T) return;
  const int b = (int)(id / a.T), f = (int)(id - (long long)b * a.T);
  Tri t;
  if (!tri_setup(a, b, f, t)) return;
  const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
  if ((long long)bw * bh > BIG_BOX) {
    const int at = atomicAdd(a.big_count, 1);
    if (at >= 0 && at < a.big_cap) a.big_list[at] = (int)id;            // one entry per (camera, triangle): B * T entries fit
    return;
  }
  for (int r = t.y0; r <= t.y1; ++r)
    for (int c = t.x0; c <= t.x1; ++c) emit(a, t, b, f, r, c);
}

__global__ __launch_bounds__(256) void raster_big_kernel(RasterArgs a) {
  const int count = (int)min((long long)max(*a.big_count, 0), a.big_cap);
  for (int e = blockIdx.x; e < count; e += gridDim.x) {
    const int id = a.big_list[e];
    if (id < 0 || (long long)id >= (long long)a.B * a.T) continue;
    const int b = id / a.T, f = id - b * a.T;
    Tri t;
    if (!tri_setup(a, b, f, t)) continue;
    const int bw = t.x1 - t.x0 + 1;
    const long long n = (long long)bw * (t.y1 - t.y0 + 1);            // at most H * W < 2^31
    for (long long k = (long long)blockIdx.y * 256 + threadIdx.x; k < n; k += 256ll * gridDim.y) {
      const int dr = (int)(k / bw);
      emit(a, t, b, f, t.y0 + dr, t.x0 + (int)(k - (long long)dr * bw));
    }
  }
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(RasterArgs a) {
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)a.H * a.W;
  if (pix >= (long long)a.B * plane) return;
  const int b = (int)(pix / plane);
  const int rc = (int)(pix - (long long)b * plane), r = rc / a.W, c = rc - r * a.W;
  const unsigned long long key = a.keys[pix];
  int f = -1;
  float depth = a.far_, lam[3] = {0.f, 0.f, 0.f};
  if (key != NO_KEY) {
    const int kf = (int)(unsigned)(key & 0xffffffffull);
    Tri t;
    float d;
    // the winner passed both in launch 2 or 3, with these bits; a key nobody wrote (scratch handed in dirty) decodes to background
    if (kf >= 0 && kf < a.T && tri_setup(a, b, kf, t) && fragment(a, t, r, c, d, lam)) {
      f = kf;
      depth = __uint_as_float((unsigned)(key >> 32));
    } else {
      lam[0] = lam[1] = lam[2] = 0.f;
    }
  }
  a.face_out[pix] = f;
  a.depth[pix] = depth;
  a.mask[pix] = f >= 0 ? 1 : 0;
  a.bary[pix * 3] = lam[0]; a.bary[pix * 3 + 1] = lam[1]; a.bary[pix * 3 + 2] = lam[2];
}

struct InterpArgs {
  const int* face; const float* bary; const int* faces; const float* attr; float* out;
  float fill;
  int B, H, W, T, V, C;
};

__global__ __launch_bounds__(256) void raster_interp_kernel(InterpArgs a) {
#pragma clang fp contract(off)
  const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long plane = (long long)a.H * a.W;
  if (pix >= (long long)a.B * plane) return;
  const int b = (int)(pix / plane);
  const long long rc = pix - (long long)b * plane;
  const int f = a.face[pix];
  int i0 = 0, i1 = 0, i2 = 0;
  bool hit = f >= 0 && f < a.T;
  if (hit) {
    i0 = a.faces[(size_t)f * 3]; i1 = a.faces[(size_t)f * 3 + 1]; i2 = a.faces[(size_t)f * 3 + 2];
    hit = (unsigned)i0 < (unsigned)a.V && (unsigned)i1 < (unsigned)a.V && (unsigned)i2 < (unsigned)a.V;
  }
  float l0 = 0.f, l1 = 0.f, l2 = 0.f;
  if (hit) { l0 = a.bary[pix * 3]; l1 = a.bary[pix * 3 + 1]; l2 = a.bary[pix * 3 + 2]; }
  float* o = a.out + (size_t)b * a.C * plane + rc;
  for (int ch = 0; ch < a.C; ++ch) {
    float v = a.fill;
    if (hit)
      v = (l0 * a.attr[(size_t)i0 * a.C + ch] + l1 * a.attr[(size_t)i1 * a.C + ch]) + l2 * a.attr[(size_t)i2 * a.C + ch];
    o[(size_t)ch * plane] = v;
  }
}

bool frame_ok(int B, int H, int W) {
  return B >= 0 && H >= 2 && W >= 2 && (long long)B * H * W <= 0x7fffffffLL;
}

unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int cips_raster_fwd(const float* vertices, const int* faces, const float* world2cam, const float* xg, const float* yg,
                               float zc, float near_, float far_, int cull, void* screen, unsigned long long* keys,
                               int* big_list, int* big_count, long long big_cap, int* face, float* bary, float* depth,
                               unsigned char* mask, int B, int V, int T, int H, int W, cips_stream_t stream) {
  if (B < 0 || V < 0 || T < 0 || !frame_ok(B, H, W)) return (int)hipErrorInvalidValue;
  if ((long long)B * V > 0x7fffffffLL || (long long)B * T > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (!world2cam || !xg || !yg || !keys || !big_count || !face || !bary || !depth || !mask) return (int)hipErrorInvalidValue;
  if ((V > 0 && (!vertices || !screen)) || (T > 0 && (!faces || !big_list))) return (int)hipErrorInvalidValue;
  if (!std::isfinite(near_) || !(near_ > 0.f) || !std::isfinite(zc) || !(zc < 0.f) || std::isnan(far_)) return (int)hipErrorInvalidValue;
  if (cull != 0 && cull != 1) return (int)hipErrorInvalidValue;
  if (big_cap < (long long)B * T) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  RasterArgs a = {};
  a.vertices = vertices; a.faces = faces; a.world2cam = world2cam; a.xg = xg; a.yg = yg;
  a.screen = (f32x4*)screen; a.keys = keys; a.big_list = big_list; a.big_count = big_count; a.big_cap = big_cap;
  a.face_out = face; a.bary = bary; a.depth = depth; a.mask = mask;
  a.zc = zc; a.near_ = near_; a.far_ = far_; a.cull = cull; a.B = B; a.V = V; a.T = T; a.H = H; a.W = W;
  hipStream_t st = (hipStream_t)stream;
  const long long pixels = (long long)B * H * W;
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)pixels * sizeof(unsigned long long), st);
  if (e != hipSuccess) return (int)e;
  if (V > 0 && T > 0) {                    // an empty mesh launches neither the vertex nor the face kernels
    e = hipMemsetAsync(big_count, 0, sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(raster_vertex_kernel, dim3(blocks((long long)B * V)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(raster_face_kernel, dim3(blocks((long long)B * T)), dim3(256), 0, st, a);
    const long long bt = (long long)B * T;
    hipLaunchKernelGGL(raster_big_kernel, dim3((unsigned)(bt < BIG_GRID_X ? bt : BIG_GRID_X), BIG_GRID_Y), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(blocks(pixels)), dim3(256), 0, st, a);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_raster_interp(const int* face, const float* bary, const int* faces, const float* attr, float fill, float* out,
                                  int B, int H, int W, int T, int V, int C, cips_stream_t stream) {
  if (V < 0 || T < 0 || C < 1 || !frame_ok(B, H, W)) return (int)hipErrorInvalidValue;
  if (!face || !bary || !out || (T > 0 && !faces) || (V > 0 && T > 0 && !attr)) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  InterpArgs a = {};
  a.face = face; a.bary = bary; a.faces = faces; a.attr = attr; a.out = out; a.fill = fill;
  a.B = B; a.H = H; a.W = W; a.T = (V > 0 ? T : 0); a.V = V; a.C = C;
  hipLaunchKernelGGL(raster_interp_kernel, dim3(blocks((long long)B * H * W)), dim3(256), 0, (hipStream_t)stream, a);
  return CIPS_CHECK_LAUNCH();
}
