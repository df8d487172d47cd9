// fit_loss.hip — the pyramid fit loss of the projection loop (cips3d_amd/projection.py) for gfx950: per-image loss and
// the full d loss / d pred in one pass over pred / target.
//
//   d_0 = pred - target, d_{l+1} = 2x2 mean of d_l;  w_0 = weight (or 1), w_{l+1} = 2x2 mean of w_l
//   loss_b = sum_{l<L} lambda_l / (C H_l W_l) * sum_{c,y,x} w_l rho(d_l),   rho(x) = x^2  or  sqrt(x^2 + eps^2) - eps
//
// Replaces, for one fitting step, the chain of ATen elementwise ops, avg_pool2d's and reductions (and their autograd
// backward) that the same loss costs as tensor operations: ~10 launches per level forward, as many backward.
//
//   launch 1  fit_tile_kernel    one workgroup per (image, 32x32 tile): levels 0..5 of both pyramids live in LDS, the loss
//                                terms of the tile are summed in a fixed tree, the gradient of those levels is stored.
//                                A level-l cell (l <= 5) lies inside one tile: H and W are multiples of 2^(L-1), and tiles
//                                start at multiples of 32, so a ragged tile holds whole cells only.
//   launch 2  fit_finish_kernel  one workgroup per image: levels 6 and 7 from the tiles' level-5 means (they exist only
//                                where every tile is whole), the tiles' partial sums in a fixed order -> loss_b, and per
//                                (channel, tile) the gradient those two levels hand down to every pixel of the tile.
//   launch 3  fit_top_kernel     (L > 6 only) adds that per-tile constant to the stored gradient.
//
// Every sum has a fixed order that depends on (C, H, W, L) alone: no atomics, two calls give the same bits, and an image
// gives the same bits whatever batch it sits in.  Bandwidth-trivial (three reads, one write per pixel); what it buys is
// launches.  The backward is cips_pyramid_loss_bwd: the stored gradient times the upstream value of its image.
#include "common.h"
#include "../../include/cips3d_hip.h"

namespace {

constexpr int TILE = 32;            // pixels per tile edge = 2^5: levels 0..5 are tile-local
constexpr int LOCAL_LEVELS = 6;
constexpr int MAX_LEVELS = 8;

struct FitArgs {
  const float* pred; const float* target; const float* weight;       // weight may be NULL (= 1)
  float* grad; float* loss;
  float* partial;      // (B, tiles)       the tiles' loss sums
  float* d5;           // (B, C, tiles)    level-5 means of d   (L > 6)
  float* w5;           // (B, tiles)       level-5 means of w   (L > 6)
  float* top;          // (B, 5 * ...)     levels 6, 7 of d and w, and the per-(channel, tile) gradient constant g5 (L > 6)
  int B, C, H, W, L, kind;
  int tiles_x, tiles_y;
  double eps;
  double lossc[MAX_LEVELS];    // lambda_l / (C H_l W_l)
  double gradc[MAX_LEVELS];    // lossc_l / 4^l: what one level-0 pixel receives of a level-l cell's derivative
};

// rho and rho' (kind 0: x^2; kind 1: Charbonnier, written as x^2 / (sqrt(x^2 + eps^2) + eps): exactly 0 at x = 0 and
// without the cancellation of sqrt(.) - eps for |x| << eps).  In fp64, like the differences they are taken of: the stored
// gradient is formed in fp64 and rounded to fp32 once, so it is the correctly rounded gradient of the definition (for
// L <= 6; the two levels above the tile add one more rounding).  A fit's first Adam steps move every style element by
// lr * g / (|g| + 1e-8): where g is near zero they magnify what the loss gradient carries in error by orders of magnitude.
// The arithmetic is a few fp64 operations per pixel and level on a kernel that is bound by its launches.
__device__ __forceinline__ void rho(int kind, double eps, double x, double* r, double* dr) {
  if (kind == 0) { *r = x * x; *dr = 2.0 * x; return; }
  const double s = sqrt(fma(x, x, eps * eps));
  *r = (x * x) / (s + eps);
  *dr = x / s;
}

// sum of the workgroup's 256 values in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ float block_sum256(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// offset of level l (1..5) in the tile-local pyramid arrays: 256 + 64 + 16 + 4 + 1 cells
__device__ __forceinline__ constexpr int lvl_off(int l) {
  return l == 1 ? 0 : l == 2 ? 256 : l == 3 ? 320 : l == 4 ? 336 : 340;
}

__global__ __launch_bounds__(256) void fit_tile_kernel(FitArgs a) {
  // levels 1..5 of d, current channel.  In fp64: a coarse mean is orders of magnitude smaller than the pixels it averages,
  // and rho' of the Charbonnier form turns an ABSOLUTE error of d_l into eps^-1 times as much gradient; the differences
  // of fp32 inputs and their means are exact to 1e-16 here, at no cost that matters (341 values per channel)
  __shared__ double sd[341];
  __shared__ float sw[341];       // levels 1..5 of w
  __shared__ float red[256];
  const int t = threadIdx.x;
  const int tile = blockIdx.x, b = blockIdx.y;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int qy = t >> 4, qx = t & 15;                      // this thread's 2x2 quad = its level-1 cell
  const int y0 = ty * TILE + 2 * qy, x0 = tx * TILE + 2 * qx;
  const int Lloc = a.L < LOCAL_LEVELS ? a.L : LOCAL_LEVELS;
  const size_t plane = (size_t)a.H * a.W;
  bool ok[4];
  size_t off[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + (k >> 1), x = x0 + (k & 1);
    ok[k] = y < a.H && x < a.W;
    off[k] = (size_t)y * a.W + x;
  }
  // L >= 2: H and W are even, a quad is inside the image or outside it as a whole
  const bool quad_ok = ok[0];

  // ---- the weight pyramid, once per tile ----
  float w0[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) w0[k] = !ok[k] ? 0.f : a.weight ? a.weight[(size_t)b * plane + off[k]] : 1.f;
  if (Lloc > 1) {
    sw[t] = 0.25f * ((w0[0] + w0[1]) + (w0[2] + w0[3]));
    __syncthreads();
    for (int l = 2; l < Lloc; ++l) {
      const int n = TILE >> l;                             // cells per tile edge at level l
      if (t < n * n) {
        const int cy = t / n, cx = t - cy * n;
        const float* s = sw + lvl_off(l - 1) + (2 * cy) * (2 * n) + 2 * cx;
        sw[lvl_off(l) + t] = 0.25f * ((s[0] + s[1]) + (s[2 * n] + s[2 * n + 1]));
      }
      __syncthreads();
    }
  }

  float acc = 0.f;                                         // this thread's share of the tile's loss
  for (int c = 0; c < a.C; ++c) {
    const size_t base = ((size_t)b * a.C + c) * plane;
    double d0[4], g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d0[k] = ok[k] ? (double)a.pred[base + off[k]] - (double)a.target[base + off[k]] : 0.0;
      double r, dr;
      rho(a.kind, a.eps, d0[k], &r, &dr);
      acc += (float)(a.lossc[0] * w0[k] * r);
      g[k] = a.gradc[0] * w0[k] * dr;
    }
    if (Lloc > 1) {
      __syncthreads();                                     // the previous channel's readers are done with sd
      sd[t] = 0.25 * ((d0[0] + d0[1]) + (d0[2] + d0[3]));
      __syncthreads();
      for (int l = 2; l < Lloc; ++l) {
        const int n = TILE >> l;
        if (t < n * n) {
          const int cy = t / n, cx = t - cy * n;
          const double* s = sd + lvl_off(l - 1) + (2 * cy) * (2 * n) + 2 * cx;
          sd[lvl_off(l) + t] = 0.25 * ((s[0] + s[1]) + (s[2 * n] + s[2 * n + 1]));
        }
        __syncthreads();
      }
      double gq = 0.0;                                     // what the levels >= 1 hand down to this quad's pixels
      for (int l = 1; l < Lloc; ++l) {
        const int n = TILE >> l;
        // the loss term of a cell is taken by its thread (level 1: every thread; above: the first n*n), where the cell
        // lies inside the image; the gradient by every thread below the cell
        const int cy = qy >> (l - 1), cx = qx >> (l - 1);
        const int cell = lvl_off(l) + cy * n + cx;
        double r, dr;
        rho(a.kind, a.eps, sd[cell], &r, &dr);
        gq += a.gradc[l] * sw[cell] * dr;
        if (t < n * n) {
          const int oy = t / n, ox = t - oy * n;
          if (ty * TILE + (oy << l) < a.H && tx * TILE + (ox << l) < a.W) {
            double r2, dr2;
            rho(a.kind, a.eps, sd[lvl_off(l) + t], &r2, &dr2);
            acc += (float)(a.lossc[l] * sw[lvl_off(l) + t] * r2);
          }
        }
      }
      if (quad_ok) {
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] += gq;
      }
      if (a.L > LOCAL_LEVELS && t == 0) a.d5[((size_t)b * a.C + c) * gridDim.x + tile] = (float)sd[340];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ok[k]) a.grad[base + off[k]] = (float)g[k];
  }
  if (a.L > LOCAL_LEVELS && t == 0) a.w5[(size_t)b * gridDim.x + tile] = sw[340];
  __syncthreads();
  const float s = block_sum256(acc, red);
  if (t == 0) a.partial[(size_t)b * gridDim.x + tile] = s;
}

// layout of FitArgs.top per image, in floats (n5 = tiles, n6 = n5 / 4, n7 = n6 / 4 cells):
//   d6 (C, n6) | w6 (n6) | d7 (C, n7) | w7 (n7) | g5 (C, n5)
__host__ __device__ inline size_t top_floats(int C, int n5) {
  const size_t n6 = n5 / 4, n7 = n6 / 4;
  return (size_t)C * n6 + n6 + (size_t)C * n7 + n7 + (size_t)C * n5;
}

__global__ __launch_bounds__(256) void fit_finish_kernel(FitArgs a) {
  __shared__ float red[256];
  const int t = threadIdx.x, b = blockIdx.x;
  const int n5 = a.tiles_x * a.tiles_y;
  float acc = 0.f;
  for (int i = t; i < n5; i += 256) acc += a.partial[(size_t)b * n5 + i];
  if (a.L > LOCAL_LEVELS) {
    // every tile is whole here (H and W are multiples of 64 or 128)
    const int x5 = a.tiles_x, x6 = x5 / 2, y6 = a.tiles_y / 2, n6 = x6 * y6;
    const int x7 = x6 / 2, y7 = y6 / 2, n7 = (a.L > 7) ? x7 * y7 : 0;
    float* top = a.top + (size_t)b * top_floats(a.C, n5);
    float* d6 = top;
    float* w6 = d6 + (size_t)a.C * n6;
    float* d7 = w6 + n6;
    float* w7 = d7 + (size_t)a.C * (n5 / 16);
    float* g5 = w7 + (n5 / 16);
    const float* d5 = a.d5 + (size_t)b * a.C * n5;
    const float* w5 = a.w5 + (size_t)b * n5;
    // level 6: planes 0..C-1 are d, plane C is w
    for (int i = t; i < (a.C + 1) * n6; i += 256) {
      const int p = i / n6, cell = i - p * n6, cy = cell / x6, cx = cell - cy * x6;
      const float* s = (p < a.C ? d5 + (size_t)p * n5 : w5) + (2 * cy) * x5 + 2 * cx;
      (p < a.C ? d6 + (size_t)p * n6 : w6)[cell] = (float)(0.25 * (((double)s[0] + s[1]) + ((double)s[x5] + s[x5 + 1])));
    }
    __syncthreads();
    for (int i = t; i < (a.C + 1) * n7; i += 256) {
      const int p = i / n7, cell = i - p * n7, cy = cell / x7, cx = cell - cy * x7;
      const float* s = (p < a.C ? d6 + (size_t)p * n6 : w6) + (2 * cy) * x6 + 2 * cx;
      (p < a.C ? d7 + (size_t)p * n7 : w7)[cell] = (float)(0.25 * (((double)s[0] + s[1]) + ((double)s[x6] + s[x6 + 1])));
    }
    __syncthreads();
    // loss terms of the two levels, then the constant each tile's pixels receive from them
    for (int i = t; i < a.C * n6; i += 256) {
      double r, dr;
      rho(a.kind, a.eps, d6[i], &r, &dr);
      acc += (float)(a.lossc[6] * w6[i % n6] * r);
    }
    for (int i = t; i < a.C * n7; i += 256) {
      double r, dr;
      rho(a.kind, a.eps, d7[i], &r, &dr);
      acc += (float)(a.lossc[7] * w7[i % n7] * r);
    }
    for (int i = t; i < a.C * n5; i += 256) {
      const int c = i / n5, tile = i - c * n5, ty = tile / x5, tx = tile - ty * x5;
      const int c6 = (ty >> 1) * x6 + (tx >> 1);
      double r, dr;
      rho(a.kind, a.eps, d6[(size_t)c * n6 + c6], &r, &dr);
      double g = a.gradc[6] * w6[c6] * dr;
      if (n7) {
        const int c7 = (ty >> 2) * x7 + (tx >> 2);
        rho(a.kind, a.eps, d7[(size_t)c * n7 + c7], &r, &dr);
        g += a.gradc[7] * w7[c7] * dr;
      }
      g5[i] = (float)g;
    }
  }
  const float s = block_sum256(acc, red);
  if (t == 0) a.loss[b] = s;
}

// grad[b, c, y, x] += g5[b, c, tile(y, x)]: one thread per pixel of a plane, blockIdx.y = plane (b * C + c)
__global__ __launch_bounds__(256) void fit_top_kernel(FitArgs a) {
  const size_t plane = (size_t)a.H * a.W;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  const int bc = blockIdx.y, b = bc / a.C, c = bc - b * a.C;
  const int y = (int)(i / a.W), x = (int)(i - (size_t)y * a.W);
  const int n5 = a.tiles_x * a.tiles_y;
  const size_t per = top_floats(a.C, n5);
  const float* g5 = a.top + (size_t)b * per + (per - (size_t)a.C * n5);
  a.grad[(size_t)bc * plane + i] += g5[(size_t)c * n5 + (y / TILE) * a.tiles_x + x / TILE];
}

__global__ __launch_bounds__(256) void fit_scale_kernel(const float* __restrict__ grad, const float* __restrict__ upstream,
                                                        float* __restrict__ out, long long per_image) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_image) return;
  const size_t j = (size_t)blockIdx.y * per_image + i;
  out[j] = grad[j] * upstream[blockIdx.y];
}

bool shape_ok(int B, int C, int H, int W, int L) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || L < 1 || L > MAX_LEVELS) return false;
  const int m = 1 << (L - 1);
  return H % m == 0 && W % m == 0;
}

}  // namespace

extern "C" long long cips_pyramid_loss_scratch(int B, int C, int H, int W, int L) {
  if (!shape_ok(B, C, H, W, L)) return -1;
  const long long tiles = (long long)((H + TILE - 1) / TILE) * ((W + TILE - 1) / TILE);
  long long n = (long long)B * tiles;                                          // partial
  if (L > LOCAL_LEVELS) n += (long long)B * C * tiles + (long long)B * tiles + (long long)B * (long long)top_floats(C, (int)tiles);
  return n;
}

extern "C" int cips_pyramid_loss_fwd(const float* pred, const float* target, const float* weight,
                                     const double* level_weights_host, int L, int kind, double eps, float* loss, float* grad,
                                     float* scratch, long long scratch_floats, int B, int C, int H, int W,
                                     cips_stream_t stream) {
  if (!pred || !target || !level_weights_host || !loss || !grad || !scratch) return (int)hipErrorInvalidValue;
  if (!shape_ok(B, C, H, W, L) || (kind != 0 && kind != 1) || (kind == 1 && !(eps > 0.0))) return (int)hipErrorInvalidValue;
  if (scratch_floats < cips_pyramid_loss_scratch(B, C, H, W, L)) return (int)hipErrorInvalidValue;
  const int tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
  const long long tiles = (long long)tiles_x * tiles_y;
  const long long planes = (long long)B * C;
  const long long pix_blocks = ((long long)H * W + 255) / 256;
  // grid limits: x < 2^31, y < 65536
  if (tiles > 0x7fffffffLL || B > 65535 || planes > 65535 || pix_blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  FitArgs a;
  a.pred = pred; a.target = target; a.weight = weight; a.grad = grad; a.loss = loss;
  a.partial = scratch;
  a.d5 = a.w5 = a.top = nullptr;
  if (L > LOCAL_LEVELS) {
    a.d5 = scratch + (size_t)B * tiles;
    a.w5 = a.d5 + (size_t)B * C * tiles;
    a.top = a.w5 + (size_t)B * tiles;
  }
  a.B = B; a.C = C; a.H = H; a.W = W; a.L = L; a.kind = kind; a.tiles_x = tiles_x; a.tiles_y = tiles_y;
  a.eps = eps;
  for (int l = 0; l < MAX_LEVELS; ++l) {
    const double cells = (double)C * (double)(H >> l) * (double)(W >> l);
    a.lossc[l] = l < L ? level_weights_host[l] / cells : 0.0;
    a.gradc[l] = l < L ? level_weights_host[l] / cells / (double)(1LL << (2 * l)) : 0.0;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fit_tile_kernel, dim3((unsigned)tiles, B), dim3(256), 0, st, a);
  hipLaunchKernelGGL(fit_finish_kernel, dim3(B), dim3(256), 0, st, a);
  if (L > LOCAL_LEVELS) hipLaunchKernelGGL(fit_top_kernel, dim3((unsigned)pix_blocks, (unsigned)planes), dim3(256), 0, st, a);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_pyramid_loss_bwd(const float* grad, const float* upstream, float* out, int B, long long per_image,
                                     cips_stream_t stream) {
  if (!grad || !upstream || !out || B <= 0 || per_image <= 0) return (int)hipErrorInvalidValue;
  const long long blocks = (per_image + 255) / 256;
  if (B > 65535 || blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_scale_kernel, dim3((unsigned)blocks, B), dim3(256), 0, (hipStream_t)stream, grad, upstream, out,
                     per_image);
  return CIPS_CHECK_LAUNCH();
}
