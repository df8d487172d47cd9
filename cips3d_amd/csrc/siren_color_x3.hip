// siren_color_x3.hip — the colour of a point on the split-bf16 / fp16 register chain of siren_x3_common.h: cips_siren_rgb_x3 and
// cips_siren_rgb_x3_grid, the forward kernel's 32 colour features projected to three channels before they leave the registers
// (rgb = [tanh](W feat + b), W (3,32): the auxiliary RGB layer of the generator, or any other 32 -> 3 map), and sigma when asked for.
// 12 (16) B per point to HBM where the forward kernel writes 132 B and a 32 -> 3 launch reads 128 B of that back.
// A source of its own (like siren_surface_x3.hip and siren_bwd_points_x3.hip): it runs only when a caller asks for colours, and as
// a separate module it leaves the listings and the kernel order of siren_fwd_x3.hip's code object as they are (that file's header says
// why its order is not to be touched).  The chain is the forward kernel's, text for text: siren_fwd_chain.inc behind the forward
// kernel's prologue, so feat and sigma are cips_siren_fwd_x3's bit for bit.
#include "siren_x3_common.h"

// siren_fwd_chain.inc stamps its phases in probe builds of the march only; this module stamps nothing
#define X3F_TS(i)

namespace {

// ------------------------------------------------------------------------------------------------------------------
// siren_fwd_x3_kernel's layout, LDS carve, staging and chunking (lane = point, a wave owns 32 points, the two lane halves hold 16 of
// the 32 colour features each: register r of half hf <-> channel c(r, hf) = (r&3) + 8(r>>2) + 4hf).  The epilogue, per point:
//   feat[c] = fmaf(accf[r], isf, bf[c])                                    the forward kernel's output fma
//   s_hf[j] = fmaf(W[j][c(15, hf)], feat[c(15, hf)], ... fmaf(W[j][c(0, hf)], feat[c(0, hf)], 0))      r = 0..15 ascending
//   y[j]    = (s_hf[j] + s_(1-hf)[j]) + b[j]                               one cross-half add (commutative: both halves agree)
//   rgb[j]  = tanh ? tanhf(y[j]) : y[j]
// — the shape of the chain's sigma dot.  W waits in LDS in the order the registers want it, PW[hf][j][r] = W[j][c(r, hf)], in the
// slot behind the output bias (O_AUX: bf at +0, the colour head's 2^-k at +128, PW at +256, b at +640 of 4096 bytes), so a lane
// reads its 48 weights as twelve 16-byte loads, every lane of a half the same address (a broadcast, no bank conflict).
// GRID: the point of index p = (i * ny + j) * nz + k is (gx[i], gy[j], gz[k]), index arithmetic only (the sigma grid kernel's rule).
constexpr int O_PW = O_AUX + 256, O_PB = O_PW + 2 * 3 * 16 * 4;
static_assert(O_PB + 3 * 4 <= O_STG, "projection weights fit the aux slot");

struct ColorX3Args {
  cips_siren_weights w;
  const float* points;               // (B, P, 3); unused with GRID
  const float *gx, *gy, *gz;         // GRID: the lattice's coordinates (nx), (ny), (nz)
  const float *pw, *pb;              // (3, 32), (3): the projection
  float* rgb;                        // (B, P, 3)
  float* sigma;                      // (B, P) or NULL
  int ny, nz;
  int tanh_out;
  int B, P, chunk;
};

template <bool HW, bool F16, bool GRID>
__global__ __launch_bounds__(512) void siren_color_x3_kernel(ColorX3Args a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  const int b = blockIdx.y;
  stage_weights_x3<HW, F16>(smem, a.w, b);
  if (threadIdx.x < CF) reinterpret_cast<float*>(smem + O_AUX)[threadIdx.x] = a.w.bf[threadIdx.x];
  if (threadIdx.x >= 64 && threadIdx.x < 64 + 96) {       // PW[hf][j][r] = W[j][(r&3) + 8(r>>2) + 4hf]
    const int i = threadIdx.x - 64, hfw = i / 48, j = (i % 48) >> 4, r = i & 15;
    reinterpret_cast<float*>(smem + O_PW)[i] = a.pw[j * CF + (r & 3) + 8 * (r >> 2) + 4 * hfw];
  }
  if (threadIdx.x >= 192 && threadIdx.x < 192 + 3) reinterpret_cast<float*>(smem + O_PB)[threadIdx.x - 192] = a.pb[threadIdx.x - 192];
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
  const float bs = a.w.bs[0];
  const float isf = F16 ? reinterpret_cast<const float*>(smem + O_AUX)[32] : 1.f;      // 2^-k of the colour head's weight image
  const bool th = a.tanh_out != 0;
  const int cstart = blockIdx.x * a.chunk;
  const int cend = min(cstart + a.chunk, a.P);
  for (int pbase = cstart + wave * 32; pbase < cend; pbase += 8 * 32) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int l31 = lane & 31, hf = lane >> 5;
    const LaneAddr LA = lane_addr(lane, sbase);
    const int p = pbase + l31;
    const bool valid = p < cend;
    const int pc = valid ? p : cend - 1;           // ragged tail: the last valid point again, nothing stored
    const long long gp = (long long)b * a.P + pc;
    float px, py, pz;
    if constexpr (GRID) {
      const unsigned r = (unsigned)pc / (unsigned)a.nz, k = (unsigned)pc - r * (unsigned)a.nz;
      const unsigned i = r / (unsigned)a.ny, j = r - i * (unsigned)a.ny;
      px = a.gx[i]; py = a.gy[j]; pz = a.gz[k];
    } else {
      px = a.points[gp * 3 + 0]; py = a.points[gp * 3 + 1]; pz = a.points[gp * 3 + 2];
    }

#include "siren_fwd_chain.inc"
    const float* bfv = reinterpret_cast<const float*>(smem + O_AUX);
    const unsigned pwb = opaque(sbase + O_PW + 192 * hf);
    float y[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float f0 = fmaf(accf[0][4 * g + 0], isf, bfv[8 * g + 4 * hf + 0]);
      const float f1 = fmaf(accf[0][4 * g + 1], isf, bfv[8 * g + 4 * hf + 1]);
      const float f2 = fmaf(accf[0][4 * g + 2], isf, bfv[8 * g + 4 * hf + 2]);
      const float f3 = fmaf(accf[0][4 * g + 3], isf, bfv[8 * g + 4 * hf + 3]);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float4 w4 = lds_ld4(pwb + 64 * j + 16 * g);
        y[j] = fmaf(w4.w, f3, fmaf(w4.z, f2, fmaf(w4.y, f1, fmaf(w4.x, f0, y[j]))));
      }
    }
    const float* pbv = reinterpret_cast<const float*>(smem + O_PB);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      y[j] += __shfl_xor(y[j], 32);
      y[j] += pbv[j];
      if (th) y[j] = tanhf(y[j]);
    }
    if (valid && hf == 0) {
      float* po = a.rgb + gp * 3;
      po[0] = y[0]; po[1] = y[1]; po[2] = y[2];
      if (a.sigma) a.sigma[gp] = sig;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace

// One launcher for both entry points, with the chunk rule of the forward (x3_chunk; a ragged tail is clamped to the last valid point
// in-kernel).  grid == NULL: points (B, P, 3).
static int siren_color_x3_launch(const cips_siren_weights* w, const float* points, const cips_grid_params* grid, const float* proj_w,
                                 const float* proj_b, int tanh_out, float* rgb, float* sigma, int B, int P, cips_stream_t stream) {
  ColorX3Args a;
  a.w = *w; a.points = points; a.pw = proj_w; a.pb = proj_b; a.rgb = rgb; a.sigma = sigma; a.tanh_out = tanh_out; a.B = B; a.P = P;
  a.gx = a.gy = a.gz = nullptr; a.ny = a.nz = 1;
  if (grid) { a.gx = grid->gx; a.gy = grid->gy; a.gz = grid->gz; a.ny = grid->ny; a.nz = grid->nz; }
  a.chunk = x3_chunk(B, P);
  dim3 g((P + a.chunk - 1) / a.chunk, B);
  x3_pick([&](auto HW_, auto F16_, auto GRID_) {
    x3_launch<siren_color_x3_kernel<decltype(HW_)::value, decltype(F16_)::value, decltype(GRID_)::value>>(g, 512, O_STG, stream, a);
  }, (w->trig_mode & 1) != 0, (w->trig_mode & 2) == 0, grid != nullptr);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_siren_rgb_x3(const cips_siren_weights* w, const float* points, const float* proj_w, const float* proj_b,
                                 int tanh_out, float* rgb, float* sigma, int B, int P, cips_stream_t stream) {
  if (!w || !points || !proj_w || !proj_b || !rgb || B <= 0 || B > 65535 || P <= 0) return (int)hipErrorInvalidValue;
  return siren_color_x3_launch(w, points, nullptr, proj_w, proj_b, tanh_out, rgb, sigma, B, P, stream);
}

extern "C" int cips_siren_rgb_x3_grid(const cips_siren_weights* w, const cips_grid_params* grid, const float* proj_w,
                                      const float* proj_b, int tanh_out, float* rgb, float* sigma, int B, cips_stream_t stream) {
  if (!w || !grid || !proj_w || !proj_b || !rgb || B <= 0 || B > 65535) return (int)hipErrorInvalidValue;
  if (!grid->gx || !grid->gy || !grid->gz || grid->nx <= 0 || grid->ny <= 0 || grid->nz <= 0) return (int)hipErrorInvalidValue;
  const long long nxy = (long long)grid->nx * grid->ny;               // < 2^62; times nz only once it is known to fit an int
  if (nxy > INT_MAX || nxy * grid->nz > INT_MAX) return (int)hipErrorInvalidValue;
  return siren_color_x3_launch(w, nullptr, grid, proj_w, proj_b, tanh_out, rgb, sigma, B, (int)(nxy * grid->nz), stream);
}
