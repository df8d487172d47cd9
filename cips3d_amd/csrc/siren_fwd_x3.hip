// siren_fwd_x3.hip — the forward kernels on the split-bf16 / fp16 register chain of siren_x3_common.h: the points / rays
// forward (cips_siren_fwd_x3, cips_siren_fwd_x3_rays) and the fused ray-march (cips_march_fwd_x3).  Both run one wave-step of
// the chain from siren_fwd_chain.inc, included as text (its header says why it is no function).
//
// The sigma kernels (siren_sigma_x3.inc, included in front of the march's entry points, i.e. in front of where the march
// kernels are instantiated) are compiled with this source.  On their own they come out
// different: with no kernel in the module that stages Wc or Wf, every call of img_addr has R = 128, hipcc specialises it before
// it is inlined, and the W1 staging loop of all sixteen instances gets other address arithmetic (same instruction count).
// Why in front of the march and no longer at the end: the place changes no kernel's instructions (the compiler's assembly of
// all 32 kernels was compared, place by place and against the build before the opacity instantiations), only the order of the
// kernels in the code object.  But behind the twelve march kernels there are now,
// tests/test_gpu_density.py::test_sigma_only_equals_the_full_forward_bit_for_bit[3-4160-0] failed on the MI355X in two runs of
// two — two launches of siren_sigma_x3_kernel<false, true, false> on the same points differed in some element — and in front
// of them the whole suite passes.  So the sigma kernel's software-trig form has a timing-dependent defect that the layout only
// hides; it is older than this placement and its cause is not found.
#include "siren_x3_common.h"

// Phase timestamps of the chain, probe builds only (-DCIPS_TUNING with CIPS_X3_MPROF set): the including kernel supplies
// x3f_ts(i) — the march stamps, the points / rays forward has no sample index and stamps nothing.  The production build emits
// nothing.
#ifdef CIPS_TUNING
#define X3F_TS(i) x3f_ts(i);
#else
#define X3F_TS(i)
#endif

namespace {

// ------------------------------------------------------------------------------------------------------------------
// Forward on the same split-bf16 register chain (default; CIPS_SIREN_FWD=f32 selects siren.hip's exact fp32 MFMA
// kernel): layer 0 on the VALU, W1 / Wc / Wf on v_mfma_f32_32x32x16_bf16 in three passes, sigma as a VALU
// dot with one cross-half add.  No weight-gradient accumulators, so eight waves (two per SIMD) share the LDS images.
struct FwdX3Args {
  cips_siren_weights w;
  const float* points;     // (B, P, 3) or NULL: generated from rg (point index = ray * S + s)
  float* feat;
  float* sigma;
  float* zout;             // optional (B, P): the depth of every generated point
  RayGen rg;
  int B, P, chunk;
};

template <bool HW, bool F16>
__global__ __launch_bounds__(512) void siren_fwd_x3_kernel(FwdX3Args a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  const int b = blockIdx.y;
  stage_weights_x3<HW, F16>(smem, a.w, b);
  if (threadIdx.x < CF) reinterpret_cast<float*>(smem + O_AUX)[threadIdx.x] = a.w.bf[threadIdx.x];   // bf[32] (aux image unused here)
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
  const float bs = a.w.bs[0];
  const float isf = F16 ? reinterpret_cast<const float*>(smem + O_AUX)[32] : 1.f;      // 2^-k of the colour head's weight image
  const int cstart = blockIdx.x * a.chunk;
  const int cend = min(cstart + a.chunk, a.P);
#ifdef CIPS_TUNING
  auto x3f_ts = [](int) {};
#endif
  for (int pbase = cstart + wave * 32; pbase < cend; pbase += 8 * 32) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int l31 = lane & 31, hf = lane >> 5;
    const LaneAddr LA = lane_addr(lane, sbase);
    const int p = pbase + l31;
    const bool valid = p < cend;
    const long long gp = (long long)b * a.P + (valid ? p : cend - 1);
    float px, py, pz, zpt = 0.f;
    if (a.points) { px = a.points[gp * 3 + 0]; py = a.points[gp * 3 + 1]; pz = a.points[gp * 3 + 2]; }
    else gen_point(a.rg, b, valid ? p : cend - 1, px, py, pz, zpt);

#include "siren_fwd_chain.inc"
    if (valid) {
      float* fo = a.feat + gp * CF + 4 * hf;
      const float* bfv = reinterpret_cast<const float*>(smem + O_AUX);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 v;
        v.x = fmaf(accf[0][4 * g + 0], isf, bfv[8 * g + 4 * hf + 0]);
        v.y = fmaf(accf[0][4 * g + 1], isf, bfv[8 * g + 4 * hf + 1]);
        v.z = fmaf(accf[0][4 * g + 2], isf, bfv[8 * g + 4 * hf + 2]);
        v.w = fmaf(accf[0][4 * g + 3], isf, bfv[8 * g + 4 * hf + 3]);
        *reinterpret_cast<float4*>(fo + 8 * g) = v;
      }
      if (hf == 0) {
        a.sigma[gp] = sig;
        if (a.zout) a.zout[gp] = zpt;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Fused ray-march, non-hierarchical sampling (the headline configuration: num_steps samples per ray, no resampling):
// ray set-up + FiLM-SIREN + alpha-composite (exp/comm/comm_utils.py:365-438, 584-679; exp/cips3d/models/
// generator.py:260-317; exp/pigan/pigan_utils.py:212-273) in ONE kernel that walks the samples along the ray.
// A wave owns 32 rays (lane & 31 = ray; the two lane halves hold 16 of the 32 feature channels each) and steps
// s = 0..S-1: generate the sample point, run the register-chain MLP of siren_point_x3 (weights resident in LDS), and
// fold the sample front-to-back into the ray's running transmittance / feature / depth accumulators — z is ascending by
// construction (|jitter offset| <= half a bin), so the merge of the hierarchical path is the identity here and the
// composite needs no cross-lane traffic at all.  HBM per ray: 4 B per sample of jitter (+ 4 B of noise when
// nerf_noise > 0) in, 128 B feature + 4 B depth out = 4 S + 132 B; the (B, n, S, 3) points and the
// (B, P, 32) per-sample features never exist in HBM unless the caller asks for them (feat / sigma / z outputs: the
// training forward keeps them for the backward).  Transmittance runs in double like ATen's CPU cumprod.
struct MarchArgs {
  cips_siren_weights w;
  RayGen rg;
  const float* noise;        // (B, n, S) standard normals or NULL
  float noise_std;
  int clamp_mode, flags;     // flags: bit0 last_back, bit1 white_back
  float *fea, *depth;        // (B, n, 32), (B, n)
  float *opacity;            // (B, n) or NULL: sum_s w_s before the last_back / white_back adjustments (cips_march_fwd_x3_geo)
  float *weights;            // (B, n, S) or NULL
  float *feat, *sigma, *zout;   // per-sample outputs (B, P, 32), (B, P), (B, P) or NULL
  int B, rays_per_wg;
  const unsigned char* clamp_pin;   // optional branch masks of the relu clamp (cips_march_fwd_x3's clamp_in / clamp_out):
  unsigned char* clamp_rec;         // branch per (ray, sample) supplied / recorded; both NULL in production
  int desync;                       // probe builds: shader cycles the second wave of every SIMD starts late (0 = together)
  int one_wave;                     // probe builds: waves 4-7 leave at once (one wave per SIMD; half the rays are not marched)
  unsigned long long* prof;         // probe builds: phase timestamps of workgroup (0,0), samples 8..11
};

// OPA: the instantiation that stores `opacity` (the debug instantiation DBG stores it too, when given); the production
// launch — no masks, no opacity — is the <HW, false, F16, false> kernel, whose code holds neither.
template <bool HW, bool DBG, bool F16, bool OPA>
__global__ __launch_bounds__(512) void siren_march_x3_kernel(MarchArgs a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  const int b = blockIdx.y;
  stage_weights_x3<HW, F16>(smem, a.w, b);
  if (threadIdx.x < CF) reinterpret_cast<float*>(smem + O_AUX)[threadIdx.x] = a.w.bf[threadIdx.x];
  __syncthreads();
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
  const float bs = a.w.bs[0];
  const RayGen& g = a.rg;
  const int S = g.S, n = g.n;
  const int cstart = blockIdx.x * a.rays_per_wg;
  const int cend = min(cstart + a.rays_per_wg, n);
  const float* M = g.c2w + (long long)b * 16;
  const float* bfv = reinterpret_cast<const float*>(smem + O_AUX);
  const float isf = F16 ? bfv[32] : 1.f;        // 2^-k of the colour head's weight image
  if (CIPS_TUNE(a.one_wave) && wave >= 4) return;
  if (CIPS_TUNE(a.desync) > 0 && wave >= 4) {
    const long long t0 = __builtin_readcyclecounter();
    while (__builtin_readcyclecounter() - t0 < (long long)a.desync) __builtin_amdgcn_s_sleep(8);
  }
  for (int rbase = cstart + wave * 32; rbase < cend; rbase += 8 * 32) {
    const int l31s = lane0 & 31, hfs = lane0 >> 5;
    const int ray_raw = rbase + l31s;
    const bool valid = ray_raw < cend;
    const int ray = valid ? ray_raw : cend - 1;
    const long long rs = ((long long)b * n + ray) * S;        // first sample of this ray in the (B, n, S) tensors
    const RayDir d = ray_dir(g, ray);
    const bool has_jit = g.jitter != nullptr;
    float bias[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bias[r] = bfv[(r & 3) + 8 * (r >> 2) + 4 * hfs];
    float F[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) F[r] = 0.f;
    float flast[16];
    double T = 1.0;
    float depth = 0.f, wsum = 0.f, wlast = 0.f, zlast = 0.f;
    // sample s: world point + depth; the depth of sample s+1 gives delta_s
    float wx, wy, wz, zs;
    ray_point(g, M, d, g.zg[0], has_jit ? g.jitter[rs] : 0.f, has_jit, wx, wy, wz, zs);
    float u_next = (has_jit && S > 1) ? g.jitter[rs + 1] : 0.f;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      const int hf = lane >> 5;
      const LaneAddr LA = lane_addr(lane, sbase);
      // next sample's point now (its jitter was requested one step ago), the one after that requested now
      float nx = 0.f, ny = 0.f, nz = 0.f, zn = 0.f;
      if (s + 1 < S) ray_point(g, M, d, g.zg[s + 1], u_next, has_jit, nx, ny, nz, zn);
      if (has_jit && s + 2 < S) u_next = g.jitter[rs + s + 2];
      const float nse = a.noise ? a.noise[rs + s] : 0.f;

      const float px = wx, py = wy, pz = wz;
#ifdef CIPS_TUNING
      auto x3f_ts = [&](int i) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        if (a.prof && blockIdx.x == 0 && blockIdx.y == 0 && lane0 == 0 && (s >> 2) == 2)
          a.prof[(((s & 3) * 8 + wave) * 8) + i] = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
      };
#endif
#include "siren_fwd_chain.inc"
      float f[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) f[r] = fmaf(accf[0][r], isf, bias[r]);
      // ---- composite (pigan_utils.py:239-258): alpha = 1 - exp(-delta * clamp(sigma + noise)), w = alpha * T ----
      const float delta = (s + 1 < S) ? (zn - zs) : 1e10f;
      const float sg = a.noise ? sig + nse * a.noise_std : sig;
      float dens = (a.clamp_mode == 1) ? ((sg > 20.f) ? sg : log1pf(expf(sg))) : fmaxf(sg, 0.f);
      if (DBG && a.clamp_mode == 0) {      // the debug instantiation only: the production kernel's code is untouched
        bool pass = sg > 0.f;
        if (a.clamp_pin) pass = a.clamp_pin[rs + s] != 0;
        if (a.clamp_rec && valid && hf == 0) a.clamp_rec[rs + s] = pass ? 1 : 0;
        dens = pass ? sg : 0.f;
      }
      const float alpha = 1.f - expf(-delta * dens);
      const float w = alpha * (float)T;
      T *= (double)(1.f - alpha + 1e-10f);
#pragma unroll
      for (int r = 0; r < 16; ++r) F[r] = fmaf(w, f[r], F[r]);
      depth = fmaf(w, zs, depth);
      wsum += w;
      if (s == S - 1) {
        wlast = w; zlast = zs;
#pragma unroll
        for (int r = 0; r < 16; ++r) flast[r] = f[r];
      }
      if (valid) {
        if (a.feat) {
          float* fo = a.feat + (rs + s) * CF + 4 * hf;
#pragma unroll
          for (int gq = 0; gq < 4; ++gq)
            *reinterpret_cast<float4*>(fo + 8 * gq) = make_float4(f[4 * gq], f[4 * gq + 1], f[4 * gq + 2], f[4 * gq + 3]);
        }
        if (hf == 0) {
          if (a.sigma) a.sigma[rs + s] = sig;
          if (a.zout) a.zout[rs + s] = zs;
          if (a.weights && !(s == S - 1 && (a.flags & 1))) a.weights[rs + s] = w;
        }
      }
      wx = nx; wy = ny; wz = nz; zs = zn;
      X3F_TS(7)
      __builtin_amdgcn_sched_barrier(0);
    }
    if (a.flags & 1) {           // last_back: weights[:, :, -1] += 1 - weights_sum (pigan_utils.py:261-263)
      const float extra = 1.f - wsum;
#pragma unroll
      for (int r = 0; r < 16; ++r) F[r] = fmaf(extra, flast[r], F[r]);
      depth = fmaf(extra, zlast, depth);
      if (a.weights && valid && hfs == 0) a.weights[rs + S - 1] = wlast + extra;
    }
    if (a.flags & 2) {           // white_back: rgb + 1 - weights_sum (:266-268)
      const float extra = 1.f - wsum;
#pragma unroll
      for (int r = 0; r < 16; ++r) F[r] += extra;
    }
    if (valid) {
      float* o = a.fea + ((long long)b * n + ray) * CF + 4 * hfs;
#pragma unroll
      for (int gq = 0; gq < 4; ++gq)
        *reinterpret_cast<float4*>(o + 8 * gq) = make_float4(F[4 * gq], F[4 * gq + 1], F[4 * gq + 2], F[4 * gq + 3]);
      if (hfs == 0 && a.depth) a.depth[(long long)b * n + ray] = depth;
      if ((DBG || OPA) && hfs == 0 && a.opacity) a.opacity[(long long)b * n + ray] = wsum;
    }
  }
}

}  // namespace

static int siren_fwd_x3_launch(const cips_siren_weights* w, const float* points, const cips_ray_params* rays, float* feat,
                               float* sigma, float* zout, int B, int P, cips_stream_t stream);

extern "C" int cips_siren_fwd_x3(const cips_siren_weights* w, const float* points, float* feat, float* sigma, int B, int P,
                                 cips_stream_t stream) {
  if (!points) return (int)hipErrorInvalidValue;
  return siren_fwd_x3_launch(w, points, nullptr, feat, sigma, nullptr, B, P, stream);
}

extern "C" int cips_siren_fwd_x3_rays(const cips_siren_weights* w, const cips_ray_params* rays, float* feat, float* sigma,
                                      float* zout, int B, cips_stream_t stream) {
  if (!rays) return (int)hipErrorInvalidValue;
  return siren_fwd_x3_launch(w, nullptr, rays, feat, sigma, zout, B, rays->W * rays->H * rays->S, stream);
}

static int siren_fwd_x3_launch(const cips_siren_weights* w, const float* points, const cips_ray_params* rays, float* feat,
                               float* sigma, float* zout, int B, int P, cips_stream_t stream) {
  if (!w || !feat || !sigma || B <= 0 || P <= 0) return (int)hipErrorInvalidValue;
  FwdX3Args a;
  a.w = *w; a.points = points; a.feat = feat; a.sigma = sigma; a.zout = zout; a.B = B; a.P = P;
  a.rg = RayGen{};
  if (!points) { const int rc = fill_raygen(a.rg, rays); if (rc) return rc; }
  a.chunk = x3_chunk(B, P);
  dim3 grid((P + a.chunk - 1) / a.chunk, B);
  const int smem = O_STG;            // weight images + FiLM vectors + the 4 KiB slot reused for the output bias
  // trig_mode bit 0: hardware sine; bit 1 (A/B runs only): the round-1..4 bf16 operand planes instead of fp16
  x3_pick([&](auto HW_, auto F16_) {
    x3_launch<siren_fwd_x3_kernel<decltype(HW_)::value, decltype(F16_)::value>>(grid, 512, smem, stream, a);
  }, (w->trig_mode & 1) != 0, (w->trig_mode & 2) == 0);
  return CIPS_CHECK_LAUNCH();
}

#include "siren_sigma_x3.inc"

#ifdef CIPS_TUNING
static unsigned long long* g_mprof = nullptr;
extern "C" int cips_march_x3_prof(unsigned long long* host_out) {       // tuning aid: copies the 4x8x8 timestamps
  if (!g_mprof) return (int)hipErrorNotReady;
  return (int)hipMemcpy(host_out, g_mprof, 4 * 8 * 8 * 8, hipMemcpyDeviceToHost);
}
#endif
static int march_fwd_x3_launch(const cips_siren_weights* w, const cips_ray_params* rays, const float* noise,
                               float noise_std, int clamp_mode, int flags, float* fea, float* depth, float* weights,
                               float* feat, float* sigma, float* z, int B, const unsigned char* clamp_in,
                               unsigned char* clamp_out, float* opacity, cips_stream_t stream) {
  if (!w || !fea || B <= 0) return (int)hipErrorInvalidValue;
  MarchArgs a;
  a.w = *w;
  const int rc = fill_raygen(a.rg, rays);
  if (rc) return rc;
  a.noise = noise; a.noise_std = noise_std; a.clamp_mode = clamp_mode; a.flags = flags;
  a.fea = fea; a.depth = depth; a.opacity = opacity; a.weights = weights; a.feat = feat; a.sigma = sigma; a.zout = z; a.B = B;
  a.clamp_pin = clamp_in; a.clamp_rec = clamp_out;
  a.desync = 0; a.one_wave = 0; a.prof = nullptr;
#ifdef CIPS_TUNING
  a.desync = cips_tune_env("CIPS_X3_MDESYNC", 0);
  a.one_wave = cips_tune_env("CIPS_X3_MONE", 0);
  if (cips_tune_env("CIPS_X3_MPROF", 0)) {
    if (!g_mprof && hipMalloc(&g_mprof, 4 * 8 * 8 * 8) != hipSuccess) g_mprof = nullptr;
    a.prof = g_mprof;
  }
#endif
  // a workgroup's 8 waves take 32 rays each: 256-ray chunks keep all of them busy; halve only for small images
  a.rays_per_wg = 256;
  const int n = a.rg.n;
  dim3 grid((n + a.rays_per_wg - 1) / a.rays_per_wg, B);
  const int smem = O_STG;
  x3_pick([&](auto HW_, auto DBG_, auto F16_, auto OPA_) {
    constexpr bool dbg = decltype(DBG_)::value, opa = decltype(OPA_)::value && !dbg;
    x3_launch<siren_march_x3_kernel<decltype(HW_)::value, dbg, decltype(F16_)::value, opa>>(grid, 512, smem, stream, a);
  }, (w->trig_mode & 1) != 0, a.clamp_pin || a.clamp_rec, (w->trig_mode & 2) == 0, a.opacity != nullptr);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_march_fwd_x3(const cips_siren_weights* w, const cips_ray_params* rays, const float* noise,
                                 float noise_std, int clamp_mode, int flags, float* fea, float* depth, float* weights,
                                 float* feat, float* sigma, float* z, int B, const unsigned char* clamp_in,
                                 unsigned char* clamp_out, cips_stream_t stream) {
  return march_fwd_x3_launch(w, rays, noise, noise_std, clamp_mode, flags, fea, depth, weights, feat, sigma, z, B, clamp_in,
                             clamp_out, nullptr, stream);
}

extern "C" int cips_march_fwd_x3_geo(const cips_siren_weights* w, const cips_ray_params* rays, const float* noise,
                                     float noise_std, int clamp_mode, int flags, float* fea, float* depth, float* weights,
                                     float* feat, float* sigma, float* z, int B, const unsigned char* clamp_in,
                                     unsigned char* clamp_out, float* opacity, cips_stream_t stream) {
  if (!w || !rays || !fea || B <= 0) return (int)hipErrorInvalidValue;
  return march_fwd_x3_launch(w, rays, noise, noise_std, clamp_mode, flags, fea, depth, weights, feat, sigma, z, B, clamp_in,
                             clamp_out, opacity, stream);
}
