/*
 * cips3d_hip.h — C-ABI of libcips3d_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the CIPS-3D generator / discriminator hot path
 * (SURVEY.md §8b).  Every entry point takes raw DEVICE pointers (fp32,
 * row-major contiguous unless a leading dimension is given), sizes, scalar
 * parameters and a hipStream_t (passed as void*), returns a hipError_t as int
 * (0 = success), allocates nothing, keeps no state and is thread-safe.
 * The Python host (cips3d_amd/ops.py) binds these through ctypes; the reference
 * binds its two CUDA ops through pybind11 (exp/comm/op/fused_bias_act.cpp:11-21,
 * exp/comm/op/upfirdn2d.cpp:12-23) and everything else through ATen.
 *
 * Each declaration cites the reference code it replaces (paths relative to the
 * reference repo root).
 */
#ifndef CIPS3D_HIP_H
#define CIPS3D_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cips_stream_t; /* hipStream_t */

/* ------------------------------------------------------------------ */
/* library info                                                        */
/* ------------------------------------------------------------------ */
int cips_version(void);          /* ABI version, bumped on signature change */
const char* cips_arch(void);     /* "gfx950" */

/* ------------------------------------------------------------------ */
/* H1  ray set-up                                                      */
/* replaces exp/comm/comm_utils.py:365-412 (get_initial_rays_trig),    */
/*          :416-438 (perturb_points), :584-679 (transform_sampled_points, */
/*          the three bmm's).  Camera sampling / cam2world (O(batch))  */
/*          stay on the host.                                          */
/* ------------------------------------------------------------------ */
/* xg[W], yg[H], zg[S]: torch.linspace grids built by the host (bit-exact
 * with the reference).  zc = -1/tan(fov/2).  cam2world (B,4,4).  jitter U
 * (B,n,S) in [0,1) or NULL (no perturbation).
 * out: points (B,n,S,3) world space, z (B,n,S), dirs (B,n,3) world space. */
int cips_rays_fwd(const float* xg, const float* yg, const float* zg, float zc,
                  const float* cam2world, const float* jitter,
                  float* points, float* z, float* dirs,
                  int B, int H, int W, int S, cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* H2  fused FiLM-SIREN NeRF MLP (3 -> 128 -> 128 -> {sigma, 64 -> 32}) */
/* replaces exp/cips3d/models/generator.py:260-317                     */
/*   (NeRFNetwork.forward_with_frequencies_phase_shifts),              */
/*   exp/comm/models/film_layer.py:78-107 (FiLMLayer.forward),         */
/*   exp/comm/models/nerf_network.py:39-45 (UniformBoxWarp).           */
/* ------------------------------------------------------------------ */
typedef struct cips_siren_weights {
  const float* w0;  /* (128,3)   siren.network.0.linear.weight */
  const float* b0;  /* (128)                                  */
  const float* w1;  /* (128,128) siren.network.1.linear.weight */
  const float* b1;  /* (128)                                  */
  const float* ws;  /* (1,128)   siren.final_layer.weight      */
  const float* bs;  /* (1)                                    */
  const float* wc;  /* (64,128)  siren.color_layer_sine.linear.weight */
  const float* bc;  /* (64)                                   */
  const float* wf;  /* (32,64)   siren.color_layer_linear.0.weight */
  const float* bf;  /* (32)                                   */
  /* per-image FiLM vectors: gain = 15*gain_fc(style)+30, bias = bias_fc(style) */
  const float* g0;  /* (B,128) */
  const float* p0;  /* (B,128) */
  const float* g1;  /* (B,128) */
  const float* p1;  /* (B,128) */
  const float* gc;  /* (B,64)  */
  const float* pc;  /* (B,64)  */
  float box_scale;  /* 2/0.24 (UniformBoxWarp) */
  int trig_mode;    /* bit 0: 0 = Cody-Waite + minimax polynomial sin/cos, 1 = v_sin_f32 / v_cos_f32 (what the Python layer passes);
                       bit 1 (x3 forward kernels only): bf16 operand planes (2^-17) instead of the default fp16 planes (2^-22) —
                       kept for the A/B of tests/test_gpu_kernels.py::test_siren_forward_x3_sigma_is_fp32_class */
} cips_siren_weights;

/* points (B,P,3) -> feat (B,P,32), sigma (B,P). */
int cips_siren_fwd(const cips_siren_weights* w, const float* points,
                   float* feat, float* sigma, int B, int P, cips_stream_t stream);

/* Backward, stage 1 ("data" pass; recomputes the forward in-kernel, saves no
 * forward activations).  In: upstream grads dfeat (B,P,32), dsigma (B,P).
 * Out (HBM staging for the weight-gradient GEMMs; split-bf16 planes x = hi + lo, [B*P][F] row-major,
 *      i.e. the k-major operands of cips_gemm_bf16x3_km with K = points):
 *   h1, h2 (B*P,128), hc (B*P,64)         recomputed activations
 *   da2 (B*P,128), dac (B*P,64)           d loss / d sine-argument of layer 1 / colour layer
 * Out (per-partial-row reductions, partial rows = cips_siren_bwd_rows(B,P),
 *      each row belongs to one image: image = row / (rows/B)):
 *   red (rows, 868): [0,128) sum_p da1 | [128,512) sum_p da1*x_c (c=0..2, 128 each)
 *                    | [512,640) sum_p da2 | [640,704) sum_p dac | [704,832) sum_p dsigma*h2
 *                    | [832,864) sum_p dfeat | [864] sum_p dsigma
 */
int cips_siren_bwd_rows(int B, int P);
int cips_siren_bwd_data(const cips_siren_weights* w, const float* points,
                        const float* dfeat, const float* dsigma,
                        void* h1_hi, void* h1_lo, void* h2_hi, void* h2_lo, void* hc_hi, void* hc_lo,
                        void* da2_hi, void* da2_lo, void* dac_hi, void* dac_lo,
                        float* red, int B, int P, cips_stream_t stream);
/* The same data pass with the five staged tensors written as fp32 rows — h1, h2, da2: (B*P, 128); hc, dac: (B*P, 64) — for
 * weight-gradient contractions on the exact-fp32 MFMA GEMM (cips_gemm_f32, a_kmajor): the all-fp32 leg, in which no split
 * operand takes part (CIPS_SIREN_BWD=staged_f32 with CIPS_INR_MODE=f32 CIPS_SIREN_FWD=f32). */
int cips_siren_bwd_data_f32(const cips_siren_weights* w, const float* points, const float* dfeat, const float* dsigma, float* h1,
                            float* h2, float* hc, float* da2, float* dac, float* red, int B, int P, cips_stream_t stream);

/* Forward on the split-bf16 matrix-core chain (the default of the Python layer; same contract as cips_siren_fwd;
 * ~1e-5 relative instead of ~1e-6, 2.3x faster): */
int cips_siren_fwd_x3(const cips_siren_weights* w, const float* points, float* feat, float* sigma,
                      int B, int P, cips_stream_t stream);

/* Backward, fused bf16x3 form (default): forward recompute, data gradients, all three weight-gradient
 * contractions and every per-feature sum over points in one kernel on v_mfma_f32_32x32x16_bf16 with 3-pass
 * split operands (fp32 accumulate); no activation staging in HBM.
 * chunks = cips_siren_bwd_x3_chunks(B,P) workgroups per image; partials of image b are rows
 * [b*chunks, (b+1)*chunks) of both outputs:
 *   sred  (B*chunks, cips_siren_bwd_x3_sred())  floats [wave w=0..3][row 0..31][col 0..7], then 4 per-wave
 *         sums of dsigma (+4 pad).  Row r of wave w is feature 32w + r; columns:
 *           0 sum_p da1 | 1..3 sum_p da1 * (x, y, z) | 4 sum_p da2 | 5 sum_p dsigma * h2
 *           | 6 sum_p dac (waves 0,1: 64 features) | 7 sum_p dfeat (waves 0 and 2: partial sums, 32 channels)
 *   gpart (B*chunks, cips_siren_bwd_x3_gpart()) floats:
 *         [0,16384)  da2^T h1 (128,128) | [16384,24576) dac^T h2 (64,128)
 *         | [24576,26624) and [26624,28672) two partial dfeat^T hc (32,64)
 * (da1, da2, dac = d loss / d sine argument of layer 0, layer 1, colour layer.)
 */
int cips_siren_bwd_x3_chunks(int B, int P);
int cips_siren_bwd_x3_gpart(void);
int cips_siren_bwd_x3_sred(void);
int cips_siren_bwd_x3(const cips_siren_weights* w, const float* points, const float* dfeat,
                      const float* dsigma, float* sred, float* gpart, int B, int P, cips_stream_t stream);

/* The 16 gradient tensors of the SIREN from the fused backward's per-workgroup partials, in one launch (chain rule of
 * exp/comm/models/film_layer.py:88-107): per-image FiLM gradients dg* / dp* (B,128 | B,64) and the batch-summed weight /
 * bias gradients in the parameters' own shapes. */
typedef struct cips_siren_grads {
  float *dg0, *dp0, *dg1, *dp1, *dgc, *dpc;          /* (B,128) x4, (B,64) x2 */
  float *dw0, *db0, *dw1, *db1, *dws, *dbs, *dwc, *dbc, *dwf, *dbf;   /* (128,3) (128) (128,128) (128) (1,128) (1) (64,128) (64) (32,64) (32) */
} cips_siren_grads;
int cips_siren_bwd_x3_finalize(const cips_siren_weights* w, const float* sred, const float* gpart, int B, int chunks,
                               const cips_siren_grads* out, cips_stream_t stream);

/* Ray parameters for in-kernel point generation (what cips_rays_fwd materialises): the sample point of
 * (image b, ray r, sample s) is recomputed from the linspace grids, the camera matrix and the jitter draw, 4 B per
 * point read instead of 12 B and no (B, n, S, 3) tensor in HBM.  Point index p = r * S + s. */
typedef struct cips_ray_params {
  const float* xg; const float* yg; const float* zg;   /* torch.linspace grids (W), (H), (S) */
  const float* cam2world;                                /* (B,4,4) */
  const float* jitter;                                   /* (B,n,S) uniforms in [0,1) or NULL */
  const float* zvals;                                    /* (B,n,S) depths or NULL; if set: point = camera origin + world ray
                                                            direction * zvals[p] (the resampled fine points,
                                                            exp/dev/nerf_inr/models/generator_nerf_inr.py:590-592) */
  float zc;                                              /* -1/tan(fov/2) */
  int H, W, S;
} cips_ray_params;

/* cips_siren_fwd_x3 with the points generated in-kernel from `rays`; zout (optional, (B,P)) receives their depths. */
int cips_siren_fwd_x3_rays(const cips_siren_weights* w, const cips_ray_params* rays, float* feat, float* sigma,
                           float* zout, int B, cips_stream_t stream);

/* Density only (replaces the SIREN evaluation of exp/pigan/scripts/extract_shapes.py:54-58, sample_generator):
 * sigma (B,P) of cips_siren_fwd_x3 without the colour branch, bit for bit; w->wc, bc, wf, bf, gc, pc are not read and may be NULL.
 * 4 B per point written instead of 132; trig_mode as for cips_siren_fwd_x3, both bits. */
int cips_siren_sigma_x3(const cips_siren_weights* w, const float* points, float* sigma, int B, int P, cips_stream_t stream);
/* A lattice of points given by its three coordinate arrays (device memory, built by the host; the kernel reads them and does
 * no coordinate arithmetic): point p = (i*ny + j)*nz + k is (gx[i], gy[j], gz[k]); nx*ny*nz <= INT_MAX. */
typedef struct cips_grid_params { const float* gx; const float* gy; const float* gz; int nx, ny, nz; } cips_grid_params;
/* the same over the lattice (gx[i], gy[j], gz[k]); sigma (B, nx, ny, nz) — no (B,P,3) points tensor in HBM */
int cips_siren_sigma_x3_grid(const cips_siren_weights* w, const cips_grid_params* grid, float* sigma, int B, cips_stream_t stream);
/* sigma and its gradient w.r.t. the point: sigma (B,P) (may be NULL: not written; otherwise cips_siren_sigma_x3's bit for bit),
 * grad (B,P,3) = d sigma / d point, row-major — the sigma chain, one transposed 128x128 layer on the split MFMAs and the
 * layer-0 cosines, ~5e-6 relative (1e-6 class on the default fp16 planes).  Colour pointers of w are not read and may be NULL. */
int cips_siren_sigma_grad_x3(const cips_siren_weights* w, const float* points, float* sigma /* may be NULL */,
                             float* grad, int B, int P, cips_stream_t stream);
/* the same over the lattice of cips_grid_params; sigma (B, nx, ny, nz) or NULL, grad (B, nx, ny, nz, 3) */
int cips_siren_sigma_grad_x3_grid(const cips_siren_weights* w, const cips_grid_params* grid, float* sigma /* may be NULL */,
                                  float* grad, int B, cips_stream_t stream);

/* The colour of a point: the 32 colour features of cips_siren_fwd_x3 projected to three channels inside the kernel, so that
 * neither the (B,P,32) features nor a second launch exist — 12 B per point written (16 with sigma) instead of 132.  With
 * feat (B,P,32) and sigma (B,P) what cips_siren_fwd_x3 writes for the same w and points, bit for bit, channel c = (r&3) + 8(r>>2) + 4h
 * for h = 0, 1 and r = 0..15:
 *   s_h[j] = fmaf(W[j][c(15,h)], feat[c(15,h)], ... fmaf(W[j][c(0,h)], feat[c(0,h)], 0.f))      sixteen fmaf, r ascending, from zero
 *   y[j]   = (s_0[j] + s_1[j]) + b[j]                                                           j = 0, 1, 2
 *   rgb[j] = tanh_out ? tanhf(y[j]) : y[j]
 * proj_w (3,32) row-major and proj_b (3) are device memory (the generator's auxiliary RGB layer, or any 32 -> 3 map); rgb (B,P,3)
 * fp32 row-major; sigma (B,P) or NULL (not written).  Every element of rgb (and sigma) is written, nothing behind the last.
 * trig_mode as for cips_siren_fwd_x3, both bits.  A NULL w / points / proj_w / proj_b / rgb, B <= 0, B > 65535 or P <= 0 returns
 * hipErrorInvalidValue before any HIP call. */
int cips_siren_rgb_x3(const cips_siren_weights* w, const float* points, const float* proj_w, const float* proj_b, int tanh_out,
                      float* rgb, float* sigma /* may be NULL */, int B, int P, cips_stream_t stream);
/* the same over the lattice of cips_grid_params (point p = (i*ny + j)*nz + k is (gx[i], gy[j], gz[k]), read by the kernel, which does
 * index arithmetic only): rgb (B, nx, ny, nz, 3), sigma (B, nx, ny, nz) or NULL; the points form's values bit for bit.  Also
 * refused: a NULL grid or coordinate array, a non-positive size, nx*ny*nz > INT_MAX. */
int cips_siren_rgb_x3_grid(const cips_siren_weights* w, const cips_grid_params* grid, const float* proj_w, const float* proj_b,
                           int tanh_out, float* rgb, float* sigma /* may be NULL */, int B, cips_stream_t stream);

/* Ray casting of the iso-surface sigma = level: per camera ray of `rays` (n = H*W rays per image; rays->jitter and rays->zvals
 * must be NULL, the walk is on the unjittered grid zg[0..S-1]) the depth of the first crossing, a hit mask, the surface point and
 * the density there.  The point at depth t is camera origin + world ray direction * t (the zvals form of cips_ray_params: the
 * direction rotated first, then scaled — the depth of cips_march_fwd_x3), sigma is cips_siren_sigma_x3's at that point bit for bit.
 * The search, per ray, with s_i = sigma(point(zg[i])):
 *   1. coarse walk i = 0, 1, ...: s_0 >= level -> hit = 2 (the ray starts inside), depth = zg[0]; else the first i >= 1 with
 *      s_{i-1} < level <= s_i -> hit = 1 and the bracket [lo, hi] = [zg[i-1], zg[i]] with s_lo, s_hi; none -> hit = 0, depth = zg[S-1];
 *   2. `refine` (0..32) bisection steps on a hit = 1 ray: mid = 0.5f * (lo + hi); sigma(mid) >= level -> hi = mid, s_hi = sigma(mid),
 *      else lo = mid, s_lo = sigma(mid);
 *   3. one secant step: depth = lo + ((level - s_lo) / (s_hi - s_lo)) * (hi - lo), every operation rounded on its own;
 *   4. one more evaluation at point(depth) -> points (B,n,3) and sigma (B,n) (hit 0 / 2: at their zg[S-1] / zg[0] point).
 * depth (B,n) fp32 and hit (B,n) uint8 are required; sigma, points and trace may be NULL.  Every element is written, nothing behind.
 * trace (B, n, S + refine, 2): every (t, sigma) the ray's wave evaluated, slot i of the coarse walk and S + k of the refinement
 * (a wave stops walking once none of its 32 rays is still searching, and skips the refinement without a hit = 1 ray); entries the
 * wave never evaluated are NaN.  A debug output on an instantiation of its own.  Colour pointers of w are not read.
 * A NULL w / rays / depth / hit / grid / camera, a non-NULL jitter / zvals, S <= 1, B <= 0, B > 65535, H*W > INT_MAX or refine
 * outside 0..32 returns hipErrorInvalidValue before any HIP call. */
int cips_siren_surface_x3(const cips_siren_weights* w, const cips_ray_params* rays, float level, int refine, float* depth,
                          unsigned char* hit, float* sigma /* may be NULL */, float* points /* may be NULL */,
                          float* trace /* may be NULL */, int B, cips_stream_t stream);

/* Indexed triangle meshes of the level set sigma = level of a volume sigma (B, nx, ny, nz) on the lattice of cips_grid_params
 * (strictly increasing coordinates; nx, ny, nz >= 2): marching tetrahedra on the Kuhn decomposition of every cell, no table of
 * cube cases, watertight by construction (replaces the mcubes / skimage step of exp/pigan/scripts/extract_shapes.py on the host).
 * A point is inside iff sigma > level (NaN: outside).  One vertex per lattice edge p -> p + d (d a non-zero 0/1 vector, edge
 * class c = 4 dx + 2 dy + dz - 1 of its lower point p) whose ends differ, at g[a] + t (g[a + d_a] - g[a]) with
 * t = (level - sigma_p) / (sigma_q - sigma_p), ordered by (p, c); triangles ordered by cell, tetrahedron, piece, wound so that
 * (P1 - P0) x (P2 - P0) points towards lower density; faces index the vertices of their own image.  The rules in full: DESIGN.md
 * section 3 "Meshes".  No atomics, fixed positions: two calls on the same input give the same bits.
 * Scratch: device memory, 4-byte aligned, cips_mesh_scratch_bytes(grid, B) bytes (at most 8 per lattice point and image), filled
 * by the count call and read by the emit call.  B <= 65535, 7 nx ny nz <= INT_MAX and 12 (nx-1)(ny-1)(nz-1) <= INT_MAX; anything
 * else, a NULL pointer or a scratch that is too small returns hipErrorInvalidValue (the size query: -1) before any HIP call. */
long long cips_mesh_scratch_bytes(const cips_grid_params* grid, int B);   /* host only: reads the three sizes */
/* count + the two levels of the scan (three launches): totals (B, 2) int64 device memory receives (vertices, triangles) per image */
int cips_mesh_count(const cips_grid_params* grid, const float* sigma, float level, int B, void* scratch, long long scratch_bytes,
                    long long* totals, cips_stream_t stream);
/* vertices + faces (two launches) behind a count call on the same grid, sigma, level, B, scratch and totals: the images' meshes
 * packed one after the other, vertices (sum V, 3) fp32 and faces (sum T, 3) int32.  Nothing beyond the totals is ever written. */
int cips_mesh_emit(const cips_grid_params* grid, const float* sigma, float level, int B, void* scratch, long long scratch_bytes,
                   const long long* totals, float* vertices, int* faces, cips_stream_t stream);

/* cips_siren_bwd_x3 with the points generated in-kernel from `rays` (P = H*W*S points per image). */
int cips_siren_bwd_x3_rays(const cips_siren_weights* w, const cips_ray_params* rays, const float* dfeat,
                           const float* dsigma, float* sred, float* gpart, int B, cips_stream_t stream);

/* Gradient w.r.t. the sample points: the vector-Jacobian product of cips_siren_fwd_x3 with the upstream gradients dfeat (B,P,32)
 * and dsigma (B,P), dpoints (B,P,3) = J^T (dfeat, dsigma), row-major.  A data-only kernel (recompute + four transposed layers on
 * three-pass split bf16, whatever trig_mode's bit 1 says); the weight gradients are cips_siren_bwd_x3's.  Every element of dpoints
 * is written; a point whose dfeat row and dsigma are zero gets exact zeros.  All pointers are required; a NULL pointer or a
 * non-positive size returns hipErrorInvalidValue before any HIP call. */
int cips_siren_bwd_points_x3(const cips_siren_weights* w, const float* points, const float* dfeat, const float* dsigma,
                             float* dpoints /* (B,P,3) */, int B, int P, cips_stream_t stream);
/* the same with the points generated in-kernel from `rays` (coarse: grids + jitter; fine: zvals), P = H*W*S: the points form's
 * result at cips_rays_fwd's points bit for bit. */
int cips_siren_bwd_points_x3_rays(const cips_siren_weights* w, const cips_ray_params* rays, const float* dfeat, const float* dsigma,
                                  float* dpoints /* (B, H*W*S, 3) */, int B, cips_stream_t stream);
/* Per-point gradients -> camera matrix.  The world point is R q + t with q the camera-space sample of `rays` (direction *
 * (depth + jitter offset), or direction * zvals), so d cam2world[:3,:3] = sum_p dpoint q^T and d cam2world[:3,3] = sum_p dpoint.
 * One launch, fixed summation order, no atomics: two calls on the same inputs give the same bits. */
int cips_rays_bwd_cam(const cips_ray_params* rays, const float* dpoints /* (B, H*W*S, 3) */,
                      float* dcam2world /* (B,4,4); row 3 written as zeros */, int B, cips_stream_t stream);

/* The fused backward over a LIST of points per image instead of all P (the points whose upstream gradient is not exactly
 * zero: every output is linear in a point's (dfeat row, dsigma), so the others add nothing).  idx (B,P) int32: image b's
 * point indices, ascending, in idx[b*P + 0 .. count[b]); count (B) int32, 0 <= count[b] <= P; both device memory, read by
 * the kernel (no host read-back: the call can be captured in a graph and replayed on other data).  Same grid, same
 * partial layout and same finalisation as cips_siren_bwd_x3; workgroup c of image b takes the list slots
 * [c*len, min((c+1)*len, count[b])), len = ceil(count[b] / chunks) rounded up to a multiple of 128, and writes all-zero
 * partials when that range is empty.  dfeat / dsigma are read at the listed points ONLY (the other rows may be
 * uninitialised).  With every point listed the result is that of cips_siren_bwd_x3, bit for bit when its chunk divides P. */
int cips_siren_bwd_x3_live(const cips_siren_weights* w, const float* points, const float* dfeat, const float* dsigma,
                           const int* idx, const int* count, float* sred, float* gpart, int B, int P, cips_stream_t stream);
int cips_siren_bwd_x3_rays_live(const cips_siren_weights* w, const cips_ray_params* rays, const float* dfeat,
                                const float* dsigma, const int* idx, const int* count, float* sred, float* gpart, int B,
                                cips_stream_t stream);

/* The list walk with the live samples dealt EVENLY to the workgroups of the launch.  The *_live forms give every image the
 * same `chunks` workgroups, so a workgroup's trip count follows its own image's live share and the launch ends in a tail of
 * the dense images; here the G = B * chunks workgroups (same grid, same sizes of sred / gpart) are dealt in proportion to the
 * images' rounds of 128 list slots.  Three calls on one stream, no host read-back anywhere (graph-capturable):
 *
 * cips_siren_bwd_x3_live_plan writes the partition (one small workgroup).  With r_b = ceil(count[b] / 128) and Rt = sum r_b,
 *   T = the smallest integer >= max(1, ceil(Rt / G)) with sum_b max(1, ceil(r_b / T)) <= G; image b gets
 *   n_b = max(1, ceil(r_b / T)) workgroups with the flat ids first_b = sum_{b' < b} n_b' .. first_b + n_b - 1, its rounds dealt
 *   as evenly as integers allow (the first r_b % n_b of them take one round more); slots = rounds * 128, the end clipped to
 *   count[b].  An image without live points keeps one workgroup with an empty range; ids from sum n_b up to G are idle.
 *   seg (G, 4) int32: image (-1: idle), first slot, end slot, rounds, per flat id;  img (B, 2) int32: first_b, n_b.
 *   count[b] is clamped to [0, P].  Equal counts give the partition of the *_live forms.
 *   cips_siren_bwd_x3_live_plan_host evaluates the same rule on host arrays (no device access).
 * cips_siren_bwd_x3_live_even / _rays_live_even: the *_live calls with `seg`.  Workgroup (x, y) has the flat id
 *   y * chunks + x, walks the slots seg says of image seg says, and writes its partials to row = flat id of sred / gpart
 *   (all-zero partials for an empty range).  Idle ids write nothing: their rows stay as they were.
 * cips_siren_bwd_x3_reduce_segments: sred_out (B, sred()) and gpart_out (B, gpart()), out[b] = the sum of rows
 *   first_b .. first_b + n_b - 1 in ascending order (deterministic; idle rows are never read).  cips_siren_bwd_x3_finalize
 *   then takes them with chunks = 1. */
int cips_siren_bwd_x3_live_plan(const int* count, int B, int P, int* seg, int* img, cips_stream_t stream);
int cips_siren_bwd_x3_live_plan_host(const int* count, int B, int P, int* seg, int* img);
int cips_siren_bwd_x3_live_even(const cips_siren_weights* w, const float* points, const float* dfeat, const float* dsigma,
                                const int* idx, const int* count, const int* seg, float* sred, float* gpart, int B, int P,
                                cips_stream_t stream);
int cips_siren_bwd_x3_rays_live_even(const cips_siren_weights* w, const cips_ray_params* rays, const float* dfeat,
                                     const float* dsigma, const int* idx, const int* count, const int* seg, float* sred,
                                     float* gpart, int B, cips_stream_t stream);
int cips_siren_bwd_x3_reduce_segments(const float* sred, const float* gpart, const int* img, int B, float* sred_out,
                                      float* gpart_out, cips_stream_t stream);
/* cips_siren_bwd_x3_reduce_segments + cips_siren_bwd_x3_finalize (chunks = 1) in one launch: the finalisation sums image
 * b's rows first_b .. first_b + n_b - 1 of sred / gpart itself, in ascending order.  The 16 gradients are those of the two
 * calls bit for bit; the per-image sums never reach memory. */
int cips_siren_bwd_x3_finalize_segments(const cips_siren_weights* w, const float* sred, const float* gpart, const int* img,
                                        int B, const cips_siren_grads* out, cips_stream_t stream);

/* Fused ray-march for NON-hierarchical sampling: ray set-up + FiLM-SIREN + alpha-composite in one kernel that walks
 * the samples along the ray (a wave owns 32 rays, one lane pair per ray; the running transmittance / feature / depth
 * accumulators live in registers).  Replaces, for hierarchical_sample=False,
 *   exp/comm/comm_utils.py:365-438, 584-679 (rays), exp/cips3d/models/generator.py:260-317 (SIREN),
 *   exp/pigan/pigan_utils.py:212-273 (fancy_integration; the merge of generator.py:1733-1752 is the identity).
 * noise (B,n,S) standard normals or NULL; clamp_mode 0 relu / 1 softplus; flags bit0 last_back, bit1 white_back.
 * out: fea (B,n,32), depth (B,n) [may be NULL]; optional: weights (B,n,S), and — for a training forward whose backward
 * needs them — the per-sample feat (B,P,32), sigma (B,P), z (B,P).  With those NULL the kernel moves 4*S + 132 B per ray
 * (SURVEY.md §8d-iii).  clamp_in / clamp_out: optional (B*n, S) branch masks of the relu clamp, as in cips_composite_fwd
 * (a separate instantiation of the kernel: the production launch, both NULL, keeps its registers). */
int cips_march_fwd_x3(const cips_siren_weights* w, const cips_ray_params* rays, const float* noise, float noise_std,
                      int clamp_mode, int flags, float* fea, float* depth, float* weights, float* feat, float* sigma,
                      float* z, int B, const unsigned char* clamp_in, unsigned char* clamp_out, cips_stream_t stream);
/* cips_march_fwd_x3 with one more optional output, opacity (B,n): the ray's sum of weights as the kernel accumulates it,
 * stored before the last_back / white_back adjustments (pigan_utils.py's weights_sum; under last_back it is NOT the constant
 * 1).  The store is in instantiations of their own: with opacity NULL this launches exactly what cips_march_fwd_x3 launches
 * and stores the same bits, and the production kernel keeps its registers.  Every other output is the same bits either way.
 * Validated before any HIP call: w, rays, fea NULL, B <= 0 or ray parameters fill_raygen refuses -> hipErrorInvalidValue. */
int cips_march_fwd_x3_geo(const cips_siren_weights* w, const cips_ray_params* rays, const float* noise, float noise_std,
                          int clamp_mode, int flags, float* fea, float* depth, float* weights, float* feat, float* sigma,
                          float* z, int B, const unsigned char* clamp_in, unsigned char* clamp_out, float* opacity,
                          cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* H3  hierarchical resampling + merge + alpha-composite               */
/* ------------------------------------------------------------------ */
/* Coarse weights + inverse-CDF resampling.
 * replaces exp/dev/nerf_inr/models/generator_nerf_inr.py:537-598
 *   (get_fine_points_and_direction), exp/pigan/pigan_utils.py:164-209
 *   (sample_pdf) and the weights part of :212-273 (fancy_integration).
 * sigma (R,S), z (R,S), noise (R,S) or NULL (noise already scaled by
 * noise_std is NOT assumed: kernel applies sigma + noise*noise_std),
 * u (R,S) uniforms, origins (B,3), dirs (R,3) with R = B*n rays.
 * out: fine_z (R,S), fine_pts (R,S,3); optional debug outs (may be NULL):
 * weights (R,S), cdf (R,S-1), inds (R,S) int64 (searchsorted result).
 * clamp_mode: 0 = relu, 1 = softplus.
 * cdf_in (optional, (R,S-1)): take the cdf from the caller instead of computing it — the "bit-exact integer bookkeeping
 * on identical float inputs" contract: with the reference's cdf and u the indices must equal
 * torch.searchsorted's exactly.
 * rays (optional): ray directions and origins are recomputed from the ray parameters (origins / dirs may then be NULL,
 * and fine_pts may be NULL when the fine pass regenerates its points from fine_z, cips_ray_params.zvals). */
int cips_resample_fwd(const float* sigma, const float* z, const float* noise, float noise_std,
                      const float* u, const float* origins, const float* dirs,
                      float* fine_z, float* fine_pts,
                      float* weights_out, float* cdf_out, long long* inds_out,
                      int B, int n, int S, int clamp_mode, const float* cdf_in, const cips_ray_params* rays,
                      cips_stream_t stream);

/* Merge (coarse + fine, ascending z) and alpha-composite.
 * replaces exp/cips3d/models/generator.py:1733-1752 (cat/sort/gather) and
 *   exp/pigan/pigan_utils.py:212-273 (fancy_integration).
 * feat_c (R,S,32), sig_c (R,S), z_c (R,S); fine set same shapes or NULL
 * (then E = S, no merge).  noise (R,E) in SORTED order or NULL.
 * out: fea (R,32), depth (R), weights (R,E) sorted order, order (R,E) int32
 * (index into [fine(0..S-1), coarse(S..2S-1)] like torch.cat([fine, coarse]);
 * for the non-hierarchical case the identity), zsorted (R,E) (may be NULL).
 * flags: bit0 last_back, bit1 white_back.
 * clamp_in / clamp_out (optional, (R,E) bytes, relu clamp only; no reference counterpart — pigan_utils.py:246-252 is the
 * clamp they describe): relu(sigma + nerf_noise * eps) is a discontinuity of the gradient — two evaluations whose
 * pre-activations differ by rounding may take different branches.  With clamp_in the branch of sample (ray, sorted
 * position k) is clamp_in[ray*E + k] (0 = clamped, else the linear branch) instead of the sign of the value computed here;
 * clamp_out receives the branch taken.  Both NULL in production; the parity tests pin the CPU oracle's branches through
 * them.  They are arguments of the call (round 5; rounds 3-4 had a process-global hook): the library keeps no state. */
int cips_composite_fwd(const float* feat_c, const float* sig_c, const float* z_c,
                       const float* feat_f, const float* sig_f, const float* z_f,
                       const float* noise, float noise_std,
                       float* fea, float* depth, float* weights, int* order, float* zsorted,
                       int R, int S, int clamp_mode, int flags, const unsigned char* clamp_in, unsigned char* clamp_out,
                       cips_stream_t stream);

/* Backward of the above w.r.t. feat/sigma of both sample sets (z has no grad:
 * fine z is detach()ed, generator_nerf_inr.py:575-579; coarse z is an input).
 * dfea (R,32) upstream.  Re-reads the forward inputs (no saved activations
 * besides `order`; order == NULL with no fine set means the identity).  clamp_in as in cips_composite_fwd. */
int cips_composite_bwd(const float* feat_c, const float* sig_c, const float* z_c,
                       const float* feat_f, const float* sig_f, const float* z_f,
                       const float* noise, float noise_std, const int* order,
                       const float* dfea,
                       float* dfeat_c, float* dsig_c, float* dfeat_f, float* dsig_f,
                       int R, int S, int clamp_mode, int flags, const unsigned char* clamp_in, cips_stream_t stream);

/* cips_composite_bwd that also reports which samples are live: live_c (R,S) / live_f (R,S; with a fine set) receive one
 * byte per sample in the order of dfeat_* / dsig_*: 1 iff the weight the sample's dfeat row is scaled with is != 0 or the
 * dsigma stored for it is != 0 (a NaN is != 0), else 0.  A relu-clamped sample (sigma + noise <= 0) has alpha == 0, so
 * both vanish; softplus comes out all ones, and so does the last sample under last_back (bit 0 of flags).  The dfeat rows
 * of samples reported 0 are NOT written (undefined); every dsigma is.  live_c == NULL (then live_f must be too): exactly
 * cips_composite_bwd. */
int cips_composite_bwd_live(const float* feat_c, const float* sig_c, const float* z_c,
                            const float* feat_f, const float* sig_f, const float* z_f,
                            const float* noise, float noise_std, const int* order,
                            const float* dfea,
                            float* dfeat_c, float* dsig_c, float* dfeat_f, float* dsig_f,
                            unsigned char* live_c, unsigned char* live_f,
                            int R, int S, int clamp_mode, int flags, const unsigned char* clamp_in, cips_stream_t stream);

/* The list form of a mask: for each of B images with P mask bytes, idx[b*P + j] (j < count[b]) = the ascending indices of
 * its non-zero bytes, count[b] their number; idx entries from count[b] on are left as they were.  Deterministic (the order
 * is the index order, no atomics), one launch, one workgroup per image. */
int cips_live_points(const unsigned char* live, int B, int P, int* idx, int* count, cips_stream_t stream);

/* The live samples of the flat path (no fine set) decided from the FORWARD pass' values.  One rule, evaluated on
 * x = sigma + noise * noise_std as cips_composite_bwd forms it: can that backward give sample k of a ray a non-zero dfeat
 * row or a non-zero dsigma, whatever dfea is?  relu: !(x <= 0) (a NaN counts as live), and the ray's last sample under
 * last_back (bit 0 of flags; white_back adds none); softplus: every sample.  On finite z, features and dfea this lists a
 * superset of the samples cips_composite_bwd_live reports 1 (equal except where w or dsigma underflow to zero behind an open
 * clamp).
 * cips_composite_has_dead_samples(clamp_mode): 1 iff the rule can leave a sample out under that clamp (relu), else 0.
 * cips_live_points_clamp: cips_live_points with the rule in place of a mask byte: sigma (B, n*S), noise (B, n*S) or NULL,
 *   P = n*S points per image (must fit an int), sample k = p % S of ray p / S.  Same outputs and ordering guarantee.
 * cips_composite_bwd_listed: cips_composite_bwd without a fine set, writing the dfeat row and the dsigma of exactly the
 *   samples the rule lists (the same bits cips_composite_bwd stores there); the rows and dsigma of the others are NOT
 *   written.  Every feature row is still read.  No clamp_in: a pinned clamp takes cips_composite_bwd_live. */
int cips_composite_has_dead_samples(int clamp_mode);
int cips_live_points_clamp(const float* sigma, const float* noise, float noise_std, int B, int n, int S, int clamp_mode,
                           int flags, int* idx, int* count, cips_stream_t stream);
int cips_composite_bwd_listed(const float* feat, const float* sigma, const float* z, const float* noise, float noise_std,
                              const float* dfea, float* dfeat, float* dsigma, int R, int S, int clamp_mode, int flags,
                              cips_stream_t stream);

/* Differentiable depth and opacity.  The `_geo` forms take the arguments of the entry point they are named after, then the
 * new ones, then the stream.
 *
 * cips_composite_fwd_geo: cips_composite_fwd with one more optional output, opacity (R) = sum_k w_k, stored before the
 *   last_back / white_back adjustments (pigan_utils.py's weights_sum: under last_back it is not the constant 1).  Every other
 *   output is cips_composite_fwd's bit for bit, with or without it.
 *   hipErrorInvalidValue, before any HIP call: R <= 0, S < 1, feat_c / sig_c / z_c / fea NULL, a feat_f without sig_f and z_f.
 *
 * cips_composite_bwd_geo / _live_geo / _listed_geo: the three compositing backwards with the upstream gradients ddepth (R)
 *   and dopacity (R) of the ray's depth and opacity next to dfea; either may be NULL (zeros).  With BOTH NULL they launch the
 *   kernel instantiation the entry points without them launch and store exactly their bits (the two terms are a template
 *   parameter of the kernel: that instantiation has no trace of them).  Otherwise, with
 *       depth = sum_k w_k z_k + [last_back] (1 - sum w) z_last,   opacity = sum_k w_k,
 *   the per-sample scalar of the reverse scan, dL/dw_k, gains two terms:
 *       dL/dw_k = (G . f_k + gd z_k) - [last_back] (G . f_last + gd z_last) - [white_back] sum(G) + go.
 *   last_back: the depth upstream sees the topped-up last weight like the features do; the opacity upstream does not (opacity
 *   is taken before the top-up).  white_back touches neither.  Everything behind dL/dw_k is unchanged: dalpha = T_k (dL/dw_k -
 *   Q), the clamp's gradient, and the dfeat rows w_k G, which do not depend on gd / go at all — only dsigma does.  z gets no
 *   gradient (depths are constants, as in the reference).
 *   Liveness keeps its meaning: a relu-clamped sample has alpha = 0 and d alpha / dx = 0 whatever the upstream is, so its row
 *   and its dsigma stay zero, _live_geo's mask follows the same (w != 0) || (dsigma != 0), _listed_geo writes by the same rule,
 *   and cips_live_points_clamp's lists remain a superset of what these backwards can make non-zero.
 *   hipErrorInvalidValue, before any HIP call: R <= 0, S < 1; feat / sigma / z / dfea / dfeat / dsigma (of the coarse set, and
 *   with a feat_f of the fine set, and then `order`) NULL; a live_f without a live_c, or with a fine set a live_c without a
 *   live_f. */
int cips_composite_fwd_geo(const float* feat_c, const float* sig_c, const float* z_c,
                           const float* feat_f, const float* sig_f, const float* z_f,
                           const float* noise, float noise_std,
                           float* fea, float* depth, float* weights, int* order, float* zsorted,
                           int R, int S, int clamp_mode, int flags, const unsigned char* clamp_in, unsigned char* clamp_out,
                           float* opacity, cips_stream_t stream);
int cips_composite_bwd_geo(const float* feat_c, const float* sig_c, const float* z_c,
                           const float* feat_f, const float* sig_f, const float* z_f,
                           const float* noise, float noise_std, const int* order,
                           const float* dfea,
                           float* dfeat_c, float* dsig_c, float* dfeat_f, float* dsig_f,
                           int R, int S, int clamp_mode, int flags, const unsigned char* clamp_in,
                           const float* ddepth, const float* dopacity, cips_stream_t stream);
int cips_composite_bwd_live_geo(const float* feat_c, const float* sig_c, const float* z_c,
                                const float* feat_f, const float* sig_f, const float* z_f,
                                const float* noise, float noise_std, const int* order,
                                const float* dfea,
                                float* dfeat_c, float* dsig_c, float* dfeat_f, float* dsig_f,
                                unsigned char* live_c, unsigned char* live_f,
                                int R, int S, int clamp_mode, int flags, const unsigned char* clamp_in,
                                const float* ddepth, const float* dopacity, cips_stream_t stream);
int cips_composite_bwd_listed_geo(const float* feat, const float* sigma, const float* z, const float* noise, float noise_std,
                                  const float* dfea, float* dfeat, float* dsigma, int R, int S, int clamp_mode, int flags,
                                  const float* ddepth, const float* dopacity, cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* generic batched fp32 GEMM on v_mfma_f32_32x32x2_f32 with fused epilogues */
/* the workhorse under H4 (bmm in exp/comm/models/mod_conv_fc.py:489),  */
/* the SIREN weight gradients, and H5 convolutions (im2col GEMM).       */
/* ------------------------------------------------------------------ */
typedef struct cips_gemm_desc {
  /* C[b] (M,N) = epilogue( A[b] (M,K) @ B[b] (K,N) ) */
  const float* A; const float* B; float* C;
  int M, N, K;
  int lda, ldb, ldc;
  long long strideA, strideB, strideC; /* elements between batches */
  int batch;
  int a_kmajor;          /* 0: A stored (M,K) row-major; 1: A stored (K,M) row-major ("TN") */
  int b_nmajor;          /* 0: B stored (K,N) row-major; 1: B stored (N,K) row-major ("NT") */
  /* ---- epilogue (all optional; every aux matrix uses ldc / strideC addressing) ---- */
  float alpha;           /* acc *= alpha (0 is treated as 1) */
  const float* bias;     /* (N) added after alpha */
  const float* bias_m;   /* (M) per-row bias (conv output channel when C is (O, Ho*Wo)) */
  int act;               /* 0 none; 1 leaky_relu(slope) ; 2 leaky_relu(slope)*act_gain */
  float slope; float act_gain;
  const float* resid;    /* after act: C2 = act(..) + resid */
  float* C2;             /* second output (written only if non-NULL) */
  const float* add;      /* before mask: s = acc + add */
  const float* rgb_g;    /* (batch*M,3) with row stride 3: s += rgb_g[m,:] @ rgb_w[:, n] */
  const float* rgb_w;    /* (3,N) row-major */
  float* C_unmasked;     /* if non-NULL, s stored here before masking */
  const float* mask;     /* C = s * (mask > 0 ? 1 : slope) * (act==2? act_gain:1) */
} cips_gemm_desc;

int cips_gemm_f32(const cips_gemm_desc* d, cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* fp32-grade GEMM on the bf16 matrix cores by 3-pass operand splitting */
/* ("bf16x3": x = hi + lo in two bf16 planes; a*b ~ ah*bh + ah*bl + al*bh, */
/* fp32 accumulate; ~1e-5 relative per layer against the 1e-3 parity bar). */
/* Used for the 17 modulated 512x512 layers of the CIPS INR head        */
/* (torch.bmm in exp/comm/models/mod_conv_fc.py:489 and its backward).  */
/* ------------------------------------------------------------------ */
typedef struct cips_gemm_x3_desc {
  /* C[b][m][n] = epilogue( sum_k A[b][m][k] * B[b][n][k] ): both operands contraction-contiguous ("NT"),
   * each given as two bf16 planes (uint16 storage). */
  const void* A_hi; const void* A_lo; const void* B_hi; const void* B_lo;
  int M, N, K;                 /* K % 32 == 0 */
  int lda, ldb;                /* elements; multiples of 8 */
  long long strideA, strideB;  /* elements between batches; multiples of 8 */
  int batch;
  /* outputs, any may be NULL */
  float* C; int ldc; long long strideC;                /* fp32 row-major */
  void* P_hi; void* P_lo; int ldp; long long strideP;  /* split planes, row-major [M][ldp] */
  void* T_hi; void* T_lo; int ldt; long long strideT;  /* split planes, transposed [N][ldt] */
  void* mask_out;              /* bf16 plane [M][ldp] of the value right after `act` (LeakyReLU gate source) */
  /* epilogue, in this order: +add, +rgb term, store C_unmasked, *gate(mask), act, store mask_out, +res, outputs */
  const float* add;            /* fp32 [M][ldc] */
  const float* rgb_g; const float* rgb_w;   /* (batch*M,3), (3,N) */
  float* C_unmasked;           /* fp32 [M][ldc] */
  const void* mask;            /* bf16 plane [M][ldp]: v *= (mask > 0 ? 1 : slope) */
  int act; float slope;        /* act 1: leaky_relu(slope) */
  const void* res_hi; const void* res_lo;   /* residual planes [M][ldp], added after act */
  /* gate planes as BIT planes (1 bit per element, bit c&7 of byte [m][c>>3], rows of ldp/8 bytes, batch stride
   * strideP/8): bit 0 of gate_bits = `mask` is one, bit 1 = `mask_out` is written as one (value > 0).  Needs
   * N % 32 == 0, ldp % 32 == 0, strideP % 32 == 0.  0 = bf16 planes as above. */
  int gate_bits;
  /* ToRGB forward folded into the epilogue (ABI 3; generator.py:949-1006, 1139-1144: rgb += out . T^T + tau): with
   * torgb_w (3, N) set, every 128-column block j of the FINAL value of a row (what P receives) leaves the partial
   * products  torgb_part[j][b*M + m][c] = sum_{n in block j} value[m][n] * torgb_w[c][n]  (c = 0..2, 4 floats per row,
   * the 4th is 0); torgb_part holds (N/128) * batch*M * 4 floats.  cips_torgb_finish adds the blocks in order, the
   * bias and (optionally) the running rgb.  Only the 256x256-tile v3 kernel implements it: cips_gemm_bf16x3 returns
   * hipErrorNotSupported for any other shape (use cips_torgb_fwd_x3 on the planes then). */
  const float* torgb_w; float* torgb_part;
  /* The addend as the split planes of a GATED tensor (ABI 4): the skip gradient of the head's backward is the previous
   * layer's un-gated gradient D, of which that layer already wrote the gated planes P = D * (gate ? 1 : slope) for its
   * own GEMMs.  With addp_hi / addp_lo ([M][ldp] planes, batch stride strideP) and addp_gate (the bit plane of that
   * gate, same layout as `mask` with gate_bits bit 0) set, the epilogue adds  (hi + lo) * (bit ? 1 : addp_gain)
   * (addp_gain = 1 / slope) in place of `add` — D is recovered to the planes' 2^-17 relative precision and the
   * producer need not write, nor this kernel read, a separate fp32 copy (C_unmasked / add: 2 x 4 bytes per element
   * saved).  Exclusive with `add`; needs `mask` as a bit plane; v3 kernel only (hipErrorNotSupported elsewhere). */
  const void* addp_hi; const void* addp_lo; const void* addp_gate; float addp_gain;
  /* Kernel choice (ABI 5; replaces the process-global cips_gemm_bf16x3_set_wide and the CIPS_X3_* environment variables):
   * 0 = automatic (production): 256x256 tiles — the v3 schedule for interior shapes, else the ragged-shape wide kernel —
   * for problems that fill the chip with them, the 256x128 kernel otherwise; 1 = the 256x128 kernel only; 2 = 256x256 tiles
   * whenever a kernel takes the shape; 3 = like 2 but never the v3 schedule.  1-3 serve the parity tests of each kernel.
   * The K-major entry points read it the same way (1: never the 256x256-tile kernel, 2 / 3: whenever the shape allows). */
  int kernel;
  /* Orientation of the B planes.  0: [N][ldb], contraction-contiguous, as stated at the top.  1: row-major [K][ldb] with
   * ldb >= N, ldb % 8 == 0, batch stride strideB (0 = shared) — the product is still C = A . B over K.  The head's dX GEMMs
   * pass the forward's weight planes wbt (B, out, in) this way instead of a transposed copy: the kernel stages the B tile as
   * k-rows and builds its MFMA fragments with LDS transpose reads, same MFMA order, bit-identical results.  Only the
   * 256x256-tile v3 kernel of cips_gemm_bf16x3 implements it, for the epilogues of the backward: gate bit plane in / planes
   * out (without or with the planes addend addp_*, rgb term included), and the plain fp32 C.  Every other descriptor with
   * b_kmajor = 1 — another shape, kernel = 1 or 3, another epilogue, the single-pass and K-major entry points — returns
   * hipErrorNotSupported and writes nothing; cips_gemm_bf16x3_takes_bkmajor tells beforehand. */
  int b_kmajor;
} cips_gemm_x3_desc;

int cips_gemm_bf16x3(const cips_gemm_x3_desc* d, cips_stream_t stream);
/* 1 when cips_gemm_bf16x3 would run this descriptor with its B planes read k-major (b_kmajor = 1; v3 kernel only) */
int cips_gemm_bf16x3_takes_bkmajor(const cips_gemm_x3_desc* d);
/* 1 when cips_gemm_bf16x3 would run this descriptor on the v3 kernel (the only one with the fused ToRGB partials) */
int cips_gemm_bf16x3_fuses_torgb(const cips_gemm_x3_desc* d);
/* 1 when cips_gemm_bf16x3 would take this descriptor's planes addend (addp_*; v3 kernel only) */
int cips_gemm_bf16x3_takes_addp(const cips_gemm_x3_desc* d);
/* rgb[m][c] = (accumulate ? rgb[m][c] : 0) + bias[c] + sum_j part[j][m][c];  part (nblocks, M, 4), rgb (M, 3) */
int cips_torgb_finish(const float* part, int nblocks, const float* bias, float* rgb, long long M, int accumulate,
                      cips_stream_t stream);
/* K-major form: C[b][m][n] = sum_k A[b][k][m] * B[b][k][n] (A planes [K][lda], B planes [K][ldb]: the row-major
 * activation / gradient planes themselves; LDS transpose reads build the fragments).  fp32 C output only. */
int cips_gemm_bf16x3_km(const cips_gemm_x3_desc* d, cips_stream_t stream);
/* Up to four K-major problems of identical shape (M, N, K, batch, leading dimensions, strides) in one launch of
 * 256x256 tiles; only the operand planes and C differ.  hipErrorNotSupported (801) when the shapes do not qualify:
 * issue them one by one with cips_gemm_bf16x3_km then. */
int cips_gemm_bf16x3_km_grouped(const cips_gemm_x3_desc* descs, int ngroups, cips_stream_t stream);

/* Single-pass forms of the five entry points above ("bf16": the AMP-class arithmetic, operands rounded to bf16, fp32
 * accumulate):  sum_k A_hi * B_hi  only.  Same descriptor, same validation and return codes, same epilogues on the fp32
 * accumulator, same hi / lo OUTPUT planes; A_lo and B_lo are ignored and may be NULL.  No 3-pass kernel is ever used: the NT
 * form runs on the 256x256-tile kernel (interior shapes with K % 128 == 0; the only one with the fused ToRGB partials and the
 * planes addend, as the queries report) or on the 256x128 kernel, the K-major forms on the 256x256-tile kernel (K % 64 == 0,
 * K >= 128; the grouped entry returns hipErrorNotSupported otherwise) or on the 256x128 / 128x128 kernels.  Relative error
 * of a product sum ~2^-9 per operand: three orders of magnitude coarser than cips_gemm_bf16x3. */
int cips_gemm_bf16(const cips_gemm_x3_desc* d, cips_stream_t stream);
int cips_gemm_bf16_fuses_torgb(const cips_gemm_x3_desc* d);
int cips_gemm_bf16_takes_addp(const cips_gemm_x3_desc* d);
int cips_gemm_bf16_km(const cips_gemm_x3_desc* d, cips_stream_t stream);
int cips_gemm_bf16_km_grouped(const cips_gemm_x3_desc* descs, int ngroups, cips_stream_t stream);

/* Implicit-GEMM convolution on the split-bf16 NT kernel (EqualConv2d forward, exp/cips3d/models/discriminator.py:40-48,
 * and — with the flipped, transposed weights — its data gradient at stride 1):
 *   y[b][o][oy*Wo+ox] = sum_{ky,kx,c} w[o][(ky*kw+kx)*C + c] * x[b][oy*stride-pad+ky][ox*stride-pad+kx][c]
 * x: NHWC split planes of B*H*W + 1 rows of C (the extra LAST ROW MUST BE ZERO: it stands in for the padding),
 * w: planes [O][kh*kw*C]; y: fp32 NCHW (B, O, Ho, Wo).  C % 32 == 0, Ho*Wo % 8 == 0; else hipErrorNotSupported. */
typedef struct cips_conv_x3_desc {
  const void* w_hi; const void* w_lo;
  const void* x_hi; const void* x_lo;
  float* y;
  int B, C, H, W, O, kh, kw, stride, pad;
  int ksplit;      /* <= 1: off.  > 1: the contraction (kh*kw*C) is cut into ksplit ranges computed by different workgroups */
  float* part;     /* (small output planes leave most CUs idle otherwise); part: ksplit * B*O*Ho*Wo floats of scratch, */
                   /* summed into y by the call.  cips_conv2d_x3_ksplit proposes a count for (B, O, N = Ho*Wo, K).   */
  const float* bias;  /* optional (O): added to every pixel of channel o                                                  */
  int act;            /* 0: none; 1: y = leaky_relu(y + bias, slope) * act_scale — EqualConv2d followed by FusedLeakyReLU */
  float slope, act_scale;   /* (discriminator.py:205-215, fused_act.py:47-86) in the GEMM epilogue                       */
} cips_conv_x3_desc;
int cips_conv2d_x3(const cips_conv_x3_desc* d, cips_stream_t stream);
int cips_conv2d_x3_ksplit(int B, int O, int N, int K);
/* Data gradient of a STRIDE-2, UNPADDED convolution (the EqualConv2d behind a Blur: exp/cips3d/models/discriminator.py:190-203)
 * without col2im: input pixel (P, Q) only receives the taps ky = P mod 2 (+2, ...), kx = Q mod 2 (+2, ...), so each of the four
 * parity classes (a, b) = (P mod 2, Q mod 2) is a small STRIDE-1 convolution over dy with its own filter bank:
 *   dxp_ab[i][c][U*Ws_b + V] = sum_{ty < Ta, tx < Tb, o} bank_ab[c][(ty*Tb + tx)*O + o] * dy[i][U - (Ta-1) + ty][V - (Tb-1) + tx][o]
 *                            = dx[i][c][2U + a][2V + b]
 * with Ta = ceil((kh-a)/2), Tb = ceil((kw-b)/2), Hs_a = ceil((H-a)/2), Ws_b = ceil((W-b)/2) and
 *   bank_ab[c][(ty*Tb + tx)*O + o] = w[o][c][a + 2(Ta-1-ty)][b + 2(Tb-1-tx)]   (planes, row pitch Ta*Tb*O, at element offset w_off[2a+b]).
 * All four run in ONE persistent launch of the implicit-GEMM kernel (longest contraction first).  dy: NHWC split planes
 * [B*Ho*Wo + 1][O] with a ZERO LAST ROW (Ho = (H-kh)/2 + 1).  Output: four compact blocks, class (a, b) at element offset
 * out_off[2a+b] of dxp as fp32 (B, C, Np_ab), Np_ab = Hs_a*Ws_b rounded up to a multiple of 8 (the padding elements are written
 * as zeros); cips_upfirdn2d_parity reads them in place of the interleaved (B, C, H, W) tensor.  O % 32 == 0, C % 8 == 0. */
typedef struct cips_conv_dgrad_s2_desc {
  const void* w_hi; const void* w_lo;
  const void* dy_hi; const void* dy_lo;
  float* dxp;
  int B, C, H, W, O, kh, kw;         /* H, W: the convolution's INPUT size */
  long long w_off[4], out_off[4];
} cips_conv_dgrad_s2_desc;
int cips_conv2d_x3_dgrad_s2(const cips_conv_dgrad_s2_desc* d, cips_stream_t stream);
/* Operand planes of convolution WEIGHTS for cips_conv2d_x3 / cips_conv2d_x3_dgrad_s2, up to cips_conv_weight_prep_max_jobs() layers
 * per launch (EqualConv2d: `weight * scale`, exp/cips3d/models/discriminator.py:33, 44): w (O, C, kh, kw) fp32 ->
 *   fwd_hi / fwd_lo: planes [O][kh*kw*C], contraction index (ky, kx, c)                                   (NULL: not written)
 *   alt_kind 1: alt_hi / alt_lo = planes [C][kh*kw*O] of the flipped, channel-transposed bank: element (c, (kh-1-ky, kw-1-kx, o))
 *               — the stride-1 data gradient's filter bank;
 *   alt_kind 2: alt_hi / alt_lo = the four parity banks of cips_conv2d_x3_dgrad_s2 at element offsets bank_off[2a+b];
 *   alt_kind 0: no alternate form.
 * hi = bf16(w * scale) (round to nearest even), lo = bf16(w * scale - hi): the values of a separate multiply + cips_split_planes. */
#define CIPS_WPREP_MAX_JOBS 24
typedef struct cips_wprep_job {
  const float* w;
  void* fwd_hi; void* fwd_lo;
  void* alt_hi; void* alt_lo;
  float scale;
  int O, C, kh, kw, alt_kind;
  int bank_off[4];
} cips_wprep_job;
int cips_conv_weight_prep_max_jobs(void);
int cips_conv_weight_prep_batch(const cips_wprep_job* jobs, int njobs, cips_stream_t stream);
/* Weight gradient of the same convolution on the K-major kernel (contraction over all B*Ho*Wo output pixels, split in
 * `nchunks` ranges whose partial sums the caller adds):
 *   part[chunk][ky*kw+kx][o][c] = sum_{q in chunk} dy[q][o] * x[pixel(q)*stride - pad + (ky,kx)][c]
 * dy: NHWC split planes [B*Ho*Wo][O]; x: NHWC split planes [B*H*W + 1][C] with a ZERO LAST ROW; part: fp32
 * (nchunks, kh*kw, O, C).  The pixel range is cut at 32-row granularity into nchunks nearly equal ranges (chunk c takes
 * k-tiles [c*T/nchunks, (c+1)*T/nchunks), T = B*Ho*Wo/32).  O, C multiples of 8, B*Ho*Wo % 32 == 0, nchunks <= T; else
 * hipErrorNotSupported. */
typedef struct cips_conv_wgrad_desc {
  const void* dy_hi; const void* dy_lo;
  const void* x_hi; const void* x_lo;
  float* part;
  int B, C, H, W, O, kh, kw, stride, pad, nchunks;
} cips_conv_wgrad_desc;
int cips_conv2d_x3_wgrad(const cips_conv_wgrad_desc* d, cips_stream_t stream);
/* Tail of the weight gradient: dw (O, C, kh, kw) = scale * sum over chunks of part (nchunks, kh*kw, O, C); scale is
 * EqualConv2d's 1/sqrt(C k^2) (discriminator.py:33, 44), which the autograd of `weight * scale` applies to the gradient. */
int cips_conv_wgrad_finish(const float* part, float* dw, int nchunks, int taps, int O, int C, float scale,
                           cips_stream_t stream);
/* Single-pass forms of the four convolution entry points above ("bf16": operands rounded to bf16, fp32 accumulate — the
 * AMP-class arithmetic of cips_gemm_bf16):  sum over the contraction of hi * hi  only.  Same descriptors, same argument
 * validation and return codes; the *_lo pointers are ignored and may be NULL.  A shape the single-pass kernels do not take
 * returns hipErrorNotSupported — it is never run 3-pass (the caller's choice: cips_conv2d_x3* is always more accurate):
 *   cips_conv2d_bf16            C % 64 == 0 (a 64-deep k-tile lies inside one tap) and at least two 64-deep k-tiles in every
 *                               chunk of the contraction: (kh*kw*C / 64) / max(ksplit, 1) >= 2
 *   cips_conv2d_bf16_ksplit     the proposal for it (chunks cut at 64-deep granularity)
 *   cips_conv2d_bf16_dgrad_s2   O % 64 == 0 and O >= 128 (the single-tap parity class contracts over O alone)
 *   cips_conv2d_bf16_wgrad      B*Ho*Wo % 64 == 0 and (B*Ho*Wo / 64) / nchunks >= 2; chunk c takes the 64-row k-tiles
 *                               [c*T/nchunks, (c+1)*T/nchunks), T = B*Ho*Wo / 64; cips_conv_wgrad_finish as before */
int cips_conv2d_bf16(const cips_conv_x3_desc* d, cips_stream_t stream);
int cips_conv2d_bf16_ksplit(int B, int O, int N, int K);
int cips_conv2d_bf16_dgrad_s2(const cips_conv_dgrad_s2_desc* d, cips_stream_t stream);
int cips_conv2d_bf16_wgrad(const cips_conv_wgrad_desc* d, cips_stream_t stream);
/* Activation operand of cips_conv2d_x3 / cips_conv2d_x3_wgrad: x (B, C, n = H*W) fp32 NCHW -> NHWC split planes
 * t_hi, t_lo (B*n + 1, C) bf16, the last row zero (read wherever a tap falls into the padding).  C % 8 == 0 (n % 4 == 0 takes
 * 16-byte loads, any other n scalar loads). */
int cips_split_planes_nhwc(const float* x, void* t_hi, void* t_lo, int B, int C, int n, cips_stream_t stream);

/* fp32 (rows, cols) [ldx] -> split bf16 planes row-major [rows][ldp] and/or transposed [cols][ldt]. */
int cips_split_planes(const float* x, void* p_hi, void* p_lo, void* t_hi, void* t_lo, int rows, int cols,
                      int ldx, int ldp, int ldt, int batch, long long stride_x, long long stride_p,
                      long long stride_t, cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* H4  CIPS INR head helpers (modulated FC, demodulated)                */
/* replaces exp/comm/models/mod_conv_fc.py:470-489 (SinStyleMod.forward_bmm) */
/* ------------------------------------------------------------------ */
/* weight (in,out) [= SinStyleMod.weight[0]], style s (B,in) [= modulation(style)].
 * out: wb (B,in,out) = W*(s+1)*demod, wbt (B,out,in) its transpose,
 * demod (B,out) = rsqrt(sum_in (W*(s+1))^2 + eps). */
int cips_modfc_prep(const float* weight, const float* s, float* wb, float* wbt, float* demod,
                    int B, int in_dim, int out_dim, float eps, cips_stream_t stream);
/* same, writing the bf16x3 operand planes: wb [in][out] and wbt [out][in], hi/lo each (wb_hi == wb_lo == NULL: wbt only). */
int cips_modfc_prep_x3(const float* weight, const float* s, void* wb_hi, void* wb_lo, void* wbt_hi,
                       void* wbt_lo, float* demod, int B, int in_dim, int out_dim, float eps,
                       cips_stream_t stream);
/* backward of prep: gwb (B,in,out) = dL/d wb  ->  dweight (in,out), ds (B,in).
 * cbuf: caller-provided scratch of B*out floats. */
int cips_modfc_prep_bwd(const float* weight, const float* s, const float* demod, const float* gwb,
                        float* cbuf, float* dweight, float* ds, int B, int in_dim, int out_dim,
                        cips_stream_t stream);

/* Batched forms: all modulated-FC layers of the CIPS head in one call (njobs <= cips_modfc_max_jobs()); same
 * per-layer contracts as cips_modfc_prep_x3 / cips_modfc_prep_bwd, one shared batch size B. */
typedef struct cips_modfc_prep_job {
  const float* weight; const float* s;        /* (in,out), (B,in) */
  void *wb_hi, *wb_lo, *wbt_hi, *wbt_lo;      /* (B,in,out) and (B,out,in) bf16 planes.  wb_hi == wb_lo == NULL: that
                                               * orientation is not written (wbt and demod are what they are with it);
                                               * exactly one of the pair NULL is hipErrorInvalidValue */
  float* demod;                               /* (B,out) */
  int in_dim, out_dim;
} cips_modfc_prep_job;
typedef struct cips_modfc_bwd_job {
  const float* weight; const float* s; const float* demod; const float* gwb;   /* gwb (B,in,out) = dL/d wb */
  float *cbuf, *dweight, *ds;                 /* scratch (B,out); outputs (in,out), (B,in) */
  int in_dim, out_dim;
} cips_modfc_bwd_job;
int cips_modfc_max_jobs(void);
int cips_modfc_prep_x3_batch(const cips_modfc_prep_job* jobs, int njobs, int B, float eps, cips_stream_t stream);
int cips_modfc_prep_bwd_batch(const cips_modfc_bwd_job* jobs, int njobs, int B, cips_stream_t stream);
/* Which kernels the two batch entries run for a job list (host only; the entry points switch on these very functions, so
 * the rule exists once).  Only the jobs' in_dim / out_dim are read, no pointer of a job is dereferenced.  Negative: minus
 * the hipError the entry point returns for these arguments.  Every form computes the same values up to the summation order;
 * the queries let a test say which kernels a shape reached. */
enum {
  CIPS_MODFC_PREP_COLSUM16 = 1,        /* bit 0: 16-byte column sums (every out_dim % 4 == 0), else the 32-column scalar sums */
  CIPS_MODFC_PREP_TILES64 = 2          /* bit 1: 64 x 64 plane tiles (also every in_dim % 8 == 0), else 32 x 32 tiles */
};
enum {
  CIPS_MODFC_BWD_SCALAR = 0,           /* three passes over G (c, dW, ds): every shape */
  CIPS_MODFC_BWD_FUSED2 = 2,           /* 16-byte column sums + ONE dW / ds pass of 2 chunks of 256 columns: every */
  CIPS_MODFC_BWD_FUSED4 = 4            /*   out_dim % 4 == 0, B <= 64, largest out_dim <= 512; 4 chunks: <= 1024 */
};
int cips_modfc_prep_x3_batch_form(const cips_modfc_prep_job* jobs, int njobs, int B);
int cips_modfc_prep_bwd_batch_form(const cips_modfc_bwd_job* jobs, int njobs, int B);
/* Co-resident form of cips_modfc_prep_bwd_batch (same results up to the summation order): kernels without LDS and with
 * <= 40 VGPRs, which get wave slots BESIDE a kernel that owns the whole LDS (the fused SIREN backward) instead of waiting
 * for it — for a caller that runs this tail on a side stream.  cbuf must hold cips_cores_colsum_parts() planes of (B, out).
 * B <= 64, out_dim % 4 == 0, else hipErrorNotSupported. */
int cips_cores_colsum_parts(void);
int cips_modfc_prep_bwd_batch_cores(const cips_modfc_bwd_job* jobs, int njobs, int B, cips_stream_t stream);

/* Grouped small Linear layers: every per-image vector of the hot path is a Linear of a style vector — the 18
 * SinStyleMod.modulation layers of the CIPS head (exp/comm/models/mod_conv_fc.py:433-436, 474) and the gain_fc / bias_fc
 * pairs of the FiLM layers (exp/comm/models/film_layer.py:59-63, 88-93).  One launch for all of them:
 *   forward   y_j (B,out_j) = x_j (B,in_j) w_j^T (out_j,in_j) + bias_j            (bias may be NULL)
 *   backward  dw_j = dy_j^T x_j, db_j = sum_b dy_j (db may be NULL), and — when dx != NULL, for jobs that all share one
 *             x — dx (B,in) = sum_j dy_j w_j (partials in `scratch`, cips_grouped_linear_scratch() floats, summed in
 *             a fixed order).  in_j % 4 == 0, in_j <= 512, njobs <= cips_grouped_linear_max_jobs(). */
typedef struct cips_glin_job {
  const float* x; const float* w; const float* bias; float* y;      /* forward */
  const float* dy; float* dw; float* db;                             /* backward */
  int in_dim, out_dim;
} cips_glin_job;
int cips_grouped_linear_max_jobs(void);
int cips_grouped_linear_fwd(const cips_glin_job* jobs, int njobs, int B, cips_stream_t stream);
long long cips_grouped_linear_scratch(const cips_glin_job* jobs, int njobs, int B);
int cips_grouped_linear_bwd(const cips_glin_job* jobs, int njobs, int B, float* dx, float* scratch,
                            long long scratch_floats, cips_stream_t stream);

/* Row-wise normalisation + activation of the z -> style mapping MLPs (exp/cips3d/models/multi_head_mapping.py:13-19
 * PixelNorm; :62-84 LayerNorm / LeakyReLU(0.2) after every Linear).  x, y (rows, cols <= 1024); stats (rows, 2) scratch
 * kept for the backward.  mode bit 0: LayerNorm (eps 1e-5, affine gamma / beta), bit 1: LeakyReLU(slope) after it,
 * bit 2: PixelNorm y = x * rsqrt(mean(x^2) + 1e-8) (alone).  Backward: dx (and d gamma, d beta through the (rows, cols)
 * scratch dyhat when bit 0 is set); `y` is the forward's output (the LeakyReLU gate is its sign). */
int cips_rownorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats, int rows, int cols,
                     int mode, float slope, cips_stream_t stream);
int cips_rownorm_bwd(const float* x, const float* y, const float* gamma, const float* stats, const float* dy, float* dx,
                     float* dyhat, float* dgamma, float* dbeta, int rows, int cols, int mode, float slope,
                     cips_stream_t stream);

/* ToRGB (generator.py:983-1006): rgb (M,3) (+)= x (M,K) @ w^T (3,K) + bias.
 * accumulate != 0: rgb += ...  */
int cips_torgb_fwd(const float* x, const float* w, const float* bias, float* rgb,
                   long long M, int K, int accumulate, cips_stream_t stream);
/* dw (3,K) = drgb^T @ x, dbias(3) = sum drgb.  Uses `partials` scratch of
 * cips_torgb_bwd_partials(M) * 4 * K floats, reduced deterministically. */
int cips_torgb_bwd_partials(long long M);
int cips_torgb_bwd_w(const float* x, const float* drgb, float* partials, float* dw, float* dbias,
                     long long M, int K, cips_stream_t stream);
/* split-plane input variants of the two ToRGB reductions (x = x_hi + x_lo, bf16 planes [M][K]). */
int cips_torgb_fwd_x3(const void* x_hi, const void* x_lo, const float* w, const float* bias, float* rgb,
                      long long M, int K, int accumulate, cips_stream_t stream);
int cips_torgb_bwd_w_x3(const void* x_hi, const void* x_lo, const float* drgb, float* partials, float* dw,
                        float* dbias, long long M, int K, cips_stream_t stream);
/* the taps of up to 8 blocks (same M; K = 512, else hipErrorNotSupported) against one drgb in two launches:
 * x_hi / x_lo: host arrays of njobs device plane pointers; partials (njobs, chunks, 4, K); dw (njobs, 3, K); dbias (njobs, 3) */
int cips_torgb_bwd_w_x3_batch(const void* const* x_hi, const void* const* x_lo, int njobs, const float* drgb,
                              float* partials, float* dw, float* dbias, long long M, int K, cips_stream_t stream);
/* co-resident form (see cips_modfc_prep_bwd_batch_cores): same arguments, layouts and scratch */
int cips_torgb_bwd_w_x3_batch_cores(const void* const* x_hi, const void* const* x_lo, int njobs, const float* drgb,
                                    float* partials, float* dw, float* dbias, long long M, int K, cips_stream_t stream);
/* dx (M,K) = drgb (M,3) @ w (3,K) [+ add]; optional copy before masking; out = dx * (mask>0 ? 1 : slope)
 * (the LeakyReLU gate of the layer below, fused).  mask / add / out_unmasked may be NULL. */
int cips_torgb_bwd_x(const float* drgb, const float* w, const float* add, const float* mask, float slope,
                     float* out_unmasked, float* out, long long M, int K, cips_stream_t stream);
/* the same with split-plane output and the gate as a bit plane (bit k&7 of byte [m][k>>3]; NULL: none):
 * p_hi / p_lo (M, K) bf16 planes of (drgb @ w) * (bit ? 1 : slope); out_unmasked: optional fp32 copy before gating.  K % 8 == 0. */
int cips_torgb_bwd_x_x3(const float* drgb, const float* w, const void* gate_bits, float slope, float* out_unmasked,
                        void* p_hi, void* p_lo, long long M, int K, cips_stream_t stream);

/* Camera pose of a batch (exp/comm/comm_utils.py:451-581: sample_camera_positions for 'gaussian' / 'normal' (uniform = 0:
 * angle = draw * stddev + mean) and 'uniform' (uniform = 1: (draw - 0.5) * 2 * stddev + mean), camera_origin_from_angles with
 * r = 1, look-at-origin forward vector, create_cam2world_matrix with up = (0, 1, 0)) in one launch:
 * theta_raw, phi_raw (B) raw draws -> pitch_yaw (B, 2) = (clamped phi, theta), origin (B, 3), cam2world (B, 4, 4). */
int cips_camera_pose(const float* theta_raw, const float* phi_raw, int uniform, float h_stddev, float h_mean,
                     float v_stddev, float v_mean, float* pitch_yaw, float* origin, float* cam2world, int B,
                     cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* H5  discriminator native ops                                        */
/* ------------------------------------------------------------------ */
/* Same contract as the reference's pybind op
 *   fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)
 * (exp/comm/op/fused_bias_act.cpp:11-21, kernel fused_bias_act_kernel.cu:18-49):
 * y = f(x + b[(i/step_b) % size_b]) * scale, act*10+grad switch:
 * 10 linear, 11/12 linear grads, 30 lrelu, 31 lrelu grad gated by sign(refer),
 * 32 second-order (=0).  bias / refer may be NULL ("empty tensor"). */
int cips_fused_bias_act(const float* x, const float* bias, const float* refer, float* y,
                        long long numel, int size_b, int step_b,
                        int act, int grad, float alpha, float scale, cips_stream_t stream);

/* Same contract as upfirdn2d_op.upfirdn2d(input[N,H,W,minor], kernel[kh,kw],
 * up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
 * (exp/comm/op/upfirdn2d.cpp:12-23, kernel upfirdn2d_kernel.cu:52-137). */
int cips_upfirdn2d(const float* input, const float* kernel, float* out,
                   int major, int in_h, int in_w, int minor, int kernel_h, int kernel_w,
                   int up_x, int up_y, int down_x, int down_y,
                   int pad_x0, int pad_x1, int pad_y0, int pad_y1, cips_stream_t stream);
/* Which kernel instantiation cips_upfirdn2d runs for these arguments (host only; the entry point switches on this very
 * function, so the rule exists once): one code per instantiation, CIPS_UPFIRDN2D_NONE when the output is empty (the call
 * launches nothing and returns 0), negative for arguments the call refuses.  Every form computes the generic kernel's
 * values bit for bit; the query lets a test say which kernel a shape reached. */
enum {
  CIPS_UPFIRDN2D_NONE = 0,
  CIPS_UPFIRDN2D_GENERIC = 1,          /* upfirdn2d_kernel: any up / down / minor, up to 64 taps */
  CIPS_UPFIRDN2D_DIRECT_1_8 = 2,       /* upfirdn2d_direct_kernel<DOWN, 1, TH>: 4 x 4 taps, up 1, minor 1; */
  CIPS_UPFIRDN2D_DIRECT_1_16 = 3,      /*   TH = 8 output rows per thread below out_h = 48, 16 from there on */
  CIPS_UPFIRDN2D_DIRECT_2_8 = 4,
  CIPS_UPFIRDN2D_DIRECT_2_16 = 5,
  CIPS_UPFIRDN2D_UP2_4 = 6,            /* upfirdn2d_up2_kernel<4>: 4 x 4 taps, up 2, down 1, minor 1 */
  CIPS_UPFIRDN2D_DOWN2_PAIRS_4 = 7,    /* upfirdn2d_down2_pairs_kernel<TH>: down 2, pad_x0 = 1, in_w = 2 out_w, out_w a power */
  CIPS_UPFIRDN2D_DOWN2_PAIRS_8 = 8,    /*   of two, pad_y0 >= 0; TH = 4 below out_h = 48, else 8 */
  CIPS_UPFIRDN2D_UP2_PAIRS_2 = 9,      /* upfirdn2d_up2_pairs_kernel<TU>: up 2, pad_x0 = pad_y0 = 2, out_w = 2 in_w, in_w a power */
  CIPS_UPFIRDN2D_UP2_PAIRS_4 = 10,     /*   of two, out_h <= 2 in_h; TU = 2 below in_h = 24, else 4 */
  CIPS_UPFIRDN2D_BLUR_1 = 11,          /* upfirdn2d_blur_kernel<DOWN> (LDS row bands): up 1, minor 1, at most 4 x 4 taps, */
  CIPS_UPFIRDN2D_BLUR_2 = 12,          /*   pads >= 0, down 1 or 2, and no register-tiled form above applies */
  CIPS_UPFIRDN2D_BLUR_SPILL = 13       /* a blur shape whose one-row band exceeds the 32 KiB of LDS: the generic kernel */
};
int cips_upfirdn2d_form(int in_h, int in_w, int minor, int kernel_h, int kernel_w,
                        int up_x, int up_y, int down_x, int down_y,
                        int pad_x0, int pad_x1, int pad_y0, int pad_y1);
/* The same op for a 4 x 4 kernel, up = down = 1, on `major` planes of in_h x in_w that are stored as the four parity blocks
 * written by cips_conv2d_x3_dgrad_s2 (pixel (y, x) of plane m at dxp[blk_off[2(y&1) + (x&1)] + m * Np + (y>>1) * Ws + (x>>1)],
 * Ws = ceil((in_w - (x&1)) / 2), Np = Hs * Ws rounded up to 8): the transpose of the Blur of a down-sampling ConvLayer
 * (discriminator.py:57-82, 190-203) applied to the stride-2 convolution's data gradient without materialising it
 * row-major.  Same taps in the same order as cips_upfirdn2d on the interleaved tensor: bit-identical results. */
int cips_upfirdn2d_parity(const float* dxp, const long long* blk_off, const float* kernel, float* out, int major,
                          int in_h, int in_w, int pad_x0, int pad_x1, int pad_y0, int pad_y1, cips_stream_t stream);

/* EqualLinear (exp/cips3d/models/discriminator.py:254-288: F.linear(input, weight * scale) [+ bias * lr_mul]) and the two
 * other bilinear forms of its autograd (each form's gradients are the other two: the R1 double-backward closes):
 *   mode 0   out (B, O) = s * a (B, K) . b^T (O, K)  [+ bias (O) * bias_scale]        a = x, b = weight
 *   mode 1   out (B, K) = s * a (B, O) . b (O, K)                                      a = dy, b = weight
 *   mode 2   out (O, K) = s * a^T (O, B) . b (B, K)                                    a = dy, b = x
 * O % 4 == 0 and K % 4 == 0: on cips_gemm_f32 (mode 0 with K >= 2048 cut into 512-wide chunks whose partial products
 * land in `scratch`, cips_equal_linear_scratch floats, and are summed in chunk order); else three streaming kernels
 * (the 512 -> 1 output layer).  bias only with mode 0. */
long long cips_equal_linear_scratch(int mode, int B, int K, int O);
int cips_equal_linear(int mode, const float* a, const float* b, const float* bias, float bias_scale, float s, float* out,
                      float* scratch, int B, int K, int O, cips_stream_t stream);

/* DiffAugment with policy 'color,translation,cutout' (exp/cips3d/models/diffaug.py:9-85; applied to every discriminator
 * input, exp/cips3d/models/discriminator.py:507-508) as one affine operator and its adjoint.  rb, rs, rc: the (B) raw
 * uniform draws of brightness / saturation / contrast; tx, ty, ox, oy: the (B) int64 draws of translation and cutout
 * centre, all made by the host with the reference's calls.  x, y (B, C <= 4, H, W); sums: 33 * B floats of scratch
 * (per-image sums, then 32 slices of partial sums per image).
 * adjoint 0: y = A x + c (affine != 0) or y = A x (affine == 0); adjoint 1: y = A^T x (the backward; its own backward
 * is the forward with affine == 0: the R1 double-backward of train.py:387-394).  cut_h / cut_w = int(size * 0.2 + 0.5).
 * Policies that leave stages out (diffaug.py:12-17 applies the listed ones): bit 1 of `affine` set = no colour stage
 * (values pass through untouched), tx = ty = 0 = no translation, cut_h = cut_w = 0 = no cutout. */
int cips_diffaug(const float* x, float* y, const float* rb, const float* rs, const float* rc, const long long* tx,
                 const long long* ty, const long long* ox, const long long* oy, float* sums, int B, int C, int H, int W,
                 int cut_h, int cut_w, int adjoint, int affine, cips_stream_t stream);
/* Progressive fade-in (discriminator.py:524-534): the 2x2 mean that F.interpolate(scale_factor=0.5, 'bilinear') computes
 * on even sizes (adjoint 1: its transpose, 0.25 g to the four sources), and out = a x + b y (y may be NULL). */
int cips_avgpool2(const float* x, float* y, long long planes, int H, int W, int adjoint, cips_stream_t stream);
int cips_axpby(const float* x, const float* y, float* out, float a, float b, long long n, cips_stream_t stream);

/* FID path: float image (B, C <= 4, H, W) -> uint8 pixels (B, H, W, C) exactly as torchvision.utils.save_image(img,
 * normalize=True, value_range=(lo, hi)) quantises them before JPEG encoding (exp/cips3d/scripts/gen_images.py:56-60;
 * torchvision/utils.py make_grid norm_ip + save_image): clamp to [lo, hi], (x - lo) * (1 / max(hi - lo, 1e-5)),
 * * 255, + 0.5, clamp to [0, 255], truncate.  Bit-exact on identical float inputs. */
int cips_image_to_u8(const float* x, unsigned char* out, int B, int C, int H, int W, float lo, float hi,
                     cips_stream_t stream);

/* Backward of FusedLeakyReLU on a (B, C, H, W) activation (exp/comm/op/fused_act.py:26-44) with the bias gradient in the
 * same pass: grad_in = (refer > 0 ? grad : grad * alpha) * scale — cips_fused_bias_act(act 3, grad 1) — and
 * part[plane][slice] = sum of grad_in over slice `slice` of plane (b, c); planes = B * C, slices =
 * cips_lrelu_bwd_bias_slices(HW); the caller adds part over images and slices to get grad_bias (C). */
int cips_lrelu_bwd_bias_slices(int HW);
int cips_lrelu_bwd_bias(const float* grad, const float* refer, float* grad_in, float* part, long long planes, int HW,
                        float alpha, float scale, cips_stream_t stream);
/* grad_bias[c] = sum over b < B, s < S of part[b][c][s] (fixed order): the tail of cips_lrelu_bwd_bias, planes = B * C */
int cips_lrelu_bwd_bias_finish(const float* part, float* grad_bias, int B, int C, int S, cips_stream_t stream);
/* cips_lrelu_bwd_bias written directly as the NHWC split planes (B*HW + 1, C; zero last row) of the gated gradient — for
 * convolutions that read their incoming gradient only through those planes the fp32 tensor never exists.  part: (B, C,
 * cips_lrelu_bwd_bias_nhwc_tiles(HW)) partial bias sums for cips_lrelu_bwd_bias_finish.  C % 8 == 0.  Plane values are those of
 * cips_lrelu_bwd_bias followed by cips_split_planes_nhwc, bit for bit. */
int cips_lrelu_bwd_bias_nhwc_tiles(int HW);
int cips_lrelu_bwd_bias_nhwc(const float* grad, const float* refer, void* t_hi, void* t_lo, float* part, int B, int C, int HW,
                             float alpha, float scale, cips_stream_t stream);

/* 1x1 convolution with C <= 4 input channels (EqualConv2d of the RGB input layers, discriminator.py:457-459):
 * y (B, O, HW) = w (O, C) . x (B, C, HW); HW % 4 == 0.  Streaming kernel, no GEMM. */
int cips_conv1x1_smallk(const float* x, const float* w, float* y, int B, int C, int O, int HW, cips_stream_t stream);
/* its data gradient: dx (B, C, HW) = w^T (C, O) . dy (B, O, HW) */
int cips_conv1x1_smallk_bwd_data(const float* dy, const float* w, float* dx, int B, int C, int O, int HW,
                                 cips_stream_t stream);
/* its weight gradient (autograd of discriminator.py:44-48 for the RGB layers): part (S, O, C), S =
 * cips_conv1x1_smallk_bwd_weight_splits(O, HW) partial rows that the caller sums over S:
 * sum_s part[s][o][c] = sum_{b,p} dy[b][o][p] x[b][c][p] */
int cips_conv1x1_smallk_bwd_weight_splits(int O, int HW);
int cips_conv1x1_smallk_bwd_weight(const float* dy, const float* x, float* part, int B, int C, int O, int HW,
                                   cips_stream_t stream);

/* im2col for the EqualConv2d GEMM path (exp/cips3d/models/discriminator.py:40-48).
 * x (B,C,H,W) NCHW -> col (B, C*kh*kw, Ho*Wo) row-major ("colT": k-major B operand, so that
 * out[b] (O, Ho*Wo) = W (O, C*kh*kw) @ col[b] lands directly in NCHW).  col2im is the adjoint
 * (gather form, deterministic). */
int cips_im2col(const float* x, float* col, int B, int C, int H, int W,
                int kh, int kw, int stride, int pad, cips_stream_t stream);
int cips_col2im(const float* col, float* dx, int B, int C, int H, int W,
                int kh, int kw, int stride, int pad, cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* Training-step tail: gradient-norm clip + Adam + EMA over all tensors of one optimiser,
 * two launches.  Replaces torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step + EMA.update
 * (exp/cips3d/scripts/train.py:420-491, exp/comm/comm_model_utils.py:97-118).
 * table_dev: device array of tensors; grad == NULL: no Adam update (parameter unused this step), ema == NULL: no EMA.
 * The tensors are walked in chunks of cips_opt_chunk() elements: chunk_tensor_dev[c] = tensor index,
 * chunk_off_dev[c] = first element; partial_dev: nchunks doubles of scratch; total_norm_dev (optional): pre-clip norm.
 * max_norm <= 0 disables clipping; `step` = this tensor's 1-based Adam step count (torch counts per parameter);
 * write_grad != 0 stores the clipped gradient back.
 * steps_dev (optional, one long long per tensor): device-side step counts — the call advances the count of every
 * tensor that has a gradient and uses it instead of the table's `step`, so neither the table nor a captured hipGraph of
 * the call goes stale from one step to the next. */
typedef struct cips_opt_tensor {
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq; float* ema; long long n; long long step;
} cips_opt_tensor;
int cips_opt_chunk(void);
int cips_opt_step(const cips_opt_tensor* table_dev, const int* chunk_tensor_dev, const long long* chunk_off_dev,
                  int nchunks, double* partial_dev, float* total_norm_dev, float max_norm, float lr,
                  float beta1, float beta2, float eps, float ema_decay, int write_grad,
                  long long* steps_dev, cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* Pyramid fit loss (csrc/fit_loss.hip): what fitting styles or a camera to an image minimises.  Replaces, per step, the
 * reference Projector's nn.MSELoss (exp/cips3d/models/st_web.py:144-186) and the ATen chain a multi-scale version of it
 * would be (sub, avg_pool2d per level, mul, pow / sqrt, mean, and their autograd backward).
 * pred, target (B,C,H,W), weight (B,1,H,W) or NULL (= 1), all fp32 contiguous on the device:
 *   d_0 = pred - target, d_{l+1} = 2x2 mean of d_l;   w_0 = weight, w_{l+1} = 2x2 mean of w_l
 *   loss[b] = sum_{l<L} level_weights[l] / (C H_l W_l) * sum_{c,y,x} w_l rho(d_l)
 *   rho(x) = x^2 (kind 0)  or  sqrt(x^2 + eps^2) - eps (kind 1, Charbonnier; eps > 0)
 * 1 <= L <= 8; H and W multiples of 2^(L-1).  level_weights_host: L doubles in HOST memory (read during the call); they and
 * eps are doubles because the gradient is formed in fp64 and rounded once: for L <= 6 it is the correctly rounded gradient.
 * The forward writes loss (B) and grad (B,C,H,W) = d loss[b] / d pred in one pass over pred / target: two launches, three
 * for L > 6.  scratch: cips_pyramid_loss_scratch(B,C,H,W,L) floats of device memory (-1: invalid shape), overwritten.
 * No atomics and a fixed summation order: equal inputs give equal bits, and image b's loss and gradient do not depend on
 * the other images of the batch.  cips_pyramid_loss_bwd: out[b] = grad[b] * upstream[b] (per_image = C*H*W elements each).
 * Invalid arguments (NULL required pointer, a size <= 0, L outside 1..8, H or W not a multiple of 2^(L-1), eps <= 0 with
 * kind 1, a scratch that is too small) return hipErrorInvalidValue before any HIP call. */
long long cips_pyramid_loss_scratch(int B, int C, int H, int W, int L);
int cips_pyramid_loss_fwd(const float* pred, const float* target, const float* weight, const double* level_weights_host,
                          int L, int kind, double eps, float* loss, float* grad, float* scratch, long long scratch_floats,
                          int B, int C, int H, int W, cips_stream_t stream);
int cips_pyramid_loss_bwd(const float* grad, const float* upstream, float* out, int B, long long per_image,
                          cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* View reprojection (csrc/reproject.hip): what the pixels of a TARGET view see of a SOURCE view, through the target's depth.
 * src (B,C,Hs,Ws), tgt_depth (B,1,Ht,Wt), src_depth (B,1,Hs,Ws) or NULL, tgt2src (B,3,4), all fp32 contiguous on the device.
 * tgt_depth: distance along the normalised ray (the renderer's depth).  tgt2src = [R | t]: a rigid transform from target-camera
 * to source-camera space.  zc_tgt, zc_src: camera-space z of the two image planes (negative: the cameras look along -z).
 * Camera (csrc/raygen.h): pixel (row i, col j) of an H x W image has x = -1 + 2j/(W-1), y = 1 - 2i/(H-1) and the direction
 * d = (x, y, zc) / |(x, y, zc)|.  For every target pixel:
 *   1. q = d * tgt_depth                                   2. q' = R q + t
 *   3. x' = q'_x zc_src / q'_z,  y' = q'_y zc_src / q'_z    4. u = (x'+1)/2 (Ws-1),  v = (1-y')/2 (Hs-1)
 *   5. in frame: tgt_depth finite and > 0;  q'_z zc_src > 0 (in front of the source camera);  -1/256 <= u <= Ws-1+1/256 and
 *      the same for v against Hs.  Then u, v are clamped to [0, Ws-1], [0, Hs-1].  (The 1/256 px of slack gives an identity
 *      warp full coverage when its last column rounds an ulp past the border.)
 *   6. bilinear sample over all C channels with u0 = min(floor(u), Ws-2), v0 = min(floor(v), Hs-2) and the weights u - u0, v - v0
 *   7. with src_depth: ds = the same sample of src_depth; visible iff |q'| <= ds + occ_tol is true (a NaN in ds: occluded)
 * Steps 1-5 and 7 run in fp64 on the fp32 inputs, (u, v) is rounded to fp32 once; step 6 is fp32.
 *   out  (B,C,Ht,Wt)        the sample where mask == 1, exact zeros elsewhere
 *   mask (B,1,Ht,Wt) uint8  1 visible, 0 not in frame, 2 in frame but occluded (never without src_depth)
 *   uv   (B,2,Ht,Wt) / NULL the clamped (u, v): the correspondence field; NaN where mask == 0
 * One launch; every output is bit-reproducible.
 * cips_reproject_bwd, where mask == 1 (the forward's mask is READ: no branch is decided again) and zero elsewhere:
 *   d_src / NULL        (B,C,Hs,Ws)  the transposed bilinear weights times dout.  Zeroed here (hipMemsetAsync on the stream), then
 *                       summed with no-return fp32 atomic adds: the ONLY output whose last bits depend on arrival order and can
 *                       differ from call to call.  NULL: neither the memset nor the adds run.
 *   d_tgt_depth / NULL  (B,1,Ht,Wt)  sum_c dout_c (d out_c/du du/ddepth + d out_c/dv dv/ddepth), with e = R d:
 *                       du/ddepth = (Ws-1)/2 zc_src (e_x q'_z - q'_x e_z) / q'_z^2,  dv/ddepth = -(Hs-1)/2 zc_src (e_y q'_z - q'_y e_z) / q'_z^2,
 *                       and the slopes of the bilinear cell; zero through a coordinate that the clamp of step 5 holds.  A gather:
 *                       plain stores, bit-reproducible.
 * No gradient goes through the mask, src_depth, tgt2src or the plane constants.  One launch (none when both outputs are NULL).
 * Invalid arguments (a required NULL pointer, B or C < 1, any of Hs, Ws, Ht, Wt < 2, a zero or non-finite zc, src_depth with a
 * negative or non-finite occ_tol, a plane of 2^31 pixels or more, B > 65535) return hipErrorInvalidValue before any HIP call. */
int cips_reproject_fwd(const float* src, const float* src_depth, const float* tgt_depth, const float* tgt2src, float zc_tgt,
                       float zc_src, float occ_tol, float* out, unsigned char* mask, float* uv, int B, int C, int Hs, int Ws,
                       int Ht, int Wt, cips_stream_t stream);
int cips_reproject_bwd(const float* dout, const float* src, const float* tgt_depth, const float* tgt2src,
                       const unsigned char* mask, float zc_tgt, float zc_src, float* d_src, float* d_tgt_depth, int B, int C,
                       int Hs, int Ws, int Ht, int Wt, cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* Mesh rasterisation (csrc/raster.hip), forward only: which triangle of an indexed mesh does the ray of pixel (r, c) hit first,
 * and at what distance along the unit ray direction — the question cips_siren_surface_x3 answers for a level set.
 * vertices (V,3) fp32, faces (T,3) int32, world2cam (B,3,4) fp32 = [R | t] (the inverse of cam2world), xg (W) = linspace(-1, 1, W)
 * and yg (H) = linspace(1, -1, H) (the grids of the ray set-up: read, not computed), zc < 0 the image-plane constant.
 * Per camera b and vertex i (computed once and stored in `screen`, so a shared vertex has one set of bits):
 *   q = R v + t;   u = (q.x zc / q.z + 1) (W-1)/2,  v = (1 - q.y zc / q.z) (H-1)/2   (pixel (r, c) has its centre at (u, v) = (c, r))
 *   valid iff q is finite and -q.z >= near
 * A triangle is dropped whole, never clipped, if a vertex index is outside [0, V), a vertex is invalid, its screen area is zero
 * or not finite, or cull == 1 and it faces away from the camera (front-facing: the geometric normal (v1-v0) x (v2-v0) points
 * towards the camera; with extract_mesh's winding that is the side of lower density).
 * Coverage: the value of edge {i, j} is ONE fp32 expression with the lower vertex index first,
 *   e = (u_hi - u_lo)(r - v_lo) - (v_hi - v_lo)(c - u_lo),
 * negated for the triangle that runs from hi to lo; pixel (r, c) is covered iff all three values have the triangle's orientation
 * sign or are zero (inclusive on every edge).  Two triangles that share an edge evaluate the same bits: no cracks.
 * Depth: with E_i the edge value opposite vertex i, w_i = E_i / q_i.z:  z = sum E / sum w,  lambda_i = w_i / sum w (the
 * perspective-correct barycentrics) and depth = (z / zc) sqrt(xg[c]^2 + yg[r]^2 + zc^2), the quantity of the renderer's depth maps.
 * A fragment whose depth is not positive and finite is dropped.
 * Winner: the smallest 64-bit key (bits of depth as fp32) << 32 | face index (64-bit atomicMin into `keys`): equal depths go to
 * the lower face index, and every output is the same bits on every call whatever order the triangles arrive in.
 *   face (B,H,W) int32, -1 for none;  bary (B,H,W,3) lambda, zeros for none;  depth (B,H,W), far for none;  mask (B,H,W) uint8 1 / 0
 * Scratch, provided by the caller and written before it is read: screen (B,V) records of 16 bytes (16-byte aligned), keys
 * (B,H,W) of 8 bytes, big_list of big_cap >= B*T ints and big_count, one int: a triangle whose clamped bounding box holds more
 * than 256 pixels is appended to the list and rasterised by workgroups in a further launch.
 * Launches: memset of keys (and of big_count), vertex, face, large-triangle, resolve kernel; with V == 0 or T == 0 the memset of
 * keys and the resolve kernel only (the background); with B == 0 none.
 * cips_raster_interp: out[b, ch, r, c] = sum_i lambda_i attr[faces[face][i], ch] for a per-vertex attribute attr (V,C), `fill`
 * where face < 0 (or where it names no face or vertex of the mesh); out (B,C,H,W) channel-major.  One launch.
 * Invalid arguments (a required NULL pointer; H or W < 2; B, V or T < 0; near <= 0 or not finite; zc >= 0 or not finite; a NaN
 * far; cull not 0 or 1; B*H*W, B*V or B*T beyond int32; big_cap < B*T; C < 1) return hipErrorInvalidValue before any HIP call. */
int cips_raster_fwd(const float* vertices, const int* faces, const float* world2cam, const float* xg, const float* yg, float zc,
                    float near_, float far_, int cull, void* screen, unsigned long long* keys, int* big_list, int* big_count,
                    long long big_cap, int* face, float* bary, float* depth, unsigned char* mask, int B, int V, int T, int H,
                    int W, cips_stream_t stream);
int cips_raster_interp(const int* face, const float* bary, const int* faces, const float* attr, float fill, float* out, int B,
                       int H, int W, int T, int V, int C, cips_stream_t stream);

/* ------------------------------------------------------------------ */
/* Baked radiance volumes (csrc/volume.hip): sigma and colour on a lattice, volume-rendered from any camera of the ray set-up
 * with the network out of the loop, and the gradients of that render with respect to the nodes and to the cameras.
 *
 * cips_volume_bake: sigma (Bv,nx,ny,nz) and rgb (Bv,nx,ny,nz,3) -> packed (Bv,nx,ny,nz,4) = r, g, b, sigma: one 16-byte record
 * per node (packed is 16-byte aligned), the two z-neighbours of a corner pair are one 32-byte access.  Bits are copied, nothing
 * is computed.  occ (Bv, ceil((nx-1)/8), ceil((ny-1)/8), ceil((nz-1)/8)): entry (I, J, K) is the maximum of sigma over the nodes
 * 8I .. min(8I+8, nx-1) (same per axis; the shared face included): every node a trilinear lookup in a cell of that brick of
 * 8 x 8 x 8 cells can read.  A maximum is exact.  The volume is taken to be finite (fmaxf drops a NaN).  Two launches.
 *
 * cips_volume_render: one ray per lane, lanes mapped to pixels in 8 x 8 tiles.  The ray of pixel (r, c) and its depths
 * z_s = zg[s] are those of gen_point (csrc/raygen.h: its ray_dir once per ray, its ray_point per sample) with xg (W), yg (H), zg (S), zc and cam2world (b,4,4): no jitter, no
 * resampled depths.  lo, hi: HOST arrays of three floats, the box of the lattice: node i of axis a sits at
 * lo[a] + i (hi[a] - lo[a]) / (n_a - 1).  With inv_h[a] = fp32(n_a - 1) / (hi[a] - lo[a]) (fp32, on the host) a sample x has
 *   u_a = (x_a - lo[a]) * inv_h[a];   inside iff 0 <= u_a <= n_a - 1 on all three axes;   cell i_a = min(floor(u_a), n_a - 2),
 *   t_a = u_a - i_a, and the four channels are interpolated by nested lerps  p + t (q - p): along z, then y, then x.
 * A sample outside has sigma = 0 and colour 0.  Compositing is cips_composite_fwd's rule without noise:
 *   delta_s = z_{s+1} - z_s, the last one 1e10;  alpha = 1 - expf(-delta clamp(sigma)),  clamp_mode 0 relu, 1 softplus;
 *   w_s = alpha_s fp32(T_s),  T_{s+1} = T_s (1 - alpha_s + 1e-10f) kept in double;  opacity = sum w (before any top-up);
 *   flags bit 0 (last_back): the last sample's weight gains 1 - sum w;  rgb = sum w c,  depth = sum w z;
 *   flags bit 1 (white_back): rgb += 1 - sum w.  Sums run in sample order in fp32.
 * flags bit 2 (skip), relu only: a sample whose brick has occ <= 0 is not fetched.  Exact: every corner <= 0 makes every nested
 * lerp <= 0 (each rounding is monotone and 0 is representable), so relu gives 0, alpha = 0, w = 0 and T is multiplied by
 * fp32(1 + 1e-10) = 1: the outputs are the same bits with the bit set or clear.  Under last_back the last sample is fetched
 * whenever it is inside (its colour takes the top-up).  With clamp_mode 1 the bit is IGNORED here (treated as clear):
 * softplus(sigma) > 0 everywhere; ops.render_volume refuses the combination.  No early ray termination (it changes bits).
 *   rgb (b,3,H,W), depth (b,1,H,W), opacity (b,1,H,W);  Bv is 1 (every camera sees volume 0) or b.
 * Invalid arguments return hipErrorInvalidValue before any HIP call: a NULL pointer (occ may be NULL only with the skip bit
 * clear); n_a < 2; H, W or S < 2; b or Bv < 0, Bv not in {1, b} (render); lo / hi not finite or hi <= lo; zc >= 0, NaN or -inf;
 * clamp_mode not 0 or 1; flags outside 0..7; packed not 16-byte aligned; nx*ny*nz, b*H*W or H*W*S beyond int32.
 * b == 0 (render) or Bv == 0 (bake) returns 0 and launches nothing. */
int cips_volume_bake(const float* sigma, const float* rgb, void* packed, float* occ, int Bv, int nx, int ny, int nz,
                     cips_stream_t stream);
int cips_volume_render(const void* packed, const float* occ, const float* lo, const float* hi, const float* xg, const float* yg,
                       const float* zg, const float* cam2world, float zc, int clamp_mode, int flags, float* rgb, float* depth,
                       float* opacity, int b, int Bv, int nx, int ny, int nz, int H, int W, int S, cips_stream_t stream);

/* cips_volume_render_bwd: the gradient of cips_volume_render's three outputs with respect to the NODES, dpacked (Bv,nx,ny,nz,4)
 * fp32 in packed's layout (r, g, b, sigma per node), so that an optimiser can step a packed volume in place.  Nothing flows to
 * the cameras, zg or the box.  Arguments: the forward's, with drgb (b,3,H,W), ddepth (b,1,H,W) and dopacity (b,1,H,W) in place
 * of the outputs; ddepth and dopacity may each be NULL, meaning zeros.
 *   Per ray, every forward quantity by the forward's own expressions (the same device functions locate the cell, T in double and
 * rounded to fp32 per prefix): x_k the interpolated sigma, c_k the interpolated colour, both 0 for a sample that is outside the
 * box or skipped.  With G = drgb at the pixel, gd = ddepth, go = dopacity, gsum = G_r + G_g + G_b:
 *     s_k = G . c_k + gd z_k;      s_off = [last_back] s_{S-1} + [white_back] gsum - go;      Q = 0;
 *     for k = S-1 .. 0:   s' = s_k - s_off;   dalpha = T_k (s' - Q);   Q = alpha_k s' + (1 - alpha_k + 1e-10f) Q;
 *                         dx_k = dalpha * delta_k expf(-delta_k dens_k) * clamp'(x_k);
 *                         w_k = alpha_k T_k (+ 1 - sum w for k = S-1 under last_back);   dc_k = w_k G.
 * clamp' is 1 for x > 0 else 0 (relu), and 1 for x > 20 else 1 / (1 + expf(-x)) (softplus): cips_composite_bwd_geo's reverse scan
 * with the colour in place of the 32 features; opacity is sum w BEFORE the top-up, so go stays out of s_{S-1}.  No division.
 *   The scatter: a fetched sample adds omega (dc_k, dx_k) to each of its cell's eight nodes, omega the product over the axes of
 * t_a or 1 - t_a with the forward's t_a, by fp32 atomic adds: the last bits of dpacked can differ from call to call.  A sample
 * with w_k == 0 and dx_k == 0 adds nothing (under relu: all empty space and every clamped sample; the last sample under
 * last_back keeps its colour row through the top-up).  The skip bit has the forward's meaning: a skipped sample has x = 0,
 * c = 0 and receives nothing, which is exact for the same reason as in the forward; dpacked is the same set of non-zero nodes
 * with the bit set or clear.
 *   flags: the forward's bits 0..2, and bit 3 for the shape of the atomic adds, which changes nothing but their order: clear,
 * the four lanes of a quad exchange their values so that each atomic instruction covers whole 16-byte nodes; set, every lane
 * adds its own four dwords (kept for scripts/bench_volume_backward.py, which measures the two).
 *   scratch: cips_volume_render_bwd_scratch(b, H, W, S) bytes = S * threads * 16 with threads = 256 b ceil(tiles / 4),
 * tiles = ceil(W / 8) ceil(H / 8): one 16-byte record (alpha, T, s, x) per sample and thread, written by the thread's forward march
 * and read back by the same thread; -1 for sizes the entry point refuses.  Contents need not be initialised.
 *   dpacked is zeroed on the stream by the entry point, then one launch.  One ray per lane in 8 x 8 tiles as the forward, no LDS.
 * Invalid arguments return hipErrorInvalidValue before any HIP call: everything the forward refuses (flags outside 0..15 here),
 * a NULL drgb, dpacked or scratch, dpacked or scratch not 16-byte aligned.  Bv == 0 returns 0; b == 0 zeroes dpacked only.
 *
 * cips_volume_occupancy: bake's occ from a PACKED volume (sigma read at stride 4 by the kernel bake uses), for a volume whose
 * nodes have moved: the same bits as cips_volume_bake gives for the same sigma.  Refuses NULLs, a packed that is not 16-byte
 * aligned, n_a < 2, nx*ny*nz beyond int32, Bv < 0 with hipErrorInvalidValue before any HIP call; Bv == 0 returns 0. */
long long cips_volume_render_bwd_scratch(int b, int H, int W, int S);
int cips_volume_render_bwd(const void* packed, const float* occ, const float* lo, const float* hi, const float* xg,
                           const float* yg, const float* zg, const float* cam2world, float zc, int clamp_mode, int flags,
                           const float* drgb, const float* ddepth, const float* dopacity, void* dpacked, void* scratch, int b,
                           int Bv, int nx, int ny, int nz, int H, int W, int S, cips_stream_t stream);
int cips_volume_occupancy(const void* packed, float* occ, int Bv, int nx, int ny, int nz, cips_stream_t stream);

/* cips_volume_render_bwd_cam: the gradient of cips_volume_render's three outputs with respect to the CAMERAS, dcam2world (b,4,4)
 * fp32.  Arguments: cips_volume_render_bwd's, with dcam2world in place of dpacked.  Nothing flows to the nodes, zg or the box.
 *   The sample depths z_k are constants, as everywhere in this library, so ddepth and dopacity reach the camera only through
 * dx_k.  Per ray the march and the reverse scan are cips_volume_render_bwd's, with its w_k (top-up included), dx_k and live rule.
 * A live sample in cell (i, j, k) with weights t gathers the forward's eight corners again and forms the slope of the
 * interpolant v(t) = (c, sigma): dv/dt_a is the difference of the cell's two bilinear faces along axis a (exact for the
 * trilinear rule), and dv/dx_a = inv_h[a] dv/dt_a.  Then
 *     dp_k = w_k (G . grad c_k) + dx_k grad sigma_k;      A = sum_k dp_k;      B = sum_k z_k dp_k      (sample order S-1 .. 0)
 * and, with world = R (dir z_k) + t and dir the unit direction of ray_dir:
 *     dcam2world[:3,:3] = sum over rays of B dir^T;     dcam2world[:3,3] = sum over rays of A;     row 3 = 0
 * (cips_rays_bwd_cam's convention, without a per-point tensor).  A sample outside the box, skipped or not live adds nothing.
 *   No atomics.  One ray per lane in 8 x 8 tiles as the forward; the wave adds its rays' twelve products by a butterfly of
 * shuffles and stores one 12-float partial per tile; a second launch (one block per image) adds an image's tiles, lane l the
 * tiles l, l + 64, ... in order, then the same butterfly, and writes all 16 entries.  Hence the SAME BITS on every call; the
 * same bits with the skip bit set or clear (a skipped sample and a fetched sample that is not live both add nothing, and the
 * scan of the live ones does not see the difference: alpha = 0 leaves Q as it is); and the same bits for camera i of a Bv = 1
 * call as for that camera alone.  The interpolant is continuous but its slope is not: a sample within rounding of a cell face
 * may take the neighbouring cell's slope, and a sigma within rounding of 0 under relu either side of relu'.
 *   scratch: cips_volume_render_bwd_cam_scratch(b, H, W, S) bytes = the records of cips_volume_render_bwd_scratch followed by
 * 48 b tiles bytes of partials; -1 for sizes the entry point refuses, among them a size beyond int64.  16-byte aligned,
 * contents need not be initialised.  Two launches, no LDS.
 * Invalid arguments return hipErrorInvalidValue before any HIP call: everything the forward refuses (flags outside 0..7), a
 * NULL drgb, dcam2world or scratch, a scratch that is not 16-byte aligned or whose size overflows.  b == 0 returns 0. */
long long cips_volume_render_bwd_cam_scratch(int b, int H, int W, int S);
int cips_volume_render_bwd_cam(const void* packed, const float* occ, const float* lo, const float* hi, const float* xg,
                               const float* yg, const float* zg, const float* cam2world, float zc, int clamp_mode, int flags,
                               const float* drgb, const float* ddepth, const float* dopacity, float* dcam2world, void* scratch,
                               int b, int Bv, int nx, int ny, int nz, int H, int W, int S, cips_stream_t stream);

/* Baked FEATURE volumes (csrc/volume.hip): the SIREN's 32 colour features on the lattice in place of a colour, composited per
 * ray into the pixel rows the INR head takes, so that a view of a baked identity is forward()'s picture and costs a
 * gather-and-composite pass plus one head pass.  Forward only: nothing here has a gradient.  A feature volume is
 *   sigma  (Bv,nx,ny,nz) fp32;
 *   planes (Bv,8,nx,ny,nz,4) fp32, 16-byte aligned: channel-group-major planes of 16-byte records, group g holding channels
 *          4g .. 4g+3 of a node — every plane has cips_volume_bake's packed layout (z-neighbours 32 contiguous bytes apart);
 *   occ    cips_volume_bake's brick maxima of sigma, same shape and bits.
 * The volume is taken to be finite (sigma and features): the occupancy drops a NaN, and the weight skip below relies on
 * 0 * f == 0.
 *
 * cips_feature_volume_bake: feat_rows (Bv, nx*ny*nz, 32), the layout NeRFNetwork.evaluate returns (16-byte aligned), is
 * transposed into planes: planes[v][g][n] = feat_rows[v][n][4g .. 4g+3].  Bits are copied, nothing is computed.  occ is written
 * by cips_volume_bake's occupancy kernel reading sigma at stride 1.  Two launches.
 * cips_feature_volume_bake_slab: the same for the x-planes x0 .. x0+sx-1 only, so that a caller can evaluate the lattice a slab at
 * a time: feat_rows is (Bv, sx*ny*nz, 32) and lands in planes[v][g][x0 .. x0+sx-1]; planes, sigma, occ, nx, ny, nz are the WHOLE
 * volume's.  occ is written only by the call with x0 + sx == nx, from the whole sigma, which the caller has completed by then.
 * cips_feature_volume_bake is the slab call with x0 = 0, sx = nx.
 * Invalid arguments return hipErrorInvalidValue before any HIP call: a NULL pointer; n_a < 2; Bv < 0; nx*ny*nz beyond int32;
 * planes or feat_rows not 16-byte aligned; a grid beyond int32 (Bv*sx*ny*nz/32 blocks); (slab) x0 < 0, sx < 1 or x0 + sx > nx.
 * Bv == 0 returns 0 and launches nothing.
 *
 * cips_feature_volume_render: cips_volume_render's rule, word for word, with 32 channels in place of 3: the same ray_dir and
 * ray_point for pixel (r, c) and depth zg[s]; the same inside test, cell and t_a from lo, hi and inv_h; sigma interpolated from
 * `sigma` and every channel from its group's plane by the same nested lerps p + t (q - p) along z, then y, then x; a sample
 * outside has sigma = 0 and features 0; the same delta, alpha, w_s = alpha_s fp32(T_s) with T in double; opacity = sum w before
 * any top-up, accumulated as fmaf(alpha_s, fp32(T_s), opacity) — the form cips_volume_render's sum takes once compiled, written
 * out here; flags bit 0 (last_back): the last sample's weight gains 1 - sum w (as a second fmaf per channel, after the sum,
 * and on the depth); fea = sum w f, depth = sum w z, in sample order by fmaf; flags bit 1 (white_back): 1 - sum w is added to
 * every one of the 32 channels, as cips_composite_fwd does for features; flags bit 2 (skip), relu only and IGNORED under
 * clamp_mode 1 as there: a sample whose brick has occ <= 0 does not gather its sigma (exact for the reason given there), the last
 * sample under last_back excepted.
 *   The weight skip, always on: a sample gathers its eight feature groups only if its weight w_s is not zero (the last sample
 * under last_back: if w_s or 1 - sum w is not zero).  fmaf(0, f, c) == c bit for bit for a finite f, so the skip is exact; it is
 * finer than the brick skip (it also drops clamped samples in occupied bricks) and ends a ray's feature traffic once fp32(T)
 * has reached 0.  Hence the same bits with the skip bit set or clear, on every call, and for camera i of a Bv = 1 call as for that
 * camera alone; and with planes whose every group is a packed (r, g, b, x) volume and sigma that volume's, fea[..., 4g .. 4g+2]
 * is cips_volume_render's rgb bit for bit.
 *   Outputs: fea (b, H*W, 32) pixel-major, 16-byte aligned — each lane stores its 128 contiguous bytes; depth (b,1,H,W);
 * opacity (b,1,H,W).  Bv is 1 (every camera sees volume 0) or b.  One ray per lane in 8 x 8 tiles, one launch, no LDS, no
 * scratch memory, no atomics, no S-sized buffer.
 * Invalid arguments return hipErrorInvalidValue before any HIP call: everything cips_volume_render refuses, with planes in
 * packed's place — a NULL pointer (occ may be NULL only with the skip bit clear); n_a < 2; H, W or S < 2; b or Bv < 0, Bv not in
 * {1, b}; lo / hi not finite or hi <= lo; zc >= 0, NaN or -inf; clamp_mode not 0 or 1; flags outside 0..7; planes or fea not
 * 16-byte aligned; nx*ny*nz, b*H*W or H*W*S beyond int32.  b == 0 returns 0 and launches nothing. */
int cips_feature_volume_bake(const float* sigma, const float* feat_rows, void* planes, float* occ, int Bv, int nx, int ny,
                             int nz, cips_stream_t stream);
int cips_feature_volume_bake_slab(const float* sigma, const float* feat_rows, void* planes, float* occ, int Bv, int nx, int ny,
                                  int nz, int x0, int sx, cips_stream_t stream);
int cips_feature_volume_render(const float* sigma, const void* planes, const float* occ, const float* lo, const float* hi,
                               const float* xg, const float* yg, const float* zg, const float* cam2world, float zc,
                               int clamp_mode, int flags, float* fea, float* depth, float* opacity, int b, int Bv, int nx, int ny,
                               int nz, int H, int W, int S, cips_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CIPS3D_HIP_H */
