// siren_bwd_x4.inc — round-4 schedule of the fused FiLM-SIREN backward (textually included by siren_bwd_x3.hip; same
// math, LDS images, staging windows, accumulator ownership and partial-sum layout as siren_bwd_x3_kernel above — the
// reference is exp/cips3d/models/generator.py:260-317 and exp/comm/models/film_layer.py:78-107).  What changed:
//  * the five dense layers of the data chain run m-major with the PREVIOUS output tile's epilogue (FiLM, sine / cosine,
//    hi / lo split) woven between the MFMAs of the current tile, five or six VALU instructions per MFMA
//    (run_layer_mm; scripts/probe/issue_overlap_probe.hip is the measurement behind it);
//  * with hardware trigonometry (HW) the sine arguments are in revolutions (stage_weights_x3<true>): v_fract + v_sin,
//    no multiply, no rint / subtract.  The backward chain carries the factor: d h2, d a2 and d p2 are 1/(2 pi) of their
//    values, d h1 and d a1 1/(2 pi)^2; the weight-gradient and column-sum accumulators they feed are multiplied back when the
//    workgroup writes its partials (the partials keep their documented meaning).
// Values computed in a slot are pinned there: sched_barrier(0) only binds the machine scheduler, and hipcc's IR-level sinking
// otherwise moves the whole (side-effect-free) epilogue below the layer's MFMAs, next to its first use.
__device__ __forceinline__ void pinf(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pinf(float& a, float& b) { asm volatile("" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void pinf(float& a, float& b, float& c, float& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
__device__ __forceinline__ void pinu(unsigned& a, unsigned& b) { asm volatile("" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void pinu(unsigned& a, unsigned& b, unsigned& c, unsigned& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }

// (siren_bwd_x3.hip's sincos_rev repeats this expression for its sine: a change here goes there too)
template <bool HW> __device__ __forceinline__ float sin_rev(float x) {
  if (HW) return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(x));
  float s_, c_; sincos_reduced(reduce_2pi(x), &s_, &c_); return s_;
}

// MODE X3_LIVE: the workgroup walks a list of point indices instead of a contiguous range (cips_siren_bwd_x3_live in
// cips3d_hip.h).  Image b's list is a.idx[b * P + 0 .. a.count[b]); workgroup (c, b) takes the slots
// [c * len, min((c + 1) * len, count[b])), len = ceil(count[b] / chunks) rounded up to whole 128-point rounds.  cstart / cend /
// pbase then count list SLOTS, and the three places that form a point index look it up; everything else in a round is the dense
// kernel's.  The trip count comes from device memory, so a replayed graph follows the data.  With every point listed in order
// the partition is the dense one whenever the dense chunk is a multiple of 128 that divides P, and the partials are
// bit-identical.
// MODE X3_EVEN: the same list walk, but image, first slot and end slot of the workgroup come from row (flat workgroup id) of the
// table a.seg that cips_siren_bwd_x3_live_plan wrote (x3_even_plan above: every workgroup of the launch gets about the same
// number of rounds, whatever its image's live share), and the partials go to row = flat id.  An idle id (image -1) leaves
// before anything is staged; the table row is the same for every thread, so the workgroup leaves together.
template <bool HW, int MODE>
__global__ __launch_bounds__(256, 1) void siren_bwd_x4_kernel(BwdX3Args a) {
  extern __shared__ __attribute__((aligned(1024))) uchar smem[];
  constexpr bool LIVE = MODE != X3_DENSE;
  int b_ = blockIdx.y, prow_ = 0, cs_ = 0, ce_ = 0;
  if constexpr (MODE == X3_EVEN) {
    prow_ = blockIdx.y * gridDim.x + blockIdx.x;
    const int* const sg = a.seg + 4 * (long long)prow_;
    b_ = __builtin_amdgcn_readfirstlane(sg[0]);
    if (b_ < 0) return;
    cs_ = __builtin_amdgcn_readfirstlane(sg[1]);
    ce_ = __builtin_amdgcn_readfirstlane(sg[2]);
  }
  const int b = b_;
  stage_weights_x3<HW>(smem, a.w, b);
  __syncthreads();
  constexpr float TWO_PI = 6.283185307179586f;

  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int cstart = blockIdx.x * a.chunk;
  int cend = min(cstart + a.chunk, a.P);
  if constexpr (MODE == X3_EVEN) {
    cstart = cs_; cend = ce_;
  } else if (LIVE) {
    const int cnt = a.count[b];
    const int len = ((cnt + a.chunks - 1) / a.chunks + 127) & ~127;
    cstart = blockIdx.x * len;
    cend = min(cstart + len, cnt);          // >= 1 unless the image has no live point at all
  }
  const int* const lidx = LIVE ? a.idx + (long long)b * a.P : nullptr;
  const unsigned sbase = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);

  // weight-gradient accumulators, owned per wave for the whole chunk; aS: column sums (see SRED)
  f32x16 aG1[4], aGc[2], aGf[1], aS[1];
  zero_acc(aG1); zero_acc(aGc); zero_acc(aGf); zero_acc(aS);
  float r_dsg = 0.f;

  // inputs of the first round
  float px, py, pz, dsg;
  {
    const int slot = cstart + wave * 32 + (lane0 & 31);
    const bool valid = slot < cend;
    int p = valid ? slot : cend - 1;
    if (LIVE) p = cend > 0 ? lidx[p] : 0;   // an image without live points: no list entry is defined, any point will do
    const long long gp = (long long)b * a.P + p;
    if (a.points) { px = a.points[gp * 3 + 0]; py = a.points[gp * 3 + 1]; pz = a.points[gp * 3 + 2]; }
    else gen_point(a.rg, b, p, px, py, pz);
    dsg = valid ? a.dsigma[gp] : 0.f;
  }

  // The first NPRE of layer 0's 16 feature groups of the NEXT round's points are produced inside the dW1 phase of the current
  // round, by the three waves that would otherwise wait at the barrier while the fourth stages its operands (a third each; the
  // first round's come from this prologue); the rest is computed at the start of the round.  NPRE trades idle-slot use against
  // the registers that carry the packed sines across the phase and the round boundary.  Measured (forward + backward at C2,
  // one box each, profiles/r4_siren_bwd_ab_microbench.log): NPRE 16 -> 161 spilled VGPRs, 3.15 ms; 8 -> 94, 3.03 ms; 4 -> 61,
  // 3.02 ms; 0 -> 39, 2.90 ms (2.97 with the dW1 loop rolled): the spill traffic lands in the layer-1 recompute and costs more
  // than the idle slots give, so the shipped value is 0 — the mechanism stays for a chain with a smaller register footprint.
  constexpr int NPRE = 0;
  Act<4> h1n;
  auto l0_groups = [&](auto G0c, auto G1c, float x, float y, float z) __attribute__((always_inline)) {
    constexpr int G0 = decltype(G0c)::value, G1 = decltype(G1c)::value;
    if (G0 >= G1) return;
    int ln = lane0;
    asm volatile("" : "+v"(ln));
    const unsigned sbase_ = (unsigned)(uintptr_t)((__attribute__((address_space(3))) uchar*)smem);
    const unsigned v64 = opaque(sbase_ + O_L0 + 64 * (ln >> 5));
    float4 pn[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) pn[e] = lds_ld4(v64 + 128 * G0 + 16 * e);
#pragma unroll
    for (int grp = G0; grp < G1; ++grp) {          // grp = 4q + g: features 32q + 8g + 4hf + {0..3}
      float4 pk[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = pn[e];
      if (grp + 1 < G1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) pn[e] = lds_ld4(v64 + 128 * (grp + 1) + 16 * e);
      }
      __builtin_amdgcn_sched_barrier(0);
      float s4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) s4[e] = sin_rev<HW>(fmaf(pk[e].x, x, fmaf(pk[e].y, y, fmaf(pk[e].z, z, pk[e].w))));
      const int q = grp >> 2, g = grp & 3;
      split2(s4[0], s4[1], h1n.hi[q][2 * g], h1n.lo[q][2 * g]);
      split2(s4[2], s4[3], h1n.hi[q][2 * g + 1], h1n.lo[q][2 * g + 1]);
      pinu(h1n.hi[q][2 * g], h1n.lo[q][2 * g], h1n.hi[q][2 * g + 1], h1n.lo[q][2 * g + 1]);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  using IC0 = std::integral_constant<int, 0>; using ICA = std::integral_constant<int, (NPRE + 2) / 3>;
  using ICB = std::integral_constant<int, (2 * NPRE + 2) / 3>; using ICN = std::integral_constant<int, NPRE>;
  using IC16 = std::integral_constant<int, 16>;
  l0_groups(IC0{}, ICN{}, px, py, pz);

  int rnd = -1;
  for (int pbase = cstart; pbase < cend; pbase += 128) {
    ++rnd;
    X3_TS(0)
    // every LDS address below is loop-invariant; laundering the lane id keeps hipcc from hoisting a few hundred
    // of them out of the loop into live registers
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int l31 = lane & 31, hf = lane >> 5;
    const LaneAddr LA = lane_addr(lane, sbase);
    const int prow = wave * 32 + l31;
    const unsigned c7 = l31 & 7;
    const unsigned m_d1 = c7 < 4 ? ~0u : 0u, m_d2 = c7 == 4 ? ~0u : 0u, m_h2 = c7 == 5 ? ~0u : 0u;
    const unsigned m_dc = c7 == 6 ? ~0u : 0u, m_df = c7 == 7 ? ~0u : 0u;

    // ---- upstream gradient of the 32 colour features: requested now, consumed after two layers ----
    float4 df4[4];
    {
      const int slot = pbase + prow;
      const bool valid = slot < cend;
      int p = valid ? slot : cend - 1;
      if (LIVE) p = lidx[p];
      const float* dp = a.dfeat + ((long long)b * a.P + p) * CF + 4 * hf;
#pragma unroll
      for (int g = 0; g < 4; ++g) df4[g] = valid ? ld4(dp + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- aux row of this point: [1, x, y, z, 1, dsigma, 1, 1] ----
    if (hf == 0) {
      uint4 ah, al;
      split2(1.f, px, ah.x, al.x); split2(py, pz, ah.y, al.y); split2(1.f, dsg, ah.z, al.z); split2(1.f, 1.f, ah.w, al.w);
      const u32x4 vh = {ah.x, ah.y, ah.z, ah.w}, vl = {al.x, al.y, al.z, al.w};
      *LDS_PTR(u32x4, sbase + O_AUX + prow * 16) = vh;
      *LDS_PTR(u32x4, sbase + O_AUX + 2048 + prow * 16) = vl;
      r_dsg += dsg;
    }

    // ws * dsigma enters d h2, which this kernel carries as d h2 / (2 pi) when the images are pre-scaled
    const float dsg_s = HW ? dsg * CIPS_INV_2PI : dsg;

    // ---- layer 0 (VALU); only the packed sines are kept, and only until layer 1 has consumed them ----
    f32x16 acc[4];
    zero_acc(acc);
    float cs2[4][16];
    Act<4> h2p;
    // state of the woven epilogues (one group of 4 features at a time)
    float rv[4], sn[4];
    float4 gq, cq;
    // FiLM + sine / cosine + split of features (q, g) of layer 1's output, in six slots of ~30 issue cycles
    auto film2_slot = [&](int q, int g, int j) __attribute__((always_inline)) {
      const float gg[4] = {gq.x, gq.y, gq.z, gq.w}, cc[4] = {cq.x, cq.y, cq.z, cq.w};
      if (HW) {
        if (j == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) rv[e] = fmaf(gg[e], acc[q][4 * g + e], cc[e]);
          rv[0] = __builtin_amdgcn_fractf(rv[0]); rv[1] = __builtin_amdgcn_fractf(rv[1]);
          pinf(rv[0], rv[1], rv[2], rv[3]);
        } else if (j == 1) {
          rv[2] = __builtin_amdgcn_fractf(rv[2]); rv[3] = __builtin_amdgcn_fractf(rv[3]);
          sn[0] = __builtin_amdgcn_sinf(rv[0]); sn[1] = __builtin_amdgcn_sinf(rv[1]);
          pinf(rv[2], rv[3], sn[0], sn[1]);
        } else if (j == 2) {
          cs2[q][4 * g + 0] = __builtin_amdgcn_cosf(rv[0]); cs2[q][4 * g + 1] = __builtin_amdgcn_cosf(rv[1]);
          sn[2] = __builtin_amdgcn_sinf(rv[2]);
          pinf(cs2[q][4 * g + 0], cs2[q][4 * g + 1]); pinf(sn[2]);
        } else if (j == 3) {
          sn[3] = __builtin_amdgcn_sinf(rv[3]);
          cs2[q][4 * g + 2] = __builtin_amdgcn_cosf(rv[2]); cs2[q][4 * g + 3] = __builtin_amdgcn_cosf(rv[3]);
          pinf(cs2[q][4 * g + 2], cs2[q][4 * g + 3]); pinf(sn[3]);
        }
      } else if (j == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bsincos<false>(fmaf(gg[e], acc[q][4 * g + e], cc[e]), &sn[e], &cs2[q][4 * g + e]);
        pinf(sn[0], sn[1], sn[2], sn[3]);
      }
      if (j == 4) { split2(sn[0], sn[1], h2p.hi[q][2 * g], h2p.lo[q][2 * g]); pinu(h2p.hi[q][2 * g], h2p.lo[q][2 * g]); }
      if (j == 5) {
        split2(sn[2], sn[3], h2p.hi[q][2 * g + 1], h2p.lo[q][2 * g + 1]);
        pinu(h2p.hi[q][2 * g + 1], h2p.lo[q][2 * g + 1]);
        if (4 * q + g + 1 < 16) {               // next group's gains / offsets
          gq = lds_ld4(LA.v16 + (O_G1 - O_L0) + 32 * (4 * q + g + 1)); cq = lds_ld4(LA.v16 + (O_C1 - O_L0) + 32 * (4 * q + g + 1));
        }
      }
    };
    {
      l0_groups(ICN{}, IC16{}, px, py, pz);      // the groups the previous round's idle slots did not cover
      gq = lds_ld4(LA.v16 + (O_G1 - O_L0)); cq = lds_ld4(LA.v16 + (O_C1 - O_L0));
      // ---- recompute layer 1, m-major: the slots of tile m carry the epilogue of tile m - 1 ----
      layer_fwd_mm<4, 4, H, O_W1H, O_W1L - O_W1H>(LA, h1n, acc, [&](int slot) __attribute__((always_inline)) {
        const int m = slot / 24, j = slot % 24;
        if (m >= 1) film2_slot(m - 1, j / 6, j % 6);
      });
    }
    X3_TS(1)
    // tile 3 of layer 1: its first group here, the other three under the colour layer's first six k-steps (which read h2 tiles
    // 0..2; k-steps 6 and 7 read tile 3 and come after slot 17)
#pragma unroll
    for (int j = 0; j < 6; ++j) { film2_slot(3, 0, j); __builtin_amdgcn_sched_barrier(0); }

    X3_TS(2)
    // ---- recompute colour sine layer, m-major ----
    f32x16 accc[2];
    zero_acc(accc);
    float csc[2][16];
    Act<2> hcp;
    float4 gcq, ccq;
    auto filmc_slot = [&](int q, int g, int j) __attribute__((always_inline)) {
      const float gg[4] = {gcq.x, gcq.y, gcq.z, gcq.w}, cc[4] = {ccq.x, ccq.y, ccq.z, ccq.w};
      if (HW) {
        if (j == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) rv[e] = fmaf(gg[e], accc[q][4 * g + e], cc[e]);
          rv[0] = __builtin_amdgcn_fractf(rv[0]); rv[1] = __builtin_amdgcn_fractf(rv[1]);
          pinf(rv[0], rv[1], rv[2], rv[3]);
        } else if (j == 1) {
          rv[2] = __builtin_amdgcn_fractf(rv[2]); rv[3] = __builtin_amdgcn_fractf(rv[3]);
          sn[0] = __builtin_amdgcn_sinf(rv[0]); sn[1] = __builtin_amdgcn_sinf(rv[1]);
          pinf(rv[2], rv[3], sn[0], sn[1]);
        } else if (j == 2) {
          csc[q][4 * g + 0] = __builtin_amdgcn_cosf(rv[0]); csc[q][4 * g + 1] = __builtin_amdgcn_cosf(rv[1]);
          sn[2] = __builtin_amdgcn_sinf(rv[2]);
          pinf(csc[q][4 * g + 0], csc[q][4 * g + 1]); pinf(sn[2]);
        } else if (j == 3) {
          sn[3] = __builtin_amdgcn_sinf(rv[3]);
          csc[q][4 * g + 2] = __builtin_amdgcn_cosf(rv[2]); csc[q][4 * g + 3] = __builtin_amdgcn_cosf(rv[3]);
          pinf(csc[q][4 * g + 2], csc[q][4 * g + 3]); pinf(sn[3]);
        }
      } else if (j == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bsincos<false>(fmaf(gg[e], accc[q][4 * g + e], cc[e]), &sn[e], &csc[q][4 * g + e]);
        pinf(sn[0], sn[1], sn[2], sn[3]);
      }
      if (j == 4) { split2(sn[0], sn[1], hcp.hi[q][2 * g], hcp.lo[q][2 * g]); pinu(hcp.hi[q][2 * g], hcp.lo[q][2 * g]); }
      if (j == 5) {
        split2(sn[2], sn[3], hcp.hi[q][2 * g + 1], hcp.lo[q][2 * g + 1]);
        pinu(hcp.hi[q][2 * g + 1], hcp.lo[q][2 * g + 1]);
        if (4 * q + g + 1 < 8) {
          gcq = lds_ld4(LA.v16 + (O_GC - O_L0) + 32 * (4 * q + g + 1)); ccq = lds_ld4(LA.v16 + (O_CC - O_L0) + 32 * (4 * q + g + 1));
        }
      }
    };
    gcq = lds_ld4(LA.v16 + (O_GC - O_L0)); ccq = lds_ld4(LA.v16 + (O_CC - O_L0));
    layer_fwd_mm<2, 4, HC, O_WCH, O_WCL - O_WCH>(LA, h2p, accc, [&](int slot) __attribute__((always_inline)) {
      if (slot < 18) film2_slot(3, 1 + slot / 6, slot % 6);
      else if (slot >= 24) filmc_slot(0, (slot - 24) / 6, (slot - 24) % 6);
    });
#pragma unroll
    for (int j = 0; j < 24; ++j) { filmc_slot(1, j / 6, j % 6); __builtin_amdgcn_sched_barrier(0); }

    X3_TS(3)
    Act<1> dfp;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      split2(df4[g].x, df4[g].y, dfp.hi[0][2 * g], dfp.lo[0][2 * g]);
      split2(df4[g].z, df4[g].w, dfp.hi[0][2 * g + 1], dfp.lo[0][2 * g + 1]);
    }

    // ---- dWf += dfeat^T hc over the workgroup's 128 points: wave -> (hc column tile w&1, point half w>>1);
    //      waves 0 and 2 also take sum_p dfeat (aux column 7) ----
    if (!CIPS_TUNE(a.dbg & 1)) {
      constexpr int DFH = 0, DFL = 8192, HCH = 16384, HCL = 32768;
      stage<1, 128, DFH, DFL>(sbase, prow, hf, dfp);
      stage<2, 128, HCH, HCL>(sbase, prow, hf, hcp);
      __syncthreads();
      const int jt = wave & 1, kh = wave >> 1;
      const unsigned mdf = jt == 0 ? m_df : 0u;          // waves 1 and 3 add zeros: no wave-dependent branches here
      Frag fa[2], fb[2], fx[2];
      // this wave's k-steps (4kh + k) and hc column block are folded into the lane bases
      const unsigned d0 = opaque(LA.sb[0] + kh * 4096), d1 = opaque(LA.sb[1] + kh * 4096);      // dfeat: k-steps 4kh..
      const unsigned h0 = opaque(d0 + jt * 8192), h1_ = opaque(d1 + jt * 8192);                  // hc: same k-steps, column block jt
      const unsigned ax = opaque(LA.ab + kh * 1024);
      stg_frag<128, DFH, DFL>(d0, d1, 0, 0, fa[0]);
      stg_frag<128, HCH, HCL>(h0, h1_, 0, 0, fb[0]);
      aux_frag(ax, 0, mdf, fx[0]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k + 1 < 4) {
          stg_frag<128, DFH, DFL>(d0, d1, 0, k + 1, fa[(k + 1) & 1]);
          stg_frag<128, HCH, HCL>(h0, h1_, 0, k + 1, fb[(k + 1) & 1]);
          aux_frag(ax, k + 1, mdf, fx[(k + 1) & 1]);
        }
        __builtin_amdgcn_sched_barrier(0);
        aGf[0] = x3f(aGf[0], fa[k & 1], fb[k & 1]);
        aS[0] = x2f(aS[0], fa[k & 1], fx[k & 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }

    X3_TS(4)
    // ---- d hc = Wf^T dfeat  (K = 32, M = 64);  dac = d hc * cos;  dpc = gc * dac ----
    zero_acc(accc);
    layer_tr<2, 2, CF, O_WFH, O_WFL - O_WFH>(LA, dfp, accc);
    Act<2> dacp, dpcp;
    {
      float4 gn = lds_ld4(LA.v16 + (O_GC - O_L0));
#pragma unroll
      for (int grp = 0; grp < 8; ++grp) {
        const float4 g4 = gn;
        if (grp + 1 < 8) gn = lds_ld4(LA.v16 + (O_GC - O_L0) + 32 * (grp + 1));
        __builtin_amdgcn_sched_barrier(0);
        const int q = grp >> 2, g = grp & 3;
        const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
        float v[4], w_[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = accc[q][4 * g + e] * csc[q][4 * g + e]; w_[e] = gg[e] * v[e]; }
        split2(v[0], v[1], dacp.hi[q][2 * g], dacp.lo[q][2 * g]);
        split2(v[2], v[3], dacp.hi[q][2 * g + 1], dacp.lo[q][2 * g + 1]);
        split2(w_[0], w_[1], dpcp.hi[q][2 * g], dpcp.lo[q][2 * g]);
        split2(w_[2], w_[3], dpcp.hi[q][2 * g + 1], dpcp.lo[q][2 * g + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    pin(dacp); pin(h2p);
    X3_TS(5)
    // ---- dWc += dac^T h2: two sub-phases of 64 points; wave -> (dac row tile w&1, h2 column tiles 2(w>>1)+{0,1});
    //      plus sum_p dsigma*h2 (h2 row tile w, aux column 5) and, on waves 0 and 1, sum_p dac (aux column 6).
    //      Fragment reads run half a k-step ahead of their MFMAs. ----
    if (!CIPS_TUNE(a.dbg & 2)) {
      constexpr int DAH = 0, DAL = 8192, H2H = 16384, H2L = 32768;
      const int it = wave & 1, jt0 = 2 * (wave >> 1);
      const unsigned mdc = wave < 2 ? m_dc : 0u;         // waves 2 and 3 add zeros: no wave-dependent branches here
      // wave-dependent column blocks folded into the lane bases (block stride of a 64-row image: 4096 B)
      const unsigned i0 = opaque(LA.sb[0] + it * 4096), i1 = opaque(LA.sb[1] + it * 4096);
      const unsigned j0 = opaque(LA.sb[0] + jt0 * 4096), j1 = opaque(LA.sb[1] + jt0 * 4096);
      const unsigned w0 = opaque(LA.sb[0] + wave * 4096), w1 = opaque(LA.sb[1] + wave * 4096);
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        if ((wave >> 1) == sp) {
          stage<2, 64, DAH, DAL>(sbase, (wave & 1) * 32 + l31, hf, dacp);
          stage<4, 64, H2H, H2L>(sbase, (wave & 1) * 32 + l31, hf, h2p);
        }
        __syncthreads();
        Frag fa, fb0, fb1, fh, fx, fy;
        stg_frag<64, DAH, DAL>(i0, i1, 0, 0, fa);
        stg_frag<64, H2H, H2L>(j0, j1, 0, 0, fb0);
        stg_frag<64, H2H, H2L>(j0, j1, 32, 0, fb1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          stg_frag<64, H2H, H2L>(w0, w1, 0, k, fh);
          aux_frag(LA.ab, 4 * sp + k, m_h2, fx);
          aux_frag(LA.ab, 4 * sp + k, mdc, fy);
          __builtin_amdgcn_sched_barrier(0);
          aGc[0] = x3f(aGc[0], fa, fb0);
          aGc[1] = x3f(aGc[1], fa, fb1);
          aS[0] = x2f(aS[0], fa, fy);
          __builtin_amdgcn_sched_barrier(0);
          if (k + 1 < 4) {
            stg_frag<64, DAH, DAL>(i0, i1, 0, k + 1, fa);
            stg_frag<64, H2H, H2L>(j0, j1, 0, k + 1, fb0);
            stg_frag<64, H2H, H2L>(j0, j1, 32, k + 1, fb1);
          }
          __builtin_amdgcn_sched_barrier(0);
          aS[0] = x3f(aS[0], fh, fx);
          __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
      }
    }

    X3_TS(6)
    // ---- d h2 = Wc^T dpc + ws * dsigma  (K = 64, M = 128), m-major;  da2 = d h2 * cos;  dp2 = g1 * da2.  A tile has only
    //      12 MFMA slots here (4 k-steps) against ~36 VALU instructions per group: three slots per group, VALU-bound ----
    zero_acc(acc);
    Act<4> da2p;
    Act<4> h1p;
    Act<4> da1p;                         // consumed tile by tile inside the d h1 layer (da1_sums): never 64 live registers
    float npx, npy, npz, ndsg;
    {
      Act<4> dp2p;
      float v4[4], w4_[4];
      float4 gq2, wq2;
      auto dh2_slot = [&](int q, int g, int j) __attribute__((always_inline)) {
        if (j == 0) {
          const float gg[4] = {gq2.x, gq2.y, gq2.z, gq2.w}, ww[4] = {wq2.x, wq2.y, wq2.z, wq2.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v4[e] = fmaf(ww[e], dsg_s, acc[q][4 * g + e]) * cs2[q][4 * g + e];
            w4_[e] = gg[e] * v4[e];
          }
          pinf(v4[0], v4[1], v4[2], v4[3]); pinf(w4_[0], w4_[1], w4_[2], w4_[3]);
          if (4 * q + g + 1 < 16) {
            gq2 = lds_ld4(LA.v16 + (O_G1 - O_L0) + 32 * (4 * q + g + 1)); wq2 = lds_ld4(LA.v16 + (O_WS - O_L0) + 32 * (4 * q + g + 1));
          }
        } else if (j == 1) {
          split2(v4[0], v4[1], da2p.hi[q][2 * g], da2p.lo[q][2 * g]);
          split2(v4[2], v4[3], da2p.hi[q][2 * g + 1], da2p.lo[q][2 * g + 1]);
          pinu(da2p.hi[q][2 * g], da2p.lo[q][2 * g], da2p.hi[q][2 * g + 1], da2p.lo[q][2 * g + 1]);
        } else {
          split2(w4_[0], w4_[1], dp2p.hi[q][2 * g], dp2p.lo[q][2 * g]);
          split2(w4_[2], w4_[3], dp2p.hi[q][2 * g + 1], dp2p.lo[q][2 * g + 1]);
          pinu(dp2p.hi[q][2 * g], dp2p.lo[q][2 * g], dp2p.hi[q][2 * g + 1], dp2p.lo[q][2 * g + 1]);
        }
      };
      gq2 = lds_ld4(LA.v16 + (O_G1 - O_L0)); wq2 = lds_ld4(LA.v16 + (O_WS - O_L0));
      layer_tr_mm<4, 4, HC, O_WCH, O_WCL - O_WCH>(LA, dpcp, acc, [&](int slot) __attribute__((always_inline)) {
        const int m = slot / 12, j = slot % 12;
        if (m >= 1) dh2_slot(m - 1, j / 3, j % 3);
      });
#pragma unroll
      for (int j = 0; j < 12; ++j) { dh2_slot(3, j / 3, j % 3); __builtin_amdgcn_sched_barrier(0); }

      // ---- inputs of the next round: requested here, a whole layer before their first use (layer 0 of the next round inside
      //      the dW1 phase below) ----
      {
        const int slot = pbase + 128 + prow;
        const bool valid = slot < cend;
        int p = valid ? slot : cend - 1;
        if (LIVE) p = lidx[p];
        const long long gp = (long long)b * a.P + p;
        if (a.points) { npx = a.points[gp * 3 + 0]; npy = a.points[gp * 3 + 1]; npz = a.points[gp * 3 + 2]; }
        else gen_point(a.rg, b, p, npx, npy, npz);
        ndsg = valid ? a.dsigma[gp] : 0.f;
      }
      // ---- d h1 = W1^T dp2  (K = 128, M = 128), m-major;  da1 = d h1 * cos(layer-0 argument), the layer-0 sines recomputed
      //      alongside for dW1: ~52 VALU instructions per group of 4 features in six slots ----
      f32x16 acc1[4];
      zero_acc(acc1);
      float4 pq[4];
      float ar[4], s1[4], c1[4], d1[4];
      auto dh1_slot = [&](int q, int g, int j) __attribute__((always_inline)) {
        if (j == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ar[e] = fmaf(pq[e].x, px, fmaf(pq[e].y, py, fmaf(pq[e].z, pz, pq[e].w)));
          pinf(ar[0], ar[1], ar[2], ar[3]);
          if (4 * q + g + 1 < 16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) pq[e] = lds_ld4(LA.v64 + 128 * (4 * q + g + 1) + 16 * e);
          }
        } else if (j == 1) {
          if (HW) {
#pragma unroll
            for (int e = 0; e < 4; ++e) ar[e] = __builtin_amdgcn_fractf(ar[e]);
            s1[0] = __builtin_amdgcn_sinf(ar[0]); s1[1] = __builtin_amdgcn_sinf(ar[1]);
            pinf(ar[0], ar[1], ar[2], ar[3]); pinf(s1[0], s1[1]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) bsincos<false>(ar[e], &s1[e], &c1[e]);
            pinf(s1[0], s1[1], s1[2], s1[3]); pinf(c1[0], c1[1], c1[2], c1[3]);
          }
        } else if (j == 2) {
          if (HW) {
            s1[2] = __builtin_amdgcn_sinf(ar[2]); s1[3] = __builtin_amdgcn_sinf(ar[3]);
            c1[0] = __builtin_amdgcn_cosf(ar[0]); c1[1] = __builtin_amdgcn_cosf(ar[1]);
            pinf(s1[2], s1[3], c1[0], c1[1]);
          }
        } else if (j == 3) {
          if (HW) { c1[2] = __builtin_amdgcn_cosf(ar[2]); c1[3] = __builtin_amdgcn_cosf(ar[3]); }
#pragma unroll
          for (int e = 0; e < 4; ++e) d1[e] = acc1[q][4 * g + e] * c1[e];
          pinf(d1[0], d1[1], d1[2], d1[3]);
        } else if (j == 4) {
          split2(s1[0], s1[1], h1p.hi[q][2 * g], h1p.lo[q][2 * g]);
          split2(s1[2], s1[3], h1p.hi[q][2 * g + 1], h1p.lo[q][2 * g + 1]);
          pinu(h1p.hi[q][2 * g], h1p.lo[q][2 * g], h1p.hi[q][2 * g + 1], h1p.lo[q][2 * g + 1]);
        } else {
          split2(d1[0], d1[1], da1p.hi[q][2 * g], da1p.lo[q][2 * g]);
          split2(d1[2], d1[3], da1p.hi[q][2 * g + 1], da1p.lo[q][2 * g + 1]);
          pinu(da1p.hi[q][2 * g], da1p.lo[q][2 * g], da1p.hi[q][2 * g + 1], da1p.lo[q][2 * g + 1]);
        }
      };
#pragma unroll
      for (int e = 0; e < 4; ++e) pq[e] = lds_ld4(LA.v64 + 16 * e);
      // sum_p da1 * [1, x, y, z] of feature tile q over this wave's OWN 32 points (round 4; was part of the dW1 phase: a third of
      // its staging and 6 of its 34 MFMAs per sub-phase).  da1 tile q goes through a wave-private 4 KiB slot behind the (now
      // 32 KiB) dW1 window and comes back feature-per-lane; the aux operand is masked to columns 0..3 AND to lane group q.  The
      // column-sum tile aS has 32 columns of which the masks (functions of lane & 7) used only 8 — lane groups 1..3 were copies
      // of group 0 — so tile q's sums land in columns 8 q + {0..3} of the SAME accumulator: no new registers; the waves' partial
      // sums are added when the workgroup writes its partials.  Same-wave LDS traffic: the DS queue is in order, no barrier.
      const unsigned prv = opaque(sbase + O_STG + 32768 + wave * 4096);
      auto da1_put = [&](int q) __attribute__((always_inline)) {          // tile q -> the wave's private slot
        const unsigned rb = opaque(prv + l31 * 64);
        const int gsw = (l31 >> 1) & 7;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          const unsigned o = rb + (((2 * gg + hf) ^ gsw) << 3);
          lds_st64(o, da1p.hi[q][2 * gg], da1p.hi[q][2 * gg + 1]);
          lds_st64(o + 2048, da1p.lo[q][2 * gg], da1p.lo[q][2 * gg + 1]);
        }
      };
      auto da1_sum = [&](int q) __attribute__((always_inline)) {          // read it back feature-per-lane, contract with aux
        const unsigned mq = ((l31 >> 3) == q && c7 < 4) ? ~0u : 0u;
        const unsigned p0 = opaque(LA.sb[0] + 32768 + wave * 4096), p1 = opaque(LA.sb[1] + 32768 + wave * 4096);
        const unsigned axw = opaque(LA.ab + wave * 512);
        Frag fd0, fd1, fy0, fy1;
        stg_frag<32, 0, 2048>(p0, p1, 0, 0, fd0);
        stg_frag<32, 0, 2048>(p0, p1, 0, 1, fd1);
        aux_frag(axw, 0, mq, fy0);
        aux_frag(axw, 1, mq, fy1);
        __builtin_amdgcn_sched_barrier(0);
        aS[0] = x3f(aS[0], fd0, fy0);
        aS[0] = x3f(aS[0], fd1, fy1);
        __builtin_amdgcn_sched_barrier(0);
      };
      // tile q's epilogue runs under tile q + 1's MFMAs; its slot is written at the first slot of tile q + 2 and read back eight
      // slots later (the LDS round trip has long completed: the read costs its own latency only)
      layer_tr_mm<4, 8, H, O_W1H, O_W1L - O_W1H>(LA, dp2p, acc1, [&](int slot) __attribute__((always_inline)) {
        const int m = slot / 24, j = slot % 24;
        if (m >= 2 && j == 0) da1_put(m - 2);
        if (m >= 2 && j == 8) da1_sum(m - 2);
        if (m >= 1) dh1_slot(m - 1, j / 6, j % 6);
      });
      X3_TS(7)
      da1_put(2);
#pragma unroll
      for (int j = 0; j < 12; ++j) { dh1_slot(3, j / 6, j % 6); __builtin_amdgcn_sched_barrier(0); }
      da1_sum(2);
#pragma unroll
      for (int j = 12; j < 24; ++j) { dh1_slot(3, j / 6, j % 6); __builtin_amdgcn_sched_barrier(0); }
      da1_put(3);
      da1_sum(3);
    }

    pin(da2p); pin(h1p);
    X3_TS(8)
    // ---- dW1 += da2^T h1: four sub-phases of 32 points; wave -> da2 row tile w, all four h1 column tiles;
    //      plus sum_p da2 (aux column 4) and sum_p da1 * [1, x, y, z] (aux columns 0..3) for row tile w ----
    if (!CIPS_TUNE(a.dbg & 4)) {
      constexpr int DAH = 0, DAL = 8192, H1H = 16384, H1L = 24576;      // 32 KiB; the last 16 KiB hold the waves' private slots
      const unsigned w0 = opaque(LA.sb[0] + wave * 2048), w1 = opaque(LA.sb[1] + wave * 2048);   // row tile w
#pragma unroll
      for (int sp = 0; sp < 4; ++sp) {
        if (sp == 1) { X3_TS(10) }
        if (wave == sp) {
          stage<4, 32, DAH, DAL>(sbase, l31, hf, da2p);
          stage<4, 32, H1H, H1L>(sbase, l31, hf, h1p);
        } else if (NPRE > 0) {
          // this wave's k-th idle sub-phase (k = sp for sp < wave, sp - 1 after its own turn): a third of the NPRE groups
          const int k = sp - (sp > wave ? 1 : 0);
          if (k == 0) l0_groups(IC0{}, ICA{}, npx, npy, npz);
          else if (k == 1) l0_groups(ICA{}, ICB{}, npx, npy, npz);
          else l0_groups(ICB{}, ICN{}, npx, npy, npz);
        }
        if (sp == 1) { X3_TS(11) }
        __syncthreads();
        if (sp == 1) { X3_TS(12) }
        const unsigned ax = opaque(LA.ab + sp * 512);      // aux k-steps 2sp + k
        Frag fa, fb0, fb1, fb2, fb3, fx;
        stg_frag<32, DAH, DAL>(w0, w1, 0, 0, fa);
        stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 0, 0, fb0);
        stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 32, 0, fb1);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 64, k, fb2);
          stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 96, k, fb3);
          aux_frag(ax, k, m_d2, fx);
          __builtin_amdgcn_sched_barrier(0);
          aG1[0] = x3f(aG1[0], fa, fb0);
          aG1[1] = x3f(aG1[1], fa, fb1);
          __builtin_amdgcn_sched_barrier(0);
          aG1[2] = x3f(aG1[2], fa, fb2);
          aG1[3] = x3f(aG1[3], fa, fb3);
          aS[0] = x2f(aS[0], fa, fx);
          __builtin_amdgcn_sched_barrier(0);
          if (k + 1 < 2) {
            stg_frag<32, DAH, DAL>(w0, w1, 0, k + 1, fa);
            stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 0, k + 1, fb0);
            stg_frag<32, H1H, H1L>(LA.sb[0], LA.sb[1], 32, k + 1, fb1);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (sp == 1) { X3_TS(13) }
        __syncthreads();
        if (sp == 1) { X3_TS(14) }
      }
    }
    px = npx; py = npy; pz = npz; dsg = ndsg;
    X3_TS(9)
  }

  const int lane = lane0, l31 = lane & 31, hf = lane >> 5;
  // ---- per-wave column sums and sum of dsigma.  Columns 4..7 of lane group 0 are this wave's row-tile sums as before; columns
  //      8 q + {0..3} hold sum_p da1 * [1, x, y, z] of feature tile q over this wave's own points: the four waves' tiles meet in
  //      the idle staging window and wave t adds tile t's four partials in wave order ----
  {
    float* part = reinterpret_cast<float*>(smem + O_STG);      // [wave][32 rows][32 columns] floats = 16 KiB
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(wave * 32 + mfma_row(r, hf)) * 32 + l31] = aS[0][r];
    __syncthreads();
    float* sr = a.sred + (long long)(MODE == X3_EVEN ? prow_ : b * a.chunks + blockIdx.x) * SRED;
    if (l31 < 8) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mfma_row(r, hf);
        // columns 0..3 are carried as 1/(2 pi)^2, column 4 (sum_p da2) as 1/(2 pi); 5..7 unscaled
        float v = aS[0][r] * ((HW && l31 == 4) ? TWO_PI : 1.f);
        if (l31 < 4) {
          v = part[(0 * 32 + row) * 32 + 8 * wave + l31];
          v += part[(1 * 32 + row) * 32 + 8 * wave + l31];
          v += part[(2 * 32 + row) * 32 + 8 * wave + l31];
          v += part[(3 * 32 + row) * 32 + 8 * wave + l31];
          if (HW) v *= TWO_PI * TWO_PI;
        }
        sr[wave * 256 + row * 8 + l31] = v;
      }
    }
    float t = r_dsg;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
    if (lane == 0) sr[1024 + wave] = t;
    if (lane == 1) sr[1028 + wave] = 0.f;
  }
  // ---- write the workgroup's partial weight gradients ----
  {
    float* gp_ = a.gpart + (long long)(MODE == X3_EVEN ? prow_ : b * a.chunks + blockIdx.x) * GPART;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) gp_[GP_G1 + (32 * wave + mfma_row(r, hf)) * H + 32 * j + l31] = aG1[j][r] * (HW ? TWO_PI : 1.f);
    const int it = wave & 1, jt0 = 2 * (wave >> 1);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) gp_[GP_GC + (32 * it + mfma_row(r, hf)) * H + 32 * (jt0 + j) + l31] = aGc[j][r];
    float* gf = gp_ + ((wave >> 1) ? GP_GF1 : GP_GF0);
#pragma unroll
    for (int r = 0; r < 16; ++r) gf[mfma_row(r, hf) * HC + 32 * (wave & 1) + l31] = aGf[0][r];
  }
}

