// siren_fwd_chain.inc — textually included by the forward kernels of siren_fwd_x3.hip (a shared __device__ function
// changes hipcc's scheduling of this hand-pinned stream: 166 -> 256 VGPRs).
// One wave-step of the forward chain.  Expects in scope: LaneAddr LA, int hf, float px, py, pz, bs and the template
// flags HW (with HW the LDS images are stage_weights_x3<true, .>'s: every sine argument comes out in revolutions, sin_rev is
// v_fract + v_sin) and F16 (operand planes of the three dense layers: fp16 with scaled weight images, stage_weights_x3<., true>,
// or bf16); defines `float sig` (sigma of the lane's point, both lane halves) and `f32x16 accf[1]` (the 16 colour-feature
// rows of this lane half WITHOUT the output bias and, with F16, still times the colour head's weight scale — the caller's
// output fma applies the 2^-k at O_AUX + 128: accf[0][r] <-> channel (r&3) + 8(r>>2) + 4hf).
    f32x16 acc[4];
    zero_acc(acc);
    X3F_TS(0)
    {
      Act<4> h1p;
      float4 pn[4];
  #pragma unroll
      for (int e = 0; e < 4; ++e) pn[e] = lds_ld4(LA.v64 + 16 * e);
  #pragma unroll
      for (int grp = 0; grp < 16; ++grp) {
        float4 pk[4];
  #pragma unroll
        for (int e = 0; e < 4; ++e) pk[e] = pn[e];
        if (grp + 1 < 16) {
  #pragma unroll
          for (int e = 0; e < 4; ++e) pn[e] = lds_ld4(LA.v64 + 128 * (grp + 1) + 16 * e);
        }
        __builtin_amdgcn_sched_barrier(0);
        float sn[4];
  #pragma unroll
        for (int e = 0; e < 4; ++e) sn[e] = sin_rev<HW>(fmaf(pk[e].x, px, fmaf(pk[e].y, py, fmaf(pk[e].z, pz, pk[e].w))));
        const int q = grp >> 2, g = grp & 3;
        split2t<F16>(sn[0], sn[1], h1p.hi[q][2 * g], h1p.lo[q][2 * g]);
        split2t<F16>(sn[2], sn[3], h1p.hi[q][2 * g + 1], h1p.lo[q][2 * g + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      X3F_TS(1)
      X3_PRIO(1);
      layer_fwd<4, 4, H, O_W1H, O_W1L - O_W1H, F16>(LA, h1p, acc);
      X3_PRIO(0);
      X3F_TS(2)
    }
    Act<4> h2p;
    float sig = 0.f;
    {
      float4 gn = lds_ld4(LA.v16 + (O_G1 - O_L0)), cn = lds_ld4(LA.v16 + (O_C1 - O_L0)), wn = lds_ld4(LA.v16 + (O_WS - O_L0));
  #pragma unroll
      for (int grp = 0; grp < 16; ++grp) {
        const float4 g4 = gn, c4 = cn, w4 = wn;
        if (grp + 1 < 16) {
          gn = lds_ld4(LA.v16 + (O_G1 - O_L0) + 32 * (grp + 1)); cn = lds_ld4(LA.v16 + (O_C1 - O_L0) + 32 * (grp + 1));
          wn = lds_ld4(LA.v16 + (O_WS - O_L0) + 32 * (grp + 1));
        }
        __builtin_amdgcn_sched_barrier(0);
        const int q = grp >> 2, g = grp & 3;
        const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, cc[4] = {c4.x, c4.y, c4.z, c4.w}, ww[4] = {w4.x, w4.y, w4.z, w4.w};
        float sn[4];
  #pragma unroll
        for (int e = 0; e < 4; ++e) {
          sn[e] = sin_rev<HW>(fmaf(gg[e], acc[q][4 * g + e], cc[e]));
          sig = fmaf(ww[e], sn[e], sig);
        }
        split2t<F16>(sn[0], sn[1], h2p.hi[q][2 * g], h2p.lo[q][2 * g]);
        split2t<F16>(sn[2], sn[3], h2p.hi[q][2 * g + 1], h2p.lo[q][2 * g + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    sig += __shfl_xor(sig, 32);
    sig += bs;

    f32x16 accc[2];
    zero_acc(accc);
    X3F_TS(3)
    X3_PRIO(1);
    layer_fwd<2, 4, HC, O_WCH, O_WCL - O_WCH, F16>(LA, h2p, accc);
    X3_PRIO(0);
    X3F_TS(4)
    Act<2> hcp;
    {
      float4 gn = lds_ld4(LA.v16 + (O_GC - O_L0)), cn = lds_ld4(LA.v16 + (O_CC - O_L0));
  #pragma unroll
      for (int grp = 0; grp < 8; ++grp) {
        const float4 g4 = gn, c4 = cn;
        if (grp + 1 < 8) { gn = lds_ld4(LA.v16 + (O_GC - O_L0) + 32 * (grp + 1)); cn = lds_ld4(LA.v16 + (O_CC - O_L0) + 32 * (grp + 1)); }
        __builtin_amdgcn_sched_barrier(0);
        const int q = grp >> 2, g = grp & 3;
        const float gg[4] = {g4.x, g4.y, g4.z, g4.w}, cc[4] = {c4.x, c4.y, c4.z, c4.w};
        float sn[4];
  #pragma unroll
        for (int e = 0; e < 4; ++e) sn[e] = sin_rev<HW>(fmaf(gg[e], accc[q][4 * g + e], cc[e]));
        split2t<F16>(sn[0], sn[1], hcp.hi[q][2 * g], hcp.lo[q][2 * g]);
        split2t<F16>(sn[2], sn[3], hcp.hi[q][2 * g + 1], hcp.lo[q][2 * g + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    f32x16 accf[1];
    zero_acc(accf);
    X3F_TS(5)
    X3_PRIO(1);
    layer_fwd<1, 2, CF, O_WFH, O_WFL - O_WFH, F16>(LA, hcp, accf);
    X3_PRIO(0);
    X3F_TS(6)
