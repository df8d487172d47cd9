// siren_sigma_dot.inc — textually included by siren_sigma_chain.inc and by siren_surface_x3.hip behind siren_sigma_w1.inc: the end of
// the forward chain up to sigma, as one text — the layer-1 sines consumed by the sigma dot as they are made, the cross-half add and
// the bias.  In scope: LaneAddr LA, `f32x16 acc[4]` (siren_sigma_w1.inc), float bs and the template flag HW; defines `float sig`
// (sigma of the lane's point, both lane halves).
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
  #pragma unroll
        for (int e = 0; e < 4; ++e) sig = fmaf(ww[e], sin_rev<HW>(fmaf(gg[e], acc[q][4 * g + e], cc[e])), sig);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    sig += __shfl_xor(sig, 32);
    sig += bs;
