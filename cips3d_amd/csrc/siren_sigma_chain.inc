// siren_sigma_chain.inc — textually included by siren_sigma_x3_kernel of siren_bwd_x3.hip: one wave-step of the forward chain
// of siren_fwd_chain.inc UP TO sigma and nothing after it (that file is left alone and not shared with this one: its header
// says what moving its code does to hipcc's schedule).  Same expectations: in scope LaneAddr LA (v16 / v64 pointing at THIS
// kernel's layer-0 packs: the FiLM vectors are addressed relative to O_L0, so a carve that keeps their spacing only moves the
// base), float px, py, pz, bs and the template flags HW and F16; defines `float sig` (sigma of the lane's point, both lane
// halves).  Every value is the forward chain's bit for bit: the same fmaf chains for layer 0 and the sigma dot (grp, e order),
// and every W1 accumulator takes the same MFMAs in the same order.  What differs is what is kept: the layer-1 sines are
// consumed by the dot as they are made (no hi / lo split of h2, no colour layers, no feature accumulators), and h1 is made one
// 32-feature tile at a time (below), which is what brings the kernel from the forward's 166 VGPRs to at most 128.
    f32x16 acc[4];
    zero_acc(acc);
    {
      // layer 0 and the W1 product, 32 layer-0 features (one tile q = k-steps 2q, 2q + 1 of all four output tiles) at a time:
      // only 16 registers of packed h1 are live next to the 64 accumulators instead of 64.  Every accumulator still takes its
      // k-steps in ascending order with the three passes of x3h / x3 — layer_fwd<4, 4, H, O_W1H, ...>'s sequence per tile.
      const unsigned wb[2][2] = {{opaque(LA.fb[0][0] + O_W1H), opaque(LA.fb[0][1] + O_W1H)},
                                 {opaque(LA.fb[1][0] + O_W1H), opaque(LA.fb[1][1] + O_W1H)}};
  #pragma unroll
      for (int q = 0; q < 4; ++q) {
        Act<1> h1q;
  #pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 pk[4];
  #pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = lds_ld4(LA.v64 + 128 * (4 * q + g) + 16 * e);
          __builtin_amdgcn_sched_barrier(0);
          float sn[4];
  #pragma unroll
          for (int e = 0; e < 4; ++e) sn[e] = sin_rev<HW>(fmaf(pk[e].x, px, fmaf(pk[e].y, py, fmaf(pk[e].z, pz, pk[e].w))));
          split2t<F16>(sn[0], sn[1], h1q.hi[0][2 * g], h1q.lo[0][2 * g]);
          split2t<F16>(sn[2], sn[3], h1q.hi[0][2 * g + 1], h1q.lo[0][2 * g + 1]);
          __builtin_amdgcn_sched_barrier(0);
        }
        auto load = [&](int t, int m, Frag& f) {            // layer_fwd's fragment of k-step 2q + t, output tile m (a copy of
                                                            // its loader: the two change together)
          const int c = q * H * 64 + m * 2048;
          put(f.h, 0, lds_b64(wb[t][0] + c));
          put(f.h, 2, lds_b64(wb[t][1] + c));
          put(f.l, 0, lds_b64(wb[t][0] + c + (O_W1L - O_W1H)));
          put(f.l, 2, lds_b64(wb[t][1] + c + (O_W1L - O_W1H)));
        };
        X3_PRIO(1);
        run_layer<4, 2, F16>(load, h1q, acc);
        X3_PRIO(0);
      }
    }
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
