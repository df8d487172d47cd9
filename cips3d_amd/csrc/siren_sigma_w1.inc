// siren_sigma_w1.inc — textually included by siren_sigma_chain.inc and siren_sigma_grad_chain.inc behind siren_sigma_point.inc, and by
// siren_surface_x3.hip behind a prologue of its own: what the wave-steps of the sigma, the sigma-gradient and the surface kernel have
// in common, as one text — layer 0 and the W1 product.  The sigma of the gradient and of the surface kernel is the sigma kernel's
// bit for bit by construction up to here.
// In scope: what the prologue defines — LaneAddr LA (v16 / v64 pointing at the sigma carve's layer-0 packs) and the point, float
// px, py, pz — and the template flags HW and F16.  Defines `f32x16 acc[4]`, the layer-1 pre-activations W1 h1 (before gain and
// offset) in register-chain layout.
    f32x16 acc[4];
    zero_acc(acc);
    {
      // layer 0 and the W1 product, 32 layer-0 features (one tile q = k-steps 2q, 2q + 1 of all four output tiles) at a time:
      // only 16 registers of packed h1 are live next to the 64 accumulators instead of 64.  Every accumulator still takes its
      // k-steps in ascending order with the three passes of x3h / x3 — layer_fwd<4, 4, H, O_W1H, ...>'s sequence per tile.
      const ImgBase wb(LA.fb, O_W1H);
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
        auto load = [&](int t, int m, Frag& f) {            // layer_fwd's fragment of k-step 2q + t, output tile m
          frag_fwd<O_W1L - O_W1H>(wb.b[t][0], wb.b[t][1], q * H * 64 + m * 2048, f);
        };
        X3_PRIO(1);
        run_layer<4, 2, F16>(load, h1q, acc);
        X3_PRIO(0);
      }
    }
