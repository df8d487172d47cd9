// siren_sigma_w1.inc — textually included by siren_sigma_chain.inc and siren_sigma_grad_chain.inc: what the wave-steps of the sigma
// and the sigma-gradient kernel have in common, as one text — the step's prologue (the laundered lane id, the LDS address bases
// on the sigma carve, the ragged-tail clamp, the point from the points array or the GRID lattice), then layer 0 and the W1
// product.  The sigma of the gradient kernel is the sigma kernel's bit for bit by construction up to here.  (Text and no
// function: as a __device__ function the prologue alone changes the kernels' listings.)
// In scope: the kernel's arguments a (points or gx / gy / gz, ny, nz, P), int b, lane0, pbase, cend, unsigned sbase and the template
// flags HW, F16, GRID.  Defines LaneAddr LA (v16 / v64 pointing at the sigma carve's layer-0 packs), int hf, bool valid (false:
// a lane past the chunk's end, working on the last valid point again; nothing is stored for it), long long gp (index of the point
// in the (B, P) outputs), float px, py, pz and `f32x16 acc[4]`, the layer-1 pre-activations W1 h1 (before gain and offset) in
// register-chain layout.
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int l31 = lane & 31, hf = lane >> 5;
    LaneAddr LA = lane_addr(lane, sbase);
    LA.v16 = opaque(sbase + SG_L0 + 16 * hf);
    LA.v64 = opaque(sbase + SG_L0 + 64 * hf);
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
