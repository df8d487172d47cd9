// siren_sigma_grad_chain.inc — textually included by siren_sigma_grad_x3_kernel (siren_sigma_x3.inc): siren_sigma_chain.inc's
// wave-step carried on to the gradient of sigma w.r.t. the point.
// In scope: what siren_sigma_point.inc asks for (it opens the step: LA, hf, valid, gp, the point), float bs, float dscale (the power of two
// the kernel puts on the layer-1 factor, 1 on bf16 planes) and the template flags HW and F16; defines `float sig` and
// `float gx, gy, gz` (both lane halves), the gradient still times  dscale  and, with HW, divided by (2 pi)^2.
//   sigma = ws . sin(a1) + bs,   dp1 = g1 * ws * cos(a1),   dh1 = W1^T dp1,   grad = sum_f pack[f].xyz cos(a0[f]) dh1[f]
// sigma is siren_sigma_chain.inc's bit for bit: the first block is the same text (siren_sigma_w1.inc).  The layer-1 epilogues stay
// separate — this one takes the cosine next to every sine and packs dp1, the sigma chain keeps nothing but the dot — and agree
// because both evaluate the same fmaf chain per feature in the same (grp, e) order; the sine of sincos_rev is sin_rev's expression.
#include "siren_sigma_point.inc"
#include "siren_sigma_w1.inc"
    // layer-1 epilogue: the accumulator of feature f is consumed as sine for the sigma dot and as cosine for dp1, which is
    // packed to split planes — the B operand of the transposed layer, k order of the register chain
    float sig = 0.f;
    Act<4> dp1;
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
        float d[4];
  #pragma unroll
        for (int e = 0; e < 4; ++e) {
          float sn, cs;
          sincos_rev<HW>(fmaf(gg[e], acc[q][4 * g + e], cc[e]), &sn, &cs);
          sig = fmaf(ww[e], sn, sig);
          d[e] = (gg[e] * ww[e]) * dscale * cs;
        }
        split2t<F16>(d[0], d[1], dp1.hi[q][2 * g], dp1.lo[q][2 * g]);
        split2t<F16>(d[2], d[3], dp1.hi[q][2 * g + 1], dp1.lo[q][2 * g + 1]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    sig += __shfl_xor(sig, 32);
    sig += bs;

    // dh1 = W1^T dp1 from the one W1 image, read transposed
    f32x16 dh1[4];
    zero_acc(dh1);
    X3_PRIO(1);
    layer_tr<4, 8, H, O_W1H, O_W1L - O_W1H, F16>(LA, dp1, dh1);
    X3_PRIO(0);

    // layer 0 again: cos(a0) from the packs, and the three components as fmaf chains over the lane half's 64 features
    float gx = 0.f, gy = 0.f, gz = 0.f;
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
      const int q = grp >> 2, g = grp & 3;
  #pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = cos_rev<HW>(fmaf(pk[e].x, px, fmaf(pk[e].y, py, fmaf(pk[e].z, pz, pk[e].w)))) * dh1[q][4 * g + e];
        gx = fmaf(pk[e].x, t, gx); gy = fmaf(pk[e].y, t, gy); gz = fmaf(pk[e].z, t, gz);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    gx += __shfl_xor(gx, 32); gy += __shfl_xor(gy, 32); gz += __shfl_xor(gz, 32);
