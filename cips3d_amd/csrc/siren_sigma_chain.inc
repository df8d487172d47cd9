// siren_sigma_chain.inc — textually included by siren_sigma_x3_kernel (siren_sigma_x3.inc): one wave-step of the forward chain
// of siren_fwd_chain.inc UP TO sigma and nothing after it (that file is left alone and not shared with this one: its header
// says what moving its code does to hipcc's schedule).  In scope: what siren_sigma_point.inc asks for (it opens the step and defines
// LA, hf, valid, gp and the point; LA.v16 / v64 point at THIS kernel's layer-0 packs: the FiLM vectors are addressed relative to
// O_L0, so a carve that keeps their spacing only moves the base) and float bs; defines `float sig` (sigma of the lane's point, both lane
// halves).  Every value is the forward chain's bit for bit: the same fmaf chains for layer 0 and the sigma dot (grp, e order),
// and every W1 accumulator takes the same MFMAs in the same order.  What differs is what is kept: the layer-1 sines are
// consumed by the dot as they are made (no hi / lo split of h2, no colour layers, no feature accumulators), and h1 is made one
// 32-feature tile at a time (siren_sigma_w1.inc, the block siren_sigma_grad_chain.inc shares), which is what brings the kernel from the forward's 166 VGPRs to at most 128.
#include "siren_sigma_point.inc"
#include "siren_sigma_w1.inc"
#include "siren_sigma_dot.inc"
