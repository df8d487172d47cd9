// siren_sigma_point.inc — textually included by siren_sigma_chain.inc and siren_sigma_grad_chain.inc in front of siren_sigma_w1.inc:
// the prologue of the sigma and the sigma-gradient kernel's wave-step — the laundered lane id, the LDS address bases on the sigma
// carve, the ragged-tail clamp, the point from the points array or the GRID lattice.  (Text and no function: as a __device__
// function the prologue alone changes the kernels' listings.)  A kernel whose point comes from somewhere else
// (siren_surface_x3.hip: from registers, many times per ray) writes its own prologue and includes siren_sigma_w1.inc alone.
// In scope: the kernel's arguments a (points or gx / gy / gz, ny, nz, P), int b, lane0, pbase, cend, unsigned sbase and the template
// flag GRID.  Defines LaneAddr LA (v16 / v64 pointing at the sigma carve's layer-0 packs), int hf, bool valid (false: a lane past
// the chunk's end, working on the last valid point again; nothing is stored for it), long long gp (index of the point in the
// (B, P) outputs) and float px, py, pz.
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

