// mesh.hip — indexed triangle meshes from a density volume: marching tetrahedra on the Kuhn decomposition of the lattice of
// cips_grid_params (DESIGN.md section 3 "Meshes"; case logic: mesh_cases.h).  Streaming and compaction work:
//
//   count   a workgroup per run of MESH_RUN consecutive lattice points (k fastest), a wave per 256 of them, in four groups of one
//           point per lane whose loads are all issued before the first is used.  A lane reads the four corners of its cell
//           with dz = 0 — four coalesced rows — and takes the dz = 1 flags from the next lane (the last lane's come from four
//           extra loads per group).  Per point the 7-bit crossing mask of its owned edges and the triangle count of its cell;
//           both summed over the wave with ballots + popcounts, over the workgroup through LDS: one pair of totals per workgroup.
//   scan    two levels.  One workgroup per SCAN_THREADS pairs scans them in place and leaves the chunk's total; one workgroup per
//           image scans the chunk totals (walking them with a carry if there are more than it has threads) and writes the
//           image's totals (vertices, triangles) as int64.
//   verts   recomputes the masks; a point's first vertex id = chunk offset + workgroup offset + the waves in front (LDS) + a
//           running exclusive prefix over the wave's groups (ballot + mbcnt); writes the per-point id and mask to scratch and
//           the vertices at their final positions.
//   faces   recomputes the triangle counts, same offsets; a triangle's vertex on edge class c of point o has the id
//           base[o] + popcount(mask[o] & ((1 << c) - 1)).
//
// No atomics, no workgroup waits for another (the phases are separate launches on the caller's stream), every output element has
// one writer at a position that depends on the input alone: two calls give the same bits.  All phases classify with the same
// predicate (sigma > level) on the same data, and every store is guarded by the image's totals, so a volume that changed between
// the calls or holds non-finite values can make positions meaningless but never a write out of range.
#include <limits.h>

#include "../../include/cips3d_hip.h"
#include "common.h"
#include "mesh_cases.h"

namespace {

constexpr int MESH_THREADS = 256;    // 4 waves
constexpr int MESH_ITEMS = 4;        // 64-point groups per wave, consecutive: a wave covers 256 consecutive lattice points
constexpr int MESH_WAVES = MESH_THREADS / 64;
constexpr int MESH_RUN = MESH_THREADS * MESH_ITEMS;        // lattice points per workgroup
constexpr int SCAN_THREADS = 512;    // pairs per chunk of the scan's first level

__constant__ mesh::Table mesh_table = mesh::make_table();

struct MeshArgs {
  const float *gx, *gy, *gz, *sigma;
  float level;
  int nx, ny, nz, P, nblk, nchunk;
  int* base;                 // (B, P)         first vertex id of each point, local to its image
  int* blk;                  // (B, nblk, 2)   per-workgroup (vertices, triangles): totals after count, offsets in the chunk after scan
  int* chunk;                // (B, nchunk, 2) per-chunk totals, then offsets in the image
  unsigned char* mask;       // (B, P)         crossing masks
  const long long* totals;   // (B, 2)
  float* verts;
  int* faces;
};

// a lattice point and its cell: indices, which of the cell's eight corners are on the lattice and which are inside (bit = corner
// 4 dx + 2 dy + dz), sigma at the point itself
struct Cell {
  int i, j, k;
  unsigned have, inside;
  float s0;
};

__device__ __forceinline__ int corner_offset(unsigned corner, int sx, int sy) {
  return (int)((corner >> 2) & 1u) * sx + (int)((corner >> 1) & 1u) * sy + (int)(corner & 1u);
}

// What a lane reads for its point p: the inside flags of the four corners of its cell with dz = 0 (row r = 2 dx + dy; strictly
// above the level is inside, so NaN is outside) and, in lanes 0..3, of row `lane` of the point behind the wave's 64 (p + 1 of lane
// 63).  No branches: a load that is not wanted reads the point itself and its flag is dropped, so that a kernel can issue the loads
// of all its groups before it uses the first.  Points behind the lattice (p >= P) get no corner but their own and nothing inside.
struct Rows {
  int i, j, k;
  unsigned have, rows;
  bool ext;
  float s0;
};

__device__ __forceinline__ Rows load_rows(const MeshArgs& a, const float* sig, int p) {
  const int lane = threadIdx.x & 63;
  const bool valid = p < a.P;
  const int pc = valid ? p : a.P - 1;
  Rows r;
  const int row = pc / a.nz;
  r.k = pc - row * a.nz; r.i = row / a.ny; r.j = row - r.i * a.ny;
  const bool hx = valid && r.i + 1 < a.nx, hy = valid && r.j + 1 < a.ny, hz = valid && r.k + 1 < a.nz;
  const int sx = a.ny * a.nz, sy = a.nz;
  const int q = p - lane + 64 + ((lane >> 1) & 1) * sx + (lane & 1) * sy;
  const bool eok = lane < 4 && q < a.P;
  r.s0 = sig[pc];
  const float v1 = sig[hy ? pc + sy : pc], v2 = sig[hx ? pc + sx : pc], v3 = sig[hx && hy ? pc + sx + sy : pc];
  const float ve = sig[eok ? q : pc];
  r.rows = (valid && r.s0 > a.level ? 1u : 0u) | (hy && v1 > a.level ? 2u : 0u) | (hx && v2 > a.level ? 4u : 0u) |
           (hx && hy && v3 > a.level ? 8u : 0u);
  r.ext = eok && ve > a.level;
  r.have = 1u | (hz ? 2u : 0u) | (hy ? 4u : 0u) | (hy && hz ? 8u : 0u) | (hx ? 16u : 0u) | (hx && hz ? 32u : 0u) |
           (hx && hy ? 64u : 0u) | (hx && hy && hz ? 128u : 0u);
  return r;
}

// The cell of a lane's point.  The corners with dz = 1 are the next point's with dz = 0: the next lane has their flags, and the
// last lane takes the four that lanes 0..3 fetched.  Every lane of the wave calls this.
__device__ __forceinline__ Cell finish_cell(const Rows& r) {
  const unsigned last = (unsigned)__ballot(r.ext) & 15u;
  unsigned next = (unsigned)__shfl_down((int)r.rows, 1);
  if ((threadIdx.x & 63) == 63) next = last;
  Cell c;
  c.i = r.i; c.j = r.j; c.k = r.k; c.s0 = r.s0; c.have = r.have;
  unsigned in = 0;
#pragma unroll
  for (int n = 0; n < 4; ++n) in |= (((r.rows >> n) & 1u) << (2 * n)) | (((next >> n) & 1u) << (2 * n + 1));
  c.inside = in & c.have;
  return c;
}

// the lattice point of the calling lane in its wave's group `it`
__device__ __forceinline__ int item_point(int it) {
  return blockIdx.x * MESH_RUN + (threadIdx.x >> 6) * (64 * MESH_ITEMS) + it * 64 + (threadIdx.x & 63);
}

// a cell whose on-lattice corners are all inside or all outside has neither a crossing nor a triangle: most cells, and whole waves
__device__ __forceinline__ bool mixed(const Cell& c) { return c.inside != 0u && c.inside != c.have; }

// sum over the wave of a small non-negative value (NBITS wide), bit plane by bit plane: ballot + popcount, and the exclusive
// prefix of the calling lane: ballot + mbcnt
template <int NBITS>
__device__ __forceinline__ int wave_prefix(int v, int* total) {
  int pre = 0, tot = 0;
#pragma unroll
  for (int b = 0; b < NBITS; ++b) {
    const unsigned long long m = __ballot((v >> b) & 1);
    pre += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)) << b;
    tot += __popcll(m) << b;
  }
  *total = tot;
  return pre;
}

// what the waves in front of the calling one counted, from every wave's own total (every thread calls it, once per kernel)
__device__ __forceinline__ int waves_before(int wave_total, int* lds) {
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = wave_total;
  __syncthreads();
  int pre = 0;
#pragma unroll
  for (int w = 0; w < MESH_WAVES - 1; ++w)
    if (w < wave) pre += lds[w];
  return pre;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_count_kernel(MeshArgs a) {
  __shared__ int lv[MESH_WAVES], lt[MESH_WAVES];
  const int b = blockIdx.y;
  const float* sig = a.sigma + (size_t)b * a.P;
  Rows r[MESH_ITEMS];
#pragma unroll
  for (int it = 0; it < MESH_ITEMS; ++it) r[it] = load_rows(a, sig, item_point(it));
  int tv = 0, tt = 0;                                   // the wave's totals: the same in every lane
#pragma unroll
  for (int it = 0; it < MESH_ITEMS; ++it) {
    const Cell c = finish_cell(r[it]);
    int nv = 0, nt = 0, wv, wt;
    if (mixed(c)) { nv = __popc(mesh::crossing_mask(c.inside, c.have)); nt = mesh::cell_triangles(c.inside, c.have); }
    wave_prefix<3>(nv, &wv);
    wave_prefix<4>(nt, &wt);
    tv += wv; tt += wt;
  }
  if ((threadIdx.x & 63) == 0) { lv[threadIdx.x >> 6] = tv; lt[threadIdx.x >> 6] = tt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    tv = tt = 0;
#pragma unroll
    for (int w = 0; w < MESH_WAVES; ++w) { tv += lv[w]; tt += lt[w]; }
    int* e = a.blk + ((size_t)b * a.nblk + blockIdx.x) * 2;
    e[0] = tv; e[1] = tt;
  }
}

// exclusive scan of one pair per thread over a workgroup of SCAN_THREADS: (*ev, *et) = the sums in front of the calling thread,
// (*tv, *tt) = the workgroup's sums.  Ends with a barrier, so it can be called again.
__device__ __forceinline__ void scan_pairs(int v, int t, int* lv, int* lt, int* ev, int* et, int* tv, int* tt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int iv = v, it = t;                                   // inclusive over the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int nv = __shfl_up(iv, off), nt = __shfl_up(it, off);
    if (lane >= off) { iv += nv; it += nt; }
  }
  if (lane == 63) { lv[wave] = iv; lt[wave] = it; }
  __syncthreads();
  int pv = 0, pt = 0, sv = 0, st = 0;
#pragma unroll
  for (int w = 0; w < SCAN_THREADS / 64; ++w) {
    const int xv = lv[w], xt = lt[w];
    if (w < wave) { pv += xv; pt += xt; }
    sv += xv; st += xt;
  }
  *ev = pv + iv - v; *et = pt + it - t; *tv = sv; *tt = st;
  __syncthreads();
}

// level 1: chunk blockIdx.x of image blockIdx.y, SCAN_THREADS pairs, scanned in place; its totals to `chunk`
__global__ __launch_bounds__(SCAN_THREADS) void mesh_scan_chunks_kernel(int* blk, int nblk, int* chunk, int nchunk) {
  __shared__ int lv[SCAN_THREADS / 64], lt[SCAN_THREADS / 64];
  int* e = blk + (size_t)blockIdx.y * nblk * 2;
  const int idx = blockIdx.x * SCAN_THREADS + threadIdx.x;
  const int v = idx < nblk ? e[2 * idx] : 0, t = idx < nblk ? e[2 * idx + 1] : 0;
  int ev, et, tv, tt;
  scan_pairs(v, t, lv, lt, &ev, &et, &tv, &tt);
  if (idx < nblk) { e[2 * idx] = ev; e[2 * idx + 1] = et; }
  if (threadIdx.x == 0) {
    int* c = chunk + ((size_t)blockIdx.y * nchunk + blockIdx.x) * 2;
    c[0] = tv; c[1] = tt;
  }
}

// level 2: image blockIdx.x's chunk totals, scanned in place SCAN_THREADS at a time with a carry; the image's totals
__global__ __launch_bounds__(SCAN_THREADS) void mesh_scan_image_kernel(int* chunk, int nchunk, long long* totals) {
  __shared__ int lv[SCAN_THREADS / 64], lt[SCAN_THREADS / 64];
  int* e = chunk + (size_t)blockIdx.x * nchunk * 2;
  int cv = 0, ct = 0;                                   // carry: the same in every thread
  for (int first = 0; first < nchunk; first += SCAN_THREADS) {
    const int idx = first + threadIdx.x;
    const int v = idx < nchunk ? e[2 * idx] : 0, t = idx < nchunk ? e[2 * idx + 1] : 0;
    int ev, et, tv, tt;
    scan_pairs(v, t, lv, lt, &ev, &et, &tv, &tt);
    if (idx < nchunk) { e[2 * idx] = cv + ev; e[2 * idx + 1] = ct + et; }
    cv += tv; ct += tt;
  }
  if (threadIdx.x == 0) { totals[2 * blockIdx.x] = cv; totals[2 * blockIdx.x + 1] = ct; }
}

// the first id (which = 0: vertex, 1: triangle) of the calling workgroup's run within its image
__device__ __forceinline__ int run_start(const MeshArgs& a, int b, int which) {
  return a.blk[((size_t)b * a.nblk + blockIdx.x) * 2 + which] +
         a.chunk[((size_t)b * a.nchunk + blockIdx.x / SCAN_THREADS) * 2 + which];
}

// where image b's vertices (which = 0) or triangles (1) start in the packed output, and how many it has
__device__ __forceinline__ long long image_start(const long long* totals, int b, int which, long long* count) {
  long long s = 0;
  for (int i = 0; i < b; ++i) s += totals[2 * i + which];
  *count = totals[2 * b + which];
  return s;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_verts_kernel(MeshArgs a) {
  __shared__ int lv[MESH_WAVES];
  const int b = blockIdx.y;
  const float* sig = a.sigma + (size_t)b * a.P;
  Cell c[MESH_ITEMS];
  unsigned m[MESH_ITEMS];
  int pre[MESH_ITEMS], run = 0;                         // ids in front of the lane's point within the wave; the wave's total
  Rows r[MESH_ITEMS];
#pragma unroll
  for (int it = 0; it < MESH_ITEMS; ++it) r[it] = load_rows(a, sig, item_point(it));
#pragma unroll
  for (int it = 0; it < MESH_ITEMS; ++it) {
    c[it] = finish_cell(r[it]);
    m[it] = mixed(c[it]) ? mesh::crossing_mask(c[it].inside, c[it].have) : 0u;
    int wv;
    pre[it] = run + wave_prefix<3>(__popc(m[it]), &wv);
    run += wv;
  }
  const int wave_first = run_start(a, b, 0) + waves_before(run, lv);
  long long count;
  const long long start = image_start(a.totals, b, 0, &count);
  const int sx = a.ny * a.nz, sy = a.nz;
#pragma unroll
  for (int it = 0; it < MESH_ITEMS; ++it) {
    const int p = item_point(it);
    if (p >= a.P) continue;
    a.base[(size_t)b * a.P + p] = wave_first + pre[it];
    a.mask[(size_t)b * a.P + p] = (unsigned char)m[it];
    if (!m[it]) continue;
    const float x0 = a.gx[c[it].i], y0 = a.gy[c[it].j], z0 = a.gz[c[it].k];
    const float ex = (c[it].have & 16u) ? a.gx[c[it].i + 1] - x0 : 0.f;        // corner 4 = (1, 0, 0) is on the lattice
    const float ey = (c[it].have & 4u) ? a.gy[c[it].j + 1] - y0 : 0.f;
    const float ez = (c[it].have & 2u) ? a.gz[c[it].k + 1] - z0 : 0.f;
    int id = wave_first + pre[it];
#pragma unroll
    for (int cl = 0; cl < 7; ++cl) {
      if (!((m[it] >> cl) & 1u)) continue;                             // a set bit: corner d is on the lattice
      const int d = cl + 1;
      const float t = (a.level - c[it].s0) / (sig[p + corner_offset(d, sx, sy)] - c[it].s0);
      if (id >= 0 && (long long)id < count) {                          // never beyond what the count call reported
        float* o = a.verts + (start + id) * 3;
        o[0] = (d & 4) ? fmaf(t, ex, x0) : x0;                         // an axis the edge does not move along: g[a] bit for bit
        o[1] = (d & 2) ? fmaf(t, ey, y0) : y0;
        o[2] = (d & 1) ? fmaf(t, ez, z0) : z0;
      }
      ++id;
    }
  }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_faces_kernel(MeshArgs a) {
  __shared__ int lt[MESH_WAVES];
  __shared__ unsigned long long tbl[96];
  if (threadIdx.x < 96) tbl[threadIdx.x] = mesh_table.e[threadIdx.x >> 4][threadIdx.x & 15];
  const int b = blockIdx.y;
  const float* sig = a.sigma + (size_t)b * a.P;
  unsigned inside[MESH_ITEMS];
  int nt[MESH_ITEMS], pre[MESH_ITEMS], run = 0;
  Rows r[MESH_ITEMS];
#pragma unroll
  for (int it = 0; it < MESH_ITEMS; ++it) r[it] = load_rows(a, sig, item_point(it));
#pragma unroll
  for (int it = 0; it < MESH_ITEMS; ++it) {
    const Cell c = finish_cell(r[it]);
    inside[it] = c.inside;
    nt[it] = mixed(c) ? mesh::cell_triangles(c.inside, c.have) : 0;
    int wt;
    pre[it] = run + wave_prefix<4>(nt[it], &wt);
    run += wt;
  }
  const int wave_first = run_start(a, b, 1) + waves_before(run, lt);   // its barrier covers tbl too
  long long count;
  const long long start = image_start(a.totals, b, 1, &count);
  const int sx = a.ny * a.nz, sy = a.nz;
#pragma unroll
  for (int it = 0; it < MESH_ITEMS; ++it) {
    if (!nt[it]) continue;                                             // a cell with triangles has all eight corners
    const int p = item_point(it);
    const int* base = a.base + (size_t)b * a.P + p;
    const unsigned char* mask = a.mask + (size_t)b * a.P + p;
    int id = wave_first + pre[it];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const int kase = mesh::tet_case(inside[it], t);
      const int n = mesh::case_triangles(kase);
      unsigned long long e = tbl[t * 16 + kase];
      for (int piece = 0; piece < n; ++piece) {
        int v[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const unsigned code = (unsigned)e & 63u;
          e >>= 6;
          const unsigned cl = code & 7u;                               // edge class; code >> 3: owner corner (never corner 7)
          const int off = corner_offset(code >> 3, sx, sy);
          v[s] = base[off] + __popc((unsigned)mask[off] & ((1u << cl) - 1u));
        }
        if (id >= 0 && (long long)id < count) {
          int* f = a.faces + (start + id) * 3;
          f[0] = v[0]; f[1] = v[1]; f[2] = v[2];
        }
        ++id;
      }
    }
  }
}

struct MeshLayout { int P, nblk, nchunk; size_t off_blk, off_chunk, off_mask, bytes; };

// sizes of the lattice and of the scratch of B images, or an error for a lattice the kernels' 32-bit indices cannot hold
int mesh_layout(const cips_grid_params* g, int B, MeshLayout* L) {
  if (!g || B <= 0 || B > 65535 || g->nx < 2 || g->ny < 2 || g->nz < 2) return (int)hipErrorInvalidValue;
  const long long nxy = (long long)g->nx * g->ny, cxy = (long long)(g->nx - 1) * (g->ny - 1);
  if (nxy > INT_MAX / 7 || nxy * g->nz > INT_MAX / 7) return (int)hipErrorInvalidValue;             // 7 vertices per point
  if (cxy * (g->nz - 1) > INT_MAX / 12) return (int)hipErrorInvalidValue;                           // 12 triangles per cell
  L->P = (int)(nxy * g->nz);
  L->nblk = (L->P + MESH_RUN - 1) / MESH_RUN;
  L->nchunk = (L->nblk + SCAN_THREADS - 1) / SCAN_THREADS;
  L->off_blk = (size_t)B * L->P * sizeof(int);
  L->off_chunk = L->off_blk + (size_t)B * L->nblk * 2 * sizeof(int);
  L->off_mask = L->off_chunk + (size_t)B * L->nchunk * 2 * sizeof(int);
  L->bytes = L->off_mask + (size_t)B * L->P;
  return 0;
}

int mesh_args(const cips_grid_params* g, const float* sigma, float level, int B, void* scratch, long long scratch_bytes,
              const long long* totals, MeshArgs* a) {
  MeshLayout L;
  if (const int rc = mesh_layout(g, B, &L)) return rc;
  if (!g->gx || !g->gy || !g->gz || !sigma || !scratch || !totals) return (int)hipErrorInvalidValue;
  if (scratch_bytes < 0 || (unsigned long long)scratch_bytes < L.bytes || ((uintptr_t)scratch & 3u)) return (int)hipErrorInvalidValue;
  a->gx = g->gx; a->gy = g->gy; a->gz = g->gz; a->sigma = sigma; a->level = level;
  a->nx = g->nx; a->ny = g->ny; a->nz = g->nz; a->P = L.P; a->nblk = L.nblk; a->nchunk = L.nchunk;
  a->base = (int*)scratch;
  a->blk = (int*)((char*)scratch + L.off_blk);
  a->chunk = (int*)((char*)scratch + L.off_chunk);
  a->mask = (unsigned char*)scratch + L.off_mask;
  a->totals = totals; a->verts = nullptr; a->faces = nullptr;
  return 0;
}

}  // namespace

extern "C" long long cips_mesh_scratch_bytes(const cips_grid_params* grid, int B) {
  MeshLayout L;
  return mesh_layout(grid, B, &L) ? -1 : (long long)L.bytes;
}

extern "C" int cips_mesh_count(const cips_grid_params* grid, const float* sigma, float level, int B, void* scratch,
                               long long scratch_bytes, long long* totals, cips_stream_t stream) {
  MeshArgs a;
  if (const int rc = mesh_args(grid, sigma, level, B, scratch, scratch_bytes, totals, &a)) return rc;
  hipLaunchKernelGGL(mesh_count_kernel, dim3(a.nblk, B), dim3(MESH_THREADS), 0, (hipStream_t)stream, a);
  if (const int rc = CIPS_CHECK_LAUNCH()) return rc;
  hipLaunchKernelGGL(mesh_scan_chunks_kernel, dim3(a.nchunk, B), dim3(SCAN_THREADS), 0, (hipStream_t)stream, a.blk, a.nblk, a.chunk,
                     a.nchunk);
  if (const int rc = CIPS_CHECK_LAUNCH()) return rc;
  hipLaunchKernelGGL(mesh_scan_image_kernel, dim3(B), dim3(SCAN_THREADS), 0, (hipStream_t)stream, a.chunk, a.nchunk, totals);
  return CIPS_CHECK_LAUNCH();
}

extern "C" int cips_mesh_emit(const cips_grid_params* grid, const float* sigma, float level, int B, void* scratch,
                              long long scratch_bytes, const long long* totals, float* vertices, int* faces, cips_stream_t stream) {
  MeshArgs a;
  if (!vertices || !faces) return (int)hipErrorInvalidValue;
  if (const int rc = mesh_args(grid, sigma, level, B, scratch, scratch_bytes, totals, &a)) return rc;
  a.verts = vertices; a.faces = faces;
  hipLaunchKernelGGL(mesh_verts_kernel, dim3(a.nblk, B), dim3(MESH_THREADS), 0, (hipStream_t)stream, a);
  if (const int rc = CIPS_CHECK_LAUNCH()) return rc;
  hipLaunchKernelGGL(mesh_faces_kernel, dim3(a.nblk, B), dim3(MESH_THREADS), 0, (hipStream_t)stream, a);
  return CIPS_CHECK_LAUNCH();
}
