// mesh_cases.h — the case logic of marching tetrahedra on the Kuhn decomposition (DESIGN.md section 3 "Meshes"), derived at
// compile time from the rules instead of typed in: plain C++17 constexpr, usable from host and device code alike.
//
// A cell's corner is named by its bits 4 dx + 2 dy + dz.  Tetrahedron t belongs to the t-th permutation pi of the axes in
// lexicographic order and has the path v0 = 0, v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = 7.  Its case is the four inside flags of
// v0..v3 (bit m: v_m).  Every edge runs from a corner o to o + d; it is owned by o, as edge class c = d - 1 (d as corner bits).
#pragma once
#include <stdint.h>

namespace mesh {

constexpr int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// corner bits of path vertex m of tetrahedron t (axis a carries the weight 4 >> a)
constexpr int path_corner(int t, int m) {
  int v = 0;
  for (int s = 0; s < m; ++s) v |= 4 >> kPerm[t][s];
  return v;
}

constexpr int corner_axis(int corner, int a) { return (corner >> (2 - a)) & 1; }

// det[r0, r1, r2] of three corner differences b_i - a_i
constexpr int det3(int a0, int b0, int a1, int b1, int a2, int b2) {
  int r[3][3] = {};
  const int a[3] = {a0, a1, a2}, b[3] = {b0, b1, b2};
  for (int i = 0; i < 3; ++i)
    for (int x = 0; x < 3; ++x) r[i][x] = corner_axis(b[i], x) - corner_axis(a[i], x);
  return r[0][0] * (r[1][1] * r[2][2] - r[1][2] * r[2][1]) - r[0][1] * (r[1][0] * r[2][2] - r[1][2] * r[2][0]) +
         r[0][2] * (r[1][0] * r[2][1] - r[1][1] * r[2][0]);
}

// a triangle vertex: the edge between path vertices a and b of tetrahedron t -> (owner corner << 3) | edge class, 6 bits
constexpr unsigned edge_code(int t, int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const int o = path_corner(t, lo), d = path_corner(t, hi) ^ o;        // the path is monotone: hi's corner contains lo's
  return (unsigned)((o << 3) | (d - 1));
}

// triangles of a tetrahedron case: min(n, 4 - n) for n inside vertices
constexpr int case_triangles(int kase) {
  const int n = (kase & 1) + ((kase >> 1) & 1) + ((kase >> 2) & 1) + ((kase >> 3) & 1);
  return n < 4 - n ? n : 4 - n;
}

struct Table { uint64_t e[6][16]; };     // six 6-bit edge codes per (tetrahedron, case): triangle n, vertex s at bits 6 (3 n + s)

constexpr uint64_t pack3(unsigned c0, unsigned c1, unsigned c2, int n) {
  return ((uint64_t)c0 | ((uint64_t)c1 << 6) | ((uint64_t)c2 << 12)) << (18 * n);
}

constexpr Table make_table() {
  Table tb = {};
  for (int t = 0; t < 6; ++t)
    for (int kase = 1; kase < 15; ++kase) {
      int in[4] = {}, out[4] = {}, ni = 0, no = 0;
      for (int m = 0; m < 4; ++m) { if ((kase >> m) & 1) in[ni++] = m; else out[no++] = m; }
      const int c[4] = {path_corner(t, 0), path_corner(t, 1), path_corner(t, 2), path_corner(t, 3)};
      if (ni == 1 || no == 1) {
        // one vertex A apart from the rest R0 R1 R2 (path order): (A R0, A R1, A R2) has its normal away from A iff
        // det[R0 - A, R1 - A, R2 - A] > 0; the normal must point away from an inside A and towards an outside one
        const int A = ni == 1 ? in[0] : out[0];
        int R[3] = {}, k = 0;
        for (int m = 0; m < 4; ++m) if (m != A) R[k++] = m;
        const int det = det3(c[A], c[R[0]], c[A], c[R[1]], c[A], c[R[2]]);
        const bool keep = (det > 0) == (ni == 1);
        tb.e[t][kase] = pack3(edge_code(t, A, R[0]), edge_code(t, A, R[keep ? 1 : 2]), edge_code(t, A, R[keep ? 2 : 1]), 0);
      } else {
        // inside A, B and outside C, D (path order): quad (AC, AD, BD, BC) as (AC, AD, BD) + (AC, BD, BC); at t = 1/2 the normal
        // is along (D - C) x (B - A), which points to the outside pair iff det[D - C, B - A, C - A] > 0
        const int A = in[0], B = in[1], C = out[0], D = out[1];
        const int det = det3(c[C], c[D], c[A], c[B], c[A], c[C]);
        const unsigned ac = edge_code(t, A, C), ad = edge_code(t, A, D), bd = edge_code(t, B, D), bc = edge_code(t, B, C);
        tb.e[t][kase] = det > 0 ? (pack3(ac, ad, bd, 0) | pack3(ac, bd, bc, 1)) : (pack3(ac, bd, ad, 0) | pack3(ac, bc, bd, 1));
      }
    }
  return tb;
}

// the 7-bit crossing mask of a point's owned edges and the triangle count of its cell, from the inside flags of the eight
// corners (bit = corner) and the corners that lie on the lattice (`have`, same bits; bit 0 is always set).  The one predicate
// every phase classifies with.
constexpr unsigned crossing_mask(unsigned inside, unsigned have) {
  const unsigned differ = (inside & 1u ? ~inside : inside) & have;     // bit d: corner d is on the lattice and differs from corner 0
  return (differ >> 1) & 0x7Fu;                                        // edge class c = d - 1
}

constexpr int tet_case(unsigned inside, int t) {
  return (int)((inside & 1u) | (((inside >> path_corner(t, 1)) & 1u) << 1) | (((inside >> path_corner(t, 2)) & 1u) << 2) |
               (((inside >> 7) & 1u) << 3));
}

constexpr int cell_triangles(unsigned inside, unsigned have) {
  if (have != 0xFFu) return 0;
  int n = 0;
  for (int t = 0; t < 6; ++t) n += case_triangles(tet_case(inside, t));
  return n;
}

}  // namespace mesh
