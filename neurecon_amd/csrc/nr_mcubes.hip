// neurecon_amd — marching cubes on the device: the step of `convert_sigma_samples_to_ply`
// (utils/mesh_util.py:13-79) that the reference hands to skimage.measure.marching_cubes (:33-35).
// Input: a device fp32 volume [n0, n1, n2] in C order (every dim >= 2) and a level.  Output: an
// indexed, welded triangle mesh as device arrays, verts fp32 [V, 3] and faces int32 [F, 3].
//
// Definitions
//   * A corner is INSIDE iff v < level.  NaN and v == level are outside.
//   * A grid edge is CROSSING iff exactly one of its ends is inside.  Every crossing edge carries
//     exactly one vertex, shared by every triangle that touches it.
//   * Each grid point owns the three edges that leave it along +axis 0, +axis 1, +axis 2.
//   * Vertex order: by the owning point's flat C index, then by axis 0, 1, 2.
//   * Face order: by the cell's flat index (the flat point index of its min corner), then by the
//     table's order within the cell.
//   * Both orders are fixed; no atomics anywhere: two runs are bit-identical.
//   * Vertex position.  Edge from the point with index i along axis a, end values v0, v1:
//     t = (level - v0) / (v1 - v0) in float64 from the fp32 inputs (never 0/0: the ends differ in
//     class); the index-space coordinate is i + t on axis a and the integer index on the other two;
//     pos = ((idx * spacing + origin) / scale) - offset per axis in float64, every operation rounded on
//     its own (dmul / dadd / ddiv / dsub of nr_common.h: the product and the sum are never contracted
//     into a fused multiply-add), rounded to fp32 once.
//   * Orientation.  With output axes 0, 1, 2 read as a right-handed x, y, z, triangle normals
//     (right-hand rule on the emitted vertex order) point toward larger volume values: outward for an
//     SDF, and a closed surface has positive signed volume.
//   * Degenerate triangles (a corner exactly at the level) are kept.
//
// Cube numbering (cell with min corner at grid point (i, j, k))
//   corner c = 4 * d0 + 2 * d1 + d2 is the grid point (i + d0, j + d1, k + d2); the case index has
//   bit c set iff corner c is inside.
//   cube edge e = 4 * a + 2 * u + w runs along axis a from its base corner to base + 1 on axis a; u, w
//   are the base corner's offsets on the other two axes in increasing axis order:
//     a = 0: base (0, u, w)     a = 1: base (u, 0, w)     a = 2: base (u, w, 0)
//   The grid point of the base corner owns the edge (its axis-a edge).
//
// Triangle table (generated at first use, mc_table()): on each of the six cube faces the four
// corner classes alone decide the segments: none (0 or 4 inside), one (1 or 3 inside: around the odd
// corner; 2 adjacent inside: between the two crossing edges), or two for the diagonal pattern, which
// is always resolved by cutting off each INSIDE corner on its own.  The rule reads nothing but the
// face's four classes, so the two cells that share a face put the same segments on it and the mesh
// is watertight.  Segments are directed so that, seen from outside the cube, the outside class lies
// to their left; every crossing edge then has one segment in and one out, the segments chain into
// closed loops (started at their lowest edge id, loops in order of that id) and each loop is
// triangulated in its own direction -- the fan from its first vertex unless that needs a diagonal
// between two cube edges of one cube face (such a diagonal lies in the face, where the neighbouring
// cell may put the same one; then the first triangulation without one): at most 5 triangles per case.
//
// Passes
//   classify  one thread per grid point -> one byte per point: bits 0-2 crossing flags of the owned
//             edges (axis 0, 1, 2), bits 3-5 the triangle count of the cell whose min corner the point
//             is (0 on the high faces); per-workgroup (256 points) vertex and triangle sums.
//   scan      exclusive scan of the per-workgroup sums in place (integers: order-free); totals {V, F}.
//   (host)    the caller reads the totals (one 16-byte copy) and allocates verts / faces.
//   verts     ranks within the workgroup from wave ballots of the flag bits (wave totals through LDS);
//             stores the point's first vertex index (32 bit) and writes its vertices.
//   faces     triangle ranks the same way from the count's three bit planes; a cube edge's vertex index
//             is the owning point's stored index + the number of its lower-axis flags.
// Workspace: 1 byte + 4 bytes per grid point and 8 bytes per 256 points, each array rounded up to
// 256 bytes: 5.03 bytes per voxel (675 MB at 512^3, beside the 512 MiB volume).
// Flat indices are 64 bit throughout; V and F must fit int32 (PLY `int`).
#include <mutex>

#include "nr_meshcommon.h"

namespace nr {

// ---------------------------------------------------------------------------------------------
// the 256-case table (host)
// ---------------------------------------------------------------------------------------------
struct McTable {
  int8_t tri[256 * 16];
  int32_t cnt[256];
  uint8_t cnt8[256];
  bool ok;
};

static void mc_corner_xyz(int c, int* p) {
  p[0] = (c >> 2) & 1;
  p[1] = (c >> 1) & 1;
  p[2] = c & 1;
}

// cube edge between two corners that differ on exactly one axis
static int mc_edge_between(int c0, int c1) {
  const int base = c0 < c1 ? c0 : c1, diff = c0 ^ c1;
  const int a = diff == 4 ? 0 : (diff == 2 ? 1 : 2);
  int p[3];
  mc_corner_xyz(base, p);
  const int u = a == 0 ? p[1] : p[0], w = a == 2 ? p[1] : p[2];
  return 4 * a + 2 * u + w;
}

// edge midpoint in doubled integer coordinates
static void mc_edge_mid2(int e, int* m) {
  const int a = e >> 2, u = (e >> 1) & 1, w = e & 1;
  int b[3];
  if (a == 0) { b[0] = 0; b[1] = u; b[2] = w; }
  else if (a == 1) { b[0] = u; b[1] = 0; b[2] = w; }
  else { b[0] = u; b[1] = w; b[2] = 0; }
  for (int q = 0; q < 3; ++q) m[q] = 2 * b[q];
  m[a] += 1;
}

// do two cube edges lie on a common cube face?
static bool mc_share_face(int x, int y) {
  auto faces = [](int e, int* f) {  // face id = 2 * axis + side
    const int a = e >> 2, u = (e >> 1) & 1, w = e & 1;
    const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
    f[0] = 2 * o0 + u;
    f[1] = 2 * o1 + w;
  };
  int fx[2], fy[2];
  faces(x, fx);
  faces(y, fy);
  return fx[0] == fy[0] || fx[0] == fy[1] || fx[1] == fy[0] || fx[1] == fy[1];
}

// Triangulate the closed polygon p[0..n) keeping its orientation, with no diagonal between two cube
// edges of one cube face: such a diagonal would lie in that face, where the neighbouring cell may put
// the same one (a doubled mesh edge).  First choice is the fan from p[0]; other apexes on backtracking.
static bool mc_triangulate(const int* p, int n, int* out, int& n_out) {
  if (n < 3) return n == 2;
  const int start = n_out;
  for (int k = n - 2; k >= 1; --k) {
    if (k > 1 && mc_share_face(p[0], p[k])) continue;
    if (k < n - 2 && mc_share_face(p[k], p[n - 1])) continue;
    n_out = start;
    out[n_out++] = p[0];
    out[n_out++] = p[k];
    out[n_out++] = p[n - 1];
    int right[12];
    for (int q = k; q < n; ++q) right[q - k] = p[q];
    if (mc_triangulate(p, k + 1, out, n_out) && mc_triangulate(right, n - k, out, n_out)) return true;
  }
  n_out = start;
  return false;
}

static void mc_build(McTable& T) {
  T.ok = true;
  for (int cs = 0; cs < 256; ++cs) {
    int next[12], indeg[12];
    for (int e = 0; e < 12; ++e) next[e] = -1, indeg[e] = 0;
    auto inside = [&](int c) { return (cs >> c) & 1; };
    // directed segment between cube edges ea, eb on the face with outward normal sign * axis fa;
    // ref: a corner of that face on one side of the segment
    auto add = [&](int ea, int eb, int ref, int fa, int sign) {
      int A[3], B[3], C[3], d[3], r[3];
      mc_edge_mid2(ea, A);
      mc_edge_mid2(eb, B);
      mc_corner_xyz(ref, C);
      for (int q = 0; q < 3; ++q) d[q] = B[q] - A[q], r[q] = 2 * C[q] - A[q];
      const int cr[3] = {d[1] * r[2] - d[2] * r[1], d[2] * r[0] - d[0] * r[2], d[0] * r[1] - d[1] * r[0]};
      const int s = cr[fa] * sign;  // > 0: ref lies to the left of A -> B seen from outside the cube
      const bool ref_left = s > 0;
      // the outside class belongs on the left
      if (ref_left == (inside(ref) != 0)) { const int t = ea; ea = eb; eb = t; }
      if (next[ea] != -1) T.ok = false;
      next[ea] = eb;
      indeg[eb]++;
    };
    for (int fa = 0; fa < 3; ++fa)
      for (int side = 0; side < 2; ++side) {
        // the face's corners in cyclic order: (0,0) (1,0) (1,1) (0,1) on its two in-plane axes
        static const int cyc[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
        const int b = fa == 0 ? 1 : 0, c = fa == 2 ? 1 : 2;
        int q[4], in[4], n_in = 0;
        for (int m = 0; m < 4; ++m) {
          int p[3];
          p[fa] = side;
          p[b] = cyc[m][0];
          p[c] = cyc[m][1];
          q[m] = 4 * p[0] + 2 * p[1] + p[2];
          in[m] = inside(q[m]);
          n_in += in[m];
        }
        const int sign = side ? 1 : -1;
        auto edge = [&](int m) { return mc_edge_between(q[m & 3], q[(m + 1) & 3]); };  // face edge m: q[m] - q[m+1]
        if (n_in == 1 || n_in == 3) {
          for (int m = 0; m < 4; ++m)
            if (in[m] == (n_in == 1)) add(edge(m + 3), edge(m), q[m], fa, sign);
        } else if (n_in == 2) {
          if (in[0] == in[2]) {  // diagonal pattern: cut off each inside corner
            for (int m = 0; m < 4; ++m)
              if (in[m]) add(edge(m + 3), edge(m), q[m], fa, sign);
          } else {
            for (int m = 0; m < 4; ++m)
              if (in[m] && in[(m + 1) & 3]) add(edge(m + 3), edge(m + 1), q[m], fa, sign);
          }
        }
      }
    // chain into loops, fan-triangulate
    int8_t* row = T.tri + cs * 16;
    for (int q = 0; q < 16; ++q) row[q] = -1;
    int nt = 0;
    bool seen[12] = {};
    for (int e = 0; e < 12; ++e) {
      if ((next[e] != -1) != (indeg[e] == 1) || indeg[e] > 1) T.ok = false;
      if (next[e] == -1 || seen[e]) continue;
      int loop[12], len = 0;
      for (int x = e; x != -1 && !seen[x] && len < 12; x = next[x]) seen[x] = true, loop[len++] = x;
      if (len < 3 || next[loop[len - 1]] != e) { T.ok = false; continue; }
      int out[30], n_out = 0;
      if (!mc_triangulate(loop, len, out, n_out) || nt + n_out / 3 > 5) { T.ok = false; continue; }
      for (int q = 0; q < n_out; ++q) row[3 * nt + q] = (int8_t)out[q];
      nt += n_out / 3;
    }
    T.cnt[cs] = nt;
    T.cnt8[cs] = (uint8_t)nt;
  }
}

static const McTable& mc_table() {
  static const McTable* T = [] {
    McTable* t = new McTable;
    mc_build(*t);
    return t;
  }();
  return *T;
}

// ---------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------
__device__ int8_t g_mc_tri[256 * 16];
__device__ uint8_t g_mc_cnt[256];

constexpr int kMcWG = 256;       // grid points per workgroup (4 waves)
constexpr int kMcScanWG = 1024;  // threads of the single scan workgroup

struct McDims {
  int64_t n0, n1, n2, n;  // n = n0 * n1 * n2
};

struct McXf {
  double spacing[3], origin[3], scale, offset[3];
};

// flat C index -> (i, j, k); 32-bit divisions whenever the grid has fewer than 2^32 points
__device__ __forceinline__ void mc_coords(const McDims& d, int64_t p, int64_t& i, int64_t& j, int64_t& k) {
  if (d.n <= 0xffffffffll) {
    const uint32_t n2 = (uint32_t)d.n2, n1 = (uint32_t)d.n1, q = (uint32_t)p;
    const uint32_t r = q / n2;
    k = q - r * n2;
    const uint32_t ii = r / n1;
    j = r - ii * n1;
    i = ii;
  } else {
    const int64_t r = p / d.n2;
    k = p - r * d.n2;
    i = r / d.n1;
    j = r - i * d.n1;
  }
}

// the 8 corner classes of the cell at p (which must have all its corners inside the grid)
__device__ __forceinline__ unsigned mc_case(const float* __restrict__ vol, const McDims& d, int64_t p, float level) {
  const int64_t s0 = d.n1 * d.n2, s1 = d.n2;
  unsigned m = 0;
  m |= (vol[p] < level ? 1u : 0u) << 0;
  m |= (vol[p + 1] < level ? 1u : 0u) << 1;
  m |= (vol[p + s1] < level ? 1u : 0u) << 2;
  m |= (vol[p + s1 + 1] < level ? 1u : 0u) << 3;
  m |= (vol[p + s0] < level ? 1u : 0u) << 4;
  m |= (vol[p + s0 + 1] < level ? 1u : 0u) << 5;
  m |= (vol[p + s0 + s1] < level ? 1u : 0u) << 6;
  m |= (vol[p + s0 + s1 + 1] < level ? 1u : 0u) << 7;
  return m;
}

__global__ __launch_bounds__(kMcWG) void mc_classify(const float* __restrict__ vol, McDims d, float level,
                                                     uint8_t* __restrict__ codes, int2* __restrict__ wgsum) {
  __shared__ int lds[kMcWG / 64];
  const int64_t p = (int64_t)blockIdx.x * kMcWG + threadIdx.x;
  unsigned code = 0;
  if (p < d.n) {
    int64_t i, j, k;
    mc_coords(d, p, i, j, k);
    const bool e0 = i + 1 < d.n0, e1 = j + 1 < d.n1, e2 = k + 1 < d.n2;
    const int64_t s0 = d.n1 * d.n2, s1 = d.n2;
    const bool c = vol[p] < level;
    if (e0 && (vol[p + s0] < level) != c) code |= 1u;
    if (e1 && (vol[p + s1] < level) != c) code |= 2u;
    if (e2 && (vol[p + 1] < level) != c) code |= 4u;
    if (e0 && e1 && e2) code |= (unsigned)g_mc_cnt[mc_case(vol, d, p, level)] << 3;
    codes[p] = (uint8_t)code;
  }
  int nv = 0, nt = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    nv += __popcll(__ballot((code >> b) & 1u));
    nt += __popcll(__ballot((code >> (3 + b)) & 1u)) << b;
  }
  int all_v, all_t;
  wave_prefix<kMcWG>(nv, lds, all_v);
  wave_prefix<kMcWG>(nt, lds, all_t);
  if (threadIdx.x == 0) wgsum[blockIdx.x] = make_int2(all_v, all_t);
}

struct McSum {  // the scan's accumulator: {vertices, triangles}, 64 bit
  int64_t v, f;
  __device__ McSum& operator+=(const McSum& o) { return v += o.v, f += o.f, *this; }
  __device__ McSum operator-(const McSum& o) const { return {v - o.v, f - o.f}; }
};

// in place: wgsum[b] = {vertices, triangles} before workgroup b; totals = {V, F}.  One workgroup
// (strip_scan).  The int32 bases are meaningful only while V, F fit int32 (the caller checks the int64
// totals before it emits).
__global__ __launch_bounds__(kMcScanWG) void mc_scan(int2* __restrict__ wgsum, int64_t nb, int64_t* __restrict__ totals) {
  __shared__ McSum s[kMcScanWG];
  const auto get = [&](int64_t q) {
    const int2 c = wgsum[q];
    return McSum{c.x, c.y};
  };
  const auto put = [&](int64_t q, const McSum& e) { wgsum[q] = make_int2((int)e.v, (int)e.f); };
  const McSum all = strip_scan<kMcScanWG>(nb, s, get, put);
  if (threadIdx.x == kMcScanWG - 1) totals[0] = all.v, totals[1] = all.f;
}

__global__ __launch_bounds__(kMcWG) void mc_verts(const float* __restrict__ vol, McDims d, float level, McXf xf,
                                                  const uint8_t* __restrict__ codes, const int2* __restrict__ wgbase,
                                                  int* __restrict__ voff, float* __restrict__ verts, int64_t n_verts) {
  __shared__ int lds[kMcWG / 64];
  const int64_t p = (int64_t)blockIdx.x * kMcWG + threadIdx.x;
  const unsigned f = p < d.n ? (codes[p] & 7u) : 0u;
  const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
  int rank = 0, wave_total = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const unsigned long long m = __ballot((f >> b) & 1u);
    rank += __popcll(m & lt);
    wave_total += __popcll(m);
  }
  int all;
  const int64_t first = (int64_t)wgbase[blockIdx.x].x + wave_prefix<kMcWG>(wave_total, lds, all) + rank;
  if (p >= d.n) return;
  voff[p] = (int)first;
  if (f == 0) return;
  int64_t ijk[3];
  mc_coords(d, p, ijk[0], ijk[1], ijk[2]);
  const int64_t dims[3] = {d.n0, d.n1, d.n2}, stride[3] = {d.n1 * d.n2, d.n2, 1};
  const double v0 = (double)vol[p], lv = (double)level;
  int64_t slot = first;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!((f >> a) & 1u) || ijk[a] + 1 >= dims[a]) continue;
    const double v1 = (double)vol[p + stride[a]];
    const double t = ddiv(dsub(lv, v0), dsub(v1, v0));
    if (slot < n_verts) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double idx = c == a ? dadd((double)ijk[c], t) : (double)ijk[c];
        const double w = ddiv(dadd(dmul(idx, xf.spacing[c]), xf.origin[c]), xf.scale);
        verts[slot * 3 + c] = (float)dsub(w, xf.offset[c]);
      }
    }
    ++slot;
  }
}

__global__ __launch_bounds__(kMcWG) void mc_faces(const float* __restrict__ vol, McDims d, float level,
                                                  const uint8_t* __restrict__ codes, const int2* __restrict__ wgbase,
                                                  const int* __restrict__ voff, int* __restrict__ faces, int64_t n_faces) {
  __shared__ int lds[kMcWG / 64];
  const int64_t p = (int64_t)blockIdx.x * kMcWG + threadIdx.x;
  const unsigned nt = p < d.n ? (unsigned)(codes[p] >> 3) : 0u;
  const unsigned long long lt = (1ull << (threadIdx.x & 63)) - 1ull;
  int rank = 0, wave_total = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const unsigned long long m = __ballot((nt >> b) & 1u);
    rank += __popcll(m & lt) << b;
    wave_total += __popcll(m) << b;
  }
  int all;
  const int64_t first = (int64_t)wgbase[blockIdx.x].y + wave_prefix<kMcWG>(wave_total, lds, all) + rank;
  if (nt == 0) return;
  int64_t i, j, k;
  mc_coords(d, p, i, j, k);
  if (i + 1 >= d.n0 || j + 1 >= d.n1 || k + 1 >= d.n2) return;  // only cells inside the grid read their corners
  const int64_t s0 = d.n1 * d.n2, s1 = d.n2;
  const int8_t* __restrict__ row = g_mc_tri + mc_case(vol, d, p, level) * 16;
  const unsigned lim = nt < 5u ? nt : 5u;
  for (unsigned t = 0; t < lim; ++t) {
    const int64_t slot = first + t;
    if (slot >= n_faces) break;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int e = row[3 * t + q];
      int vi = 0;
      if (e >= 0) {  // a row shorter than the stored count cannot happen; stay in bounds regardless
        const int a = e >> 2, u = (e >> 1) & 1, w = e & 1;
        const int d0 = a == 0 ? 0 : u, d1 = a == 0 ? u : (a == 1 ? 0 : w), d2 = a == 2 ? 0 : w;
        const int64_t owner = p + d0 * s0 + d1 * s1 + d2;
        vi = voff[owner] + __popc((unsigned)codes[owner] & ((1u << a) - 1u));
      }
      faces[slot * 3 + q] = vi;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
constexpr int64_t kMcMaxDim = (int64_t)1 << 30;
constexpr int64_t kMcMaxPoints = (int64_t)1 << 38;  // 2^30 workgroups

struct McPlan {
  McDims d;
  int64_t nb;
  size_t o_codes, o_voff, o_wg, total;
};

static bool mc_plan(int64_t n0, int64_t n1, int64_t n2, McPlan& p) {
  if (n0 < 2 || n1 < 2 || n2 < 2 || n0 > kMcMaxDim || n1 > kMcMaxDim || n2 > kMcMaxDim) return false;
  if (n0 > kMcMaxPoints / n1 || n0 * n1 > kMcMaxPoints / n2) return false;
  p.d = McDims{n0, n1, n2, n0 * n1 * n2};
  p.nb = (p.d.n + kMcWG - 1) / kMcWG;
  size_t o = 0;
  p.o_codes = o; o += a256((size_t)p.d.n);
  p.o_voff = o; o += a256((size_t)p.d.n * 4);
  p.o_wg = o; o += a256((size_t)p.nb * 8);
  p.total = o;
  return true;
}

// the table in this device's memory, uploaded once per device (blocking copy: visible to every stream)
static int mc_upload_table() {
  static std::mutex mu;
  static bool done[64] = {};
  int dev = 0;
  NR_HIP_CHECK(hipGetDevice(&dev));
  NR_REQUIRE(dev >= 0 && dev < 64, NR_ERR_UNSUPPORTED, "nr_mc: device index above 63");
  const McTable& T = mc_table();
  NR_REQUIRE(T.ok, NR_ERR_UNSUPPORTED, "nr_mc: internal error, the generated table is inconsistent");
  std::lock_guard<std::mutex> g(mu);
  if (done[dev]) return NR_OK;
  NR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_mc_tri), T.tri, sizeof(T.tri)));
  NR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_mc_cnt), T.cnt8, sizeof(T.cnt8)));
  done[dev] = true;
  return NR_OK;
}

}  // namespace nr

using namespace nr;

extern "C" {

int nr_mc_table(int8_t* tri, int32_t* counts) {
  NR_REQUIRE(tri && counts, NR_ERR_ARG, "nr_mc_table: null argument");
  const McTable& T = mc_table();
  NR_REQUIRE(T.ok, NR_ERR_UNSUPPORTED, "nr_mc_table: internal error, the generated table is inconsistent");
  for (int q = 0; q < 256 * 16; ++q) tri[q] = T.tri[q];
  for (int q = 0; q < 256; ++q) counts[q] = T.cnt[q];
  return NR_OK;
}

size_t nr_mc_workspace_bytes(int64_t n0, int64_t n1, int64_t n2) {
  McPlan pl;
  return mc_plan(n0, n1, n2, pl) ? pl.total : 0;
}

int nr_mc_count(const float* volume, int64_t n0, int64_t n1, int64_t n2, float level, void* workspace,
                size_t workspace_bytes, int64_t* totals, void* stream) {
  McPlan pl;
  NR_REQUIRE(mc_plan(n0, n1, n2, pl), NR_ERR_ARG,
             "nr_mc_count: bad dims (need 2 <= n <= 2^30 on every axis and at most 2^38 points)");
  NR_REQUIRE(volume && totals, NR_ERR_ARG, "nr_mc_count: null argument");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_mc_count: workspace too small");
  int rc = mc_upload_table();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int2* wg = (int2*)(ws + pl.o_wg);
  NR_LAUNCH("mc_classify", (double)pl.d.n, mc_classify, dim3((unsigned)pl.nb), dim3(kMcWG), st, volume, pl.d, level,
            (uint8_t*)(ws + pl.o_codes), wg);
  NR_LAUNCH("mc_scan", (double)pl.nb, mc_scan, dim3(1), dim3(kMcScanWG), st, wg, pl.nb, totals);
  return NR_OK;
}

int nr_mc_emit(const float* volume, int64_t n0, int64_t n1, int64_t n2, float level, const double* spacing,
               const double* origin, double scale, const double* offset, void* workspace, size_t workspace_bytes,
               int64_t n_verts, int64_t n_faces, float* verts, int64_t verts_cap, int32_t* faces, int64_t faces_cap,
               void* stream) {
  McPlan pl;
  NR_REQUIRE(mc_plan(n0, n1, n2, pl), NR_ERR_ARG,
             "nr_mc_emit: bad dims (need 2 <= n <= 2^30 on every axis and at most 2^38 points)");
  NR_REQUIRE(volume && spacing && origin && offset, NR_ERR_ARG, "nr_mc_emit: null argument");
  NR_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_verts <= INT32_MAX && n_faces <= INT32_MAX, NR_ERR_ARG,
             "nr_mc_emit: vertex and face counts must fit int32");
  NR_REQUIRE(verts_cap >= n_verts && faces_cap >= n_faces, NR_ERR_ARG,
             "nr_mc_emit: output capacity below the vertex / face count");
  NR_REQUIRE((verts || n_verts == 0) && (faces || n_faces == 0), NR_ERR_ARG, "nr_mc_emit: null output");
  NR_REQUIRE(workspace && workspace_bytes >= pl.total, NR_ERR_WORKSPACE, "nr_mc_emit: workspace too small");
  if (n_verts == 0 && n_faces == 0) return NR_OK;
  int rc = mc_upload_table();
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const uint8_t* codes = (const uint8_t*)(ws + pl.o_codes);
  int* voff = (int*)(ws + pl.o_voff);
  const int2* wg = (const int2*)(ws + pl.o_wg);
  McXf xf;
  for (int c = 0; c < 3; ++c) xf.spacing[c] = spacing[c], xf.origin[c] = origin[c], xf.offset[c] = offset[c];
  xf.scale = scale;
  NR_LAUNCH("mc_verts", (double)pl.d.n, mc_verts, dim3((unsigned)pl.nb), dim3(kMcWG), st, volume, pl.d, level, xf, codes,
            wg, voff, verts, n_verts);
  NR_LAUNCH("mc_faces", (double)pl.d.n, mc_faces, dim3((unsigned)pl.nb), dim3(kMcWG), st, volume, pl.d, level, codes, wg,
            voff, faces, n_faces);
  return NR_OK;
}

}  // extern "C"
