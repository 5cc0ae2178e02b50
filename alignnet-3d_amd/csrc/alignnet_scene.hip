// Spinning-LiDAR scene generator (the SynthCars-style datasets of tp_utils/pointcloud.py:945-971,1055-1186), gfx950 only.
//
// Replaces trimesh + embree in SyntheticScene.generate_pointcloud_embree: the 64 x 4500-ray sensor (vfov 26.9 deg, 360 deg) is cast against
// a posed triangle mesh, the first hit per ray is kept in ascending ray index (the reference's 20 ray parts, concatenated), and the clipped
// range-dependent noise (:1133-1136) is added.  The semantics are DEFINED by tests/scene_ref.py (fp64, NumPy); what is this project's own:
//  - the intersection is the scalar-triple-product form of Moeller-Trumbore with the origin at 0.  Per triangle (posed vertices v0, v1, v2, e1 = v1 - v0,
//    e2 = v2 - v0):  N = e1 x e2,  A = e2 x v0,  Bv = v0 x e1,  c = v0 . N;  per ray d:  den = d . N,  u = d . A / den,  v = d . Bv / den,  t = c / den;
//    hit when den != 0, u >= 0, v >= 0, u + v <= 1, t > 0 (two-sided; a zero-area triangle has N = 0 and never hits).  Everything is fp64 and every
//    product and sum is rounded as written (no fused multiply-add: an exact zero of N or den must stay one), so the ten numbers per triangle and the three
//    dot products per ray are bit for bit the restatement's.  The kernel tests the signs of the numerators instead of dividing (u >= 0 exactly when d . A
//    and den agree in sign; u + v <= 1 as |d . A + d . Bv| <= |den|, which differs from the quotient form only within a few ulp of an edge, inside the
//    restatement's undecided band of 1e-9) and divides once per hit.  Equal t: the lower triangle index wins, whatever the order of the LDS stage.
//  - the noise stream is the dataset sampler's counter hash (alignnet_dataset.hip: mix64 + Box-Muller) keyed by (seed, scene id, cloud, ray index): a
//    result never depends on the batch it was generated in.  It is NOT np.random.randn's stream (parity unpinned by construction, as for the sampler).
//
// Stages of one alignnet_scene_generate (B scenes x 2 clouds against the uploaded mesh library):
//  1. scene_window_kernel, one workgroup per cloud: every triangle marks the columns its azimuth interval covers (tri_reach: +- 1e-6 column of margin) in an
//     LDS difference array (integer atomics: order-free); a triangle whose xy projection holds the z axis (holds_axis) covers all 4500.  The window is the complement of the
//     largest uncovered gap of the circle of columns, so it may wrap 4499 -> 0.  The windows come back to the host (one small copy), which deals
//     (cloud, tile of 8 window columns) work items: a batch of small far objects and one near object both become hundreds of workgroups.
//  2. scene_cast_kernel (the SCAN, alignnet_set_option "scene_cast" = 0, the default), one workgroup (four waves) per tile; lane = elevation row, a wave
//     takes two of the tile's columns.  The cloud's triangles go through LDS in chunks of 512: each is posed (Rz(angle) (scale v) + position, fp64), culled against the tile's azimuth sector by two exact side tests
//     with a relative margin (all three vertices strictly before the first column's half plane, or strictly behind the last one's: conservative, so what is
//     left is decided in fp64 as above), and the survivors' ten numbers are compacted into LDS (ballot prefix: deterministic order).  The inner loop
//     (cast_triangle per staged triangle, shared with the binned cast; the hit decision and the tie rule are keep_nearest, shared with the band loop) reads one triangle as a broadcast and tests it against the wave's two columns.  Cost model: every tile poses and side-tests all T triangles of its cloud
//     (T / 256 per thread, latency-bound on the vertex gathers) and intersects 64 x 8 rays with the few that overlap its 0.64 deg sector; a car of some
//     hundred triangles is one chunk, a 10^5-triangle model is 200 chunks per tile.  t per ray goes to a [row][window column] table (inf = miss).
//  2b. the BINNED cast ("scene_cast" = 1: every cloud; 2: clouds of more than kSceneBinAuto triangles) removes the T / 256 term: per cloud the triangles
//     are binned to the window's tiles once, and a tile poses only the triangles of its own list.
//       scene_bin_tally_kernel    grid (cloud, slice of the mesh): every triangle is posed once, its tile range found (tri_reach, which the WINDOW kernel calls too --
//                                 the atan2 interval of its three vertices widened by kColMargin columns; every tile when its xy projection holds the z axis
//                                 or it spans half the circle; a zero-area triangle reaches nothing and is dropped) and counted in an LDS histogram of the
//                                 window's tiles, which is added onto the (cloud, tile) counters (integer atomics: order-free);
//       scene_bin_offsets_kernel  one workgroup: exclusive scan of the counters into the 64-bit (cloud, tile) offset table, counters cleared; the total
//                                 goes to the host (the one extra copy of a call), which grows the list buffer (4 bytes per entry);
//       scene_bin_fill_kernel     the tally's grid and the tally's ranges again (the same function on the same numbers), a global atomic cursor per tile
//                                 (the cleared counters) hands out the slots: the ORDER inside a list depends on the run, the SET does not;
//       scene_bincast_kernel      one workgroup per (cloud, tile) as in the scan; walks the tile's list in chunks of lds_triangles, poses each listed
//                                 triangle with the same pose() and tri_setup() (re-posing per entry: a table of posed triangles would be 88 B x T x
//                                 clouds), stages the ten numbers in LDS and runs cast_triangle over them.  Equal t goes to the lower triangle index whatever the
//                                 order, so the result does not depend on the fill order, and it is bit for bit the scan's.
//     Why the lists are conservative: a ray of column c can only hit a triangle when its xy direction lies in the angular span of the triangle's xy
//     projection as seen from the z axis.  When the projection does not hold the axis and spans less than half the circle, that span is the interval
//     between the extreme vertex azimuths (the projection is convex); column c sits at column coordinate c to 1e-13, the interval is widened by 1e-6 column
//     and rounded outwards to whole columns: the margin is seven orders of magnitude above atan2's error, and that alone makes the range conservative.
//     (It is also the function by which the window is chosen -- a column outside every interval is cast by neither path -- but the scan culls inside
//     the window by exact side tests, not by these intervals.)  A range that leaves the window would be clamped to it.
//     Measured (tools/scene_cast_rate.py, profiles/scene_cast_rate.json; 512 clouds, whole calls): the binned cast is NOT ahead of the scan at 516, 5,001,
//     20,001 or 100,002 triangles (0.79 - 0.95 x).  Both casts are bound by the inner loop -- every staged triangle against all 64 x 8 rays of the tile, about
//     0.6 - 0.8 ns of chip time per (tile, triangle) entry -- and the scan's side tests leave it the same entries; the T / 256 term that binning removes is
//     the small one (cast kernel 13.6 -> 12.8 ms at 20,001 triangles) and the binning costs more (1.6 ms there).  Fewer rays per entry -- binning by
//     elevation row inside a tile, for which these lists are the input -- is the step that would pay (2c).  The default stays the scan.
//  2c. BY ELEVATION BAND ("scene_rows" = 1, orthogonal to "scene_cast"; 0, the default, is exactly the kernels above): scene_band_scan_kernel and
//     scene_band_list_kernel keep the two stagings (stage_scan_pass; stage_list_chunk, which the binned cast runs without the masks) and replace the inner loop.  A staged triangle gets an 8-bit mask of the bands of 8 rows it can
//     reach (in SceneTri::pad; the rule and why it is conservative stand above the kernels) and is intersected only with those cells of 8 rows x 8
//     columns, a lane being one ray; the four waves share the staged entries and merge their candidates per ray at the end.  Bit for bit the scan.
//     Measured: tools/scene_rows_rate.py, profiles/scene_rows_rate.json, DESIGN.md 4.9c.
//  3. scene_count_kernel (hits per (cloud, row)), scene_scan_kernel (exclusive scan in (scene, row) order per cloud index: the offsets table),
//     scene_scatter_kernel (per (cloud, row): columns in ascending COLUMN order -- a wrapped window starts at column 0 -- ballot prefix, location = t d in
//     fp64 rounded to float, + noise).  Counts, a scan, a scatter: no atomics that could reorder points.
#include "engine.h"
#include "host_util.h"
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace {

constexpr int kRows = 64, kCols = 4500, kRays = kRows * kCols;
constexpr int kTileCols = 8, kCastThreads = 256, kColsPerWave = kTileCols / (kCastThreads / 64);
constexpr int kLdsTriangles = 512;        // triangles per LDS chunk as shipped (88 bytes each: three workgroups per CU)
constexpr int kSceneBinAuto = kLdsTriangles;   // "scene_cast" = 2: clouds whose mesh has more triangles take the binned cast: where the scan leaves one LDS chunk,
                                               // NOT a measured crossover (none exists up to 100,002 triangles: the header above)
constexpr int kMaxTiles = (kCols + kTileCols - 1) / kTileCols;   // 563 tiles in the all-column window
constexpr int kBinSlices = 32;            // most workgroups per cloud of the tally / fill kernels (256 triangles per pass each)
constexpr double kColMargin = 1e-6;       // columns of margin around a triangle's azimuth interval (fp64 atan2 is good to 1e-13 column)
constexpr double kSideMargin = 1e-12;     // relative margin of the side tests (their rounding error is 4e-16 of the same scale)

struct SceneTri { double N[3], A[3], Bv[3], c; int id, pad; };
static_assert(sizeof(SceneTri) == 88, "LDS budget");

struct SceneCloud {
  double cs, sn, scale, px, py, pz;   // pose: Rz (scale v) + p
  long long v0, f0;                   // first vertex / face of the mesh in the library
  long long tbase;                    // first entry of this cloud's [64][count] table of t
  unsigned long long scene_id;
  int nf, first, count, which;        // faces; window (first column, columns); cloud index 0 / 1
  float strength;
  int bt0;                            // binned cast: the cloud's first entry in the (cloud, tile) offset table; -1: the cloud takes the scan
};

struct V3 { double x, y, z; };

__device__ __forceinline__ V3 pose(const SceneCloud& c, const double* __restrict__ v)
{
#pragma clang fp contract(off)
  const double sx = c.scale * v[0], sy = c.scale * v[1], sz = c.scale * v[2];
  V3 r;
  r.x = (c.cs * sx - c.sn * sy) + c.px;
  r.y = (c.sn * sx + c.cs * sy) + c.py;
  r.z = sz + c.pz;
  return r;
}

__device__ __forceinline__ void tri_setup(const V3& a, const V3& b, const V3& cc, SceneTri& t)
{
#pragma clang fp contract(off)
  const double e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z, e2x = cc.x - a.x, e2y = cc.y - a.y, e2z = cc.z - a.z;
  t.N[0] = e1y * e2z - e1z * e2y; t.N[1] = e1z * e2x - e1x * e2z; t.N[2] = e1x * e2y - e1y * e2x;
  t.A[0] = e2y * a.z - e2z * a.y; t.A[1] = e2z * a.x - e2x * a.z; t.A[2] = e2x * a.y - e2y * a.x;
  t.Bv[0] = a.y * e1z - a.z * e1y; t.Bv[1] = a.z * e1x - a.x * e1z; t.Bv[2] = a.x * e1y - a.y * e1x;
  t.c = (a.x * t.N[0] + a.y * t.N[1]) + a.z * t.N[2];
}

// ---- stage 1: the azimuth window of a cloud --------------------------------------------------------------------------------------------
// column coordinate of a direction in the xy plane: h = atan2(x, y) in degrees, column = (h + 180) / 0.08
__device__ __forceinline__ double col_coord(double x, double y) { return (atan2(x, y) * 57.29577951308232 + 180.0) * (kCols / 360.0); }

// does the xy projection of the posed triangle (a, b, d) hold the z axis (with margin)?  o_k = cross of consecutive vertices; their sum is twice
// the projected area.  ONE rule for the window, the tile lists and the band masks: their conservativeness arguments name the same triangles.
__device__ __forceinline__ bool holds_axis(const V3& a, const V3& b, const V3& d)
{
#pragma clang fp contract(off)
  const double o1 = a.x * b.y - a.y * b.x, o2 = b.x * d.y - b.y * d.x, o3 = d.x * a.y - d.y * a.x;
  const double ext = fmax(fmax(fabs(a.x) + fabs(a.y), fabs(b.x) + fabs(b.y)), fabs(d.x) + fabs(d.y));
  const double m = kSideMargin * ext * ext;
  if (fabs(o1 + o2 + o3) > m) return (o1 >= -m && o2 >= -m && o3 >= -m) || (o1 <= m && o2 <= m && o3 <= m);
  // the projection is a segment: it holds the axis when two vertices lie on opposite sides of it
  return fmin(fmin(a.x * b.x + a.y * b.y, b.x * d.x + b.y * d.y), d.x * a.x + d.y * a.y) <= m;
}

// col_coord as a call: one body of fp64 atan2 per kernel instead of three inlined copies each (which spilled scalar registers in the tally and the fill)
__device__ __attribute__((noinline)) double col_coord_call(double x, double y) { return col_coord(x, y); }

// Which columns a triangle can reach: 0 = none (zero area: never hit), 1 = the n columns from column *s on (they may wrap 4499 -> 0), 2 = every
// column (its xy projection holds the z axis, or it spans half the circle).  The window, the tally and the fill all call it on the same numbers, so
// they see the same ranges (contraction off and one shared atan2 body: the inlined copies round alike; the fill is bounded by the tallied lengths
// regardless).  Nothing depends on their agreeing: a range is conservative on its own, because the 1e-6 column margin is seven orders above the
// error of fp64 atan2 (1e-13 column) -- a column outside every interval can be hit by no ray -- and a range that leaves the window is clamped to it.
__device__ __forceinline__ int tri_reach(const SceneCloud& c, const double* __restrict__ verts, const int* __restrict__ fi, int* s, int* n)
{
#pragma clang fp contract(off)
  const V3 a = pose(c, verts + (c.v0 + fi[0]) * 3), b = pose(c, verts + (c.v0 + fi[1]) * 3), d = pose(c, verts + (c.v0 + fi[2]) * 3);
  SceneTri t;
  tri_setup(a, b, d, t);
  if (t.N[0] == 0.0 && t.N[1] == 0.0 && t.N[2] == 0.0) return 0;
  if (holds_axis(a, b, d)) return 2;
  const double c0 = col_coord_call(a.x, a.y);
  double d1 = col_coord_call(b.x, b.y) - c0, d2 = col_coord_call(d.x, d.y) - c0;
  d1 -= kCols * rint(d1 / kCols); d2 -= kCols * rint(d2 / kCols);   // into [-2250, 2250]
  const double lo = c0 + fmin(0.0, fmin(d1, d2)), hi = c0 + fmax(0.0, fmax(d1, d2));
  if (hi - lo >= kCols / 2 - 1.0) return 2;
  const long long ca = (long long)floor(lo - kColMargin), cb = (long long)ceil(hi + kColMargin);
  int first = (int)(ca % kCols); if (first < 0) first += kCols;
  *s = first; *n = (int)(cb - ca + 1);
  return 1;
}

__device__ int next_bit(const unsigned* w, int p, bool want_set)   // first position >= p whose bit is set / clear, -1 if none below kCols
{
  constexpr int kWords = (kCols + 31) / 32;
  int i = p >> 5;
  if (i >= kWords) return -1;
  unsigned m = (want_set ? w[i] : ~w[i]) & (0xffffffffu << (p & 31));
  while (m == 0) {
    if (++i >= kWords) return -1;
    m = want_set ? w[i] : ~w[i];
  }
  const int q = i * 32 + __ffs(m) - 1;
  return q < kCols ? q : -1;
}

__global__ __launch_bounds__(256) void scene_window_kernel(const SceneCloud* __restrict__ clouds, const double* __restrict__ verts,
                                                           const int* __restrict__ faces, int* __restrict__ win /*[clouds][2]*/)
{
  constexpr int kWords = (kCols + 31) / 32, kPer = 18;   // 250 threads x 18 columns
  __shared__ int diff[kCols + 1];
  __shared__ unsigned words[kWords];
  __shared__ int wsum[4];
  __shared__ int s_full;
  const SceneCloud c = clouds[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i <= kCols; i += 256) diff[i] = 0;
  for (int i = tid; i < kWords; i += 256) words[i] = 0;
  if (tid == 0) s_full = 0;
  __syncthreads();
  for (int f = tid; f < c.nf; f += 256) {
    int s = 0, n = 0;
    const int kind = tri_reach(c, verts, faces + (c.f0 + f) * 3, &s, &n);
    if (kind == 2) s_full = 1;
    else if (kind == 1) {
      atomicAdd(&diff[s], 1);
      if (s + n <= kCols) atomicAdd(&diff[s + n], -1);
      else { atomicAdd(&diff[0], 1); atomicAdd(&diff[s + n - kCols], -1); }
    }
  }
  __syncthreads();
  if (s_full) { if (tid == 0) { win[blockIdx.x * 2] = 0; win[blockIdx.x * 2 + 1] = kCols; } return; }
  // coverage = prefix sum of the difference array > 0: thread t takes columns 18 t .. 18 t + 17
  int own = 0;
  if (tid < kCols / kPer)
    for (int k = 0; k < kPer; ++k) own += diff[tid * kPer + k];
  int inc = own;
  for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int run = inc - own;
  for (int w = 0; w < wave; ++w) run += wsum[w];
  if (tid < kCols / kPer) {
    unsigned bits = 0;
    for (int k = 0; k < kPer; ++k) { run += diff[tid * kPer + k]; if (run > 0) bits |= 1u << k; }
    const int p = tid * kPer, sh = p & 31;
    if (bits) {
      atomicOr(&words[p >> 5], bits << sh);
      if (sh + kPer > 32) atomicOr(&words[(p >> 5) + 1], bits >> (32 - sh));
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int s0 = next_bit(words, 0, true);
    int first = 0, count = 0;
    if (s0 >= 0) {
      int best_len = 0, best_start = 0, pos = s0;
      for (;;) {
        const int g = next_bit(words, pos, false);   // first uncovered column behind the arc that starts at pos
        if (g < 0) { if (s0 > best_len) { best_len = s0; best_start = 0; } break; }   // covered up to 4499: the gap is [0, s0)
        const int n = next_bit(words, g, true);
        if (n < 0) { const int len = kCols - g + s0; if (len > best_len) { best_len = len; best_start = g; } break; }
        if (n - g > best_len) { best_len = n - g; best_start = g; }
        pos = n;
      }
      first = (best_start + best_len) % kCols; count = kCols - best_len;
      if (best_len == 0) first = 0;
    }
    win[blockIdx.x * 2] = first; win[blockIdx.x * 2 + 1] = count;
  }
}

// ---- stage 2: the cast ---------------------------------------------------------------------------------------------------------------------
// The hit decision of every cast, once: the signs of the numerators against den (the header's form of u >= 0, v >= 0, u + v <= 1, t > 0), one
// division per hit, and the tie rule -- equal t goes to the lower triangle index.  Every cross-mode equality rests on there being one copy.
__device__ __forceinline__ void keep_nearest(double cc, int id, double den, double un, double vn, double& best, int& bid)
{
#pragma clang fp contract(off)
  const double sum = un + vn;
  const bool hit = den > 0.0 ? (un >= 0.0 && vn >= 0.0 && sum <= den && cc > 0.0)
                             : (den < 0.0 && un <= 0.0 && vn <= 0.0 && sum >= den && cc < 0.0);
  if (hit) {
    const double tt = cc / den;
    if (tt > 0.0 && (tt < best || (tt == best && id < bid))) { best = tt; bid = id; }
  }
}

// the whole-tile loop's arithmetic: one staged triangle against the wave's columns of one elevation row (dz . N2, dz . A2, dz . Bv2 formed once)
__device__ __forceinline__ void cast_triangle(const SceneTri& t, const double (&dx)[kColsPerWave], const double (&dy)[kColsPerWave], double dz,
                                              double (&best)[kColsPerWave], int (&bid)[kColsPerWave])
{
#pragma clang fp contract(off)
  const double N0 = t.N[0], N1 = t.N[1], N2 = t.N[2], A0 = t.A[0], A1 = t.A[1], A2 = t.A[2], B0 = t.Bv[0], B1 = t.Bv[1], B2 = t.Bv[2], cc = t.c;
  const int id = t.id;
  const double nz = dz * N2, az = dz * A2, bz = dz * B2;
#pragma unroll
  for (int q = 0; q < kColsPerWave; ++q) {
    const double den = (dx[q] * N0 + dy[q] * N1) + nz;
    const double un = (dx[q] * A0 + dy[q] * A1) + az;
    const double vn = (dx[q] * B0 + dy[q] * B1) + bz;
    keep_nearest(cc, id, den, un, vn, best[q], bid[q]);
  }
}

struct SceneCastArgs {
  const SceneCloud* clouds; const int* tiles /*[tiles][2] = cloud, tile of the window*/;
  const double* verts; const int* faces; const double* dir /*[4500] x | [4500] y | [64] z*/;
  double* t; int* tri;          // [64][count] per cloud at tbase; tri only in the traced instantiation
  int lds_triangles;
};

// what every cast kernel starts from: its (cloud, tile) work item
struct SceneTile {
  SceneCloud c; int ci, j0, ncol;   // the cloud (a copy) and its index, the tile's first window column, its columns (the last tile may be ragged)
  double ax, ay, bx, by;            // the tile's azimuth sector, for the scan staging: the directions of its first and last column
};

template <bool kSector>
__device__ __forceinline__ SceneTile tile_begin(const SceneCastArgs& a)
{
  SceneTile tl;
  tl.ci = a.tiles[blockIdx.x * 2]; tl.j0 = a.tiles[blockIdx.x * 2 + 1] * kTileCols;
  tl.c = a.clouds[tl.ci];
  tl.ncol = min(kTileCols, tl.c.count - tl.j0);
  tl.ax = tl.ay = tl.bx = tl.by = 0.0;
  if constexpr (kSector) {
    const int col_a = (tl.c.first + tl.j0) % kCols, col_b = (tl.c.first + tl.j0 + tl.ncol - 1) % kCols;   // (the window may wrap)
    tl.ax = a.dir[col_a]; tl.ay = a.dir[kCols + col_a]; tl.bx = a.dir[col_b]; tl.by = a.dir[kCols + col_b];
  }
  return tl;
}

// the SCAN ("scene_cast" = 0, "scene_rows" = 0): the reference every other setting is tested against.  Its staging pass stays written out here (the band
// loop's is stage_scan_pass), and the lane set-up and the store here and in scene_bincast_kernel: as functions they move this kernel's registers off
// the 80 VGPRs the tests pin, or cost the two kernels instructions (tried piece by piece)
template <bool kTrace>
__global__ __launch_bounds__(kCastThreads) void scene_cast_kernel(const SceneCastArgs a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  SceneTri* tris = reinterpret_cast<SceneTri*>(lds_raw);
  __shared__ int wcnt[kCastThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SceneTile tl = tile_begin<true>(a);
  const SceneCloud& c = tl.c;
  const int j0 = tl.j0, ncol = tl.ncol;
  const double ax = tl.ax, ay = tl.ay, bx = tl.bx, by = tl.by;
  const double dz = a.dir[2 * kCols + lane];
  double dx[kColsPerWave], dy[kColsPerWave], best[kColsPerWave];
  int bid[kColsPerWave];
#pragma unroll
  for (int q = 0; q < kColsPerWave; ++q) {
    const int j = j0 + wave * kColsPerWave + q;
    const int col = (c.first + min(j, c.count - 1)) % kCols;   // (a column past the tile's end runs along on the last one; never stored)
    dx[q] = a.dir[col]; dy[q] = a.dir[kCols + col];
    best[q] = INFINITY; bid[q] = -1;
  }
  const int L = a.lds_triangles;
  for (int f0 = 0; f0 < c.nf; f0 += L) {
    const int fend = min(c.nf, f0 + L);
    int n = 0;   // triangles staged so far (the same in every thread)
    for (int r0 = f0; r0 < fend; r0 += kCastThreads) {
      const int f = r0 + tid;
      bool keep = false;
      SceneTri tr;
      if (f < fend) {
        const int* fi = a.faces + (c.f0 + f) * 3;
        const V3 p = pose(c, a.verts + (c.v0 + fi[0]) * 3), q = pose(c, a.verts + (c.v0 + fi[1]) * 3), r = pose(c, a.verts + (c.v0 + fi[2]) * 3);
        // side of a column's half plane: s = dir_x y - dir_y x = |p| sin(column azimuth - point azimuth) (> 0: the point lies before the column)
        const double mp = kSideMargin * 120.0 * (fabs(p.x) + fabs(p.y)), mq = kSideMargin * 120.0 * (fabs(q.x) + fabs(q.y)), mr = kSideMargin * 120.0 * (fabs(r.x) + fabs(r.y));
        const bool before = ax * p.y - ay * p.x > mp && ax * q.y - ay * q.x > mq && ax * r.y - ay * r.x > mr;
        const bool behind = bx * p.y - by * p.x < -mp && bx * q.y - by * q.x < -mq && bx * r.y - by * r.x < -mr;
        keep = !before && !behind;
        if (keep) { tri_setup(p, q, r, tr); tr.id = f; tr.pad = 0; }
      }
      const unsigned long long m = __ballot(keep);
      if (lane == 0) wcnt[wave] = __popcll(m);
      __syncthreads();
      int base = n, total = 0;
#pragma unroll
      for (int w = 0; w < kCastThreads / 64; ++w) { const int k = wcnt[w]; if (w < wave) base += k; total += k; }
      if (keep) tris[base + __popcll(m & ((1ull << lane) - 1ull))] = tr;
      n += total;
      __syncthreads();
    }
    for (int k = 0; k < n; ++k) cast_triangle(tris[k], dx, dy, dz, best, bid);   // every lane reads the same address: a broadcast
    __syncthreads();   // the stage is rewritten by the next chunk
  }
#pragma unroll
  for (int q = 0; q < kColsPerWave; ++q) {
    const int j = j0 + wave * kColsPerWave + q;
    if (j < j0 + ncol) {
      const long long o = c.tbase + (long long)lane * c.count + j;
      a.t[o] = best[q];
      if constexpr (kTrace) a.tri[o] = bid[q];
    }
  }
}

// ---- stage 2b: the binned cast -------------------------------------------------------------------------------------------------------------
// the tiles of the cloud's window that the n columns from column s on touch: at most two runs [k0, k1] (the second when the columns pass the
// window's column 4500, which only the all-column window allows); columns outside the window are dropped.  Returns the number of runs.
__device__ __forceinline__ int reach_tiles(const SceneCloud& c, int s, int n, int (&k0)[2], int (&k1)[2])
{
  int js = s - c.first; if (js < 0) js += kCols;   // window column of the first one
  const int je = js + n - 1;
  int runs = 0;
  if (js < c.count) { k0[runs] = js / kTileCols; k1[runs] = min(je, c.count - 1) / kTileCols; ++runs; }
  if (je >= kCols) { k0[runs] = 0; k1[runs] = min(je - kCols, c.count - 1) / kTileCols; ++runs; }
  return runs;
}

// grid (clouds, slices): lengths of the tile lists of the clouds on the binned path
__global__ __launch_bounds__(256) void scene_bin_tally_kernel(const SceneCloud* __restrict__ clouds, const double* __restrict__ verts,
                                                              const int* __restrict__ faces, int* __restrict__ cnt)
{
  __shared__ int hist[kMaxTiles];
  __shared__ int s_all;
  const SceneCloud c = clouds[blockIdx.x];
  if (c.bt0 < 0 || c.count <= 0) return;   // (uniform: the whole workgroup leaves)
  const int tid = threadIdx.x, ntile = (c.count + kTileCols - 1) / kTileCols;
  for (int k = tid; k < ntile; k += 256) hist[k] = 0;
  if (tid == 0) s_all = 0;
  __syncthreads();
  for (int f = blockIdx.y * 256 + tid; f < c.nf; f += gridDim.y * 256) {
    int s = 0, n = 0, k0[2], k1[2];
    const int kind = tri_reach(c, verts, faces + (c.f0 + f) * 3, &s, &n);
    if (kind == 2) atomicAdd(&s_all, 1);
    else if (kind == 1) {
      const int runs = reach_tiles(c, s, n, k0, k1);
      for (int r = 0; r < runs; ++r)
        for (int k = k0[r]; k <= k1[r]; ++k) atomicAdd(&hist[k], 1);
    }
  }
  __syncthreads();
  const int all = s_all;
  for (int k = tid; k < ntile; k += 256) {
    const int v = hist[k] + all;
    if (v) atomicAdd(&cnt[c.bt0 + k], v);
  }
}

// one workgroup of 1024: exclusive scan of the n list lengths -> off [n + 1] (64-bit); the lengths are cleared (the fill's cursors)
__global__ __launch_bounds__(1024) void scene_bin_offsets_kernel(int* __restrict__ cnt, long long* __restrict__ off, int n)
{
  __shared__ long long part[1024];
  const int tid = threadIdx.x;
  const long long per = ((long long)n + 1023) / 1024, lo = min((long long)n, tid * per), hi = min((long long)n, lo + per);
  long long s = 0;
  for (long long e = lo; e < hi; ++e) s += cnt[e];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < 1024; ++i) { const long long v = part[i]; part[i] = run; run += v; }
    off[n] = run;
  }
  __syncthreads();
  long long run = part[tid];
  for (long long e = lo; e < hi; ++e) { off[e] = run; run += cnt[e]; cnt[e] = 0; }
}

// grid (clouds, slices) as the tally: the triangle indices into their tiles' lists
__global__ __launch_bounds__(256) void scene_bin_fill_kernel(const SceneCloud* __restrict__ clouds, const double* __restrict__ verts,
                                                             const int* __restrict__ faces, int* __restrict__ cur, const long long* __restrict__ off,
                                                             int* __restrict__ list)
{
  const SceneCloud c = clouds[blockIdx.x];
  if (c.bt0 < 0 || c.count <= 0) return;
  const int ntile = (c.count + kTileCols - 1) / kTileCols;
  for (int f = blockIdx.y * 256 + threadIdx.x; f < c.nf; f += gridDim.y * 256) {
    int s = 0, n = 0, k0[2], k1[2], runs = 0;
    const int kind = tri_reach(c, verts, faces + (c.f0 + f) * 3, &s, &n);
    if (kind == 2) { runs = 1; k0[0] = 0; k1[0] = ntile - 1; }
    else if (kind == 1) runs = reach_tiles(c, s, n, k0, k1);
    for (int r = 0; r < runs; ++r)
      for (int k = k0[r]; k <= k1[r]; ++k) {
        const long long b = off[c.bt0 + k], len = off[c.bt0 + k + 1] - b;
        const int slot = atomicAdd(&cur[c.bt0 + k], 1);
        if (slot < len) list[b + slot] = f;   // (never beyond the tallied length)
      }
  }
}

struct SceneBinCastArgs {
  SceneCastArgs c;               // tiles: the binned clouds' (cloud, tile) items, in the order of the offset table
  const long long* off;          // [items + 1]
  const int* list;
};

// ---- stage 2c: both casts by elevation band ("scene_rows" = 1) --------------------------------------------------------------------------------
// The tile and the workgroup stay (8 window columns x 64 rows, 256 threads); the unit of work becomes a CELL, one band of 8 consecutive rows x the
// tile's 8 columns = 64 rays = one wave.  A lane is a ray: column lane & 7 of the tile, row 8 b + (lane >> 3) in band b.  A staged triangle carries
// an 8-bit band mask in SceneTri::pad and is intersected only with the cells whose bit is set (a wave-uniform skip).
//
// THE MASK RULE, and why it is conservative.  A ray of column c and row r has the direction d = (dir_x[c], dir_y[c], dir_z[r]) and meets the
// triangle at P = t d, t > 0, so P.z = t dir_z[r] and rho(P) = sqrt(P.x^2 + P.y^2) = t n_c with n_c = sqrt(dir_x[c]^2 + dir_y[c]^2):
//     dir_z[r] = n_c s(P),   s(P) = P.z / rho(P).
// Over the triangle P.z lies between the extreme vertex z, and rho between rho_min, the distance from the z axis to the triangle's xy projection
// when that does not hold the axis -- the smallest of the three point-to-segment distances, which an edge can attain strictly inside itself, so
// it is NOT the smallest vertex rho -- and rho_max, the largest vertex rho (rho is convex).  By the signs of z_min and z_max:
//     s_lo = z_min / (z_min >= 0 ? rho_max : rho_min),   s_hi = z_max / (z_max >= 0 ? rho_min : rho_max),
// and with n_lo <= n_c <= n_hi over the tile's columns dir_z[r] lies in [min(s_lo n_lo, s_lo n_hi), max(s_hi n_lo, s_hi n_hi)].  Bit b is set iff
// one of the band's eight dir_z values lies in that interval, compared one by one (a ballot over lane = row): the table may be any finite numbers.
// The margin.  s_lo and s_hi are widened by kBandMargin (1 + |s|), 1e-8: seven orders above the rounding of the dozen fp64 operations behind them
// (the closest point of an edge is p + t e, good to 1e-16 rho_max absolute, and rho_min > 1e-6 rho_max is required below, so rho_min is good to
// 1e-10 relative), and 1e-6 of a row of the default sensor.  The same margin has to cover what cast_ray calls a hit: it tests the rounded
// numerators un, vn, un + vn against the rounded den, each off by at most E = 2e-15 |d| e_max P_max (e_max the longest edge, P_max the farthest
// vertex; their own rounding included), so a "hit" can lie at barycentric coordinates as far as eta = 2 E / |den| outside [0, 1].  At a hit
// |den| = |c| |d| / |P| >= |c| |d| / (5 P_max) while eta < 1/2, hence eta <= kBandEta e_max P_max^2 / |c| with kBandEta = 2e-14, the point lies
// within dev = 2 eta e_max of the triangle, and s moves by at most (dev / rho_min) (1 + |s|) (|grad s| = sqrt(1 + s^2) / rho).  A triangle gets
// the interval only when eta < 1/2 and dev < kBandMargin rho_min / 2.  Everything else gets EVERY band: a projection that holds the z axis
// (the test of tri_reach, rho_min = 0), rho_min <= 1e-6 rho_max, a plane through or next to the sensor (c = 0: an edge-on face, whose hits are
// decided by rounding alone) or a sliver.  A face of zero area (N = 0 exactly: den = 0, never hit) gets no band.
constexpr int kBands = kRows / 8;
constexpr double kBandMargin = 1e-8, kBandEta = 2e-14;
static_assert(kTileCols == 8 && kCastThreads == 256 && kBands == 8, "a cell is 8 rows x 8 columns, one wave; the mask is 8 bits");

// squared distance from the origin to the segment p .. q of the xy plane
__device__ __forceinline__ double seg_dist2(const V3& p, const V3& q)
{
#pragma clang fp contract(off)
  const double ex = q.x - p.x, ey = q.y - p.y, ee = ex * ex + ey * ey;
  const double t = ee > 0.0 ? fmin(fmax(-(p.x * ex + p.y * ey) / ee, 0.0), 1.0) : 0.0;
  const double x = p.x + t * ex, y = p.y + t * ey;
  return x * x + y * y;
}

// [*lo, *hi]: where dir_z[r] of a row that can hit the posed triangle (a, b, d) lies, for the columns with n_lo <= n_c <= n_hi (the rule above)
__device__ __forceinline__ void band_interval(const V3& a, const V3& b, const V3& d, const SceneTri& t, double n_lo, double n_hi, double* lo, double* hi)
{
#pragma clang fp contract(off)
  if (t.N[0] == 0.0 && t.N[1] == 0.0 && t.N[2] == 0.0) { *lo = INFINITY; *hi = -INFINITY; return; }   // zero area: no band
  *lo = -INFINITY; *hi = INFINITY;   // every band, unless all of the following holds
  if (holds_axis(a, b, d)) return;
  const double ra = a.x * a.x + a.y * a.y, rb = b.x * b.x + b.y * b.y, rd = d.x * d.x + d.y * d.y;
  const double rmax2 = fmax(fmax(ra, rb), rd), rmin2 = fmin(fmin(seg_dist2(a, b), seg_dist2(b, d)), seg_dist2(d, a));
  if (!(rmin2 > 1e-12 * rmax2)) return;
  const double rmin = sqrt(rmin2), rmax = sqrt(rmax2);
  const double p2 = fmax(fmax(ra + a.z * a.z, rb + b.z * b.z), rd + d.z * d.z);
  const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = d.x - b.x, vy = d.y - b.y, vz = d.z - b.z, wx = a.x - d.x, wy = a.y - d.y, wz = a.z - d.z;
  const double e2 = fmax(fmax((ux * ux + uy * uy) + uz * uz, (vx * vx + vy * vy) + vz * vz), (wx * wx + wy * wy) + wz * wz);
  // eta < 1/2 and dev = 2 eta e_max < kBandMargin rho_min / 2, eta = kBandEta e_max P_max^2 / |c|, without dividing (a NaN or c = 0 fails both)
  const double g = kBandEta * p2, ac = fabs(t.c);
  if (!((g * g) * e2 < 0.25 * (ac * ac)) || !(4.0 * (g * e2) < (kBandMargin * rmin) * ac)) return;
  const double zmin = fmin(fmin(a.z, b.z), d.z), zmax = fmax(fmax(a.z, b.z), d.z);
  double s_lo = zmin / (zmin >= 0.0 ? rmax : rmin), s_hi = zmax / (zmax >= 0.0 ? rmin : rmax);
  s_lo -= kBandMargin * (1.0 + fabs(s_lo)); s_hi += kBandMargin * (1.0 + fabs(s_hi));
  *lo = fmin(s_lo * n_lo, s_lo * n_hi); *hi = fmax(s_hi * n_lo, s_hi * n_hi);
}

// the band masks of a wave's triangles, one per lane (have = false: none, mask 0): one triangle at a time, its interval read from its lane and
// every lane answering for the row of its own number (dzl = dir_z[lane]); the ballot's byte b is band b.  Called by whole waves.
__device__ __forceinline__ int band_masks(bool have, double lo, double hi, double dzl, int lane)
{
  int mine = 0;
  for (unsigned long long todo = __ballot(have); todo; todo &= todo - 1) {
    const int src = __ffsll((long long)todo) - 1;
    const double l = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(lo), src), __builtin_amdgcn_readlane(__double2loint(lo), src));
    const double u = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(hi), src), __builtin_amdgcn_readlane(__double2loint(hi), src));
    unsigned long long x = __ballot(l <= dzl && dzl <= u);
    x |= x >> 4; x |= x >> 2; x |= x >> 1;                                            // bit 8 b: some row of band b
    const int mask = (int)(((x & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);   // ... gathered into bit b
    if (lane == src) mine = mask;
  }
  return mine;
}

// one staged triangle against ONE ray: cast_triangle's expressions in cast_triangle's shape (xn, xa, xb: the ray's dx N0 + dy N1, dx A0 + dy A1,
// dx B0 + dy B1, which the bands of a lane share)
__device__ __forceinline__ void cast_ray(const SceneTri& t, double xn, double xa, double xb, double dz, double& best, int& bid)
{
#pragma clang fp contract(off)
  const double nz = dz * t.N[2], az = dz * t.A[2], bz = dz * t.Bv[2];
  keep_nearest(t.c, t.id, xn + nz, xa + az, xb + bz, best, bid);
}

struct SceneBandArgs {
  SceneBinCastArgs b;            // (off and list: the list staging only)
  int* cells;                    // [tiles][8] staged triangles per (tile, band) whose bit is set; the traced instantiations only
};

// the rays of a lane and what the staging needs of the tile.  Balance: the bands an object covers are few and adjacent, so fixed bands per wave
// would leave most waves idle; instead wave w takes the staged entries k = w mod 4 over all their set bands, with best / bid per band in
// registers under an unrolled wave-uniform test, and the four candidates per ray are merged through LDS at the end by the tie rule (the
// smallest (t, triangle) of a ray in any order is the scan's).  That needs no list of (entry, band) pairs, no prefix sum and no atomics.
struct BandLane { double dx, dy, dz[kBands], best[kBands]; int bid[kBands]; };

__device__ __forceinline__ void band_begin(const SceneCastArgs& a, const SceneCloud& c, int j0, int ncol, int lane, BandLane& r, double* n_lo, double* n_hi)
{
  const int col = (c.first + j0 + min(lane & 7, ncol - 1)) % kCols;   // (a column past the tile's end runs along on the last one; never stored)
  r.dx = a.dir[col]; r.dy = a.dir[kCols + col];
#pragma unroll
  for (int b = 0; b < kBands; ++b) { r.dz[b] = a.dir[2 * kCols + 8 * b + (lane >> 3)]; r.best[b] = INFINITY; r.bid[b] = -1; }
  double lo = INFINITY, hi = 0.0;
  for (int q = 0; q < ncol; ++q) {
    const int cq = (c.first + j0 + q) % kCols;
    const double x = a.dir[cq], y = a.dir[kCols + cq], n = sqrt(x * x + y * y);
    lo = fmin(lo, n); hi = fmax(hi, n);
  }
  *n_lo = lo; *n_hi = hi;
}

// the n staged triangles against the tile: wave w takes k = w, w + 4, ...
__device__ __forceinline__ void band_cast(const SceneTri* tris, int n, int wave, BandLane& r)
{
#pragma clang fp contract(off)
  for (int k = wave; k < n; k += kCastThreads / 64) {
    const SceneTri& t = tris[k];   // every lane reads the same address: a broadcast
    const int mask = __builtin_amdgcn_readfirstlane(t.pad);
    if (mask == 0) continue;
    const double xn = r.dx * t.N[0] + r.dy * t.N[1], xa = r.dx * t.A[0] + r.dy * t.A[1], xb = r.dx * t.Bv[0] + r.dy * t.Bv[1];
#pragma unroll
    for (int b = 0; b < kBands; ++b)
      if (mask & (1 << b)) cast_ray(t, xn, xa, xb, r.dz[b], r.best[b], r.bid[b]);
  }
}

// traced: threads 0 .. 7 count the staged triangles whose bit of their band is set
__device__ __forceinline__ int band_tally(const SceneTri* tris, int n, int band)
{
  int s = 0;
  for (int k = 0; k < n; ++k) s += (tris[k].pad >> band) & 1;
  return s;
}

// the four waves' candidates per ray, two bands at a time through 6 KiB of LDS; t (and the triangle) to the [row][window column] table
template <bool kTrace>
__device__ __forceinline__ void band_merge_store(const SceneCastArgs& a, const SceneCloud& c, int j0, int ncol, const BandLane& r,
                                                 double (*mt)[2][64], int (*mi)[2][64])
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int g = 0; g < kBands / 2; ++g) {
    mt[wave][0][lane] = r.best[2 * g]; mt[wave][1][lane] = r.best[2 * g + 1];
    mi[wave][0][lane] = r.bid[2 * g]; mi[wave][1][lane] = r.bid[2 * g + 1];
    __syncthreads();
    if (tid < 128) {
      const int h = tid >> 6;
      double bt = mt[0][h][lane];
      int bi = mi[0][h][lane];
#pragma unroll
      for (int w = 1; w < kCastThreads / 64; ++w) {
        const double tt = mt[w][h][lane];
        const int id = mi[w][h][lane];
        if (tt < bt || (tt == bt && id < bi)) { bt = tt; bi = id; }
      }
      if ((lane & 7) < ncol) {
        const long long o = c.tbase + (long long)(8 * (2 * g + h) + (lane >> 3)) * c.count + j0 + (lane & 7);
        a.t[o] = bt;
        if constexpr (kTrace) a.tri[o] = bi;
      }
    }
    __syncthreads();
  }
}

// ---- the shared stagings and their kernels: the binned cast (list staging, whole-tile loop) and the two band kernels ---------------------------
// what the band masks need of the tile: the extreme column norms, and dir_z of the row of the lane's own number (band_masks: lane = row)
struct BandRule { double n_lo, n_hi, dzl; };

// THE SCAN STAGING of the band loop, one pass: faces r0 .. r0 + 255 (below fend) of the cloud are posed, culled against the tile's sector and given
// their band masks (a triangle of no band is not staged); the survivors' ten numbers are compacted behind the n triangles already staged (ballot
// prefix: the order is the faces').  Returns the new count, the same in every thread.  scene_cast_kernel keeps its own copy of this pass
// without the masks: its registers and instructions, which tests pin, change as soon as any part of the pass is a function.
__device__ __forceinline__ int stage_scan_pass(const SceneCastArgs& a, const SceneTile& tl, const BandRule& br, int r0, int fend, int n, SceneTri* tris,
                                               int* wcnt)
{
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SceneCloud& c = tl.c;
  const int f = r0 + tid;
  bool keep = false;
  SceneTri tr;
  double lo = 0.0, hi = 0.0;
  if (f < fend) {
    const int* fi = a.faces + (c.f0 + f) * 3;
    const V3 p = pose(c, a.verts + (c.v0 + fi[0]) * 3), q = pose(c, a.verts + (c.v0 + fi[1]) * 3), v = pose(c, a.verts + (c.v0 + fi[2]) * 3);
    // side of a column's half plane: s = dir_x y - dir_y x = |p| sin(column azimuth - point azimuth) (> 0: the point lies before the column)
    const double mp = kSideMargin * 120.0 * (fabs(p.x) + fabs(p.y)), mq = kSideMargin * 120.0 * (fabs(q.x) + fabs(q.y)), mv = kSideMargin * 120.0 * (fabs(v.x) + fabs(v.y));
    const bool before = tl.ax * p.y - tl.ay * p.x > mp && tl.ax * q.y - tl.ay * q.x > mq && tl.ax * v.y - tl.ay * v.x > mv;
    const bool behind = tl.bx * p.y - tl.by * p.x < -mp && tl.bx * q.y - tl.by * q.x < -mq && tl.bx * v.y - tl.by * v.x < -mv;
    keep = !before && !behind;
    if (keep) { tri_setup(p, q, v, tr); tr.id = f; band_interval(p, q, v, tr, br.n_lo, br.n_hi, &lo, &hi); }
  }
  tr.pad = band_masks(keep, lo, hi, br.dzl, lane);
  keep = keep && tr.pad != 0;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  int base = n, total = 0;
#pragma unroll
  for (int w = 0; w < kCastThreads / 64; ++w) { const int k = wcnt[w]; if (w < wave) base += k; total += k; }
  if (keep) tris[base + __popcll(m & ((1ull << lane) - 1ull))] = tr;
  __syncthreads();
  return n + total;
}

// THE LIST STAGING, one chunk: the n entries from list on are posed (re-posing per entry: a table of posed triangles would be 88 B x T x clouds)
// and staged in the list's order; an entry that is not a face of this mesh becomes a triangle that no ray hits.  kBand: with the band mask (no
// face: no band); whole waves go round, because band_masks ballots.
template <bool kBand>
__device__ __forceinline__ void stage_list_chunk(const SceneCastArgs& a, const SceneCloud& c, const int* __restrict__ list, int n, SceneTri* tris,
                                                 const BandRule& br = BandRule())
{
  const int tid = threadIdx.x, lane = tid & 63;
  for (int k0 = 0; (kBand ? k0 : k0 + tid) < n; k0 += kCastThreads) {   // (kBand: whole waves go round)
    const int k = k0 + tid;
    const int f = k < n ? list[k] : -1;
    const bool face = (unsigned)f < (unsigned)c.nf;
    SceneTri tr;
    double lo = 0.0, hi = 0.0;
    if (face) {
      const int* fi = a.faces + (c.f0 + f) * 3;
      const V3 p = pose(c, a.verts + (c.v0 + fi[0]) * 3), q = pose(c, a.verts + (c.v0 + fi[1]) * 3), v = pose(c, a.verts + (c.v0 + fi[2]) * 3);
      tri_setup(p, q, v, tr);
      if constexpr (kBand) band_interval(p, q, v, tr, br.n_lo, br.n_hi, &lo, &hi);
    } else {
      tr.N[0] = tr.N[1] = tr.N[2] = tr.A[0] = tr.A[1] = tr.A[2] = tr.Bv[0] = tr.Bv[1] = tr.Bv[2] = tr.c = 0.0;
    }
    tr.id = f; tr.pad = 0;
    if constexpr (kBand) tr.pad = band_masks(face, lo, hi, br.dzl, lane);
    if (k < n) tris[k] = tr;
  }
}

// the binned cast: the tile's list in chunks of lds_triangles
template <bool kTrace>
__global__ __launch_bounds__(kCastThreads) void scene_bincast_kernel(const SceneBinCastArgs b)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  SceneTri* tris = reinterpret_cast<SceneTri*>(lds_raw);
  const SceneCastArgs& a = b.c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SceneTile tl = tile_begin<false>(a);
  const SceneCloud& c = tl.c;
  const int j0 = tl.j0, ncol = tl.ncol;
  const double dz = a.dir[2 * kCols + lane];
  double dx[kColsPerWave], dy[kColsPerWave], best[kColsPerWave];
  int bid[kColsPerWave];
#pragma unroll
  for (int q = 0; q < kColsPerWave; ++q) {
    const int j = j0 + wave * kColsPerWave + q;
    const int col = (c.first + min(j, c.count - 1)) % kCols;   // (a column past the tile's end runs along on the last one; never stored)
    dx[q] = a.dir[col]; dy[q] = a.dir[kCols + col];
    best[q] = INFINITY; bid[q] = -1;
  }
  const long long e0 = b.off[blockIdx.x], e1 = b.off[(long long)blockIdx.x + 1];
  const int L = a.lds_triangles;
  for (long long s0 = e0; s0 < e1; s0 += L) {
    const int n = (int)min((long long)L, e1 - s0);
    stage_list_chunk<false>(a, c, b.list + s0, n, tris);
    __syncthreads();
    for (int k = 0; k < n; ++k) cast_triangle(tris[k], dx, dy, dz, best, bid);   // every lane reads the same address: a broadcast
    __syncthreads();   // the stage is rewritten by the next chunk
  }
#pragma unroll
  for (int q = 0; q < kColsPerWave; ++q) {
    const int j = j0 + wave * kColsPerWave + q;
    if (j < j0 + ncol) {
      const long long o = c.tbase + (long long)lane * c.count + j;
      a.t[o] = best[q];
      if constexpr (kTrace) a.tri[o] = bid[q];
    }
  }
}

// the scan's staging under the band loop
template <bool kTrace>
__global__ __launch_bounds__(kCastThreads) void scene_band_scan_kernel(const SceneBandArgs s)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  SceneTri* tris = reinterpret_cast<SceneTri*>(lds_raw);
  __shared__ int wcnt[kCastThreads / 64];
  __shared__ double mt[kCastThreads / 64][2][64];
  __shared__ int mi[kCastThreads / 64][2][64];
  const SceneCastArgs& a = s.b.c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SceneTile tl = tile_begin<true>(a);
  BandLane r;
  BandRule br;
  br.dzl = a.dir[2 * kCols + lane];
  band_begin(a, tl.c, tl.j0, tl.ncol, lane, r, &br.n_lo, &br.n_hi);
  int cells = 0;
  const int L = a.lds_triangles;
  for (int f0 = 0; f0 < tl.c.nf; f0 += L) {
    const int fend = min(tl.c.nf, f0 + L);
    int n = 0;   // triangles staged so far (the same in every thread)
    for (int r0 = f0; r0 < fend; r0 += kCastThreads) n = stage_scan_pass(a, tl, br, r0, fend, n, tris, wcnt);
    band_cast(tris, n, wave, r);
    if constexpr (kTrace) if (tid < kBands) cells += band_tally(tris, n, tid);
    __syncthreads();   // the stage is rewritten by the next chunk
  }
  band_merge_store<kTrace>(a, tl.c, tl.j0, tl.ncol, r, mt, mi);
  if constexpr (kTrace) if (tid < kBands) s.cells[(long long)blockIdx.x * kBands + tid] = cells;
}

// the list staging under the band loop
template <bool kTrace>
__global__ __launch_bounds__(kCastThreads) void scene_band_list_kernel(const SceneBandArgs s)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  SceneTri* tris = reinterpret_cast<SceneTri*>(lds_raw);
  __shared__ double mt[kCastThreads / 64][2][64];
  __shared__ int mi[kCastThreads / 64][2][64];
  const SceneCastArgs& a = s.b.c;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SceneTile tl = tile_begin<false>(a);
  BandLane r;
  BandRule br;
  br.dzl = a.dir[2 * kCols + lane];
  band_begin(a, tl.c, tl.j0, tl.ncol, lane, r, &br.n_lo, &br.n_hi);
  int cells = 0;
  const long long e0 = s.b.off[blockIdx.x], e1 = s.b.off[(long long)blockIdx.x + 1];
  const int L = a.lds_triangles;
  for (long long s0 = e0; s0 < e1; s0 += L) {
    const int n = (int)min((long long)L, e1 - s0);
    stage_list_chunk<true>(a, tl.c, s.b.list + s0, n, tris, br);
    __syncthreads();
    band_cast(tris, n, wave, r);
    if constexpr (kTrace) if (tid < kBands) cells += band_tally(tris, n, tid);
    __syncthreads();   // the stage is rewritten by the next chunk
  }
  band_merge_store<kTrace>(a, tl.c, tl.j0, tl.ncol, r, mt, mi);
  if constexpr (kTrace) if (tid < kBands) s.cells[(long long)blockIdx.x * kBands + tid] = cells;
}

// ---- stage 3: compaction into ray order + noise ---------------------------------------------------------------------------------------------
// position k of a window in ascending COLUMN order -> (column, window column)
__device__ __forceinline__ void ordered_col(const SceneCloud& c, int k, int* col, int* j)
{
  const int wrap = max(0, c.first + c.count - kCols);   // columns 0 .. wrap - 1 are the window's tail
  if (k < wrap) { *col = k; *j = k + kCols - c.first; }
  else { *col = c.first + (k - wrap); *j = k - wrap; }
}

// grid (clouds, 64 rows)
__global__ __launch_bounds__(256) void scene_count_kernel(const SceneCloud* __restrict__ clouds, const double* __restrict__ t, int* __restrict__ rowcount)
{
  __shared__ int wsum[4];
  const SceneCloud c = clouds[blockIdx.x];
  const double* row = t + c.tbase + (long long)blockIdx.y * c.count;
  int n = 0;
  for (int j = threadIdx.x; j < c.count; j += 256) n += row[j] < INFINITY ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) rowcount[blockIdx.x * kRows + blockIdx.y] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup of 1024: per cloud index w, the exclusive scan of rowcount in (scene, row) order -> rowoff; offsets [B + 1][2]
__global__ __launch_bounds__(1024) void scene_scan_kernel(const int* __restrict__ rowcount, long long* __restrict__ rowoff, long long* __restrict__ offsets, int B)
{
  __shared__ long long part[1024];
  const int tid = threadIdx.x;
  const long long n = (long long)B * kRows, per = (n + 1023) / 1024;
  for (int w = 0; w < 2; ++w) {
    const long long lo = min(n, tid * per), hi = min(n, lo + per);
    long long s = 0;
    for (long long e = lo; e < hi; ++e) s += rowcount[((e / kRows) * 2 + w) * kRows + e % kRows];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
      long long run = 0;
      for (int i = 0; i < 1024; ++i) { const long long v = part[i]; part[i] = run; run += v; }
      offsets[(long long)B * 2 + w] = run;
    }
    __syncthreads();
    long long run = part[tid];
    for (long long e = lo; e < hi; ++e) {
      const long long i = ((e / kRows) * 2 + w) * kRows + e % kRows;
      rowoff[i] = run;
      if (e % kRows == 0) offsets[(e / kRows) * 2 + w] = run;
      run += rowcount[i];
    }
    __syncthreads();
  }
}

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// grid (clouds, 64 rows)
__global__ __launch_bounds__(256) void scene_scatter_kernel(const SceneCloud* __restrict__ clouds, const double* __restrict__ t, const double* __restrict__ dir,
                                                            const long long* __restrict__ rowoff, uint64_t seed, float clip, float* __restrict__ out0,
                                                            float* __restrict__ out1)
{
  __shared__ int wcnt[4];
  const SceneCloud c = clouds[blockIdx.x];
  const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* row = t + c.tbase + (long long)r * c.count;
  float* out = (c.which ? out1 : out0) + rowoff[blockIdx.x * kRows + r] * 3;
  const double dz = dir[2 * kCols + r];
  int done = 0;   // points of this row written so far (the same in every thread)
  for (int k0 = 0; k0 < c.count; k0 += 256) {
    const int k = k0 + tid;
    int col = 0, j = 0;
    double tt = INFINITY;
    if (k < c.count) { ordered_col(c, k, &col, &j); tt = row[j]; }
    const bool hit = tt < INFINITY;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    int base = done, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int n = wcnt[w]; if (w < wave) base += n; total += n; }
    if (hit) {
      float v[3] = {(float)(tt * dir[col]), (float)(tt * dir[kCols + col]), (float)(tt * dz)};
      if (c.strength > 0.f) {
        // the dataset sampler's stream (alignnet_dataset.hip), keyed by (seed, scene id, cloud, ray index)
        const uint64_t ray = (uint64_t)r * kCols + (uint64_t)col;
        const uint64_t key = mix64(seed ^ (c.scene_id * 0x9E3779B97F4A7C15ull) ^ ((2 * ray + (uint64_t)c.which) * 0xD1B54A32D192ED03ull));
        const uint64_t k2 = mix64(key + 0x632BE59BD9B4E019ull), k3 = mix64(key + 0xC6BC279692B5C323ull);
        const float u0 = ((float)(k2 >> 40) + 0.5f) * (1.0f / 16777216.0f), u1 = (float)((k2 >> 16) & 0xFFFFFF) * (1.0f / 16777216.0f);
        const float u2 = ((float)(k3 >> 40) + 0.5f) * (1.0f / 16777216.0f), u3 = (float)((k3 >> 16) & 0xFFFFFF) * (1.0f / 16777216.0f);
        const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
        const float z0 = r0 * cosf(6.28318530718f * u1), z1 = r0 * sinf(6.28318530718f * u1), z2 = r1 * cosf(6.28318530718f * u3);
        v[0] += fminf(fmaxf(c.strength * z0, -clip), clip);
        v[1] += fminf(fmaxf(c.strength * z1, -clip), clip);
        v[2] += fminf(fmaxf(c.strength * z2, -clip), clip);
      }
      float* o = out + (size_t)(base + __popcll(m & ((1ull << lane) - 1ull))) * 3;
      o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
    done += total;
    __syncthreads();
  }
}

// ---- host state ------------------------------------------------------------------------------------------------------------------------------
struct SceneWS {
  // mesh library (alignnet_scene_upload_meshes)
  int M = -1;                               // -1: nothing uploaded
  std::vector<long long> moff;              // [M + 1][2] first vertex / face
  std::vector<double> centroid;             // [M][3], normalised frame
  double* d_verts = nullptr; int* d_faces = nullptr;
  double* d_dir = nullptr;                  // sensor tables
  // work buffers, grown on demand
  SceneCloud* d_clouds = nullptr; int* d_win = nullptr; int* d_rowcount = nullptr; long long* d_rowoff = nullptr;   // per cloud
  size_t cap_clouds = 0, cap_win = 0, cap_rowcount = 0, cap_rowoff = 0;
  int* d_tiles = nullptr; size_t cap_tiles = 0;
  double* d_t = nullptr; int* d_tri = nullptr; size_t cap_t = 0, cap_tri = 0;
  // binned cast: list lengths / fill cursors and offsets per (cloud, tile) of the binned clouds, the triangle lists
  int* d_bincnt = nullptr; long long* d_binoff = nullptr; size_t cap_bincnt = 0, cap_binoff = 0;
  int* d_binlist = nullptr; size_t cap_binlist = 0;
  int* d_cells = nullptr; size_t cap_cells = 0;   // the band read-back: [tiles][8]
  // the last result (alignnet_scene_generate)
  int B = -1;
  std::vector<long long> offsets;           // [B + 1][2]
  long long* d_offsets = nullptr; size_t cap_off = 0;
  float* d_pts[2] = {nullptr, nullptr}; size_t cap_pts[2] = {0, 0};
};

SceneWS* sws(alignnet_handle* h) { return static_cast<SceneWS*>(h->scene_ws); }

void default_sensor(std::vector<double>& dir)
{
  dir.resize(2 * kCols + kRows);
  const double vfov = 26.9, hfov = 360.0;
  for (int c = 0; c < kCols; ++c) {
    const double hangle = -hfov / 2.0 + hfov / kCols * c;
    dir[c] = std::sin(hangle / 180. * M_PI) * 120.0; dir[kCols + c] = std::cos(hangle / 180. * M_PI) * 120.0;
  }
  for (int r = 0; r < kRows; ++r) dir[2 * kCols + r] = std::tan((-vfov / 2.0 + vfov / (kRows - 1) * r) / 180. * M_PI) * 120.0;
}

int ensure_ws(alignnet_handle* h)
{
  if (h->scene_ws) return 0;
  SceneWS* w = new SceneWS();
  h->scene_ws = w;
  std::vector<double> dir;
  default_sensor(dir);
  HIP_TRY(h, hipMalloc(&w->d_dir, dir.size() * sizeof(double)));
  HIP_TRY(h, hipMemcpy(w->d_dir, dir.data(), dir.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

struct SceneTrace {
  int lds_triangles; double* t; int32_t* triangle; int32_t* window; int32_t* lds_triangles_used;
  bool binned; int32_t* tile_counts /*[kMaxTiles]*/; int64_t* entries;   // the binned read-back
  bool rows; int32_t* cell_counts /*[kMaxTiles][8]*/; int64_t* cells;    // the band read-back
};

// one cast launch: one workgroup per tile, none for no tiles; the traced instantiation writes the read-backs' records
template <class Args>
void launch_cast(void (*plain)(Args), void (*traced)(Args), bool trace, size_t tiles, size_t lds, hipStream_t stream, const Args& args)
{
  if (tiles > 0) hipLaunchKernelGGL(trace ? traced : plain, dim3((unsigned)tiles), dim3(kCastThreads), lds, stream, args);
}

// B scenes x 2 clouds (or, traced: ONE cloud, pose [4]); results stay on the device
int run_scene(alignnet_handle* h, const char* fn, const int32_t* mesh, const double* scale, const double* poses, const int64_t* scene_ids, int nclouds,
              uint64_t seed, double sigma, double clip, const SceneTrace* trace)
{
  const std::string name(fn);
  SceneWS* w = sws(h);
  const int B = trace ? 1 : nclouds / 2, per = trace ? 1 : 2;
  std::vector<SceneCloud> cl((size_t)nclouds);
  for (int i = 0; i < nclouds; ++i) {
    const int b = i / per;
    if (mesh[b] < 0 || mesh[b] >= w->M) return fail(h, name + ": mesh " + std::to_string(mesh[b]) + " out of range");
    if (!std::isfinite(scale[b])) return fail(h, name + ": non-finite scale");
    const double* p = poses + (size_t)i * 4;
    for (int k = 0; k < 4; ++k) if (!std::isfinite(p[k])) return fail(h, name + ": non-finite pose");
    SceneCloud& c = cl[i];
    std::memset(&c, 0, sizeof(c));
    c.cs = std::cos(p[3]); c.sn = std::sin(p[3]); c.scale = scale[b]; c.px = p[0]; c.py = p[1]; c.pz = p[2];
    c.v0 = w->moff[(size_t)mesh[b] * 2]; c.f0 = w->moff[(size_t)mesh[b] * 2 + 1];
    c.nf = (int)(w->moff[(size_t)(mesh[b] + 1) * 2 + 1] - c.f0);
    c.scene_id = scene_ids ? (unsigned long long)scene_ids[b] : (unsigned long long)b;
    c.which = trace ? 0 : i % 2;
    if (sigma > 0.0) {
      // mesh.centroid of the posed mesh (area-weighted; a similarity keeps the weights): max(0.005, sigma |centroid| / 80), pointcloud.py:1134
      const double* g = &w->centroid[(size_t)mesh[b] * 3];
      const double sx = c.scale * g[0], sy = c.scale * g[1], sz = c.scale * g[2];
      const double x = (c.cs * sx - c.sn * sy) + c.px, y = (c.sn * sx + c.cs * sy) + c.py, z = sz + c.pz;
      c.strength = (float)std::max(0.005, sigma * std::sqrt(x * x + y * y + z * z) / 80.);
    }
  }
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  const size_t nc = (size_t)nclouds;
  if (grow(h, &w->d_clouds, &w->cap_clouds, nc) || grow(h, &w->d_win, &w->cap_win, nc * 2)) return 1;
  if (grow(h, &w->d_rowcount, &w->cap_rowcount, nc * kRows) || grow(h, &w->d_rowoff, &w->cap_rowoff, nc * kRows)) return 1;
  if (grow(h, &w->d_offsets, &w->cap_off, (size_t)(B + 1) * 2)) return 1;
  w->B = -1;   // no result until this call has finished
  w->offsets.assign((size_t)(B + 1) * 2, 0);
  std::vector<int> win((size_t)nclouds * 2, 0), tiles;
  if (nclouds > 0) {
    HIP_TRY(h, hipMemcpyAsync(w->d_clouds, cl.data(), cl.size() * sizeof(SceneCloud), hipMemcpyHostToDevice, h->stream));
    {
      alignnet::ProfScope prof_scope(h, alignnet::PK_SCENE_WINDOW);
      hipLaunchKernelGGL(scene_window_kernel, dim3(nclouds), dim3(256), 0, h->stream, w->d_clouds, w->d_verts, w->d_faces, w->d_win);
    }
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(win.data(), w->d_win, win.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  // deal the work: (cloud, tile of the window); the t tables and the point blobs are sized by the windows.  Which cast a cloud takes ("scene_cast";
  // the read-backs choose their own) depends on its mesh alone, never on what else is in the call; the binned clouds' tiles come behind the scan's.
  const int mode = trace ? (trace->binned ? 1 : 0) : h->scene_cast;
  const bool rows = trace ? trace->rows : h->scene_rows != 0;
  std::vector<int> btiles;
  int nbinned = 0, max_nf = 0;
  size_t nt = 0, npts[2] = {0, 0};
  for (int i = 0; i < nclouds; ++i) {
    SceneCloud& c = cl[i];
    c.first = win[(size_t)i * 2]; c.count = win[(size_t)i * 2 + 1];
    if (c.first < 0 || c.first >= kCols || c.count < 0 || c.count > kCols) return fail(h, name + ": window out of range (internal)");
    c.tbase = (long long)nt;
    nt += (size_t)c.count * kRows;
    npts[c.which] += (size_t)c.count * kRows;
    const bool binned = mode == 1 || (mode == 2 && c.nf > kSceneBinAuto);
    c.bt0 = binned ? (int)(btiles.size() / 2) : -1;
    if (binned) { ++nbinned; max_nf = std::max(max_nf, c.nf); }
    std::vector<int>& dst = binned ? btiles : tiles;
    for (int k = 0; k * kTileCols < c.count; ++k) { dst.push_back(i); dst.push_back(k); }
  }
  const size_t nscan = tiles.size() / 2, nbt = btiles.size() / 2;
  if (nscan + nbt > 0x7fffffffu) return fail(h, name + ": too many tiles in one call");
  tiles.insert(tiles.end(), btiles.begin(), btiles.end());
  if (grow(h, &w->d_t, &w->cap_t, nt)) return 1;
  if (trace && grow(h, &w->d_tri, &w->cap_tri, nt)) return 1;
  if (trace && rows && grow(h, &w->d_cells, &w->cap_cells, (nscan + nbt) * kBands)) return 1;
  if (grow(h, &w->d_tiles, &w->cap_tiles, tiles.size())) return 1;
  for (int k = 0; k < 2; ++k) if (grow(h, &w->d_pts[k], &w->cap_pts[k], npts[k] * 3)) return 1;
  int L = kLdsTriangles;
  if (trace && trace->lds_triangles > 0) L = trace->lds_triangles;
  long long bin_entries = 0;   // entries of all tile lists of this call
  if (nclouds > 0) {
    HIP_TRY(h, hipMemcpyAsync(w->d_clouds, cl.data(), cl.size() * sizeof(SceneCloud), hipMemcpyHostToDevice, h->stream));
    if (!tiles.empty()) HIP_TRY(h, hipMemcpyAsync(w->d_tiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (nbt > 0) {
      // bin the triangles of the binned clouds to their tiles: lengths, offsets (the total comes back: the lists are sized by it), lists
      if (grow(h, &w->d_bincnt, &w->cap_bincnt, nbt) || grow(h, &w->d_binoff, &w->cap_binoff, nbt + 1)) return 1;
      const dim3 bgrid((unsigned)nclouds, (unsigned)std::min(kBinSlices, std::max(1, (max_nf + 255) / 256)));
      HIP_TRY(h, hipMemsetAsync(w->d_bincnt, 0, nbt * sizeof(int), h->stream));
      {
        alignnet::ProfScope prof_scope(h, alignnet::PK_SCENE_BIN);
        hipLaunchKernelGGL(scene_bin_tally_kernel, bgrid, dim3(256), 0, h->stream, w->d_clouds, w->d_verts, w->d_faces, w->d_bincnt);
        hipLaunchKernelGGL(scene_bin_offsets_kernel, dim3(1), dim3(1024), 0, h->stream, w->d_bincnt, w->d_binoff, (int)nbt);
      }
      HIP_TRY(h, hipGetLastError());
      HIP_TRY(h, hipMemcpyAsync(&bin_entries, w->d_binoff + nbt, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      if (bin_entries < 0) return fail(h, name + ": tile lists out of range (internal)");
      if (grow(h, &w->d_binlist, &w->cap_binlist, (size_t)bin_entries)) return 1;
      if (bin_entries > 0) {
        alignnet::ProfScope prof_scope(h, alignnet::PK_SCENE_BIN);
        hipLaunchKernelGGL(scene_bin_fill_kernel, bgrid, dim3(256), 0, h->stream, w->d_clouds, w->d_verts, w->d_faces, w->d_bincnt, w->d_binoff, w->d_binlist);
      }
      HIP_TRY(h, hipGetLastError());
    }
    if (!tiles.empty()) {
      SceneCastArgs a;
      a.clouds = w->d_clouds; a.tiles = w->d_tiles; a.verts = w->d_verts; a.faces = w->d_faces; a.dir = w->d_dir; a.t = w->d_t; a.tri = w->d_tri;
      a.lds_triangles = L;
      const size_t lds = (size_t)L * sizeof(SceneTri);
      alignnet::ProfScope prof_scope(h, rows ? alignnet::PK_SCENE_BAND : alignnet::PK_SCENE_CAST);
      // the list staging's tiles come behind the scan staging's; by elevation band the grids, the stage and the tile order are the same, and the cell
      // counts of the list tiles follow those of the scan tiles, as the tiles do
      const bool traced = trace != nullptr;
      const SceneBinCastArgs scan = {a, w->d_binoff, w->d_binlist};
      SceneBinCastArgs list = scan;
      list.c.tiles = w->d_tiles + nscan * 2;
      if (rows) {
        launch_cast(scene_band_scan_kernel<false>, scene_band_scan_kernel<true>, traced, nscan, lds, h->stream, SceneBandArgs{scan, w->d_cells});
        launch_cast(scene_band_list_kernel<false>, scene_band_list_kernel<true>, traced, nbt, lds, h->stream,
                    SceneBandArgs{list, traced ? w->d_cells + nscan * kBands : nullptr});
      } else {
        launch_cast(scene_cast_kernel<false>, scene_cast_kernel<true>, traced, nscan, lds, h->stream, a);
        launch_cast(scene_bincast_kernel<false>, scene_bincast_kernel<true>, traced, nbt, lds, h->stream, list);
      }
    }
    HIP_TRY(h, hipGetLastError());
  }
  if (trace) {
    // the record: t and triangle per ray of the window, laid out by ray index on the host
    std::vector<double> t(nt); std::vector<int> tri(nt);
    std::vector<long long> boff(nbt + 1, 0);
    if (trace->binned && nbt) HIP_TRY(h, hipMemcpyAsync(boff.data(), w->d_binoff, boff.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    std::vector<int> cells((nscan + nbt) * kBands, 0);
    if (rows && !cells.empty()) HIP_TRY(h, hipMemcpyAsync(cells.data(), w->d_cells, cells.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (nt) {
      HIP_TRY(h, hipMemcpyAsync(t.data(), w->d_t, nt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipMemcpyAsync(tri.data(), w->d_tri, nt * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < kRays; ++i) { trace->t[i] = std::numeric_limits<double>::infinity(); trace->triangle[i] = -1; }
    const SceneCloud& c = cl[0];
    for (int r = 0; r < kRows; ++r)
      for (int j = 0; j < c.count; ++j) {
        const size_t ray = (size_t)r * kCols + (size_t)((c.first + j) % kCols), o = (size_t)r * c.count + j;
        trace->t[ray] = t[o]; trace->triangle[ray] = tri[o];
      }
    trace->window[0] = c.first; trace->window[1] = c.count;
    *trace->lds_triangles_used = L;
    if (trace->binned) {
      for (int k = 0; k < kMaxTiles; ++k) trace->tile_counts[k] = (size_t)k < nbt ? (int32_t)(boff[k + 1] - boff[k]) : 0;
      *trace->entries = bin_entries;
    }
    if (rows) {
      *trace->cells = 0;
      for (size_t k = 0; k < (size_t)kMaxTiles * kBands; ++k) {
        trace->cell_counts[k] = k < cells.size() ? cells[k] : 0;
        *trace->cells += trace->cell_counts[k];
      }
    }
    return 0;
  }
  if (nclouds > 0) {
    alignnet::ProfScope prof_scope(h, alignnet::PK_SCENE_COMPACT);
    hipLaunchKernelGGL(scene_count_kernel, dim3(nclouds, kRows), dim3(256), 0, h->stream, w->d_clouds, w->d_t, w->d_rowcount);
    hipLaunchKernelGGL(scene_scan_kernel, dim3(1), dim3(1024), 0, h->stream, w->d_rowcount, w->d_rowoff, w->d_offsets, B);
    hipLaunchKernelGGL(scene_scatter_kernel, dim3(nclouds, kRows), dim3(256), 0, h->stream, w->d_clouds, w->d_t, w->d_dir, w->d_rowoff, seed, (float)clip,
                       w->d_pts[0], w->d_pts[1]);
  }
  HIP_TRY(h, hipGetLastError());
  if (nclouds > 0)
    HIP_TRY(h, hipMemcpyAsync(w->offsets.data(), w->d_offsets, w->offsets.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  w->B = B;
  h->scene_binned_clouds = nbinned; h->scene_bin_entries = bin_entries;
  return 0;
}

}  // namespace

extern "C" void alignnet_scene_free(alignnet_handle* h)
{
  if (!h || !h->scene_ws) return;
  SceneWS* w = sws(h);
  if (h->stream) hipStreamSynchronize(h->stream);
  void* const ptrs[] = {w->d_verts, w->d_faces, w->d_dir, w->d_clouds, w->d_win, w->d_rowcount, w->d_rowoff, w->d_tiles, w->d_t, w->d_tri, w->d_offsets,
                        w->d_pts[0], w->d_pts[1], w->d_bincnt, w->d_binoff, w->d_binlist, w->d_cells};
  for (void* p : ptrs) if (p) hipFree(p);
  delete w;
  h->scene_ws = nullptr;
}

extern "C" int alignnet_scene_set_sensor(alignnet_handle* h, const double* dir_x, const double* dir_y, const double* dir_z)
{
  if (!h) return 1;
  if (!dir_x || !dir_y || !dir_z) return fail(h, "alignnet_scene_set_sensor: null table");
  for (int c = 0; c < kCols; ++c) if (!std::isfinite(dir_x[c]) || !std::isfinite(dir_y[c])) return fail(h, "alignnet_scene_set_sensor: non-finite direction");
  for (int r = 0; r < kRows; ++r) if (!std::isfinite(dir_z[r])) return fail(h, "alignnet_scene_set_sensor: non-finite direction");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (ensure_ws(h)) return 1;
  SceneWS* w = sws(h);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipMemcpy(w->d_dir, dir_x, kCols * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(w->d_dir + kCols, dir_y, kCols * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(h, hipMemcpy(w->d_dir + 2 * kCols, dir_z, kRows * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

extern "C" int alignnet_scene_free_meshes(alignnet_handle* h)
{
  if (!h) return 1;
  if (!h->scene_ws) return 0;
  SceneWS* w = sws(h);
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (w->d_verts) hipFree(w->d_verts);
  if (w->d_faces) hipFree(w->d_faces);
  w->d_verts = nullptr; w->d_faces = nullptr; w->M = -1; w->moff.clear(); w->centroid.clear();
  return 0;
}

extern "C" int alignnet_scene_upload_meshes(alignnet_handle* h, const double* vertices, const int32_t* faces, const int64_t* offsets, const double* centroids,
                                            int32_t M)
{
  if (!h) return 1;
  const std::string name("alignnet_scene_upload_meshes");
  if (M < 0 || !offsets || (M > 0 && !centroids)) return fail(h, name + ": M < 0 or a null table");
  if (offsets[0] != 0 || offsets[1] != 0) return fail(h, name + ": offsets must start at 0");
  for (int m = 0; m < M; ++m) {
    const int64_t nv = offsets[(m + 1) * 2] - offsets[m * 2], nf = offsets[(m + 1) * 2 + 1] - offsets[m * 2 + 1];
    if (nv < 0 || nf < 0) return fail(h, name + ": offsets must be non-decreasing");
    if (nv > 0x7fffffff || nf > 0x7fffffff / 3) return fail(h, name + ": mesh " + std::to_string(m) + " too large");
    for (int k = 0; k < 3; ++k) if (!std::isfinite(centroids[m * 3 + k])) return fail(h, name + ": non-finite centroid of mesh " + std::to_string(m));
  }
  const size_t nv = (size_t)offsets[(size_t)M * 2], nf = (size_t)offsets[(size_t)M * 2 + 1];
  if ((nv && !vertices) || (nf && !faces)) return fail(h, name + ": null vertices / faces");
  for (size_t i = 0; i < nv * 3; ++i) if (!std::isfinite(vertices[i])) return fail(h, name + ": non-finite vertex " + std::to_string(i / 3));
  for (int m = 0; m < M; ++m) {
    const int64_t mv = offsets[(m + 1) * 2] - offsets[m * 2];
    for (int64_t f = offsets[m * 2 + 1] * 3; f < offsets[(m + 1) * 2 + 1] * 3; ++f)
      if (faces[f] < 0 || faces[f] >= mv)
        return fail(h, name + ": face " + std::to_string(f / 3 - offsets[m * 2 + 1]) + " of mesh " + std::to_string(m) + " names vertex " + std::to_string(faces[f]) +
                           " (the mesh has " + std::to_string(mv) + ")");
  }
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (ensure_ws(h)) return 1;
  if (alignnet_scene_free_meshes(h)) return 1;
  SceneWS* w = sws(h);
  HIP_TRY(h, hipMalloc(&w->d_verts, std::max<size_t>(nv, 1) * 3 * sizeof(double)));
  HIP_TRY(h, hipMalloc(&w->d_faces, std::max<size_t>(nf, 1) * 3 * sizeof(int)));
  if (nv) HIP_TRY(h, hipMemcpy(w->d_verts, vertices, nv * 3 * sizeof(double), hipMemcpyHostToDevice));
  if (nf) HIP_TRY(h, hipMemcpy(w->d_faces, faces, nf * 3 * sizeof(int), hipMemcpyHostToDevice));
  w->moff.assign(offsets, offsets + (size_t)(M + 1) * 2);
  w->centroid.assign(centroids, centroids + (size_t)M * 3);
  w->M = M;
  w->B = -1;
  return 0;
}

extern "C" int alignnet_scene_generate(alignnet_handle* h, const int32_t* mesh, const double* scale, const double* poses, const int64_t* scene_ids, int32_t B,
                                       uint64_t seed, double sigma, double clip, int64_t* offsets)
{
  if (!h) return 1;
  const std::string name("alignnet_scene_generate");
  if (!h->scene_ws || sws(h)->M < 0) return fail(h, name + ": no meshes uploaded");
  if (B < 0 || B > (1 << 20)) return fail(h, name + ": B out of range");
  if (B > 0 && (!mesh || !scale || !poses)) return fail(h, name + ": null argument");
  if (!std::isfinite(sigma) || (sigma > 0.0 && !(clip > 0.0 && std::isfinite(clip)))) return fail(h, name + ": sigma must be finite, clip > 0 with noise on");
  if (run_scene(h, name.c_str(), mesh, scale, poses, scene_ids, 2 * B, seed, sigma, clip, nullptr)) return 1;
  if (offsets) for (size_t i = 0; i < sws(h)->offsets.size(); ++i) offsets[i] = sws(h)->offsets[i];
  return 0;
}

extern "C" int alignnet_scene_read(alignnet_handle* h, float* points1, float* points2)
{
  if (!h) return 1;
  if (!h->scene_ws || sws(h)->B < 0) return fail(h, "alignnet_scene_read: nothing generated yet");
  SceneWS* w = sws(h);
  float* const dst[2] = {points1, points2};
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  for (int k = 0; k < 2; ++k) {
    const size_t n = (size_t)w->offsets[(size_t)w->B * 2 + k];
    if (n && dst[k]) HIP_TRY(h, hipMemcpyAsync(dst[k], w->d_pts[k], n * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int alignnet_scene_install_dataset(alignnet_handle* h, const float* labels)
{
  if (!h) return 1;
  if (!h->scene_ws || sws(h)->B < 0) return fail(h, "alignnet_scene_install_dataset: nothing generated yet");
  SceneWS* w = sws(h);
  if (w->B < 1 || !labels) return fail(h, "alignnet_scene_install_dataset: no scenes or null labels");
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
  return alignnet_dataset_install(h, w->d_pts[0], w->d_pts[1], true, reinterpret_cast<const int64_t*>(w->offsets.data()), labels, w->B,
                                  "alignnet_scene_install_dataset");
}

// what the three read-backs share; bad: what the entry point's own checks found (null: nothing), reported in its place between the common ones
static int debug_cast(alignnet_handle* h, const char* fn, const char* bad, int32_t mesh, double scale, const double* pose, const SceneTrace& tr)
{
  if (!h) return 1;
  const std::string name(fn);
  if (!h->scene_ws || sws(h)->M < 0) return fail(h, name + ": no meshes uploaded");
  if (bad) return fail(h, name + ": " + bad);
  if (tr.lds_triangles < 0 || tr.lds_triangles > kLdsTriangles)
    return fail(h, name + ": lds_triangles must be in [0, " + std::to_string(kLdsTriangles) + "] (0 = as shipped)");
  return run_scene(h, fn, &mesh, &scale, pose, nullptr, 1, 0, 0.0, 0.0, &tr);
}

extern "C" int alignnet_debug_scene_cast(alignnet_handle* h, int32_t mesh, double scale, const double* pose, int32_t lds_triangles, double* t, int32_t* triangle,
                                         int32_t* window, int32_t* lds_triangles_used)
{
  const char* bad = !pose || !t || !triangle || !window || !lds_triangles_used ? "null argument" : nullptr;
  const SceneTrace tr = {lds_triangles, t, triangle, window, lds_triangles_used, false, nullptr, nullptr};
  return debug_cast(h, "alignnet_debug_scene_cast", bad, mesh, scale, pose, tr);
}

extern "C" int alignnet_debug_scene_cast_binned(alignnet_handle* h, int32_t mesh, double scale, const double* pose, int32_t lds_triangles, double* t,
                                                int32_t* triangle, int32_t* window, int32_t* lds_triangles_used, int32_t* tile_counts, int64_t* entries)
{
  const char* bad = !pose || !t || !triangle || !window || !lds_triangles_used || !tile_counts || !entries ? "null argument" : nullptr;
  const SceneTrace tr = {lds_triangles, t, triangle, window, lds_triangles_used, true, tile_counts, entries};
  return debug_cast(h, "alignnet_debug_scene_cast_binned", bad, mesh, scale, pose, tr);
}

extern "C" int alignnet_debug_scene_cast_rows(alignnet_handle* h, int32_t mesh, double scale, const double* pose, int32_t lds_triangles, int32_t binned,
                                              int32_t* window, double* t, int32_t* triangle, int32_t* lds_triangles_used, int32_t* cell_counts,
                                              int64_t* cells)
{
  const char* bad = !pose || !t || !triangle || !window || !lds_triangles_used || !cell_counts || !cells ? "null argument"
                    : binned != 0 && binned != 1 ? "binned must be 0 or 1" : nullptr;
  std::vector<int32_t> tile_counts(kMaxTiles);
  int64_t entries = 0;
  const SceneTrace tr = {lds_triangles, t, triangle, window, lds_triangles_used, binned != 0, tile_counts.data(), &entries, true, cell_counts, cells};
  return debug_cast(h, "alignnet_debug_scene_cast_rows", bad, mesh, scale, pose, tr);
}
